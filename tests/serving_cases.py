"""Shared helpers for the factor-consumer tests: golden fixture decoding and a
vectorised exact restatement of the reference scoring order for larger
synthetic cases (NumPy elementwise multiply then add == Python float ops)."""
import numpy as np

from conftest import load_golden

KS = (3, 11, 64)


def fixture(k):
    d = load_golden(f"serving_k{k}.npz")
    d["als_ids"] = {int(m): j for j, m in enumerate(d["als_keys"])}
    d["med"] = {int(m): float(v) for m, v in zip(d["med_keys"], d["med_vals"])}
    o = d["u_off"]
    d["lists"] = [[(int(m), float(r)) for m, r in zip(d["u_mid"][o[u]:o[u + 1]],
                                                      d["u_r"][o[u]:o[u + 1]])]
                  for u in range(len(o) - 1)]
    t = d["t_off"]
    d["t_lists"] = [[(int(m), float(r)) for m, r in zip(d["t_mid"][t[i]:t[i + 1]],
                                                        d["t_r"][t[i]:t[i + 1]])]
                    for i in range(len(t) - 1)]
    ro = d["rec_off"]
    d["recs"] = [[(float(s), int(m)) for s, m in zip(d["rec_score"][ro[u]:ro[u + 1]],
                                                    d["rec_mid"][ro[u]:ro[u + 1]])]
                 for u in range(len(ro) - 1)]
    return d


def exact_scores(X, Vc, med):
    """Reference order for many users x candidates: s = 0; s += x_j v_j ...;
    s += bias; s += median (models.py:725-731), all in fp64 without FMA."""
    X = np.atleast_2d(X)
    k = Vc.shape[1]
    s = np.zeros((X.shape[0], Vc.shape[0]))
    for j in range(k):
        s = s + X[:, j:j + 1] * Vc[None, :, j]
    s = s + X[:, k:k + 1]
    return s + med[None, :]


def exact_top_n(scores, mids, excluded, n):
    """recommend.py:93-106 on one score row: (score, movie id) descending,
    skipping excluded movie ids, first n."""
    order = np.lexsort((-mids.astype(np.int64), -scores))
    out = []
    for c in order:
        if int(mids[c]) in excluded:
            continue
        out.append((float(scores[c]), int(mids[c])))
        if len(out) >= n:
            break
    return out


def synthetic_table(k, n_als, n_med_only, seed, ties=20):
    rs = np.random.RandomState(seed)
    ids = rs.choice(np.arange(1, 10 * (n_als + n_med_only)), n_als + n_med_only, replace=False)
    V = rs.normal(0, 0.6, (n_als, k))
    med = rs.choice(np.arange(1, 11) / 2.0, n_als)
    for _ in range(ties):
        a, b = rs.choice(n_als, 2, replace=False)
        V[b], med[b] = V[a], med[a]
    als_ids = {int(m): j for j, m in enumerate(ids[:n_als])}
    keys = list(ids[:n_als]) + list(ids[n_als:])
    vals = list(med) + list(rs.choice(np.arange(1, 11) / 2.0, n_med_only))
    order = rs.permutation(len(keys))
    medians = {int(keys[i]): float(vals[i]) for i in order}
    return V.reshape(-1), als_ids, medians


# --------------------------------------------------------------------------
# Host model of the top-N select's path and the inputs designed to reach each
# of its paths (tests/test_serving_select_model.py pins the paths on the CPU,
# tests/test_gpu_serving_edges.py runs the same inputs on the device).
# --------------------------------------------------------------------------
SEL_BINS = 2048     # linear bins of the fast path == buffer of the select (SEL_CAP)
SEL_DIGIT = 11      # radix digit, bits
SEL_BITS = 96       # 64 key bits, then the 32 movie-id bits


def score_keys(scores):
    """The order-preserving 64-bit key of each score: a larger score has the
    larger key, and -0.0 has +0.0's key."""
    s = np.asarray(scores, np.float64) + 0.0            # -0.0 + 0.0 == +0.0
    b = s.view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def select_walk(scores, mids, N, excluded=None, count_above=True):
    """The path the documented rule of the top-N select takes on one user's
    row, restated on the host: ``scores`` and ``mids`` of every candidate,
    ``excluded`` an optional boolean mask (an excluded candidate is not
    counted, but the user's [min, max] score range still includes it).

    Rule.  (1) Fast path: 2,048 equal-width bins over [min, max]; the boundary
    bin is the highest one with at least N candidates at or above it (bin 0 if
    there are fewer than N); it fits when the candidates at or above the
    boundary bin number at most 2,048.  It is not tried when min == max or
    the bin scale is not finite.  (2) Otherwise an MSB radix walk over the
    composite (score key, movie id), 64 + 32 bits, that starts at the first
    bit where the smallest and largest key differ (bit 64 when all keys are
    equal) and takes 11-bit digits (fewer at the end): per level the boundary
    digit is the highest one with N or more candidates at or above it counting
    those above the prefix so far; the walk stops when they number at most
    2,048 or all 96 bits are consumed.

    Returns ``(fast_path_fits, levels, above_before_last_level,
    straddles_key_id_boundary, collected)``: ``levels`` radix levels walked (0
    on the fast path), the number of candidates strictly above the prefix when
    the last level began, whether some level's digit held key bits and id
    bits, and the number of candidates handed to the final sort.

    ``count_above=False`` walks as a select would that forgot the candidates
    above the prefix when it places the boundary (``collected`` is still the
    true number at or above that boundary): for pinning that an input tells
    the two apart."""
    scores = np.asarray(scores, np.float64)
    mids = np.asarray(mids, np.int64)
    live = np.ones(len(scores), bool) if excluded is None else ~np.asarray(excluded, bool)
    smin, smax = float(scores.min()) + 0.0, float(scores.max()) + 0.0
    with np.errstate(divide="ignore", over="ignore"):
        scale = np.float64(SEL_BINS) / (np.float64(smax) - np.float64(smin))
    if smax > smin and np.isfinite(scale):
        bins = np.minimum(SEL_BINS - 1, (((scores[live] + 0.0) - smin) * scale).astype(np.int64))
        at_or_above = np.cumsum(np.bincount(bins, minlength=SEL_BINS)[::-1])[::-1]
        reach = np.flatnonzero(at_or_above >= N)
        collected = int(at_or_above[reach.max() if len(reach) else 0])
        if collected <= SEL_BINS:
            return True, 0, 0, False, collected
    keys = score_keys(scores)
    comp = [(int(k) << 32) | int(m) for k, m in zip(keys[live], mids[live])]   # 96 bits
    diff = int(keys.min()) ^ int(keys.max())
    pos = 64 - diff.bit_length() if diff else 64
    prefix = (int(keys.min()) << 32) >> (SEL_BITS - pos)      # the top `pos` bits
    above = levels = above_last = 0
    straddles = False
    while True:
        D = min(SEL_DIGIT, SEL_BITS - pos)
        straddles |= pos < 64 < pos + D
        levels += 1
        above_last = above
        low = SEL_BITS - pos - D
        digits = np.array([(x >> low) & ((1 << D) - 1) for x in comp
                           if x >> (SEL_BITS - pos) == prefix], np.int64)
        in_prefix = np.cumsum(np.bincount(digits, minlength=1 << D)[::-1])[::-1]
        at_or_above = in_prefix + (above if count_above else 0)
        reach = np.flatnonzero(at_or_above >= N)
        b = int(reach.max()) if len(reach) else 0
        prefix = (prefix << D) | b
        pos += D
        if at_or_above[b] <= SEL_BINS or pos >= SEL_BITS:
            bound = prefix << (SEL_BITS - pos)
            return False, levels, above_last, straddles, sum(1 for x in comp if x >= bound)
        above += int(in_prefix[b + 1]) if b + 1 < (1 << D) else 0


def value_table(values, mids):
    """``MovieTable`` arguments ``(k, V, als_ids, medians)`` of a table whose
    scores for the user row ``[1.0, 0.0]`` are exactly ``values``: k = 1,
    V[c] = values[c], every median 0.0, candidates in ``mids`` order.  Then
    ((0 + 1 v) + 0) + 0.0 == v bit for bit -- but for v = -0.0, whose score
    is +0.0 (a sum that starts at +0.0 is never -0.0).  A user row
    ``[x0, 0.0]`` scales or negates the scores by x0."""
    values = np.asarray(values, np.float64)
    mids = [int(m) for m in mids]
    assert len(set(mids)) == len(mids) == len(values)
    return 1, values.copy(), {m: c for c, m in enumerate(mids)}, {m: 0.0 for m in mids}


def distinct_ids(rs, n, hi):
    """n distinct movie ids below hi, in random order."""
    ids = np.unique(rs.randint(0, hi, 2 * n + 64).astype(np.int64))
    assert len(ids) >= n
    return rs.permutation(ids)[:n]


def select_inputs():
    """The inputs that reach each path of the select, by name:
    ``dict(values, mids, N, top)``; ``top`` are movie ids of the leading group
    (what the exclusion cases remove)."""
    out = {}
    rs = np.random.RandomState(11)
    # R1: the range is set by three outliers, so the cluster falls into one
    # linear bin; the cluster differs 20 bits below the outliers' first bit
    v = np.concatenate([[100.0, 101.0, 102.0], 3.0 + np.arange(9000) * 2.0 ** -30])
    p = rs.permutation(len(v))
    mids = rs.permutation(np.arange(1, len(v) + 1))
    out["R1"] = dict(values=v[p], mids=mids, N=1000, top=mids[np.argsort(-v[p])[:40]])
    # R2: a tie group wider than the buffer with the N-th place inside it;
    # ids from the whole 31-bit range ("spread"), or consecutive ("dense": the
    # cut is decided in the ids' low bits)
    v = np.concatenate([4.0 + np.arange(1, 101) / 128.0, np.full(5000, 3.5),
                        3.0 - np.arange(3000) / 4096.0])
    for name, mids in (("R2", distinct_ids(rs, len(v), 2 ** 31 - 1)),
                       ("R2_dense", 2 ** 30 + 12345 + rs.permutation(len(v)))):
        p = rs.permutation(len(v))
        out[name] = dict(values=v[p], mids=mids, N=400, top=mids[np.argsort(-v[p])[:130]])
    # R3: g candidates tied at the top, at and around the buffer's size
    for g in (2047, 2048, 2049):
        v = np.concatenate([np.full(g, 4.0), np.full(3000, 2.0)])
        for name, mids in ((f"R3_{g}", rs.permutation(np.arange(1, len(v) + 1))),
                           (f"R3_{g}_spread", distinct_ids(rs, len(v), 2 ** 31 - 1))):
            p = rs.permutation(len(v))
            tied = mids[v[p] == 4.0]
            out[name] = dict(values=v[p], mids=mids, N=1024, top=np.sort(tied)[-30:])
    # R6: 1,000 leaders above a cluster of ten 300-way ties that sits in one
    # linear bin: the last level begins with 1,000 above and needs 24 more; a
    # walk that forgot the 1,000 would take four of the ties, 2,200 in all
    v = np.concatenate([4.0 + np.arange(1, 1001) / 1024.0,
                        np.repeat(3.5 - np.arange(1, 11) * 2.0 ** -30, 300),
                        3.0 - np.arange(2000) / 4096.0])
    p = rs.permutation(len(v))
    mids = rs.permutation(np.arange(1, len(v) + 1))
    out["R6"] = dict(values=v[p], mids=mids, N=1024, top=mids[np.argsort(-v[p])[:40]])
    # R5: all scores equal, the order is the ids' alone, from their top bits on
    mids = distinct_ids(rs, 5000, 2 ** 31 - 1)
    mids[:2] = (2 ** 31 - 2, 5)
    out["R5"] = dict(values=np.full(5000, 2.75), mids=mids, N=400, top=np.sort(mids)[-50:])
    return out


def select_exclusions(inp):
    """Per input the exclusion sets its users run with: none, members of the
    leading group, and all but N - 7 candidates (fewer than N remain)."""
    rs = np.random.RandomState(len(inp["mids"]))
    mids = np.asarray(inp["mids"])
    few = set(int(m) for m in rs.permutation(mids)[:len(mids) - (inp["N"] - 7)])
    return [set(), set(int(m) for m in inp["top"]), few]


def signs_input():
    """Negative, zero (both signs) and positive values in one table:
    ``dict(values, mids, users)`` with ``users`` a list of ``(x0, excluded
    movie ids)``.  The 3,000 negatives are clustered (one linear bin), the
    3,000 positives spread, and there are 50 each of 0.0 and -0.0.
      0: x0 = 1                the positives lead
      1: x0 = -1               the cluster leads, negated: radix walk from bit 0
      2: x0 = 0                every score 0.0
      3: x0 = 1, 350 positives left   N = 400 cuts inside the zeros
      4: x0 = 1, 100 positives left   N = 400 cuts inside the negative cluster"""
    rs = np.random.RandomState(23)
    neg = -(3.0 + np.arange(3000) * 2.0 ** -30)
    pos = np.unique(rs.uniform(0.5, 100.0, 3100))[:3000]
    v = np.concatenate([neg, pos, np.full(50, 0.0), np.full(50, -0.0)])
    p = rs.permutation(len(v))
    v = v[p]
    mids = distinct_ids(rs, len(v), 2 ** 31 - 1)
    pm = rs.permutation(mids[v > 0])
    users = [(1.0, set()), (-1.0, set()), (0.0, set()),
             (1.0, set(int(m) for m in pm[350:])), (1.0, set(int(m) for m in pm[100:]))]
    return dict(values=v, mids=mids, users=users)
