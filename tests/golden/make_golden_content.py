"""Golden fixture for the content model (tag least squares), generated from the
REFERENCE's own Python code.

Run in the build container (needs /root/reference; writes nothing there):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_content.py

Imported from the reference (plain NumPy/SciPy modules, no data files read):
  * ``python/app_local/models.py``  -- ``TagLS_UserProfile``: profile, A, the
    ``scipy.sparse.linalg.lsqr`` solve and ``predict``.  The module's
    ``linalg.lsqr`` is wrapped to capture (A, b) and the full return of every
    solve;
  * ``python/full_data/my_util.py`` -- ``compute_ranking_agreement``.

Fixture  content_small.npz
  movie data    movie_genres (mg_*), movie_tags (mt_*: ln(count) + 1),
                tag_counts (tc_*), movie_medians in insertion order (med_*)
  lists         CSR (l_off, l_mid, l_r) with a name each (l_name)
  per list      p, profile, x_ref, itn_ref, istop_ref
                traj_x: SciPy's x after j = 1 .. 2 max(itn) iterations with the
                  stops disabled (atol = btol = conlim = 0, iter_lim = j)
                itn_perm: stop iterations, default settings, of 16 row
                  permutations of (A, b), 8 as CSR and 8 as dense arrays
                stable: all 16 equal itn_ref
                s_u: largest |x_variant - x_ref|_inf / max(1, |x_ref|_inf) of
                  the same 16 variants at stops disabled, iter_lim = itn_ref
                scores of every candidate, the top-60 list (rec_*)
  test lists    (t_off, t_mid, t_r) with the reference agreement (nan = None)
                and pair counts; a test list with a counted pair whose order
                could flip inside the score rounding bound is redrawn (dropped
                after 20 draws)
The generator asserts that the NumPy restatement of tests/content_cases.py
meets the acceptance rules on this fixture, and prints the measured spread.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference/python"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REF, "app_local"))
import models as ref_models  # noqa: E402  (reference: app_local/models.py)
sys.path.pop(0)
sys.path.insert(0, os.path.join(REF, "full_data"))
import my_util as ref_util  # noqa: E402  (reference: full_data/my_util.py)
sys.path.pop(0)

import content_cases as C  # noqa: E402

SEED = 20
HALF = np.arange(1, 11) / 2.0
SIZES = [2, 3, 4, 5, 9, 10, 11, 19, 20, 21, 30, 31, 50, 70, 71, 100, 150, 151, 200, 310, 311,
         400, 600]
N_VAR = 16
TOP = 60

captured = []
_lsqr = ref_models.linalg.lsqr


def _spy(A, b, **kw):
    r = _lsqr(A, b, **kw)
    captured.append((A.copy(), np.array(b, copy=True), r))
    return r


ref_models.linalg.lsqr = _spy


def movie_data(rs):
    n_movies, n_tags, n_genres = 660, 300, 19
    mids = [int(m) for m in rs.choice(np.arange(1, 30000), n_movies, replace=False)]
    tids = sorted(int(t) for t in rs.choice(np.arange(1, 66800), n_tags - 1, replace=False))
    tids.append(66814)                                   # the reference's largest tag id
    zipf = 1.0 / np.arange(1, n_tags + 1)
    zipf /= zipf.sum()
    special = {"none": mids[0:6], "few": mids[6:18], "equal": mids[18:22], "co": mids[22:30]}
    co_tags = (70001, 70002)
    genres, raw = {}, {}
    for m in mids[30:]:
        if rs.rand() >= 0.05:
            genres[m] = set(int(g) for g in rs.choice(n_genres, rs.randint(1, 5), replace=False))
        if rs.rand() >= 0.40:
            ts = rs.choice(n_tags, rs.randint(1, 12), replace=False, p=zipf)
            raw[m] = {tids[t]: int(rs.randint(1, 40)) for t in ts}
    for m in special["few"]:
        genres[m] = [{3}, {7}, {3, 7}][rs.randint(3)]
    for m in special["equal"]:
        genres[m] = {1, 2, 5}
    for m in special["co"]:
        genres[m] = set(int(g) for g in rs.choice(n_genres, 2, replace=False))
        c = int(rs.randint(1, 40))
        raw[m] = {co_tags[0]: c, co_tags[1]: c}
    tag_counts = {}
    for d in raw.values():
        for t, c in d.items():
            tag_counts[t] = tag_counts.get(t, 0) + c
    movie_tags = {m: {t: math.log(c) + 1 for t, c in d.items()} for m, d in raw.items()}
    no_med = set(mids[-40:])                             # genres / tags but no median
    keys = [m for m in mids if m not in no_med]
    keys = [keys[i] for i in rs.permutation(len(keys))]  # dict insertion order
    med = {m: float(rs.choice(HALF)) for m in keys}
    return mids, genres, movie_tags, tag_counts, med, special


def rating_lists(rs, med, special):
    pool = np.array(list(med))
    rate = lambda ms: [(int(m), float(rs.choice(HALF))) for m in ms]   # noqa: E731
    lists, names = [], []
    for rep in range(2):
        for n in SIZES:
            lists.append(rate(rs.choice(pool, n, replace=False)))
            names.append(f"len{n}_{rep}")
    lists.append(rate(special["none"][:5]))
    names.append("featureless")
    lists.append(rate(special["few"]))
    names.append("few_ids")
    lists.append(rate(special["equal"]))
    names.append("tie_by_id")
    base = list(rs.choice(pool, 15, replace=False))
    lists.append(rate(base + base[:3]))
    names.append("listed_twice")
    lists.append([(int(m), med[int(m)]) for m in rs.choice(pool, 12, replace=False)])
    names.append("b_zero")
    lists.append(rate(list(special["co"]) + list(rs.choice(pool, 12, replace=False))))
    names.append("cooccur")
    return lists, names


def variants(rs, A, b, itn_ref, x_ref):
    """Stop iterations and the fixed-iteration spread under row permutations."""
    n = A.shape[0]
    dense = A.toarray()
    itn_perm, spread = [], 0.0
    for i in range(N_VAR):
        pm = rs.permutation(n)
        Ap = A[pm] if i < N_VAR // 2 else dense[pm]
        bp = b[pm]
        itn_perm.append(_lsqr(Ap, bp, iter_lim=1000)[2])
        if itn_ref > 0:
            xv = _lsqr(Ap, bp, atol=0, btol=0, conlim=0, iter_lim=itn_ref)[0]
            spread = max(spread, C.rel_inf(xv, x_ref))
    return itn_perm, spread


def main():
    rs = np.random.RandomState(SEED)
    mids, genres, movie_tags, tag_counts, med, special = movie_data(rs)
    lists, names = rating_lists(rs, med, special)
    med_keys = np.array(list(med), np.int64)
    med_vals = np.array([med[m] for m in med], np.float64)
    d = dict(movie_genres=genres, movie_tags=movie_tags, tag_counts=tag_counts, med=med,
             med_keys=med_keys, med_vals=med_vals)
    B = len(lists)
    p = np.zeros(B, np.int32)
    profile = np.full((B, C.MAXF), -1, np.int32)
    x_ref = np.zeros((B, C.ROW))
    itn_ref = np.zeros(B, np.int32)
    istop_ref = np.zeros(B, np.int32)
    itn_perm = np.zeros((B, N_VAR), np.int32)
    s_u = np.zeros(B)
    scores = np.zeros((B, len(med)))
    traj, traj_off = [], [0]
    rec_off, rec_mid, rec_score = [0], [], []
    t_lists, agreement, n_agree, n_dis = [], [], [], []
    all_mids = np.array(mids)
    for u, lst in enumerate(lists):
        captured.clear()
        model = ref_models.TagLS_UserProfile(genres, lst, movie_tags, tag_counts, med)
        A, b, res = captured[0]
        p[u] = len(model.profile)
        profile[u, :p[u]] = model.profile
        x_ref[u] = C.x_row(res[0])
        istop_ref[u], itn_ref[u] = res[1], res[2]
        if itn_ref[u] > 0:      # the stops change no arithmetic: the same bits without them
            xf = _lsqr(A, b, atol=0, btol=0, conlim=0, iter_lim=int(itn_ref[u]))[0]
            assert np.array_equal(xf, res[0])
        itn_perm[u], s_u[u] = variants(rs, A, b, int(itn_ref[u]), res[0])
        J = 2 * max(int(itn_ref[u]), int(itn_perm[u].max())) if itn_ref[u] > 0 else 0
        for j in range(1, J + 1):
            traj.append(C.x_row(_lsqr(A, b, atol=0, btol=0, conlim=0, iter_lim=j)[0]))
        traj_off.append(len(traj))
        sc = np.array([model.predict(int(m)) for m in med_keys])
        scores[u] = sc
        rated = dict(lst)
        top = sorted(((float(s), int(m)) for s, m in zip(sc, med_keys) if int(m) not in rated),
                     reverse=True)[:TOP]
        rec_mid += [m for _, m in top]
        rec_score += [s for s, _ in top]
        rec_off.append(len(rec_mid))
        # held-out list: some movies without a median; no pair inside the rounding bound
        # (two movies with the same attributes and median tie in any implementation)
        attr = C.attr_matrix(model.profile, d)
        bound = dict(zip(med_keys.tolist(), C.score_bound(model.profile, res[0], d, attr).tolist()))
        same = {int(m): (attr[c].tobytes(), med[int(m)]) for c, m in enumerate(med_keys)}
        for _ in range(20):
            tl = [(int(m), float(rs.choice(HALF))) for m in rs.choice(all_mids, 25, replace=False)]
            kept = [(m, a) for m, a in tl if model.predict(m) is not None]
            pred = [(m, model.predict(m)) for m, _ in kept]
            safe = all(ai == aj or same[mi] == same[mj] or abs(pi - pj) > bound[mi] + bound[mj]
                       for (mi, ai), (_, pi) in zip(kept, pred)
                       for (mj, aj), (_, pj) in zip(kept, pred))
            if safe:
                break
        else:
            tl, kept, pred = [], [], []
        val = ref_util.compute_ranking_agreement(kept, pred) if len(pred) > 1 else None
        _, ag, dg = C.agreement_counts([a for _, a in kept], np.array([q for _, q in pred]))
        assert val is None or val == ag / (ag + dg)
        t_lists.append(tl)
        agreement.append(np.nan if val is None else val)
        n_agree.append(ag if val is not None else 0)
        n_dis.append(dg if val is not None else 0)
    stable = np.all(itn_perm == itn_ref[:, None], axis=1)

    # the restatement must meet the rules on this fixture
    fx = dict(d, itn_ref=itn_ref, istop_ref=istop_ref, stable=stable,
              traj=[np.array(traj[a:b]).reshape(-1, C.ROW)
                    for a, b in zip(traj_off[:-1], traj_off[1:])])
    errs, itn_cpu, istop_cpu = [], [], []
    for u, lst in enumerate(lists):
        m = C.CpuModel(lst, fx, atol=0, btol=0, conlim=0, iter_lim=int(itn_ref[u]))
        assert m.profile == profile[u, :p[u]].tolist(), names[u]
        errs.append(C.rel_inf(C.x_row(m.x), x_ref[u]))
        m = C.CpuModel(lst, fx)
        itn_cpu.append(m.itn)
        istop_cpu.append(m.istop)
    rep = {}
    C.check_fixed_iteration(errs, s_u, rep)
    C.check_stop(itn_cpu, istop_cpu, fx)
    miss = int(np.sum(stable & ((np.array(itn_cpu) != itn_ref) | (np.array(istop_cpu) != istop_ref))))
    print(f"lists {B}; stable {int(stable.sum())}; restatement misses {miss} stable stops; "
          f"max s_u {s_u.max():.3e}; restatement worst e_u / max(s_u, 2^-40) "
          f"{rep['worst_ratio']:.2f}, over their own bound {rep['over']}")

    def csr(dct, values):
        keys = list(dct)
        off = np.zeros(len(keys) + 1, np.int64)
        off[1:] = np.cumsum([len(dct[k]) for k in keys])
        return np.array(keys, np.int64), off, values(keys)

    mg_mid, mg_off, mg_gid = csr(genres, lambda ks: np.array(
        [g for k in ks for g in sorted(genres[k])], np.int32))
    mt_mid, mt_off, mt_tid = csr(movie_tags, lambda ks: np.array(
        [t for k in ks for t in movie_tags[k]], np.int64))
    mt_val = np.array([v for k in movie_tags for v in movie_tags[k].values()], np.float64)
    l_off = np.zeros(B + 1, np.int64)
    l_off[1:] = np.cumsum([len(l) for l in lists])
    t_off = np.zeros(B + 1, np.int64)
    t_off[1:] = np.cumsum([len(l) for l in t_lists])
    out = dict(
        mg_mid=mg_mid, mg_off=mg_off, mg_gid=mg_gid, mt_mid=mt_mid, mt_off=mt_off, mt_tid=mt_tid,
        mt_val=mt_val, tc_tid=np.array(list(tag_counts), np.int64),
        tc_cnt=np.array(list(tag_counts.values()), np.int64), med_keys=med_keys,
        med_vals=med_vals, l_off=l_off,
        l_mid=np.array([m for l in lists for m, _ in l], np.int64),
        l_r=np.array([r for l in lists for _, r in l], np.float64), l_name=np.array(names),
        p=p, profile=profile, x_ref=x_ref, itn_ref=itn_ref, istop_ref=istop_ref,
        traj_off=np.array(traj_off, np.int64) * C.ROW,
        traj_x=np.array(traj, np.float64).reshape(-1), itn_perm=itn_perm,
        stable=stable.astype(np.int8), s_u=s_u, scores=scores,
        rec_off=np.array(rec_off, np.int64), rec_mid=np.array(rec_mid, np.int64),
        rec_score=np.array(rec_score, np.float64), t_off=t_off,
        t_mid=np.array([m for l in t_lists for m, _ in l], np.int64),
        t_r=np.array([r for l in t_lists for _, r in l], np.float64),
        agreement=np.array(agreement), n_agree=np.array(n_agree, np.int64),
        n_disagree=np.array(n_dis, np.int64), seed=SEED, numpy=np.__version__)
    path = os.path.join(HERE, "content_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
