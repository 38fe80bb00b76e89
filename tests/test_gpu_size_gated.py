"""Kernel instantiations that a size threshold selects at launch time, at the
smallest shapes that cross each threshold.

A. The pointer-gather Gram (``gram_kernel<4, ..., BUF = false>`` and
   ``gram_pair_kernel<..., BUF = false>``, ``launch_gram_nb``): taken when the
   opposite factor table holds 2 GiB or more -- C5's items Gram on every
   rank.  A shard context that owns 128 users and 96 items costs little more
   than its replicated U table, so an 8.5 M-row table (2.18 GB at k = 64,
   4.35 GB at k = 128) is crossed with ~7 k ratings: row byte offsets beyond
   2^31 and 2^32, the XCD-dealt work list (``build_work_xcd``), the fused CG
   start of those instantiations, the users whose x rows sit at the top of
   the table, and ``predict``.
B. Non-temporal G tile loads (``NT = true`` of ``cg_onepass_kernel`` /
   ``cg_resident_kernel``, by size above 320 MiB per iteration): forced with
   ``MR_OPT_CG_TILE_NT`` and held to the documented "results are identical
   in every mode", bit for bit.
C. More than one chunk per wave at NB <= 4 (the k <= 64 loop of the one-pass
   and the resident kernel): at least three chunks per wave on both sides,
   the two kernels bit-identical in every sweep mode and equal, to summation
   order, to the two-kernel iteration that runs one wave per entity.
"""
import numpy as np
import pytest

from conftest import rel_err
from test_gpu_parity import expected_layout
from test_gpu_scale import init_factor_rows

pytestmark = pytest.mark.gpu


def _reset_chunk():
    from movie_recommender_amd import _lib
    _lib.check(_lib.lib().mr_set_gram_chunk(2048), "reset chunk")


# ---------------------------------------------------------------------------
# A. Gram gathers from a table of 2 GiB or more
# ---------------------------------------------------------------------------
A_USERS = 8_500_000
A_ITEMS = 96
A_OWNED = 128
A_CHUNK = 64
# item list lengths: the 32-rating halves and the peeled last half (0, 1, 31
# ... 97), one item spread over the whole table, a few more heavy ones
A_EDGE_LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 96, 97]
A_HEAVY_LENGTHS = [3000, 640, 200, 130]


def _size_gated_ratings(k, seed):
    """The item view (every rating, ordered by (item, user id)), the user
    view (the owned users' ratings) and the ids around each 2^31 / 2^32 byte
    mark of the U table."""
    rng = np.random.default_rng(seed)
    U, I, own = A_USERS, A_ITEMS, A_OWNED
    u0 = U - own
    row_bytes = 4 * ((k + 15) // 16 * 16)
    marks = [m for m in (1 << 31, 1 << 32) if m < U * row_bytes]
    assert marks and all(m % row_bytes == 0 for m in marks)   # a row starts at each mark
    edge = np.array([0, U - 1] + [m // row_bytes + d for m in marks for d in (-1, 0, 1)],
                    np.int64)
    lens = A_EDGE_LENGTHS + A_HEAVY_LENGTHS
    lens = np.array(lens + list(rng.integers(2, 60, I - len(lens))), np.int64)
    lens = rng.permutation(lens)

    def pick(n):
        fixed = np.concatenate([rng.choice(edge, min(len(edge), n // 8), replace=False),
                                u0 + rng.choice(own, min(own, n // 3), replace=False)])
        ids = np.unique(fixed)
        while len(ids) < n:
            ids = np.unique(np.concatenate([ids, rng.integers(0, U, n - len(ids))]))
        return ids

    users = [pick(int(n)) for n in lens]
    iu = np.concatenate(users).astype(np.int32)
    ii = np.repeat(np.arange(I, dtype=np.int32), lens)
    ir = rng.normal(0, 1, len(iu)).astype(np.float32).astype(np.float64)
    sel = np.flatnonzero(iu >= u0)
    sel = sel[np.lexsort((ii[sel], iu[sel]))]
    return (iu, ii, ir), (iu[sel], ii[sel], ir[sel]), lens, edge, marks, row_bytes


def _pos_of(ref_users, u0, u1):
    """Positions of the users [u0, u1) in the sorted ``ref_users`` (all present)."""
    p = np.searchsorted(ref_users, np.arange(u0, u1))
    assert np.array_equal(ref_users[p], np.arange(u0, u1))
    return p


@pytest.mark.parametrize("k", [64, 128])
def test_gram_gathers_from_table_over_2gib(gpu, k):
    """An unattached shard context over an 8.5 M-user table (k = 64: 2.18 GB,
    row 8,388,608 starts at byte 2^31, ``gram_kernel<4, BUF = false>``; k =
    128: 4.35 GB, rows 4,194,304 and 8,388,608 start at bytes 2^31 and 2^32,
    ``gram_pair_kernel<BUF = false>``), factors seeded on the device:
      1. the items Gram against fp64 NumPy at 2e-5 (the project's Gram
         tolerance), the empty item exactly 0, and the XCD-dealt work list
         against its host restatement;
      2. every item that neither context splits bit-identical to an ordinary
         context over only the referenced users (``BUF = true``);
      3. the fused CG start of the items side: r0 = G x - c to 1e-13, p0 = -r0;
      4. the owned users (x rows at the top of the table): Gram and r0;
      5. ``predict`` for users on both sides of each byte mark."""
    from movie_recommender_amd.engine import AlsContext
    seed = 11
    U, I, own = A_USERS, A_ITEMS, A_OWNED
    u0 = U - own
    iv, uv, lens, edge, marks, row_bytes = _size_gated_ratings(k, seed)
    iu, ii, ir = iv
    table_bytes = (U + 1) * row_bytes
    path = "gram_kernel<4, BUF=false>" if k == 64 else "gram_pair_kernel<BUF=false>"
    print(f"k={k}: U table {table_bytes} bytes ({table_bytes / 2 ** 30:.2f} GiB), byte marks at "
          f"rows {[m // row_bytes for m in marks]}, {len(ir)} ratings, items Gram by {path}",
          flush=True)
    assert table_bytes >= 1 << 31
    assert 6000 <= len(ir) <= 8000
    # conditions on the inputs (CPU)
    heavy = int(np.argmax(lens))
    hu = iu[ii == heavy].astype(np.int64)
    assert np.all(np.bincount(hu * 8 // U, minlength=8) > 0)
    assert np.all(np.isin(edge, hu)) and np.all(np.isin(np.arange(u0, U), hu))
    assert set(A_EDGE_LENGTHS) <= set(lens.tolist())
    unsplit = np.flatnonzero((lens <= A_CHUNK) & (lens <= 2048))
    assert len(unsplit) >= 80 and np.count_nonzero(lens > A_CHUNK) >= 4
    # the referenced users' rows and the item table from the hash
    ref_users = np.unique(iu)
    Uh = init_factor_rows(seed, 0, ref_users, k)              # [n, k + 1]
    Vh = init_factor_rows(seed, 1, np.arange(I), k)           # [I, k]
    pos = np.searchsorted(ref_users, iu)
    off = np.concatenate([[0], np.cumsum(lens)])
    try:
        with AlsContext(uv[0], uv[1], uv[2], k, U, I, user_range=(u0, U), item_range=(0, I),
                        item_view=iv, gram_chunk=A_CHUNK) as ctx:
            assert ctx.local_size("users") == (u0, own, len(uv[2]))
            assert ctx.local_size("items") == (0, I, len(ir))
            ctx.init_factors(seed)
            # heavy items go through build_work_xcd (table > 16 MiB)
            _, idx, _, (wb, wl, we, ws) = ctx.layout("items")
            _, eidx, _, work = expected_layout(ii, iu, ir, I, chunk=A_CHUNK,
                                               xcd_table_bytes=U * row_bytes, k=k, n_other=U)
            w = np.array(work, np.int64)
            assert np.array_equal(idx, eidx)
            assert np.array_equal(wb, w[:, 0]) and np.array_equal(wl, w[:, 1])
            assert np.array_equal(we, w[:, 2]) and np.array_equal(ws, w[:, 3])
            assert np.count_nonzero(ws >= 0) > 8          # chunks of split items, dealt by XCD
            # 1. items Gram against fp64 NumPy
            ctx.build_normal_equations("items")
            G, c = ctx.normal_equations("items", np.arange(I))
            worst = [0.0, 0.0]
            for e in range(I):
                rows = Uh[pos[off[e]:off[e + 1]]]
                a = rows[:, :k]
                wgt = ir[off[e]:off[e + 1]] - rows[:, k]
                Gr, cr = a.T @ a, a.T @ wgt
                if lens[e] == 0:
                    assert np.all(G[e] == 0) and np.all(c[e] == 0)
                    continue
                eg = np.max(np.abs(G[e] - Gr)) / np.max(np.abs(Gr))
                ec = np.max(np.abs(c[e] - cr)) / max(np.max(np.abs(cr)), 1.0)
                worst = [max(worst[0], eg), max(worst[1], ec)]
                assert eg < 2e-5 and ec < 2e-5, (e, int(lens[e]), eg, ec)
            print(f"k={k}: items Gram worst error G {worst[0]:.2e}, c {worst[1]:.2e}", flush=True)
            # 2. bitwise against BUF = true on the referenced users only
            with AlsContext(pos.astype(np.int32), ii, ir, k, len(ref_users), I) as small:
                assert (len(ref_users) + 1) * row_bytes < 1 << 31
                small.set_factors(Uh, Vh)
                small.build_normal_equations("items")
                Gs, cs = small.normal_equations("items", np.arange(I))
            for e in unsplit:
                assert np.array_equal(G[e], Gs[e]) and np.array_equal(c[e], cs[e]), \
                    (int(e), int(lens[e]))
            # 4a. users Gram (gathers the small V table; local ids)
            ctx.build_normal_equations("users")
            Gu, cu = ctx.normal_equations("users", np.arange(own))
            lu = (uv[0] - u0).astype(np.int64)
            for e in range(own):
                s = np.flatnonzero(lu == e)
                a = np.hstack([Vh[uv[1][s]], np.ones((len(s), 1))])
                Gr, cr = a.T @ a, a.T @ uv[2][s]
                assert np.max(np.abs(Gu[e] - Gr)) / max(np.max(np.abs(Gr)), 1e-30) < 2e-5, e
                assert np.max(np.abs(cu[e] - cr)) / max(np.max(np.abs(cr)), 1.0) < 2e-5, e
            # 5. predict on both sides of each byte mark
            rng = np.random.default_rng(seed + 1)
            near = np.concatenate([m // row_bytes + rng.integers(-1000, 1000, 24) for m in marks])
            pu = np.concatenate([edge, near, rng.integers(0, U, 200 - len(edge) - len(near))])
            pi = rng.integers(0, I, len(pu))
            for m in marks:
                assert np.any(pu < m // row_bytes) and np.any(pu >= m // row_bytes)
            Up = init_factor_rows(seed, 0, pu, k)
            want = np.einsum("nj,nj->n", Up[:, :k], Vh[pi]) + Up[:, k]
            got = ctx.predict(pu, pi)
            print(f"k={k}: predict error {rel_err(got, want):.2e}", flush=True)
            assert rel_err(got, want) <= 1e-12
            # 3. / 4b. the fused CG start (max_iteration 0): r0 = G x - c, p0 = -r0
            for side, Gm, cm, x0 in (("items", G, c, Vh),
                                     ("users", Gu, cu, Uh[_pos_of(ref_users, u0, U)])):
                its, rr = ctx.half_step(side, 0.01, 0)
                rv, pv, _ = ctx.cg_vectors(side)
                r0 = np.einsum("eij,ej->ei", Gm, x0).ravel() - cm.ravel()
                sc = np.max(np.abs(r0))
                print(f"k={k} {side}: start rr {rr:.6e}, r0 error {np.max(np.abs(rv - r0)) / sc:.2e}",
                      flush=True)
                assert np.max(np.abs(rv - r0)) <= 1e-13 * sc, (side, np.max(np.abs(rv - r0)) / sc)
                assert np.array_equal(pv, -rv), side
    finally:
        _reset_chunk()


# ---------------------------------------------------------------------------
# B. Non-temporal tile loads are bitwise neutral
# ---------------------------------------------------------------------------
# (k, scale) as the ML-full shape shrinks; the last two are large enough that
# NB > 4 (one entity per chunk, 2 blocks per CU) has more chunks than waves on
# both sides (at scale 0.05 only the k = 96 users side has: 2,141 users)
@pytest.mark.parametrize("k,scale,many", [(32, 0.02, False), (64, 0.02, False),
                                          (96, 0.05, False), (128, 0.05, False),
                                          (96, 0.1, True), (128, 0.2, True)])
def test_nontemporal_tile_loads_are_bitwise_neutral(gpu, k, scale, many):
    """MR_OPT_CG_TILE_NT 0 against 1 (the ``NT = true`` instantiations of the
    one-pass and the resident kernel, otherwise chosen above 320 MiB of
    per-iteration stream): the policy only changes the cache hint of the G
    tile loads, so factors, CG counts and every half-step's (count, rr) are
    bit-identical -- launch-per-iteration and resident, NB = 2 ... 8."""
    from movie_recommender_amd import synth
    from movie_recommender_amd.engine import AlsContext
    rs = synth.movielens_like("ml-full", k, scale=scale)
    rng = np.random.RandomState(7)
    U0 = rng.uniform(-1, 1, rs.num_users * (k + 1))
    V0 = rng.uniform(-1, 1, rs.num_items * k)
    with AlsContext(rs.user_ids, rs.item_ids, rs.ratings, k, rs.num_users,
                    rs.num_items) as ctx:
        ctx.set_timing(True)
        for side, E in (("users", rs.num_users), ("items", rs.num_items)):
            for resident in (False, True):
                g = ctx.cg_grid(side, resident=resident, nt=True)
                assert g > 0, (side, resident)
                if many:
                    assert E > 4 * g, (side, E, g)     # NB > 4: one entity per chunk
        for resident in (0, 1):
            ctx.set_option("cg_resident", resident)
            outs = []
            for nt in (0, 1):
                ctx.set_option("cg_tile_nt", nt)
                ctx.set_factors(U0, V0)
                ctx.reset_stats()
                ctx.iterate(2)
                trace = [ctx.half_step(side, 0.01, m) for side, m in
                         (("users", 0), ("items", 1), ("users", 3), ("items", 200))]
                st = ctx.stats()
                kl = st["kernel_launches"]
                outs.append((ctx.get_factors(), st["cg_users_total"], st["cg_items_total"], trace,
                             kl["resident_users"], kl["resident_items"]))
            (Ua, Va), cua, cia, tra, rua, ria = outs[0]
            (Ub, Vb), cub, cib, trb, rub, rib = outs[1]
            print(f"k={k} resident={resident}: {rs.num_users} users, {rs.num_items} items, CG "
                  f"{cua}/{cia}, resident launches {rub}/{rib}", flush=True)
            if resident:
                assert min(rua, ria, rub, rib) > 0, (rua, ria, rub, rib)
            else:
                assert rua == ria == rub == rib == 0
            assert (cua, cia) == (cub, cib) and cua + cia > 4, (cua, cia, cub, cib)
            assert tra == trb, (tra, trb)
            assert np.array_equal(Ua, Ub) and np.array_equal(Va, Vb)


# ---------------------------------------------------------------------------
# C. Several chunks per wave at NB <= 4
# ---------------------------------------------------------------------------
# ML-full shape at 3/4 of its size (users with >= 65 ratings, items with >=
# 64: a well-posed set at k = 32 and k = 64): 75 k users, 38 k items -- three
# chunks per wave need 61,440 users / 36,864 items at k = 32 (one-pass grids
# of 1,280 / 1,536 blocks on a 256-CU chip) and 49,152 / 24,576 at k = 64
C_SCALE = 0.75


@pytest.fixture(scope="module")
def ml_three_quarters():
    from movie_recommender_amd import synth
    return synth.movielens_like("ml-full", 64, scale=C_SCALE)


@pytest.mark.parametrize("k", [32, 64])
def test_several_chunks_per_wave(gpu, ml_three_quarters, k):
    """The chunk loop of ``cg_onepass_kernel`` / ``cg_resident_kernel`` at
    NB <= 4 with at least three chunks per wave on both sides (asserted from
    the context's own grids).  From one fp32 start, ``half_step(side, 0.01,
    m)`` for m = 1, 2, 4: the resident solve and the launch-per-iteration one
    pass are bit-identical to each other and across the three sweep modes;
    against the two-kernel iteration (``cg_onepass`` 0: one wave per entity,
    no chunk loop, itself pinned to the fp64 oracle within 1e-10 / 1e-9 step
    + 2 ulp by test_cg_iterations_vs_oracle, hence twice that here): equal CG
    counts, rr within 2e-10, x within 2e-9 step + 4 ulp."""
    from movie_recommender_amd.engine import AlsContext
    rs = ml_three_quarters
    nU, nI = rs.num_users, rs.num_items
    rng = np.random.RandomState(5)
    U0 = rng.uniform(-1, 1, nU * (k + 1)).astype(np.float32).astype(np.float64)
    V0 = rng.uniform(-1, 1, nI * k).astype(np.float32).astype(np.float64)
    with AlsContext(rs.user_ids, rs.item_ids, rs.ratings, k, nU, nI) as ctx:
        for side, E, xc in (("users", nU, 4), ("items", nI, 2)):     # xchunk_of, NB <= 4
            for resident in (False, True):
                for nt in (False, True):
                    g = ctx.cg_grid(side, resident=resident, nt=nt)
                    chunks = -(-E // xc)
                    print(f"k={k} {side} resident={resident} nt={nt}: {chunks} chunks, "
                          f"{4 * g} waves", flush=True)
                    assert g > 0 and chunks >= 3 * 4 * g, (side, resident, nt, E, g)

        def run(side, m, onepass, resident, sweep):
            ctx.set_option("cg_onepass", onepass)
            ctx.set_option("cg_resident", resident)
            ctx.set_option("cg_sweep", sweep)
            ctx.set_factors(U0, V0)
            its, rr = ctx.half_step(side, 0.01, m)
            Ux, Vx = ctx.get_factors()
            return its, rr, (Ux if side == "users" else Vx)

        for side, x0 in (("users", U0), ("items", V0)):
            for m in (1, 2, 4):
                it2, rr2, x2 = run(side, m, 0, 0, 1)
                first = None
                for sweep in (0, 1, 2):
                    for resident in (1, 0):
                        got = run(side, m, 1, resident, sweep)
                        if first is None:
                            first = got
                            continue
                        assert got[:2] == first[:2], (side, m, sweep, resident, got[:2], first[:2])
                        assert np.array_equal(got[2], first[2]), (side, m, sweep, resident)
                it1, rr1, x1 = first
                step = np.max(np.abs(x2 - x0))
                dx = np.max(np.abs(x1 - x2))
                print(f"k={k} {side} m={m}: CG {it1} / {it2}, rr {rr1:.12e} / {rr2:.12e}, "
                      f"|dx| {dx:.3e}, step {step:.3e}", flush=True)
                assert it1 == it2, (side, m, it1, it2)
                assert abs(rr1 - rr2) <= 2e-10 * abs(rr2), (side, m, rr1, rr2)
                assert dx <= 2e-9 * step + 4 * np.spacing(np.float32(1)), (side, m, dx, step)
