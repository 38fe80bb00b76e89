"""bench.py's multi-rank launch (VERDICT r03 "do this" 1): ``--gpus N``
without a launcher starts N ranks under torch.distributed.run as a child
process and relays their one JSON line; a rank count that differs from
``--gpus`` is refused.  On the one-GPU box the ranks share GPU 0 through the
test-only ``--device-map 0,0 --comm gloo``; the one-pass CG's exact sums make
the sharded run take the single-GPU trajectory, so the CG counts must be
equal (DESIGN.md "Order-independent CG sums")."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--shape", "ml-full", "--scale", "0.125", "--k", "64", "--steps", "3", "--warmup", "2",
         "--full", "--no-cpu"]


def run_bench(args, timeout=600, env=None):
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT, env=dict(os.environ, **(env or {})))
    return r


def test_world_size_mismatch_is_refused():
    """A launcher world that differs from --gpus is an error, never a
    silently mislabelled line (CPU: refused before anything loads)."""
    r = run_bench(["--gpus", "1"], timeout=120, env={"WORLD_SIZE": "2"})
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout)
    assert "refusing" in r.stderr
    r = run_bench(["--gpus", "4"], timeout=120, env={"WORLD_SIZE": "2", "RANK": "0",
                                                       "LOCAL_RANK": "0"})
    assert r.returncode == 2 and r.stdout == ""


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """--dump-outputs writes float32 tables; beyond the byte budget a fixed,
    seeded sample of rows, the same from call to call (CPU: a stand-in
    context)."""
    import numpy as np
    import bench

    class Ctx:
        num_users, num_items, k = 700, 300, 7

        def get_factors(self):
            rng = np.random.RandomState(3)
            return rng.uniform(-1, 1, 700 * 8), rng.uniform(-1, 1, 300 * 7)

    bench.dump_outputs(str(tmp_path / "a"), Ctx())
    U, V = np.load(tmp_path / "a" / "U.npy"), np.load(tmp_path / "a" / "V.npy")
    Uf, Vf = Ctx().get_factors()
    assert U.dtype == V.dtype == np.float32 and U.shape == (700, 8) and V.shape == (300, 7)
    assert np.array_equal(U, Uf.reshape(700, 8).astype(np.float32))
    assert np.array_equal(V, Vf.reshape(300, 7).astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_BUDGET", 10_000)
    bench.dump_outputs(str(tmp_path / "b"), Ctx())
    bench.dump_outputs(str(tmp_path / "c"), Ctx())
    Ub, Vb = np.load(tmp_path / "b" / "U.npy"), np.load(tmp_path / "b" / "V.npy")
    assert Ub.nbytes + Vb.nbytes <= 10_000 and 0 < Ub.shape[0] < 700 and 0 < Vb.shape[0] < 300
    assert np.array_equal(Ub, np.load(tmp_path / "c" / "U.npy"))
    assert np.array_equal(Vb, np.load(tmp_path / "c" / "V.npy"))
    rows = {r.tobytes() for r in U}
    assert all(r.tobytes() in rows for r in Ub)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(gpu, tmp_path):
    """Without --full the line carries the headline fields only, --steps sets
    the timed steps, and --dump-outputs leaves the last step's factors."""
    import numpy as np
    plain = [a for a in SMALL if a not in ("--full", "--no-cpu")]
    r = run_bench(["--gpus", "1", "--dump-outputs", str(tmp_path)] + plain)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    a = json.loads(lines[0])
    assert a["steps"] == 3 and a["warmup"] == 2 and a["unit"] == "ratings/s"
    assert a["higher_is_better"] is True and a["dtype"] == "f32+f64"
    assert a["ms_per_step"] > 0
    assert a["value"] == pytest.approx(a["config"]["n_ratings"] / (a["ms_per_step"] / 1e3),
                                       rel=1e-3)
    for key in ("roofline", "kernels", "cpu_baseline", "same_window", "trajectory"):
        assert key not in a
    U, V = np.load(tmp_path / "U.npy"), np.load(tmp_path / "V.npy")
    k = a["config"]["k"]
    assert U.dtype == V.dtype == np.float32
    assert U.shape == (a["config"]["users"], k + 1) and V.shape == (a["config"]["items"], k)
    assert np.isfinite(U).all() and np.isfinite(V).all() and np.abs(V).max() > 0


@pytest.mark.gpu
def test_bench_gpus2_matches_gpus1(gpu):
    one = run_bench(["--gpus", "1"] + SMALL)
    assert one.returncode == 0, one.stderr[-3000:]
    two = run_bench(["--gpus", "2", "--comm", "gloo", "--device-map", "0,0"] + SMALL)
    assert two.returncode == 0, two.stderr[-3000:]
    lines1 = [ln for ln in one.stdout.splitlines() if ln.strip()]
    lines2 = [ln for ln in two.stdout.splitlines() if ln.strip()]
    assert len(lines1) == 1 and len(lines2) == 1, (one.stdout, two.stdout)
    a, b = json.loads(lines1[0]), json.loads(lines2[0])
    assert a["n_gpus"] == 1 and b["n_gpus"] == 2
    assert b["config"]["parallelism"] == "shard2"
    assert b["config"]["cg_scalars"].startswith("peer")
    sh = b["config"]["shards"]
    assert len(sh) == 2
    assert sh[0]["users"][0] == 0 and sh[0]["users"][1] == sh[1]["users"][0]
    assert sh[1]["users"][1] == a["config"]["users"] and sh[1]["items"][1] == a["config"]["items"]
    assert sh[0]["user_ratings"] + sh[1]["user_ratings"] == a["config"]["n_ratings"]
    assert sh[0]["item_ratings"] + sh[1]["item_ratings"] == a["config"]["n_ratings"]
    assert min(s["user_ratings"] for s in sh) > 0.3 * a["config"]["n_ratings"]
    # N-invariance at bench level: the same CG iterations in the window and
    # in every iteration of the trajectory
    assert a["cg_iterations"] == b["cg_iterations"], (a["cg_iterations"], b["cg_iterations"])
    assert a["trajectory"]["cg_per_iteration"] == b["trajectory"]["cg_per_iteration"]
    assert a["trajectory"]["matches_timed_region"] and b["trajectory"]["matches_timed_region"]
    assert a["same_window"]["cg_users"] == b["same_window"]["cg_users"]
    assert a["same_window"]["trajectory_cg_matches"]
    # the sharded line decomposes its step (VERDICT r05 "do this" 3)
    dc = b["decomposition"]
    assert dc["exchange_ms_per_step"] > 0 and dc["peer_wait_ms_per_step"] > 0
    assert dc["peer_reductions_per_step"] >= 2     # >= one per half-step's solve
    assert len(dc["compute_ms_per_step_by_rank"]) == 2
    assert min(dc["compute_ms_per_step_by_rank"]) > 0
    assert dc["step_ms_max"] >= dc["step_ms_min"] > 0
    assert abs(dc["step_ms_max"] - b["ms_per_step"]) <= 1e-3 * b["ms_per_step"] + 1e-3
    m = dc["model"]
    assert dc["model_step_ms"] == pytest.approx(m["compute_ms"] + m["exchange_ms"]
                                                + m["peer_reductions_ms"], abs=1e-3)
    assert "decomposition" not in a


@pytest.mark.gpu
def test_bench_forced_shard_world1_resident_peer(gpu):
    """One rank through the whole sharded path on its own GPU: RCCL
    communicator, the peer all-reduce (mapped onto its own buffer) and the
    resident CG solve together -- the combination an N-GPU run uses, which the
    shared-GPU layouts above cannot run (they switch the resident solve off).
    Same trajectory as the unsharded run, a decomposed line, and the peer
    reductions counted."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1",
           "MASTER_PORT": str(port)}
    one = run_bench(["--gpus", "1"] + SMALL)
    assert one.returncode == 0, one.stderr[-3000:]
    sh = run_bench(["--gpus", "1", "--force-shard"] + SMALL, env=env)
    assert sh.returncode == 0, sh.stderr[-3000:]
    a = json.loads([ln for ln in one.stdout.splitlines() if ln.strip()][0])
    b = json.loads([ln for ln in sh.stdout.splitlines() if ln.strip()][0])
    assert b["config"]["parallelism"] == "shard1"
    assert b["config"]["cg_scalars"].startswith("peer"), b["config"]["cg_scalars"]
    assert "resident_users" in b["kernels"] and "resident_items" in b["kernels"]
    assert a["cg_iterations"] == b["cg_iterations"]
    assert a["trajectory"]["cg_per_iteration"] == b["trajectory"]["cg_per_iteration"]
    dc = b["decomposition"]
    assert dc["peer_reductions_per_step"] >= 2 and dc["peer_wait_ms_per_step"] > 0
