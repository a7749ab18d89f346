"""`python bench.py --gpus 2` end to end on the one-GPU box: no launcher, the two ranks share cuda:0 over gloo
(GNM_BENCH_SHARE_GPU=1, the bench's test hook) -- everything of the N > 1 path except RCCL itself: self-launch,
per-rank pools, hipGraph replay or eager, the flat-gradient all-reduce, max-over-ranks timing, one JSON line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_two_ranks_without_a_launcher():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["GNM_BENCH_SHARE_GPU"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--batch", "32", "--pool", "64",
                        "--steps", "4", "--warmup", "2", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["scaling"] == "weak"
    assert out["config"]["global_batch"] == 64 and out["config"]["graphs_per_gpu"] == 32
    assert out["value"] > 0 and out["ms_per_step"] < 200, out["ms_per_step"]     # round 1: 279-404 ms through gloo
    # the object the first real `bench.py --gpus 8` line will carry: who took part, what the
    # collective was, how the launch mode was chosen, and that the ranks agree where they must
    cc = out["collective"]
    assert cc["world"] == 2 and cc["backend"] == "gloo" and cc["forced_single_rank_test_hook"] is False
    assert cc["op"].startswith("gloo staging"), cc
    assert set(cc["launch_mode_trial_ms"]) >= {"graph", "eager"} and cc["launch_mode"] in cc["launch_mode_trial_ms"], cc
    rc = cc["rank_check"]
    assert rc["params_agree_after_broadcast"] is True and rc["grads_agree_after_allreduce"] is True, rc
    assert rc["grad_abs_sum"] > 0 and len(rc["final_loss_per_rank"]) == 2
    assert all(v == v and abs(v) < 1e6 for v in rc["final_loss_per_rank"])


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--neighbor-pooling", "max"], ["--config", "c4", "--batch", "8", "--pool", "8"],
                                   ["--graph", "off"], ["--no-learn-eps", "--graph-pooling", "average"]])
def test_bench_other_configurations_print_one_line(extra):
    """the non-default bench configurations (DESIGN.md section 6's matrix) keep working: one JSON line, a finite loss"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline"]
    if "--batch" not in extra:
        cmd += ["--batch", "16", "--pool", "16"]
    r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["value"] > 0
    assert out["final_loss"] == out["final_loss"] and abs(out["final_loss"]) < 1e6      # finite


@pytest.mark.gpu
def test_bench_rccl_path_at_world_size_one():
    """The part of the N > 1 path a one-GPU box CAN run on RCCL itself (two ranks may not share a GPU under RCCL):
    GNM_BENCH_FORCE_DIST=1 initialises the "nccl" process group at world size 1 and runs the multi-rank step path on
    it -- communicator init, the AVG all-reduce of the flat gradient buffer (gnm/parallel.py), its capture inside the
    step's hipGraph, the launch-mode trial.  Lines that had never executed before round 3."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["GNM_BENCH_FORCE_DIST"] = "1"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "32", "--pool", "64",
                        "--steps", "4", "--warmup", "2", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    cc = out["collective"]
    assert cc["backend"] == "nccl" and cc["forced_single_rank_test_hook"] is True
    assert cc["op"].startswith(("AVG", "SUM")), cc
    assert set(cc["launch_mode_trial_ms"]) >= {"graph", "eager"}, cc
    assert out["value"] > 0 and out["final_loss"] == out["final_loss"]
    print("collective:", json.dumps(cc))


@pytest.mark.gpu
def test_bench_dump_outputs_are_reproducible(tmp_path):
    """--dump-outputs DIR: the last timed step's loss, parameter gradients and BatchNorm statistics as float32 .npy
    files; the same arguments give bitwise the same files, and --steps decides which step that is"""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}

    def run(tag, steps):
        d = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "16", "--pool", "64",
                            "--steps", str(steps), "--warmup", "2", "--no-cpu-baseline", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == steps
        files = sorted(os.listdir(d))
        arrays = {f[:-4]: np.load(d / f) for f in files}
        assert sum(os.path.getsize(d / f) for f in files) <= 64 * 1000 * 1000
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
        assert float(arrays["loss"]) == np.float32(out["final_loss"])
        return arrays

    a, b, c = run("a", 3), run("b", 3), run("c", 4)
    assert sorted(a) == sorted(b) == sorted(c)
    grads = [k for k in a if k.startswith("grad.")]
    assert "grad.eps" in grads and "grad.mlps.0.linears.0.weight" in grads and len(grads) > 20, sorted(a)
    assert any(k.startswith("buffer.") and k.endswith("running_mean") for k in a), sorted(a)
    assert any(np.abs(a[k]).max() > 0 for k in grads)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not all(np.array_equal(a[k], c[k]) for k in grads), "--steps 4 dumped the same step as --steps 3"


@pytest.mark.gpu
def test_bench_full_adds_what_a_plain_run_leaves_out():
    """A plain run prints the headline without the figures that cost time or launches of their own; --full adds the
    CPU baseline (config C1: the first 32 graphs of the pool) and the CSR gather timing next to the matrix-core kernel"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}

    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "16", "--pool", "32",
                            "--steps", "3", "--warmup", "1"] + list(extra),
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        return json.loads(lines[0])

    plain, full = run(), run("--full")
    assert plain["cpu_baseline"] is None
    assert plain["roofline"]["mean_launch_ms"] > 0 and "csr_gather" not in plain["roofline"]
    c = full["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1
    assert full["roofline"]["csr_gather"]["median_launch_ms"] > 0
