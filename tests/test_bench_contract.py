"""bench.py contract: runs on CPU with a tiny config and prints one valid
JSON line with the driver-required keys."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--model", "mltc-tiny",
         "--batch", "2", "--seq", "32", "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in d, key
    assert d["metric"] == "train_tokens_per_s"
    assert d["value"] > 0
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["config"]["parallelism"] == "dp1"


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's arrays as float .npy,
    identically from run to run (seeded weights, batch and sample); --steps
    sets the timed step count; --full is accepted."""
    import numpy as np

    def run(out, steps, *extra):
        r = subprocess.run(
            [sys.executable, os.path.join(REPO, "bench.py"), "--model",
             "mltc-tiny", "--batch", "2", "--seq", "32", "--steps", str(steps),
             "--warmup", "1", "--dump-outputs", str(out), *extra],
            capture_output=True, text=True, timeout=600, cwd=REPO)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["steps"] == steps and d["ms_per_step"] > 0
        return {f[:-4]: np.load(os.path.join(out, f))
                for f in sorted(os.listdir(out))}

    a = run(tmp_path / "a", 2)
    b = run(tmp_path / "b", 2, "--full")
    c = run(tmp_path / "c", 3)
    assert sorted(a) == ["grads", "loss", "master", "params"]
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.isfinite(a[name]).all(), name
        assert np.array_equal(a[name], b[name]), name
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["grads"].any()
    # one more timed step moves the weights: --steps is really honoured
    assert not np.array_equal(a["master"], c["master"])


def test_bench_torchrun_world2_cpu():
    """Rehearse the driver's multi-GPU launch on CPU (gloo, ws=2)."""
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29612", os.path.join(REPO, "bench.py"),
         "--model", "mltc-tiny", "--batch", "2", "--seq", "32",
         "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 4
    assert d["n_gpus"] == 2 or d["n_gpus"] == 1  # CPU fallback reports --gpus
