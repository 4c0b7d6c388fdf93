"""bench.py --gpus N without a launcher around it (the form the driver uses): it must start its own
N ranks as fresh child processes before anything touches the GPU and relay ONE JSON line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(extra)
    return env


def test_self_launch_without_a_gpu_fails_in_the_ranks_not_in_the_launcher():
    """No GPU here: the two child ranks must be started (and refuse, loudly: no CPU fallback); the
    parent relays their failure instead of demanding an external torchrun."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--workload", "bb", "--cpu-pivots", "0"],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "needs an MI355X" in p.stderr
    assert "must be launched with" not in p.stderr
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_self_launch_two_ranks_rehearsal_on_one_gpu():
    """`python bench.py --gpus 2 --workload bb` un-wrapped, in the one-GPU rehearsal mode (both
    ranks share GPU 0, the library's collectives carried over gloo): one JSON line, two ranks."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--workload", "bb", "--bb-vars", "48",
                        "--bb-cons", "6", "--bb-levels", "5", "--cpu-pivots", "0"],
                       env=_env(LPR_BENCH_SHARED_GPU="1"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and "rehearsal" in out
    assert out["config"]["nodes_processed"] > 1 and out["value"] > 0


def _bench_line(*argv):
    p = subprocess.run([sys.executable, BENCH, *argv], env=_env(), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_steps_and_warmup_are_checked_before_any_work():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr


@pytest.mark.gpu
def test_dump_outputs_are_float_bounded_and_repeat_bit_for_bit(tmp_path):
    """Two runs with the same arguments dump the same arrays, byte for byte, in float64."""
    import numpy as np
    args = ["--m", "512", "--n", "1024", "--steps", "8", "--warmup", "2", "--cpu-pivots", "0"]
    dumps = []
    for run in ("a", "b"):
        out = _bench_line(*args, "--dump-outputs", str(tmp_path / run))
        assert out["steps"] == 8 and out["ms_per_step"] > 0
        dumps.append({f: np.load(tmp_path / run / f) for f in sorted(os.listdir(tmp_path / run))})
    a, b = dumps
    assert sorted(a) == sorted(b) and {"result.npy", "x.npy", "basis.npy", "pivot_log.npy"} <= set(a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), f
        assert a[f].tobytes() == b[f].tobytes(), f
    # probe pivot + warm-up + timed steps, all in the pivot log of the one LP replica
    assert a["pivot_log.npy"].shape[0] == a["result.npy"][3]


@pytest.mark.gpu
def test_steps_beyond_one_lp_replica_are_all_timed():
    """More steps than one headline LP holds before its optimum: the timed region goes on with a
    second replica, and the result line still reports exactly the steps asked for."""
    out = _bench_line("--steps", "5000", "--warmup", "2", "--cpu-pivots", "0")
    assert out["steps"] == 5000 and out["config"]["lp_replicas"] == 2
    assert out["ms_per_step"] > 0 and out["value"] > 0
