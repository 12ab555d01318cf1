"""`python bench.py --gpus N` starts its own rank processes when it is not already under torch.distributed.run.
The launcher (bench.launch_ranks: fresh child processes, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 /
MASTER_PORT, rank 0 relays the JSON line) is driven here on the CPU: the children run the gloo self-test instead of
the GPU benchmark, everything before that point is the production path."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [2, 3])
def test_bench_spawns_its_ranks_and_relays_rank0(n):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--launcher-selftest"],
                       env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                 # ONE line, from rank 0
    out = json.loads(lines[0])
    assert out["world"] == n and out["selftest"] == n * (n + 1) / 2 and out["backend"] == "gloo"


def test_single_process_path_is_not_spawned():
    import bench
    assert callable(bench.launch_ranks) and callable(bench.launcher_selftest)


def test_profile_json_belongs_to_the_full_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--profile-json", "unused.json"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--full" in r.stderr
    h = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout


FULL_ONLY = ("roofline", "attention", "kernels", "other_precisions", "other_configs", "gather", "cpu_baseline", "cpu_baseline_c1")


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_plain_run_times_k_steps_and_dumps_the_same_outputs_every_run(tmp_path):
    """A plain run prints the headline alone for exactly --steps timed steps; --dump-outputs holds the same parameters and Adam
    moments whatever the conditioning did (15 ms of untimed steps in one run, none in the other)."""
    import numpy as np
    dirs = []
    for i, cond in enumerate(("15", "0")):
        d = tmp_path / ("run%d" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3",
                            "--condition-ms", cond, "--dump-outputs", str(d)], capture_output=True, text=True, timeout=380)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert out["steps"] == 12 and out["warmup"] == 3 and out["ms_per_step"] > 0
        assert out["value"] == pytest.approx(128 * 1e3 / out["ms_per_step"], rel=1e-3)
        assert out["unit"] == "sequences/s" and out["higher_is_better"] is True and out["dtype"]
        assert not [k for k in FULL_ONLY if k in out]
        dirs.append(d)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"loss.npy", "auc.npy", "param.item_emb.npy", "adam_m.item_emb.npy", "adam_v.item_emb.npy"} <= set(names)
    assert sum(os.path.getsize(dirs[0] / n) for n in names) <= 64_000_000 + 256 * len(names)
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), n
        if n in ("loss.npy", "auc.npy"):
            np.testing.assert_allclose(a, b, rtol=1e-5, err_msg=n)      # (float-atomic sums over the batch)
        else:
            assert np.array_equal(a, b), n
    assert np.abs(np.load(dirs[0] / "adam_m.item_emb.npy")).max() > 0       # the steps moved the state
