"""bench.py on one GPU: a plain run prints the headline figure and nothing it needs another run for, and --dump-outputs writes
what the timed path computed in its last step -- the same arrays on every run with the same arguments, and the operator's own
output for that step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(argv, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"bench.py {argv} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _last_step(name, n):
    """What the bench's operator returns in its last step: every step filters the same resident chunk, with the chunk's own
    tail as history from the second step on."""
    import torch

    import bench
    from qdsp_amd import ops

    op = bench.make_op(ops, name, 0)
    x = ops.synth_iq(n, seed=1234, device=0)
    op.process(x)
    y = op.process(x)
    torch.cuda.synchronize()
    op.close()
    return y


def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    n = 1 << 20
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--log2n", "20", "--spinup-ms", "20"]
    a = _run_bench(argv + ["--dump-outputs", str(tmp_path / "a")])
    b = _run_bench(argv + ["--dump-outputs", str(tmp_path / "b")])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in a, key
    assert a["steps"] == 3 and a["warmup"] == 1 and a["config"]["samples_per_gpu_per_step"] == n
    assert abs(a["value"] - n / (a["ms_per_step"] * 1e-3) / 1e6) < 0.01 * a["value"]
    assert not {"chain", "channelizer", "channelizer_m8", "block_call", "cpu_baseline"} & set(a)
    assert "kernel_ms_isolated" not in a["roofline"]
    assert os.listdir(tmp_path / "a") == ["fir256.npy"]
    ya, yb = np.load(tmp_path / "a" / "fir256.npy"), np.load(tmp_path / "b" / "fir256.npy")
    assert ya.dtype == np.float32 and ya.shape == (n, 2)          # 8 MiB: within its share, written whole
    assert np.array_equal(ya, yb)
    import torch

    want = torch.view_as_real(_last_step("fir256", n)).cpu().numpy()
    assert np.array_equal(ya, want)


def test_full_run_dumps_a_sample_of_every_leg(tmp_path):
    import bench

    n = 1 << 24
    line = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--log2n", "24", "--spinup-ms", "20", "--full",
                       "--no-cpu-baseline", "--no-block-call", "--dump-outputs", str(tmp_path)])
    assert {"chain", "channelizer", "channelizer_m8"} <= set(line) and "kernel_ms_isolated" in line["roofline"]
    names = ("fir256", "xlate_fir_decim8", "chan64", "chan64m8")
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in names)
    assert sum(os.path.getsize(tmp_path / f"{k}.npy") for k in names) <= 64 << 20
    share = bench.DUMP_BYTES // len(names)
    for k in names:
        y = np.load(tmp_path / f"{k}.npy")
        assert y.dtype == np.float32 and y.nbytes == share, (k, y.shape)   # every output here is larger than its share
    bench.dump_output(_last_step("fir256", n), str(tmp_path / "want.npy"), share)
    assert np.array_equal(np.load(tmp_path / "fir256.npy"), np.load(tmp_path / "want.npy"))
