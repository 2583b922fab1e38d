"""The library's dispatch against the recorded map (tests/golden/dispatch_map.txt, written by scripts/dispatch_map.py): every row of
the map's default settings, every rung of up to 2^20 samples, one call on a fresh handle, and the kernel family behind it must be the
map's.  tests/test_sanitizers_cpu.py recomputes the whole map with the host-only selector (qdsp_amd/csrc/select.cpp) on a box without a
GPU; this test ties that selector to what the library launches.  No numerics here: they stay with the other suites."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import dispatch_map as DM  # noqa: E402

MAX_COUNT = 1 << 20
ROWS = [DM.parse_row(ln.strip()) for ln in open(os.path.join(ROOT, "tests", "golden", "dispatch_map.txt")) if ln.strip() and not ln.startswith("#")]
CLASSES = sorted({r[1] for r in ROWS if r[0] == "default"})


@pytest.fixture(scope="module")
def noise():
    import torch

    gen = torch.Generator(device="cuda").manual_seed(99)
    x = torch.randn(2 * MAX_COUNT, dtype=torch.float32, device="cuda", generator=gen) * 0.25
    out = torch.empty(2 * (10 * MAX_COUNT + 16), dtype=torch.float32, device="cuda")      # (the largest ratio of the map is 6)
    return x, torch.view_as_complex(x.view(-1, 2)), out, torch.view_as_complex(out.view(-1, 2))


def test_map_holds_the_grid():
    """The fixture is the map of the whole grid (scripts/dispatch_map.py rows(), default and parity settings) and names its revision."""
    first = open(os.path.join(ROOT, "tests", "golden", "dispatch_map.txt")).readline()
    assert first.startswith("# dispatch map of ") and len(first.split()[4].rstrip(":")) == 40, first
    grid = [(c, l, m, t, mode) for c, l, m, t, mode in DM.rows()]
    for settings in ("default", "parity"):
        assert [r[1:6] for r in ROWS if r[0] == settings] == grid, settings
    assert all(len(r[6]) == len(DM.ladder_of(r[2], r[3])) for r in ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_library_launches_what_the_map_names(cls, noise):
    import torch

    from conftest import kname
    from qdsp_amd import ops

    for k in list(DM.PARITY) + ["QDSP_HIP_FIR_MODE", "QDSP_HIP_FIR_PICK", "QDSP_HIP_NO_FIR_TABLE", "QDSP_HIP_NO_DECIM_TABLE"]:
        assert k not in os.environ, f"{k} overrides the default dispatch"
    x, xc, out, outc = noise
    real = cls.endswith("_r")
    wrong, calls = [], 0
    for settings, c, interp, decim, taps, mode, rungs in ROWS:
        if settings != "default" or c != cls:
            continue
        for count, family in rungs:
            if count > MAX_COUNT:
                continue
            op = DM.make_op(ops, cls, interp, decim, taps, mode)      # a fresh handle per call
            op.process(x[:count] if real else xc[:count], out if real else outc)
            got = kname(op)
            op.close()
            calls += 1
            if got != family:
                wrong.append((interp, decim, taps, mode, count, family, got))
    torch.cuda.synchronize()
    assert calls > 0 and not wrong, f"{len(wrong)} of {calls} calls, first: {wrong[:5]}"
