"""The 4096-point overlap-save kernels (qdsp_amd/csrc/fft_fir.hip) read their per-lane tables -- the filter spectrum Hf and the pass-A
twiddles TA -- entry-major ([16][256]: a wave reads 512 contiguous bytes per entry); QDSP_HIP_FFT_TBL=0 keeps the lane-major layout
([256][16]) for comparison.  The two layouts hold the same values and every kernel uses them in the same order, and the two LDS-DMA
kernels deal their segments out as a tapered grid (long workgroups, then short ones): none of this may change one bit of any output.

Checked here: every consumer of the tables (FIR<complex_t> in its three forms, the pruned decimators per segment and grouped, the
fused VFO, real data) gives bit-identical results under both layouts, the default layout stays inside the project's overlap-save
tolerance against the FP64 oracle, and the persistent segment loop of the LDS-DMA kernel (first segment guarded, later ones
prefetched, ragged tail, uneven split over the workgroups) equals the plain kernel bit for bit."""
import numpy as np
import pytest

import oracle as O
from conftest import kname, rel_rms
from test_gpu_parity import TOL_FFT, dev, run_blocks

pytestmark = pytest.mark.gpu

N = 90_000
SIZES = [40_001, 4096, 3, 20_000, 25_900]   # (test_fft_fir_dma_forms_agree's sequence: first, interior-DMA and last segments)
GROUPED_LDS = (2 * 4352 + 16 * 17) * 8      # fir_fft_dec_kernel: exchange buffer + staging + pass-B twiddles


@pytest.fixture(scope="module")
def ops():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from qdsp_amd import ops as _ops

    assert "gfx950" in _ops.device_info(0)["arch"]
    return _ops


@pytest.fixture(autouse=True)
def _pin_the_4096_point_kernels(monkeypatch):
    """Oracle-sized calls go to the one-wave 1024-point form, the polyphase decimators or a measured exception by default: this module is
    about the 4096-point kernels, so it pins them the way tests/conftest.py does for test_gpu_parity."""
    monkeypatch.setenv("QDSP_HIP_FFT1K_MAX_COUNT", "0")
    monkeypatch.setenv("QDSP_HIP_DECIM_SETTING", "0")
    monkeypatch.setenv("QDSP_HIP_NO_PFB", "1")


@pytest.fixture(scope="module")
def x90k():
    return O.synth_iq(0, N, seed=5)


def random_taps(ntaps):
    rng = np.random.default_rng(7 + ntaps)
    return (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)


@pytest.mark.parametrize("ntaps", [2, 256, 2049])
def test_layouts_agree_in_every_fir_form(ops, monkeypatch, x90k, ntaps):
    taps = random_taps(ntaps)
    out = {}
    for dma, name in (("0", "fir_fft_kernel"), ("1", "fir_fft_dma_kernel"), ("2", "fir_fft_dmapk_kernel")):
        for tbl in ("0", "1"):
            monkeypatch.setenv("QDSP_HIP_FFT_DMA", dma)
            monkeypatch.setenv("QDSP_HIP_FFT_TBL", tbl)
            f = ops.Fir(taps)
            f.set_mode(f.FFT)
            out[dma, tbl] = run_blocks(f, x90k, SIZES)
            assert f.last_kernel()["name"] == name
    for dma in ("0", "1", "2"):
        assert np.array_equal(out[dma, "0"], out[dma, "1"]), f"QDSP_HIP_FFT_DMA={dma}: the two table layouts differ"
    assert np.array_equal(out["0", "1"], out["1", "1"])
    w64 = O.Fir(taps, acc=O.ACC_F64).process(x90k)
    for dma in ("0", "1", "2"):
        err = rel_rms(out[dma, "1"], w64)
        print(f"ntaps {ntaps} QDSP_HIP_FFT_DMA={dma}: rel rms vs FP64 oracle {err:.3e}")
        assert err < TOL_FFT


def both_layouts(monkeypatch, make, run):
    res = []
    for tbl in ("0", "1"):
        monkeypatch.setenv("QDSP_HIP_FFT_TBL", tbl)
        op = make()
        op.set_mode(op.FFT)
        res.append(run(op))
        assert kname(op) == "fir_fft_kernel", op.last_kernel()
    return res[0], res[1], op


@pytest.mark.parametrize("dec", [2, 4, 8, 16])
def test_layouts_agree_in_the_per_segment_decimators(ops, monkeypatch, x90k, dec):
    """fir_fft_kernel<dec>: the pruned inverse re-reads the pass-A twiddles from the table in every segment."""
    taps = random_taps(256)
    y0, y1, op = both_layouts(monkeypatch, lambda: ops.Resampler(taps, 1, dec), lambda op: run_blocks(op, x90k, SIZES))
    assert op.last_kernel()["lds_bytes"] != GROUPED_LDS
    assert len(y1) > 0 and np.array_equal(y0, y1)
    want = run_blocks(O.Resampler(taps, 1, dec, acc=O.ACC_F64), x90k, SIZES)
    assert len(y1) == len(want) and rel_rms(y1, want) < TOL_FFT


@pytest.mark.parametrize("dec", [4, 8, 16])
def test_layouts_agree_in_the_grouped_decimators(ops, monkeypatch, dec):
    """fir_fft_dec_kernel<dec> takes calls of at least 1024 groups of dec segments (3840 samples each at 256 taps): one such call, a
    ragged last group, compared on the device; the start of the output against the FP64 oracle."""
    import torch

    taps = random_taps(256)
    n = 3840 * 1024 * dec + 4992
    x = ops.synth_iq(n, seed=11 + dec, device=0)
    y0, y1, op = both_layouts(monkeypatch, lambda: ops.Resampler(taps, 1, dec, max_block=0), lambda op: op.process(x).clone())
    assert op.last_kernel()["lds_bytes"] == GROUPED_LDS, op.last_kernel()
    assert y1.numel() == n // dec and torch.equal(y0, y1)
    head = 8 * 3840
    want = O.Resampler(taps, 1, dec, acc=O.ACC_F64).process(O.synth_iq(0, head, seed=11 + dec))
    assert rel_rms(y1[: head // dec].cpu().numpy(), want) < TOL_FFT


def test_layouts_agree_in_the_fused_vfo(ops, monkeypatch, x90k):
    taps = random_taps(256)
    inc = ops.phase_delta(1.0, 0.1234)
    for dec in (3, 8):   # fir_fft_kernel<1, true> (full inverse, every third output kept: tables in registers) and <8, true> (re-read per segment)
        y0, y1, _ = both_layouts(monkeypatch, lambda: ops.Vfo(taps, 1, dec, inc), lambda op: run_blocks(op, x90k, SIZES))
        assert len(y1) > 0 and np.array_equal(y0, y1)


def test_layouts_agree_on_real_data(ops, monkeypatch, x90k):
    taps = random_taps(256)
    xr = np.ascontiguousarray(x90k.real)
    y0, y1, _ = both_layouts(monkeypatch, lambda: ops.Fir(taps, complex_data=False), lambda op: run_blocks(op, xr, SIZES))
    assert y1.dtype == np.float32 and np.array_equal(y0, y1)
    assert rel_rms(y1, O.Fir(taps, complex_data=False, acc=O.ACC_F64).process(xr)) < TOL_FFT


def test_persistent_loop_prefetch_and_tapered_grid(ops, monkeypatch):
    """One aligned call of 549 whole segments and 1 234 samples with 256 workgroup slots (QDSP_HIP_FFT_WG_PER_CU=1): fir_fft_kernel runs
    it as 256 workgroups of two to three segments each; the LDS-DMA kernels as their tapered grid (fft_fir.hip.h) -- 256 long workgroups
    of two segments, 256 apart, and 38 short ones of one.  The first segment is guarded (history), a long workgroup's second one is
    prefetched by LDS-DMA behind its predecessor's last pass, the last segment is cut short by the end of the input: the smallest size at
    which the loop, the prefetch hand-over, an uneven split and both kinds of workgroup occur.  A call of exactly 256 segments takes no
    short workgroups."""
    taps = random_taps(256)            # overlap 256 -> 3840 new samples per segment
    n = 3840 * 549 + 1234
    xh = O.synth_iq(0, n, seed=17)
    x = dev(xh)
    monkeypatch.setenv("QDSP_HIP_FFT_WG_PER_CU", "1")
    out, out256 = {}, {}
    for dma, tbl in (("0", "1"), ("1", "1"), ("1", "0"), ("2", "1")):
        monkeypatch.setenv("QDSP_HIP_FFT_DMA", dma)
        monkeypatch.setenv("QDSP_HIP_FFT_TBL", tbl)
        f = ops.Fir(taps, max_block=0)
        f.set_mode(f.FFT)
        out[dma, tbl] = f.process(x).cpu().numpy()
        assert f.last_kernel()["name"] == {"0": "fir_fft_kernel", "1": "fir_fft_dma_kernel", "2": "fir_fft_dmapk_kernel"}[dma]
        # 550 segments: 256 workgroups (and the history hand-over), or 256 long ones, 38 short ones (and the hand-over)
        assert f.last_kernel()["grid"] == (256 + 1 if dma == "0" else 256 + 38 + 1), f.last_kernel()
        g = ops.Fir(taps, max_block=0)
        g.set_mode(g.FFT)
        out256[dma, tbl] = g.process(x[: 3840 * 256]).cpu().numpy()
        assert g.last_kernel()["grid"] == 256 + 1, g.last_kernel()
    assert np.array_equal(out["1", "1"], out["0", "1"])
    assert np.array_equal(out["1", "1"], out["1", "0"])
    assert np.array_equal(out256["1", "1"], out256["0", "1"]) and np.array_equal(out256["1", "1"], out["1", "1"][: 3840 * 256])
    y = out["1", "1"]
    H = len(taps) - 1
    for a, b in ((0, 3 * 3840), (3840 * 274 - 100, 3840 * 277 + 100), (n - 3 * 3840, n)):   # start, middle, end: three segments each
        lo = max(a - H, 0)
        want = O.Fir(taps, acc=O.ACC_F64).process(xh[lo:b])[a - lo:]
        assert rel_rms(y[a:b], want) < TOL_FFT, (a, b)
        assert rel_rms(out["2", "1"][a:b], want) < TOL_FFT, (a, b)
