"""QDSP_HIP_FFT_NT is the cache policy of the sample stream in the two LDS-DMA forms of the 4096-point overlap-save FIR
(qdsp_amd/csrc/fft_fir.hip: fir_fft_dma_kernel, fir_fft_dmapk_kernel): bit 0 makes the LDS-DMA of an interior segment's rows
non-temporal, bit 1 its eight 16-byte stores.  A cache policy moves the same values in the same order, so it may not change one bit of
any output: every comparison here is np.array_equal against QDSP_HIP_FFT_NT=0 of the same kernel.

Checked: a stream cut into ragged calls (guarded first segment, interior DMA segments, ragged tail) at the smallest, the everyday and the
largest overlap of the path; the persistent segment loop on the tapered grid, where a long workgroup's second segment arrives by the
(non-temporal) DMA behind its predecessor's (non-temporal) stores; a second operator and a copy to the host right behind the FIR on the
same stream with no synchronisation between (non-temporal stores are not write-through: the kernel boundary is what makes the bytes
visible); and an input that is not 16-byte aligned, which the LDS-DMA path declines whatever the policy."""
import numpy as np
import pytest

import oracle as O
from conftest import rel_rms
from test_gpu_parity import TOL_FFT, dev, run_blocks

pytestmark = pytest.mark.gpu

N = 90_000
SIZES = [40_001, 4096, 3, 20_000, 25_900]   # first (history), interior (DMA) and last (end of input) segments
NAMES = {"0": "fir_fft_kernel", "1": "fir_fft_dma_kernel", "2": "fir_fft_dmapk_kernel"}
N_LOOP = 3840 * 549 + 1234                  # 256 taps: 549 whole segments and a cut one
DEFAULT = None                              # QDSP_HIP_FFT_NT unset


@pytest.fixture(scope="module")
def ops():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from qdsp_amd import ops as _ops

    assert "gfx950" in _ops.device_info(0)["arch"]
    return _ops


@pytest.fixture(autouse=True)
def _pin_the_4096_point_kernels(monkeypatch):
    """As tests/test_gpu_fft_tables.py: oracle-sized calls would go to the one-wave 1024-point form by default."""
    monkeypatch.setenv("QDSP_HIP_FFT1K_MAX_COUNT", "0")
    monkeypatch.setenv("QDSP_HIP_DECIM_SETTING", "0")
    monkeypatch.setenv("QDSP_HIP_NO_PFB", "1")


@pytest.fixture(scope="module")
def x90k():
    return O.synth_iq(0, N, seed=5)


@pytest.fixture(scope="module")
def loop_input():
    """The 549-segment call: host samples, taps, and the FP64 oracle on three three-segment windows (start, middle, end)."""
    taps = random_taps(256)
    xh = O.synth_iq(0, N_LOOP, seed=17)
    H = len(taps) - 1
    windows = []
    for a, b in ((0, 3 * 3840), (3840 * 274 - 100, 3840 * 277 + 100), (N_LOOP - 3 * 3840, N_LOOP)):
        lo = max(a - H, 0)
        windows.append((a, b, O.Fir(taps, acc=O.ACC_F64).process(xh[lo:b])[a - lo:]))
    return xh, taps, windows


def random_taps(ntaps):
    rng = np.random.default_rng(7 + ntaps)
    return (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)


def set_nt(monkeypatch, nt):
    if nt is DEFAULT:
        monkeypatch.delenv("QDSP_HIP_FFT_NT", raising=False)
    else:
        monkeypatch.setenv("QDSP_HIP_FFT_NT", nt)


@pytest.mark.parametrize("ntaps", [2, 256, 2049])
def test_policy_changes_no_bit_of_a_stream_in_pieces(ops, monkeypatch, x90k, ntaps):
    """Overlap 2 (rounded up from 1), 256 and 2048 -- the path's limit: there rows 0-7 of every segment are overlap and only rows 8-15 are stored."""
    taps = random_taps(ntaps)
    out = {}
    for dma in ("0", "1", "2"):
        for nt in (("0",) if dma == "0" else ("0", "1", "2", "3", DEFAULT)):
            monkeypatch.setenv("QDSP_HIP_FFT_DMA", dma)
            set_nt(monkeypatch, nt)
            f = ops.Fir(taps)
            f.set_mode(f.FFT)
            out[dma, nt] = run_blocks(f, x90k, SIZES)
            assert f.last_kernel()["name"] == NAMES[dma], (dma, nt, f.last_kernel())
    for dma in ("1", "2"):
        for nt in ("1", "2", "3", DEFAULT):
            assert np.array_equal(out[dma, nt], out[dma, "0"]), f"QDSP_HIP_FFT_DMA={dma}: QDSP_HIP_FFT_NT={nt} differs from 0"
    assert np.array_equal(out["1", "0"], out["0", "0"])
    w64 = O.Fir(taps, acc=O.ACC_F64).process(x90k)
    for dma in ("1", "2"):
        err = rel_rms(out[dma, DEFAULT], w64)
        print(f"ntaps {ntaps} QDSP_HIP_FFT_DMA={dma}, default policy: rel rms vs FP64 oracle {err:.3e}")
        assert err < TOL_FFT


def test_policy_in_the_persistent_loop(ops, monkeypatch, loop_input):
    """One call of 3840 * 549 + 1234 samples on 256 workgroup slots: 256 long workgroups of two segments, 256 apart, 38 short ones of one, and the
    history hand-over.  The smallest size at which a long workgroup's second segment arrives by the DMA behind its predecessor's stores, at which
    short workgroups occur, and at which the last segment is cut by the end of the input."""
    xh, taps, windows = loop_input
    x = dev(xh)
    monkeypatch.setenv("QDSP_HIP_FFT_WG_PER_CU", "1")
    for dma in ("1", "2"):
        monkeypatch.setenv("QDSP_HIP_FFT_DMA", dma)
        out = {}
        for nt in ("0", "1", "2", "3"):
            set_nt(monkeypatch, nt)
            f = ops.Fir(taps, max_block=0)
            f.set_mode(f.FFT)
            out[nt] = f.process(x).cpu().numpy()
            assert f.last_kernel()["name"] == NAMES[dma] and f.last_kernel()["grid"] == 256 + 38 + 1, (dma, nt, f.last_kernel())
        for nt in ("1", "2", "3"):
            assert np.array_equal(out[nt], out["0"]), f"QDSP_HIP_FFT_DMA={dma}: QDSP_HIP_FFT_NT={nt} differs from 0"
        for a, b, want in windows:
            err = rel_rms(out["3"][a:b], want)
            print(f"QDSP_HIP_FFT_DMA={dma} [{a}, {b}): rel rms vs FP64 oracle {err:.3e}")
            assert err < TOL_FFT, (dma, a, b)


def test_a_consumer_right_behind_the_stores(ops, monkeypatch, loop_input):
    """The 549-segment call on the default grid (every XCD has written), then a 2-tap FIR reading the output buffer on the same stream and a copy of
    that buffer to the host, nothing in between: under the default policy and with both bits set, bit-equal to the same chain with plain stores."""
    xh, taps, _ = loop_input
    x = dev(xh)
    two = np.array([0.75, -0.5], dtype=np.float32)
    res = {}
    for nt in ("0", DEFAULT, "3"):
        set_nt(monkeypatch, nt)
        f = ops.Fir(taps, max_block=0)
        f.set_mode(f.FFT)
        g = ops.Fir(two, max_block=0)
        y = f.process(x)
        z = g.process(y)
        res[nt] = (y.cpu().numpy(), z.cpu().numpy())
        assert f.last_kernel()["name"] == "fir_fft_dma_kernel", f.last_kernel()
    for nt in (DEFAULT, "3"):
        assert np.array_equal(res[nt][0], res["0"][0]), f"QDSP_HIP_FFT_NT={nt}: the copy to the host differs"
        assert np.array_equal(res[nt][1], res["0"][1]), f"QDSP_HIP_FFT_NT={nt}: the consumer read something else"
    # (and the consumer did read the FIR's output: a 2-tap filter of it, two FP32 roundings per sample -- 1e-6 is sixteen ulps)
    assert rel_rms(res["0"][1][:4096], O.Fir(two, acc=O.ACC_F64).process(res["0"][0][:4096])) < 1e-6


def test_unaligned_input_declines_under_every_policy(ops, monkeypatch, x90k):
    """An input view that starts one sample (8 bytes) into its buffer: no 16-byte loads, so fir_fft_kernel runs it, whatever the policy says."""
    taps = random_taps(256)
    buf = dev(np.concatenate([np.zeros(1, np.complex64), x90k]))
    x = buf[1:]
    assert x.data_ptr() % 16 == 8 and x.is_contiguous()
    out = {}
    for nt in ("0", "1", "2", "3"):
        set_nt(monkeypatch, nt)
        f = ops.Fir(taps)
        f.set_mode(f.FFT)
        out[nt] = f.process(x).cpu().numpy()
        assert f.last_kernel()["name"] == "fir_fft_kernel", (nt, f.last_kernel())
    for nt in ("1", "2", "3"):
        assert np.array_equal(out[nt], out["0"])
    assert rel_rms(out["0"], O.Fir(taps, acc=O.ACC_F64).process(x90k)) < TOL_FFT
    # two samples in: 16-byte aligned, so the LDS-DMA kernel takes it (the default policy is then plain accesses: no 64-byte boundaries) -- same bits
    buf2 = dev(np.concatenate([np.zeros(2, np.complex64), x90k]))
    x2 = buf2[2:]
    assert x2.data_ptr() % 64 == 16
    for nt in (DEFAULT, "3"):
        set_nt(monkeypatch, nt)
        f = ops.Fir(taps)
        f.set_mode(f.FFT)
        y = f.process(x2).cpu().numpy()
        assert f.last_kernel()["name"] == "fir_fft_dma_kernel", (nt, f.last_kernel())
        assert np.array_equal(y, out["0"])
