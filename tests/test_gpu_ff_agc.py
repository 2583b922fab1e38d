"""FeedForwardAGC on the GPU (qdsp_hip_ffagc_*, ops.FeedForwardAgc, dsp::FeedForwardAGC<T>) against `ffagc_ref` of
tests/test_ff_agc_cpu.py, itself pinned to the block's equations written out in C++.  Every comparison is for equal bits: the level
is a maximum of floats, one rounded product and one rounded sum, and the output one IEEE division -- nothing leaves room for a
tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from qdsp_amd import capi, ops
from test_ff_agc_cpu import F32, MAX_WINDOW, TILE, _same_bits, amplitude, divide, ffagc_ref

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "demod_check")
KERNEL = "ff_agc_kernel"
KINDS = ("real", "complex")
WINDOWS = (1, 2, 7, 1024, 4096)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def bits(t):
    """A float or complex tensor as int32 words."""
    import torch

    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and _same_bits(a.view(F32), b.view(F32))


def noise(kind, n, seed, amp=1.0):
    """Gaussian samples whose amplitude steps by 30 dB every 700 samples: the level of nearly every window is set somewhere else."""
    rng = np.random.default_rng(seed)
    env = amp * np.repeat(10.0 ** rng.uniform(-2, 1, n // 700 + 1), 700)[:n]
    re_ = (rng.standard_normal(n) * env).astype(F32)
    if kind == "real":
        return re_
    z = np.empty(n, np.complex64)
    z.real, z.imag = re_, (rng.standard_normal(n) * env * 3).astype(F32)
    return z


def lds_bytes(window):
    return 2 * ((TILE + window - 1 + 3) & ~3) * 4


def counts_for(window):
    c = (1, window - 2, window - 1, window, window + 1, TILE - 1, TILE, TILE + 1, TILE + window - 1, 3 * TILE + 5)
    return sorted({n for n in c if n >= 1})


# ---- 1. one call from reset ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("kind", KINDS)
def test_one_call_from_reset(torch, kind, window):
    counts = counts_for(window)
    x = noise(kind, counts[-1], seed=window)
    xt = torch.from_numpy(x).cuda()
    op = ops.FeedForwardAgc(kind, max_block=counts[-1], window=window)
    assert capi.load().qdsp_hip_ffagc_window(op._h) == window and op.fill() == 0
    for n in counts:
        op.reset()
        want, hist = ffagc_ref(x[:n], window)
        assert len(want) == max(0, n - (window - 1))
        assert op.out_size(n) == len(want), (n, op.out_size(n))
        y = op.process(xt[:n])
        assert y.numel() == len(want) and op.fill() == len(hist) == n - len(want), (n, y.numel(), op.fill())
        assert op.out_size(0) == 0 and op.out_size(1) == (1 if op.fill() == window - 1 else 0)
        assert same(y.cpu().numpy(), want), (kind, window, n)
        assert same(op.get_history(), hist), (kind, window, n)
        tiles = -(-len(want) // TILE)
        if tiles + (op.fill() > 0):
            assert op.last_kernel() == {"name": KERNEL, "grid": tiles + (op.fill() > 0), "block": 256,
                                        "lds_bytes": lds_bytes(window) if tiles else 0}, (n, op.last_kernel())
        op.reset()
        assert same(op.process(x[:n]), want), ("host", kind, window, n)


# ---- 2. the outputs do not depend on the cuts ------------------------------------------------------------------------------------
def ragged_bounds(window, n):
    b = [1, 5, window - 1, window, window + TILE + 3, window + TILE + 4, 2 * window + TILE + 2, 2 * window + 2 * TILE + 2, n - 1, n]
    return [0] + sorted({v for v in b if 0 < v <= n})


@pytest.mark.parametrize("window", [7, 1024, 4096])
@pytest.mark.parametrize("kind", KINDS)
def test_cut_invariance(torch, kind, window):
    n = 3 * TILE + 2 * window + 11
    x = noise(kind, n, seed=3 + window)
    xt = torch.from_numpy(x).cuda()
    want = ffagc_ref(x, window)[0]
    one = ops.FeedForwardAgc(kind, max_block=n, window=window)
    assert same(one.process(xt).cpu().numpy(), want) and one.fill() == window - 1
    bounds = ragged_bounds(window, n)
    silent = [b for b in bounds[1:] if b < window]
    assert len(silent) >= 2, "consecutive calls that emit nothing"
    for path in ("device", "host"):
        op = ops.FeedForwardAgc(kind, max_block=n, window=window)
        got = []
        for a, b in zip(bounds, bounds[1:]):
            expect = op.out_size(b - a)
            y = op.process(xt[a:b]).cpu().numpy() if path == "device" else op.process(x[a:b])
            assert len(y) == expect == max(0, b - (window - 1)) - max(0, a - (window - 1)), (path, a, b)
            assert op.fill() == min(b, window - 1)
            got.append(y)
        assert same(np.concatenate(got), want), (path, kind, window)
    # the history carried into a fresh handle mid-stream, at a silent cut and at an emitting one
    for cut in (silent[-1], bounds[-4]):
        a_ = ops.FeedForwardAgc(kind, max_block=n, window=window)
        head = a_.process(xt[:cut]).cpu().numpy()
        hist = a_.get_history()
        assert len(hist) == a_.fill() == min(cut, window - 1) and same(hist, x[cut - len(hist):cut])
        b_ = ops.FeedForwardAgc(kind, max_block=n, window=window)
        b_.set_history(hist)
        assert b_.fill() == len(hist)
        tail = b_.process(xt[cut:]).cpu().numpy()
        assert same(np.concatenate([head, tail]), want), (kind, window, cut)


# ---- 3. the peak at every position relative to a tile ---------------------------------------------------------------------------
@pytest.mark.parametrize("window", [7, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_one_peak_scales_exactly_window_outputs(torch, kind, window):
    n = 3 * TILE + window + 5                        # outputs 0 .. 3 TILE + 5: tile 1 is whole, its halo ends at 2 TILE + window - 2
    x0 = noise(kind, n, seed=11, amp=1e-3)
    nout = n - (window - 1)
    op = ops.FeedForwardAgc(kind, max_block=n, window=window)
    base = op.process(torch.from_numpy(x0).cuda()).cpu().numpy()
    assert same(base, ffagc_ref(x0, window)[0])
    peak = F32(100.0)
    level = amplitude(np.asarray([peak], np.complex64 if kind == "complex" else F32))[0]
    for pos in (TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 2 * TILE + window - 2, 2 * TILE + window - 1, window - 1, nout - 1, n - 1):
        x = x0.copy()
        x[pos] = peak                                # (complex: re = 100, im = 0)
        op.reset()
        y = op.process(torch.from_numpy(x).cuda()).cpu().numpy()
        assert same(y, ffagc_ref(x, window)[0]), (kind, window, pos)
        changed = np.flatnonzero(y.view(F32).reshape(nout, -1) != base.view(F32).reshape(nout, -1))
        changed = set(changed // (2 if kind == "complex" else 1))
        lo, hi = max(0, pos - window + 1), min(pos, nout - 1)
        under = set(range(lo, hi + 1))                # (at pos itself the quotient may be what it was: a sample that set its own level)
        assert changed <= under and under - changed <= {pos}, (kind, window, pos, lo, hi, sorted(changed ^ under)[:6])
        scaled = np.delete(np.arange(lo, hi + 1), pos - lo) if pos <= hi else np.arange(lo, hi + 1)
        assert same(y[scaled], divide(x[scaled], level)), "the peak's level under every window that holds it"
        if pos <= hi:
            assert y[pos].real == peak / level


# ---- 4. batches on the real producer ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bank(torch):
    """A 64-channel uniform channelizer over noise plus three tones: two calls of (64, 4096) rows."""
    nchan, M = 64, 64
    taps = O.lowpass_taps_f64(256, 1.0 / 64.0)
    incs = [ops.phase_delta(1.0, -(c - 31.5) / 64.0) for c in range(nchan)]
    chn = ops.Channelizer(taps, 1, M, incs, max_block=0)
    n = 64 * 4096
    rows = []
    for call in range(2):
        t = np.arange(call * n, (call + 1) * n, dtype=np.float64)
        x = 0.02 * O.synth_iq(call * n, n, seed=8).astype(np.complex128)
        for c, amp in ((5, 1.0), (20, 0.3), (47, 0.1)):
            x += amp * np.exp(2j * np.pi * ((c - 31.5) / 64.0) * t)
        y = chn.process(torch.from_numpy(x.astype(np.complex64)).cuda())
        assert chn.last_kernel()["name"] == "chan_uniform_kernel" and y.shape == (nchan, chn.out_size(n))
        rows.append(y.clone())
    return nchan, rows


@pytest.mark.parametrize("pad", [37, 0])             # rows padded by an odd number of samples: the narrow stores; unpadded: 16-byte stores
@pytest.mark.parametrize("kind", KINDS)
def test_batch_on_channelizer_output(torch, bank, kind, pad):
    nchan, rows = bank
    no = rows[0].shape[1]
    window = 1024
    dt = torch.complex64 if kind == "complex" else torch.float32
    sentinel = 7 - 7j if kind == "complex" else 7.0
    am = ops.AmDemod(nchan=nchan)
    op = ops.FeedForwardAgc(kind, nchan=nchan, window=window)
    singles = [ops.FeedForwardAgc(kind, window=window) for _ in range(nchan)]
    for call, yc in enumerate(rows):
        xin = torch.full((nchan, no + pad), 3.0, dtype=dt, device="cuda")
        if kind == "complex":
            xin[:, :no] = yc
        else:
            am.process_batch(yc, xin)                # a float batch: |x| - mean of every row
        keep = xin.clone()
        obuf = torch.full((nchan, no + pad), sentinel, dtype=dt, device="cuda")
        expect = op.out_size(no)
        y = op.process_batch(xin[:, :no], obuf)
        assert y.shape == (nchan, expect) and expect == (no - (window - 1) if call == 0 else no) and op.fill() == window - 1
        assert op.last_kernel() == {"name": KERNEL, "grid": -(-expect // TILE) + 1, "block": 256, "lds_bytes": lds_bytes(window)}
        assert bool((obuf[:, expect:] == sentinel).all()), "nothing beyond the outputs is written, the padding neither"
        assert torch.equal(bits(xin), bits(keep)), "the input is only read"
        for c, s in enumerate(singles):
            ys = s.process(xin[c, :no].contiguous())
            assert torch.equal(bits(ys), bits(y[c])), (kind, pad, call, c)
        if call == 0:
            r0 = xin[0, :no].cpu().numpy()
            assert same(y[0].cpu().numpy(), ffagc_ref(r0, window)[0])
        top = torch.view_as_real(y)[..., 0].abs().max() if kind == "complex" else y.abs().max()
        assert float(top) <= 1.0, "|re| / level never exceeds 1"


# ---- 5. NaN and Inf stay where they are -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_nan_and_inf_locality(torch, kind):
    window, n = 1024, 3 * TILE + 1024 + 5
    x = noise(kind, n, seed=23)
    clean = ffagc_ref(x, window)[0]
    nout = len(clean)
    rows = np.stack([x, x, x])
    k_re, k_im, k_inf = TILE - 3, TILE + 1500, 2 * TILE + 1100
    rows[1, k_re] = np.nan if kind == "real" else complex(np.nan, 0.25)
    if kind == "complex":
        rows[1, k_im] = complex(rows[1, k_im].real, np.nan)
    rows[1, k_inf] = np.inf if kind == "real" else complex(np.inf, 0.5)
    op = ops.FeedForwardAgc(kind, nchan=3, window=window)
    y = op.process_batch(torch.from_numpy(rows).cuda()).cpu().numpy()
    assert y.shape == (3, nout)
    assert same(y[0], clean) and same(y[2], clean), "no other row"
    assert same(y[1], ffagc_ref(rows[1], window)[0])
    re_ = y[1].real if kind == "complex" else y[1]
    bad = np.flatnonzero(~same_each(y[1], clean))
    under_inf = np.arange(k_inf - window + 1, k_inf + 1)
    assert sorted(set(bad) - set(under_inf)) == ([k_re, k_im] if kind == "complex" else [k_re]), "a NaN: its own index only, in no level"
    assert np.isnan(re_[k_re]) and np.isnan(re_[k_inf]) and np.count_nonzero(np.isnan(y[1].view(F32))) == (3 if kind == "complex" else 2)
    if kind == "complex":
        assert np.isnan(y[1, k_im].imag) and y[1, k_im].real == clean[k_im].real and y[1, k_re].imag == F32(0.25) / level_at(rows[1], k_re, window)
        assert y[1, k_inf].imag == 0
    assert not np.any(re_[under_inf[:-1]]) and len(under_inf) == window, "+Inf: exactly the W outputs whose window holds it"
    assert same(y[1, k_inf + 1:], clean[k_inf + 1:]) and same(y[1, k_im + 1:under_inf[0]], clean[k_im + 1:under_inf[0]])


def same_each(a, b):
    """Per sample: equal bits (any NaN equal to any NaN) in every float of it."""
    a, b = np.asarray(a).view(F32).reshape(len(a), -1), np.asarray(b).view(F32).reshape(len(b), -1)
    return np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)), axis=1)


def level_at(x, p, window):
    with np.errstate(all="ignore"):
        a = amplitude(x[p:p + window])
    return max(F32(1e-4), a[~np.isnan(a)].max())


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------
def test_same_call_twice_gives_the_same_bits(torch):
    nchan, n = 64, 3 * TILE + 5
    g = torch.Generator(device="cuda").manual_seed(5)
    for kind in KINDS:
        x = torch.randn((nchan, n, 2) if kind == "complex" else (nchan, n), device="cuda", generator=g)
        x = torch.view_as_complex(x) if kind == "complex" else x
        op = ops.FeedForwardAgc(kind, nchan=nchan)
        hist = x[0, :700].cpu().numpy()
        op.set_history(hist)
        y1 = op.process_batch(x).clone()
        assert y1.shape == (nchan, n + 700 - 1023) and op.fill() == 1023
        op.set_history(hist)
        y2 = op.process_batch(x)
        assert torch.equal(bits(y1), bits(y2))
        op.reset()
        assert op.fill() == 0 and op.process_batch(x).shape == (nchan, n - 1023)


# ---- 7. argument errors, harness helpers -------------------------------------------------------------------------------------------
def test_argument_errors(torch):
    L = capi.load()
    h = C.c_void_p()
    for kind, nchan, mb, window in ((2, 1, 10, 1024), (-1, 1, 10, 1024), (0, 0, 10, 1024), (1, 70_000, 10, 1024), (0, 1, -5, 1024),
                                    (0, 1, 10, 0), (1, 1, 10, -3), (1, 1, 10, MAX_WINDOW + 1)):
        assert L.qdsp_hip_ffagc_create(C.byref(h), 0, kind, nchan, mb, window) == EINVAL, (kind, nchan, mb, window)
    assert L.qdsp_hip_ffagc_create(None, 0, 0, 1, 10, 8) == EINVAL
    re1, cx1 = ops.FeedForwardAgc("real", max_block=100, window=8), ops.FeedForwardAgc("complex", max_block=100, window=8)
    re2, cx2 = ops.FeedForwardAgc("real", nchan=2, max_block=100, window=8), ops.FeedForwardAgc("complex", nchan=2, max_block=100, window=8)
    x = np.zeros((101, 2), np.float32)
    y = np.zeros((101, 2), np.float32)
    for one, two in ((re1, re2), (cx1, cx2)):
        proc, ex = L.qdsp_hip_ffagc_process, L.qdsp_hip_ffagc_process_ex
        assert proc(one._h, x.ctypes.data, 101, y.ctypes.data) == ESIZE
        assert proc(one._h, x.ctypes.data, -1, y.ctypes.data) == EINVAL
        assert proc(one._h, x.ctypes.data, 0, y.ctypes.data) == 0
        assert proc(one._h, None, 10, y.ctypes.data) == EINVAL and proc(one._h, x.ctypes.data, 10, None) == EINVAL
        assert proc(two._h, x.ctypes.data, 10, y.ctypes.data) == EINVAL             # host path: one channel
        assert ex(one._h, x.ctypes.data, 7, 10, y.ctypes.data, 0) == EINVAL
        assert ex(one._h, x.ctypes.data, 0, 10, y.ctypes.data, 3) == EINVAL           # deferred without an event
        assert one.fill() == 0 and L.qdsp_hip_ffagc_out_size(one._h, -1) == EINVAL
        assert L.qdsp_hip_ffagc_get_history(two._h, 2, x.ctypes.data) == EINVAL and L.qdsp_hip_ffagc_get_history(two._h, 0, None) == EINVAL
        assert L.qdsp_hip_ffagc_set_history(two._h, 2, x.ctypes.data, 3) == EINVAL and L.qdsp_hip_ffagc_set_history(two._h, 0, x.ctypes.data, 8) == EINVAL
        assert L.qdsp_hip_ffagc_set_history(two._h, -2, x.ctypes.data, 3) == EINVAL and L.qdsp_hip_ffagc_set_history(two._h, 0, None, 3) == EINVAL
        assert L.qdsp_hip_ffagc_set_history(two._h, -1, x.ctypes.data, 7) == 0 and two.fill() == 7 and L.qdsp_hip_ffagc_reset(two._h) == 0
    xt = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    yt = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    bd = L.qdsp_hip_ffagc_process_batch_dev
    for two, es in ((re2, 4), (cx2, 8)):
        mis = es // 2
        assert bd(two._h, xt.data_ptr(), 400, 399, yt.data_ptr(), 400, None) == EINVAL
        assert bd(two._h, xt.data_ptr(), 400, 400, yt.data_ptr(), 392, None) == EINVAL          # 393 outputs per row
        assert bd(two._h, xt.data_ptr() + mis, 10, 10, yt.data_ptr(), 10, None) == EINVAL
        assert bd(two._h, xt.data_ptr(), 10, 10, yt.data_ptr() + mis, 10, None) == EINVAL
        assert bd(two._h, xt.data_ptr(), -1, 10, yt.data_ptr(), 10, None) == EINVAL
        assert bd(two._h, None, 10, 10, yt.data_ptr(), 10, None) == EINVAL
        assert bd(two._h, xt.data_ptr(), 10, 10, None, 10, None) == EINVAL
        assert bd(two._h, xt.data_ptr(), 0, 0, yt.data_ptr(), 0, None) == 0
        # any overlap of the two row spans: in place, shifted, the output inside the input rows, the input inside the output rows
        p = xt.data_ptr()
        assert bd(two._h, p, 100, 100, p, 100, None) == EINVAL
        assert bd(two._h, p, 100, 100, p + es, 100, None) == EINVAL
        assert bd(two._h, p, 100, 100, p + 199 * es, 100, None) == EINVAL
        assert bd(two._h, p + 185 * es, 100, 100, p, 93, None) == EINVAL
        assert two.fill() == 0, "a refused call takes nothing in"
        assert bd(two._h, p, 100, 100, p + 200 * es, 93, None) == 93 and two.fill() == 7          # the spans touch and do not overlap
        L.qdsp_hip_ffagc_reset(two._h)
        assert bd(two._h, p, 5, 100, p, 100, None) == 0 and two.fill() == 5, "a call that writes nothing overlaps nothing"
    # handle kinds do not mix, in either direction
    fm, de = ops.FmDemod(250e3, 75e3), ops.Deemp(48e3, 50e-6)
    ssb, fir = ops.SsbDemod(48_000.0, 3_000.0, 0), ops.Fir(np.ones(8, np.float32))
    agc, sq, sfm = ops.Agc(1.0, 48e3), ops.Squelch(-50.0), ops.StereoFmDemod(250e3, 75e3)
    args = (xt.data_ptr(), 10, yt.data_ptr(), None)
    for other in (fm, de, ssb, fir, agc, sq, sfm):
        assert L.qdsp_hip_ffagc_process_dev(other._h, *args) == EINVAL and L.qdsp_hip_ffagc_process(other._h, x.ctypes.data, 10, y.ctypes.data) == EINVAL
        assert L.qdsp_hip_ffagc_reset(other._h) == EINVAL and L.qdsp_hip_ffagc_fill(other._h) == EINVAL
        assert L.qdsp_hip_ffagc_window(other._h) == EINVAL and L.qdsp_hip_ffagc_out_size(other._h, 10) == EINVAL
        assert L.qdsp_hip_ffagc_get_history(other._h, 0, x.ctypes.data) == EINVAL
        assert L.qdsp_hip_ffagc_set_history(other._h, 0, x.ctypes.data, 1) == EINVAL
    for mine in (re1, cx1):
        assert L.qdsp_hip_demod_process_dev(mine._h, *args) == EINVAL and L.qdsp_hip_demod_reset(mine._h) == EINVAL
        assert L.qdsp_hip_deemp_process_dev(mine._h, *args) == EINVAL and L.qdsp_hip_deemp_reset(mine._h) == EINVAL
        assert L.qdsp_hip_ssb_cf32_process_dev(mine._h, *args) == EINVAL
        assert L.qdsp_hip_fir_cf32_process_dev(mine._h, *args) == EINVAL
        assert L.qdsp_hip_agc_process_dev(mine._h, *args) == EINVAL and L.qdsp_hip_agc_reset(mine._h) == EINVAL
        assert L.qdsp_hip_squelch_process_dev(mine._h, *args) == EINVAL and L.qdsp_hip_squelch_reset(mine._h) == EINVAL
        assert L.qdsp_hip_stereo_fm_process_dev(mine._h, *args) == EINVAL and L.qdsp_hip_stereo_fm_reset(mine._h) == EINVAL
        assert mine.fill() == 0
    torch.cuda.synchronize()


def test_last_kernel_done_event_and_time(torch):
    L = capi.load()
    ev = C.c_void_p()
    capi.check(L.qdsp_hip_event_create(0, C.byref(ev)))
    n = 1 << 20
    for kind, x in (("complex", torch.view_as_complex(torch.randn((n, 2), device="cuda"))), ("real", torch.randn(n, device="cuda"))):
        op = ops.FeedForwardAgc(kind)
        assert L.qdsp_hip_set_done_event(op._h, ev) == 0
        assert op.time_dev(x, torch.empty_like(x), 3) > 0 and op.fill() == 1023
        assert op.last_kernel() == {"name": KERNEL, "grid": n // TILE + 1, "block": 256, "lds_bytes": lds_bytes(1024)}
        op.reset()
        hx = x[:3000].cpu().numpy()
        hy = np.zeros_like(hx)
        assert op.process_ex(hx.ctypes.data, 0, 1000, hy.ctypes.data, 3) == 0 and op.fill() == 1000      # host out, deferred; nothing yet
        assert op.last_kernel() == {"name": KERNEL, "grid": 1, "block": 256, "lds_bytes": 0} and not np.any(hy.view(F32))
        assert op.process_ex(hx[1000:].ctypes.data, 0, 2000, hy.ctypes.data, 3) == 1977
        assert same(hy[:1977], ffagc_ref(hx, 1024)[0]) and not np.any(hy[1977:].view(F32))
        one = ops.FeedForwardAgc(kind, window=1)     # no lag, no history: the tiles alone
        y = one.process(x[:TILE + 1])
        assert one.last_kernel() == {"name": KERNEL, "grid": 2, "block": 256, "lds_bytes": lds_bytes(1)} and one.fill() == 0
        assert same(y.cpu().numpy(), ffagc_ref(x[:TILE + 1].cpu().numpy(), 1)[0])
    capi.check(L.qdsp_hip_event_destroy(ev))


# ---- 8. the block graph ------------------------------------------------------------------------------------------------------------
N, BLOCK, DECIM = 240_000, 24_000, 10
VFO_ARGS = ["300000", "2400000", "240000", "200000"]    # offset, inSR, outSR, bandwidth: 2.4 Msps -> 240 ksps


@pytest.fixture(scope="module")
def graph(tmp_path_factory):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL, timeout=300)
    d = tmp_path_factory.mktemp("ffagcgraph")
    x = O.synth_iq(0, N, seed=42)
    x[N // 2:] *= np.float32(0.1)                   # the second half 20 dB weaker
    x.tofile(d / "x.cf32")
    subprocess.run([BIN, "vfo", str(d / "x.cf32"), str(d / "v.cf32"), str(BLOCK)] + VFO_ARGS, check=True, timeout=180,
                   capture_output=True, text=True)
    v = np.fromfile(d / "v.cf32", dtype=np.complex64)
    assert len(v) == N // DECIM
    return d, v


@pytest.mark.parametrize("link", ["dev", "host"])
def test_vfo_then_feed_forward_agc_blocks(graph, link):
    d, v = graph
    out = d / f"ffagc_{link}.cf32"
    r = subprocess.run([BIN, "ffagc", link, str(d / "x.cf32"), str(out), str(BLOCK)] + VFO_ARGS, check=True, timeout=180,
                       capture_output=True, text=True)
    assert "graph ok" in r.stdout and f"{link if link == 'host' else 'device'} link" in r.stdout
    y = np.fromfile(out, dtype=np.complex64)
    assert len(y) == N // DECIM - 1023
    vb = BLOCK // DECIM
    op = ops.FeedForwardAgc("complex", max_block=vb)
    got = np.concatenate([op.process(v[a:a + vb]) for a in range(0, len(v), vb)])      # one run() per VFO output block
    assert same(y, got)
    assert same(y, ffagc_ref(v, 1024)[0]), "and the stream as a whole"
    assert float(np.abs(y.real).max()) <= 1.0
