"""Squelch and AGC on the GPU (qdsp_hip_squelch_*, qdsp_hip_agc_*, ops.Squelch, ops.Agc, dsp::Squelch, dsp::AGC) against the numpy
restatements of tests/test_level_cpu.py.  Squelch: the decision of `squelch_ref` at levels 0.01 dB either side of the call's own mean
(the device's mean is within 1e-4 dB of the restatement's), an open row the bits of the input, a closed row +0.0.  AGC: bit-identical
to `agc_ref` wherever the call's maximum sets the level; where the decayed level stands, the level within `agc_decay_bound` of the
exact decay and the outputs the bits of x * (1.0f / level)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from qdsp_amd import capi, ops
from test_level_cpu import (F32, ROW_TILES, SIZES, TILE, _same_bits, agc_decay, agc_ref, decay_error_ratio, squelch_cases, squelch_mean_db,
                            squelch_ref)

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "demod_check")
ROW, APPLY = "level_row_kernel", "level_apply_kernel"
LONG = 3 * ROW_TILES * TILE + 5


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def form_of(n):
    return ROW if -(-n // TILE) <= ROW_TILES else APPLY


def bits(t):
    """A float or complex tensor as int32 words."""
    import torch

    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def agc_input(n, amp, peak, seed):
    """Gaussian noise of standard deviation `amp` with one sample of exactly `peak` in the middle."""
    x = (np.random.default_rng(seed).standard_normal(n) * amp).astype(F32)
    x[n // 2] = peak
    return x


# ---- 1. squelch against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_squelch_against_the_restatement(torch, n):
    sq = ops.Squelch(-50.0, max_block=n)
    assert not sq.is_open()
    cache = {}
    for name, x, db, level, want_open in squelch_cases(n):
        if id(x) not in cache:
            cache[id(x)] = torch.from_numpy(x).cuda()
        want, ref_open = squelch_ref(x, level)
        assert ref_open == want_open
        sq.set_level(float(level))
        y = sq.process(cache[id(x)]).cpu().numpy()
        assert sq.last_kernel()["name"] == form_of(n), (n, name)
        print(f"n={n} {name}: mean {float(db):.4f} dB, level {float(level):.4f} dB, open {sq.is_open()}")
        assert sq.is_open() == want_open, (n, name)
        assert _same_bits(y.view(F32), want.view(F32)), (n, name)
        if not want_open:
            assert not np.any(y.view(np.uint32)), "+0.0 in every float"
        yh = sq.process(x)                          # the host entry point runs the same launch
        assert sq.is_open() == want_open and _same_bits(yh.view(F32), y.view(F32)), (n, name)
    assert len(sq.process(np.zeros(0, np.complex64))) == 0 and sq.is_open() == want_open      # count 0: a no-op
    sq.reset()
    assert not sq.is_open()


# ---- 2. AGC, peak regime --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_agc_peak_regime_is_bit_identical(torch, n):
    cfr = F32(3.0 / n)                              # about 3 dB per call
    for path in ("device", "host"):
        agc = ops.Agc(float(cfr), 1.0, max_block=n)
        assert agc.level() == 0
        lvl = F32(0)
        for k in range(3):
            x = agc_input(n, 0.3 * 1.2 ** k, 3.0 * 1.2 ** k, seed=k)
            want, new = agc_ref(x, lvl, cfr)
            assert x.max() > 1.01 * agc_decay(lvl, cfr, n), "peak regime"
            lvl = new
            y = agc.process(torch.from_numpy(x).cuda()).cpu().numpy() if path == "device" else agc.process(x)
            assert agc.last_kernel()["name"] == form_of(n), (n, k)
            assert _same_bits(y, want), (n, path, k)
            assert _same_bits([agc.level()], [lvl]), (n, path, k, agc.level(), lvl)


def test_agc_ragged_cuts_of_one_row(torch):
    n = 100_003
    cuts = [0, 1, 8, 4104, 4104 + 65_537, n]
    x = (np.random.default_rng(4).standard_normal(n) * 0.25).astype(F32)
    for k, a in enumerate(cuts[:-1]):
        x[a] = 4.0 * 1.3 ** k                       # every call brings its own peak
    cfr = F32(F32(20.0) / F32(48_000.0))
    xt = torch.from_numpy(x).cuda()
    for path in ("device", "host"):
        agc = ops.Agc(20.0, 48_000.0, max_block=n)
        lvl = F32(0)
        for a, b in zip(cuts, cuts[1:]):
            want, lvl = agc_ref(x[a:b], lvl, cfr)
            assert lvl == x[a]
            y = agc.process(xt[a:b]).cpu().numpy() if path == "device" else agc.process(x[a:b])
            assert _same_bits(y, want) and _same_bits([agc.level()], [lvl]), (path, a, b)
    # set_level + process == a fresh block started from that level
    a_, b_ = ops.Agc(20.0, 48_000.0), ops.Agc(20.0, 48_000.0)
    a_.process(xt[:5000])
    a_.set_level(7.5)
    b_.set_level(7.5)
    assert a_.level() == F32(7.5)
    assert _same_bits(a_.process(xt[5000:9000]).cpu().numpy(), b_.process(xt[5000:9000]).cpu().numpy()) and a_.level() == b_.level()


# ---- 3. AGC, decay regime -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [TILE + 1, LONG])
def test_agc_decay_regime(torch, n):
    cfr = F32(1.0 / n)                              # about 1 dB per call
    agc = ops.Agc(float(cfr), 1.0, max_block=n)
    agc.process(torch.from_numpy(agc_input(n, 0.5, 8.0, seed=1)).cuda())
    prev = agc.level()
    assert prev == F32(8.0)
    for k in range(3):
        x = (np.random.default_rng(10 + k).standard_normal(n) * 0.01).astype(F32)
        y = agc.process(torch.from_numpy(x).cuda()).cpu().numpy()
        assert agc.last_kernel()["name"] == form_of(n)
        lvl = agc.level()
        assert x.max() < 0.5 * lvl < lvl < prev, "decay regime"
        ratio = float(decay_error_ratio(lvl, prev, cfr, n))
        print(f"n={n} call {k}: level {prev} -> {lvl}, |error| / bound {ratio:.3f}")
        assert ratio <= 1.0, (n, k, prev, lvl)
        assert _same_bits(y, x * F32(F32(1.0) / lvl)), (n, k)
        prev = lvl
    # the first call from level 0 with no positive sample: x * inf
    agc.reset()
    assert agc.level() == 0
    x = -np.abs(agc_input(n, 1.0, 0.0, seed=5))
    x[::5] = 0.0
    x[1::5] = -0.0
    want, lvl = agc_ref(x, F32(0), cfr)
    assert lvl == 0 and np.all(np.isnan(want[::5])) and np.all(want[2::5] == -np.inf)
    y = agc.process(torch.from_numpy(x).cuda()).cpu().numpy()
    assert _same_bits(y, want) and _same_bits([agc.level()], [lvl])


# ---- 4. batch on the real producer -------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("pad", [37, 0])             # rows padded by an odd number of samples: the scalar path; unpadded: the vector path
def test_squelch_batch_on_channelizer_output(torch, bank, pad):
    nchan, rows = bank
    no = rows[0].shape[1]
    db = np.asarray([float(squelch_mean_db(r)) for r in rows[0].cpu().numpy()])
    mid = 0.5 * (db.min() + db.max())
    levels = np.asarray([mid + 0.5 * (c % 3 - 1) for c in range(nchan)], F32)
    sq = ops.Squelch(levels, nchan=nchan)
    singles = [ops.Squelch(float(levels[c])) for c in range(nchan)]
    for call, yc in enumerate(rows):
        xin = torch.full((nchan, no + pad), 3 + 3j, dtype=torch.complex64, device="cuda")
        xin[:, :no] = yc
        obuf = torch.full((nchan, no + pad), 7 - 7j, dtype=torch.complex64, device="cuda")
        y = sq.process_batch(xin[:, :no], obuf)
        assert sq.last_kernel()["name"] == form_of(no)
        if pad:
            assert bool((obuf[:, no:] == 7 - 7j).all()), "the padding is not written"
        opened = [sq.is_open(c) for c in range(nchan)]
        assert any(opened) and not all(opened), (call, opened)
        for c, s in enumerate(singles):              # same tiling, same order: the same bits
            ys = s.process(yc[c].contiguous())
            assert torch.equal(bits(ys), bits(y[c])) and s.is_open() == opened[c], (pad, call, c)
            assert torch.equal(bits(y[c]), bits(yc[c]) if opened[c] else torch.zeros_like(bits(yc[c]))), (pad, call, c)


@pytest.mark.parametrize("pad", [37, 0])
def test_am_then_agc_batch_on_channelizer_output(torch, bank, pad):
    nchan, rows = bank
    no = rows[0].shape[1]
    am = ops.AmDemod(nchan=nchan)
    falls = np.asarray([10.0 * (1 + c % 4) for c in range(nchan)], F32)
    agc = ops.Agc(falls, 3_906.25, nchan=nchan)
    singles = [ops.Agc(float(falls[c]), 3_906.25) for c in range(nchan)]
    for call, yc in enumerate(rows):
        fbuf = torch.full((nchan, no + pad), 5.0, dtype=torch.float32, device="cuda")
        f = am.process_batch(yc, fbuf)
        obuf = torch.full((nchan, no + pad), 7.0, dtype=torch.float32, device="cuda")
        y = agc.process_batch(f, obuf)
        assert agc.last_kernel()["name"] == form_of(no)
        if pad:
            assert bool((obuf[:, no:] == 7.0).all()), "the padding is not written"
        for c, s in enumerate(singles):
            ys = s.process(f[c].contiguous())
            assert torch.equal(bits(ys), bits(y[c])) and _same_bits([s.level()], [agc.level(c)]), (pad, call, c)
        lv = np.asarray([agc.level(c) for c in range(nchan)])
        assert float(y.max()) <= 1.0 and np.all(np.isfinite(lv)) and np.all(lv > 0)      # (AM's output |x| - mean has a positive peak in every row)


# ---- 5. NaN and Inf stay where they are ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [TILE + 1, LONG])
def test_nan_and_inf_locality(torch, n):
    name, x, db, level, want_open = squelch_cases(n)[2]              # gauss -6 dB, open
    assert want_open
    rows = np.stack([x, x, x])
    rows[1, n // 2] = np.nan + 0j
    sq = ops.Squelch(float(level), nchan=3)
    y = sq.process_batch(torch.from_numpy(rows).cuda()).cpu().numpy()
    assert [sq.is_open(c) for c in range(3)] == [True, False, True]
    assert _same_bits(y[0].view(F32), x.view(F32)) and _same_bits(y[2].view(F32), x.view(F32)) and not np.any(y[1].view(np.uint32))
    y = sq.process_batch(torch.from_numpy(np.stack([x, x, x])).cuda()).cpu().numpy()     # the next call is unaffected
    assert [sq.is_open(c) for c in range(3)] == [True] * 3 and _same_bits(y[1].view(F32), x.view(F32))
    # AGC: a NaN sample is a NaN output at its index only, and the level does not see it
    cfr = F32(1.0 / n)
    xa = agc_input(n, 0.3, 2.0, seed=2)
    want, lvl = agc_ref(xa, F32(0), cfr)
    xb = xa.copy()
    k = n // 3
    xb[k] = np.nan
    agc = ops.Agc(float(cfr), 1.0)
    y = agc.process(torch.from_numpy(xb).cuda()).cpu().numpy()
    assert np.isnan(y[k]) and _same_bits(np.delete(y, k), np.delete(want, k)) and _same_bits([agc.level()], [lvl])
    # +Inf pins the level at Inf until reset
    xb[k] = np.inf
    y = agc.process(torch.from_numpy(xb).cuda()).cpu().numpy()
    assert agc.level() == np.inf and _same_bits(y, agc_ref(xb, lvl, cfr)[0]) and np.isnan(y[k]) and not np.any(np.delete(y, k))
    y = agc.process(torch.from_numpy(xa).cuda()).cpu().numpy()
    assert agc.level() == np.inf and not np.any(y)
    agc.reset()
    assert agc.level() == 0
    assert _same_bits(agc.process(torch.from_numpy(xa).cuda()).cpu().numpy(), want)


# ---- 6. in place, 7. determinism -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [ROW_TILES * TILE - 4, LONG])          # even row stride: the vector path; odd: scalar
def test_in_place_equals_out_of_place(torch, n):
    nchan = 4
    L = capi.load()
    g = torch.Generator(device="cuda").manual_seed(3)
    amp = torch.tensor([1.0, 0.01, 1.0, 0.01], device="cuda")[:, None]
    xc = torch.view_as_complex(torch.randn((nchan, n + 2, 2), device="cuda", generator=g)) * amp
    a, b = ops.Squelch(-10.0, nchan=nchan), ops.Squelch(-10.0, nchan=nchan)
    want = a.process_batch(xc, count=n)
    assert a.last_kernel()["name"] == form_of(n)
    buf = xc.clone()
    got = b.process_batch(buf, buf, count=n)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(bits(got), bits(want))
    assert [a.is_open(c) for c in range(nchan)] == [b.is_open(c) for c in range(nchan)] == [True, False, True, False]
    assert torch.equal(bits(buf[:, n:]), bits(xc[:, n:])), "the padding is not written"
    # the same buffer with another stride is not "in place"; neither is a shifted one
    assert L.qdsp_hip_squelch_process_batch_dev(b._h, buf.data_ptr(), 100, n + 2, buf.data_ptr(), n + 4, None) == EINVAL
    assert L.qdsp_hip_squelch_process_batch_dev(b._h, buf.data_ptr(), 100, n + 2, buf.data_ptr() + 8, n + 2, None) == EINVAL
    xf = torch.randn((nchan, n + 4), device="cuda", generator=g) * amp         # (float rows: four samples per 16 bytes)
    c, d = ops.Agc(5.0, 1000.0, nchan=nchan), ops.Agc(5.0, 1000.0, nchan=nchan)
    for call in range(2):
        want = c.process_batch(xf, count=n)
        assert c.last_kernel()["name"] == form_of(n)
        buf = xf.clone()
        got = d.process_batch(buf, buf, count=n)
        assert got.data_ptr() == buf.data_ptr() and torch.equal(bits(got), bits(want))
        assert [c.level(k) for k in range(nchan)] == [d.level(k) for k in range(nchan)]
        xf = xf * 0.5
    assert L.qdsp_hip_agc_process_batch_dev(d._h, buf.data_ptr(), 100, n + 4, buf.data_ptr(), n + 6, None) == EINVAL
    assert L.qdsp_hip_agc_process_batch_dev(d._h, buf.data_ptr(), 100, n + 4, buf.data_ptr() + 4, n + 4, None) == EINVAL


def test_same_call_twice_gives_the_same_bits(torch):
    nchan, n = 64, LONG
    g = torch.Generator(device="cuda").manual_seed(5)
    xf = torch.randn((nchan, n), device="cuda", generator=g)
    agc = ops.Agc(50.0, 48_000.0, nchan=nchan)
    agc.set_level(0.125)
    y1 = agc.process_batch(xf).clone()
    assert agc.last_kernel()["name"] == APPLY
    l1 = [agc.level(c) for c in range(nchan)]
    agc.set_level(0.125)
    y2 = agc.process_batch(xf)
    assert torch.equal(bits(y1), bits(y2)) and l1 == [agc.level(c) for c in range(nchan)]
    xc = torch.view_as_complex(torch.randn((nchan, n, 2), device="cuda", generator=g)) * torch.linspace(0.01, 2.0, nchan, device="cuda")[:, None]
    sq = ops.Squelch(-6.0, nchan=nchan)
    z1 = sq.process_batch(xc).clone()
    assert sq.last_kernel()["name"] == APPLY
    o1 = [sq.is_open(c) for c in range(nchan)]
    z2 = sq.process_batch(xc)
    assert torch.equal(bits(z1), bits(z2)) and o1 == [sq.is_open(c) for c in range(nchan)] and any(o1) and not all(o1)


# ---- 8. argument errors, harness helpers -----------------------------------------------------------------------------------------
def test_argument_errors(torch):
    L = capi.load()
    h = C.c_void_p()
    for nchan, mb in ((0, 10), (70_000, 10), (1, -5)):
        assert L.qdsp_hip_squelch_create(C.byref(h), 0, nchan, mb) == EINVAL
        assert L.qdsp_hip_agc_create(C.byref(h), 0, nchan, mb) == EINVAL
    sq2, sq1 = ops.Squelch(-50.0, nchan=2, max_block=100), ops.Squelch(-50.0, max_block=100)
    ag2, ag1 = ops.Agc(1.0, 48e3, nchan=2, max_block=100), ops.Agc(1.0, 48e3, max_block=100)
    x = np.zeros((101, 2), np.float32)
    y = np.zeros((101, 2), np.float32)
    for p, one, two in (("qdsp_hip_squelch", sq1, sq2), ("qdsp_hip_agc", ag1, ag2)):
        proc, ex = getattr(L, p + "_process"), getattr(L, p + "_process_ex")
        assert proc(one._h, x.ctypes.data, 101, y.ctypes.data) == ESIZE
        assert proc(one._h, x.ctypes.data, -1, y.ctypes.data) == EINVAL
        assert proc(one._h, x.ctypes.data, 0, y.ctypes.data) == 0
        assert proc(two._h, x.ctypes.data, 10, y.ctypes.data) == EINVAL             # host path: one channel
        assert ex(one._h, x.ctypes.data, 7, 10, y.ctypes.data, 0) == EINVAL
        assert ex(one._h, x.ctypes.data, 0, 10, y.ctypes.data, 3) == EINVAL           # deferred without an event
    inf, nan = float("inf"), float("nan")
    for fall, sr in ((1.0, 0.0), (1.0, -48e3), (1.0, inf), (1.0, nan), (inf, 48e3), (nan, 48e3)):
        assert L.qdsp_hip_agc_set(ag1._h, 0, fall, sr) == EINVAL, (fall, sr)
    assert L.qdsp_hip_agc_set(ag2._h, 2, 1.0, 48e3) == EINVAL and L.qdsp_hip_agc_set(ag2._h, -1, -3.0, 48e3) == 0
    assert L.qdsp_hip_squelch_set_level(sq2._h, 2, -10.0) == EINVAL and L.qdsp_hip_squelch_set_level(sq2._h, -1, -10.0) == 0
    p, o = C.c_float(), C.c_int()
    assert L.qdsp_hip_agc_get_level(ag2._h, 2, C.byref(p)) == EINVAL and L.qdsp_hip_agc_get_level(ag2._h, 0, None) == EINVAL
    assert L.qdsp_hip_agc_set_level(ag2._h, 5, 1.0) == EINVAL
    assert L.qdsp_hip_squelch_get_open(sq2._h, -1, C.byref(o)) == EINVAL and L.qdsp_hip_squelch_get_open(sq2._h, 0, None) == EINVAL
    xt = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    yt = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    for bd, two, mis in ((L.qdsp_hip_squelch_process_batch_dev, sq2, 4), (L.qdsp_hip_agc_process_batch_dev, ag2, 2)):
        assert bd(two._h, xt.data_ptr(), 400, 399, yt.data_ptr(), 400, None) == EINVAL
        assert bd(two._h, xt.data_ptr(), 400, 400, yt.data_ptr(), 300, None) == EINVAL
        assert bd(two._h, xt.data_ptr() + mis, 10, 10, yt.data_ptr(), 10, None) == EINVAL
        assert bd(two._h, xt.data_ptr(), 10, 10, yt.data_ptr() + mis, 10, None) == EINVAL
        assert bd(two._h, xt.data_ptr(), -1, 10, yt.data_ptr(), 10, None) == EINVAL
        assert bd(two._h, None, 10, 10, yt.data_ptr(), 10, None) == EINVAL
        assert bd(two._h, xt.data_ptr(), 10, 10, None, 10, None) == EINVAL
        assert bd(two._h, xt.data_ptr(), 0, 0, yt.data_ptr(), 0, None) == 0
    # handle kinds do not mix, in either direction
    fm, de = ops.FmDemod(250e3, 75e3), ops.Deemp(48e3, 50e-6)
    ssb = ops.SsbDemod(48_000.0, 3_000.0, 0)
    fir = ops.Fir(np.ones(8, np.float32))
    args = (xt.data_ptr(), 10, yt.data_ptr(), None)
    for other in (fm, de, ssb, fir, ag1):
        assert L.qdsp_hip_squelch_process_dev(other._h, *args) == EINVAL
        assert L.qdsp_hip_squelch_reset(other._h) == EINVAL and L.qdsp_hip_squelch_set_level(other._h, 0, 1.0) == EINVAL
        assert L.qdsp_hip_squelch_get_open(other._h, 0, C.byref(o)) == EINVAL
    for other in (fm, de, ssb, fir, sq1):
        assert L.qdsp_hip_agc_process_dev(other._h, *args) == EINVAL
        assert L.qdsp_hip_agc_reset(other._h) == EINVAL and L.qdsp_hip_agc_set(other._h, 0, 1.0, 1.0) == EINVAL
        assert L.qdsp_hip_agc_get_level(other._h, 0, C.byref(p)) == EINVAL and L.qdsp_hip_agc_set_level(other._h, 0, 1.0) == EINVAL
    for mine in (sq1, ag1):
        assert L.qdsp_hip_demod_process_dev(mine._h, *args) == EINVAL and L.qdsp_hip_demod_reset(mine._h) == EINVAL
        assert L.qdsp_hip_deemp_process_dev(mine._h, *args) == EINVAL and L.qdsp_hip_deemp_reset(mine._h) == EINVAL
        assert L.qdsp_hip_ssb_cf32_process_dev(mine._h, *args) == EINVAL
        assert L.qdsp_hip_fir_cf32_process_dev(mine._h, *args) == EINVAL
    torch.cuda.synchronize()


def test_done_event_and_time(torch):
    L = capi.load()
    ev = C.c_void_p()
    capi.check(L.qdsp_hip_event_create(0, C.byref(ev)))
    n = 1 << 20
    for op, x in ((ops.Squelch(-50.0), torch.view_as_complex(torch.randn((n, 2), device="cuda"))), (ops.Agc(1.0, 48e3), torch.randn(n, device="cuda"))):
        assert L.qdsp_hip_set_done_event(op._h, ev) == 0
        assert op.time_dev(x, torch.empty_like(x), 3) > 0
        assert op.last_kernel() == {"name": APPLY, "grid": 512, "block": 256, "lds_bytes": 256 * (8 if x.is_complex() else 4)}
        hx = x[:1000].cpu().numpy()
        hy = np.empty_like(hx)
        op.process_ex(hx.ctypes.data, 0, 1000, hy.ctypes.data, 3)                # host out, deferred: the event is there now
        assert op.last_kernel()["name"] == ROW
        want = hx if x.is_complex() else hx * F32(F32(1.0) / op.level())         # (open at -50 dB; the level of the long row stands)
        assert _same_bits(hy.view(F32), want.view(F32))
    capi.check(L.qdsp_hip_event_destroy(ev))


# ---- 9. the block graph ------------------------------------------------------------------------------------------------------------
N, BLOCK, DECIM = 240_000, 24_000, 10
VFO_ARGS = ["300000", "2400000", "240000", "200000"]    # offset, inSR, outSR, bandwidth: 2.4 Msps -> 240 ksps


@pytest.fixture(scope="module")
def graph(tmp_path_factory):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL, timeout=300)
    d = tmp_path_factory.mktemp("levelgraph")
    x = O.synth_iq(0, N, seed=42)
    x[N // 2:] *= np.float32(0.1)                   # the second half 20 dB weaker
    x.tofile(d / "x.cf32")
    subprocess.run([BIN, "vfo", str(d / "x.cf32"), str(d / "v.cf32"), str(BLOCK)] + VFO_ARGS, check=True, timeout=180,
                   capture_output=True, text=True)
    v = np.fromfile(d / "v.cf32", dtype=np.complex64)
    assert len(v) == N // DECIM
    return d, v


def run_graph(d, mode, link, param):
    out = d / f"{mode}_{link}.bin"
    r = subprocess.run([BIN, mode, link, str(d / "x.cf32"), str(out), str(BLOCK)] + VFO_ARGS + [param],
                       check=True, timeout=180, capture_output=True, text=True)
    assert "graph ok" in r.stdout and f"{link if link == 'host' else 'device'} link" in r.stdout
    return out


@pytest.mark.parametrize("link", ["dev", "host"])
def test_vfo_then_squelch_blocks(graph, link):
    d, v = graph
    vb = BLOCK // DECIM
    db = [float(squelch_mean_db(v[a:a + vb])) for a in range(0, len(v), vb)]
    loud, quiet = min(db[:len(db) // 2]), max(db[len(db) // 2 + 1:])
    assert loud - quiet > 8                         # (10 log10 of a mean MAGNITUDE: a tenth of the amplitude is 10 of these dB)
    level = 0.5 * (loud + quiet)
    y = np.fromfile(run_graph(d, "squelch", link, repr(level)), dtype=np.complex64)
    assert len(y) == len(v)
    sq = ops.Squelch(float(np.float32(level)), max_block=vb)
    opened = []
    for a in range(0, len(v), vb):                  # one run() per VFO output block
        assert _same_bits(y[a:a + vb].view(F32), sq.process(v[a:a + vb]).view(F32)), a
        opened.append(sq.is_open())
        assert opened[-1] == squelch_ref(v[a:a + vb], np.float32(level))[1]
    assert opened[0] and not opened[-1] and opened == sorted(opened, reverse=True), "the gate closes mid-stream"
    assert np.any(y[:vb]) and not np.any(y[-vb:].view(np.uint32))


@pytest.mark.parametrize("link", ["dev", "host"])
def test_am_then_agc_blocks(graph, link):
    d, v = graph
    vb = BLOCK // DECIM
    y = np.fromfile(run_graph(d, "agc", link, "2400"), dtype=np.float32)
    assert len(y) == len(v)
    am = ops.AmDemod(max_block=vb)
    agc = ops.Agc(2400.0, 240_000.0, max_block=vb)
    levels = []
    for a in range(0, len(v), vb):
        assert _same_bits(y[a:a + vb], agc.process(am.process(v[a:a + vb]))), a
        levels.append(float(agc.level()))
    assert levels[0] > 2 * levels[-1] > 0 and float(np.max(y)) <= 1.0
