"""FM / FM stereo / AM / SSB demodulators on the GPU (qdsp_hip_demod_*, qdsp_hip_ssb_cf32_*) against the float32 restatement of
src/dsp/demodulator.h that tests/test_demod_cpu.py pins to the C++ reference arithmetic: FM bit for bit (call boundaries,
non-finite inputs, 2^28-sample calls and 64 batched channelizer channels included), AM to the ulp, SSB bit for bit against the
xlator's real part."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from qdsp_amd import capi, ops
from test_demod_cpu import _same_bits, am_mag, edge_vectors, fast_arctan2, fm_ref, phasor_speed

pytestmark = pytest.mark.gpu

SR, DEV = 250_000.0, 75_000.0
EINVAL, ESIZE = -10001, -10003


def rand_iq(n, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def ulp(v):
    return np.spacing(np.abs(np.float32(v))).astype(np.float32)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def cuts_of(n, sizes=(1, 7, 4096, 65_537)):
    c = [0]
    for s in sizes:
        c.append(min(n, c[-1] + s))
    return c + [n]


# ---- FM ----------------------------------------------------------------------------------------------------------------------
def test_fm_float_bit_exact_across_ragged_calls(torch):
    n = 1 << 20
    x = rand_iq(n)
    want, _ = fm_ref(x, phasor_speed(SR, DEV))
    assert _same_bits(ops.FmDemod(SR, DEV, max_block=n).process(x), want)
    cuts = cuts_of(n)
    d = ops.FmDemod(SR, DEV, max_block=n)
    assert _same_bits(np.concatenate([d.process(x[a:b]) for a, b in zip(cuts, cuts[1:])]), want)
    # the same on the device path (unaligned rows after the odd cuts: the scalar loads)
    xt = torch.from_numpy(x).cuda()
    dd = ops.FmDemod(SR, DEV)
    y = torch.cat([dd.process(xt[a:b]) for a, b in zip(cuts, cuts[1:])]).cpu().numpy()
    assert _same_bits(y, want)
    assert dd.last_kernel()["name"] == "fm_demod_kernel"


def test_fm_stereo_is_the_float_output_twice(torch):
    n = 300_001
    x = rand_iq(n, 2)
    want, _ = fm_ref(x, phasor_speed(48_000.0, 5_000.0))
    y = ops.FmDemod(48_000.0, 5_000.0, stereo=True, max_block=n).process(x)
    assert y.shape == (n, 2) and _same_bits(y[:, 0], want) and _same_bits(y[:, 1], want)
    yd = ops.FmDemod(48_000.0, 5_000.0, stereo=True).process(torch.from_numpy(x).cuda()).cpu().numpy()
    assert _same_bits(yd[:, 0], want) and _same_bits(yd[:, 1], want)


def test_fm_edge_vectors(torch):
    mark = np.asarray([0.5 + 0.5j, complex(np.nan, 0.25), 0.3 + 0.1j, 0.2 - 0.4j], np.complex64)
    x = np.concatenate([edge_vectors(), mark, rand_iq(1000, 3), edge_vectors()[::-1]])
    want, last = fm_ref(x, phasor_speed(SR, DEV))
    d = ops.FmDemod(SR, DEV)
    y = d.process(x)
    assert _same_bits(y, want)
    assert np.array_equal(np.isfinite(y), np.isfinite(want))
    # a NaN sample poisons its own output and the next one, nothing else
    k = len(edge_vectors()) + 1
    assert np.isnan(y[k]) and np.isnan(y[k + 1]) and np.isfinite(y[k + 2]) and np.isfinite(y[k - 1])
    assert _same_bits([d.get_phase()], [last])
    yd = ops.FmDemod(SR, DEV).process(torch.from_numpy(x).cuda()).cpu().numpy()
    assert _same_bits(yd, want)


def test_fm_recovers_a_tone():
    fs, dev, f = 250_000.0, 75_000.0, 1_000.0
    n = 200_000
    t = np.arange(n) / fs
    m = np.sin(2 * np.pi * f * t)
    x = np.exp(1j * 2 * np.pi * dev * np.cumsum(m) / fs).astype(np.complex64)
    y = ops.FmDemod(fs, dev, max_block=n).process(x)
    assert np.corrcoef(y[1:], m[1:])[0, 1] > 0.99
    gain = np.dot(y[1:], m[1:]) / np.dot(m[1:], m[1:])      # (fast_arctan2's octant error ripples around the tone: peaks of ~1.06)
    assert abs(gain - 1.0) < 0.01


def test_fm_device_path_runs_without_host_sync(torch):
    n = 3_000_000
    xt = torch.from_numpy(rand_iq(n, 4)).cuda()
    one = ops.FmDemod(SR, DEV).process(xt).cpu().numpy()
    d = ops.FmDemod(SR, DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y1 = d.process(xt[:1_234_567])
        y2 = d.process(xt[1_234_567:])
    s.synchronize()
    assert _same_bits(torch.cat([y1, y2]).cpu().numpy(), one)
    want, last = fm_ref(xt.cpu().numpy(), phasor_speed(SR, DEV))
    assert _same_bits(one, want)
    assert _same_bits([d.get_phase()], [last])
    d.reset()
    assert d.get_phase() == 0
    d.set_phase(float(last))
    y3 = d.process(xt[:1000]).cpu().numpy()
    assert _same_bits(y3, fm_ref(xt[:1000].cpu().numpy(), phasor_speed(SR, DEV), last)[0])


def test_fm_full_size_call(torch):
    n = (1 << 28) + 12_345                 # 2^31 + 98 760 input bytes
    x = ops.synth_iq(n, seed=99)
    d = ops.FmDemod(SR, DEV)
    y = d.process(x)
    torch.cuda.synchronize()
    sp = phasor_speed(SR, DEV)
    for a in (0, n // 2 - 777, n - 70_001):
        b = min(n, a + 70_001)
        xw = x[max(a - 1, 0):b].cpu().numpy()
        prev = np.float32(0) if a == 0 else fast_arctan2(xw[:1].imag, xw[:1].real)[0]
        want, _ = fm_ref(xw[1:] if a else xw, sp, prev)
        assert _same_bits(y[a:b].cpu().numpy(), want), a
    del x, y
    torch.cuda.empty_cache()


def test_fm_batched_on_channelizer_output(torch):
    nchan, M = 64, 64
    taps = O.lowpass_taps_f64(256, 1.0 / 64.0)
    incs = [ops.phase_delta(1.0, -(c - 31.5) / 64.0) for c in range(nchan)]
    chn = ops.Channelizer(taps, 1, M, incs, max_block=0)
    devs = np.asarray([1_000.0 + 250.0 * c for c in range(nchan)], np.float32)
    fm = ops.FmDemod(SR / M, devs, nchan=nchan)
    singles = [ops.FmDemod(SR / M, float(devs[c])) for c in range(nchan)]
    phases = [np.float32(0)] * nchan
    for call, n in enumerate((64 * 4099, 64 * 2000 + 64 * 7)):
        x = ops.synth_iq(n, first_sample=call * 10**7, seed=5)
        no = chn.out_size(n)
        buf = torch.empty((nchan, no + 37), dtype=torch.complex64, device="cuda")   # out_stride > count, odd: scalar loads
        yc = chn.process(x, buf)
        assert yc.stride(0) == no + 37 and yc.shape[1] == no
        y = fm.process_batch(yc).cpu().numpy()
        assert fm.last_kernel()["name"] == "fm_demod_kernel" and fm.last_kernel()["grid"] > 0
        yh = yc.cpu().numpy()
        for c in range(nchan):
            want, phases[c] = fm_ref(yh[c], phasor_speed(SR / M, devs[c]), phases[c])
            assert _same_bits(y[c], want), (call, c)
            ys = singles[c].process(yc[c].contiguous()).cpu().numpy()
            assert _same_bits(ys, want), (call, c)
    # aligned rows (even stride): the vector loads
    x = ops.synth_iq(64 * 4096, seed=6)
    yc = chn.process(x)
    fa = ops.FmDemod(SR / M, devs, nchan=nchan)
    y = fa.process_batch(yc).cpu().numpy()
    yh = yc.cpu().numpy()
    for c in (0, 17, 63):
        assert _same_bits(y[c], fm_ref(yh[c], phasor_speed(SR / M, devs[c]))[0])


# ---- AM ----------------------------------------------------------------------------------------------------------------------
def _check_am(y, x):
    m = am_mag(x)
    mu = np.mean(m.astype(np.float64))
    avg = np.float32(np.median(m.astype(np.float64) - y.astype(np.float64)))
    assert np.all(np.abs((y + avg) - m) <= ulp(np.maximum(m, avg))), "out + avg != |x|"
    assert abs(np.float64(avg) - mu) <= ulp(mu)
    assert np.max(np.abs(y.astype(np.float64) - (m - mu))) <= 2 * ulp(np.max(m))


def test_am(torch):
    x = rand_iq(1_000_000, 8)
    d = ops.AmDemod(max_block=1_000_000)
    _check_am(d.process(x), x)
    assert d.last_kernel()["name"] == "am_sub_kernel"
    yd = ops.AmDemod().process(torch.from_numpy(x).cuda()).cpu().numpy()
    _check_am(yd, x)
    # every call subtracts its own mean
    a, b = x[:1000] * np.float32(3), x[1000:4000]
    ya, yb = d.process(a), d.process(b)
    _check_am(ya, a)
    _check_am(yb, b)
    assert abs(np.mean(ya)) < 1e-5 and abs(np.mean(yb)) < 1e-5
    assert np.array_equal(d.process(x[:1]), np.zeros(1, np.float32))
    # batched: per-channel means
    nchan, n = 5, 70_001
    xs = np.stack([rand_iq(n, 20 + c) * np.float32(c + 1) for c in range(nchan)])
    xt = torch.zeros((nchan, n + 3), dtype=torch.complex64, device="cuda")
    xt[:, :n] = torch.from_numpy(xs).cuda()
    y = ops.AmDemod(nchan=nchan).process_batch(xt, count=n).cpu().numpy()
    for c in range(nchan):
        _check_am(y[c], xs[c])
    # 2^27 samples: 1024 partials per channel
    big = ops.synth_iq(1 << 27, seed=3)
    yb = ops.AmDemod().process(big)
    w = slice((1 << 26) - 5000, (1 << 26) + 5000)
    m = am_mag(big[w].cpu().numpy())
    avg = np.float32(np.median(m.astype(np.float64) - yb[w].cpu().numpy()))
    mu = float(torch.sqrt(big.real.double() ** 2 + big.imag.double() ** 2).mean())
    assert abs(float(avg) - mu) <= 2 * ulp(mu)


# ---- SSB ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [ops.SsbDemod.USB, ops.SsbDemod.LSB, ops.SsbDemod.DSB])
@pytest.mark.parametrize("volk_gain", [True, False])
def test_ssb_is_the_xlators_real_part(torch, mode, volk_gain):
    sr, bw = 48_000.0, 2_700.0
    inc = ops.ssb_phase_delta(sr, bw, mode)
    n = 400_003
    x = ops.synth_iq(n, seed=11).cpu().numpy()
    s = ops.SsbDemod(sr, bw, mode, max_block=n)
    xl = ops.Xlator(phase_inc=inc, max_block=n)
    s.set_volk_gain(volk_gain)
    xl.set_volk_gain(volk_gain)
    cuts = cuts_of(n, (1, 7, 4096, 100_000))
    y = np.concatenate([s.process(x[a:b]) for a, b in zip(cuts, cuts[1:])])
    w = np.concatenate([xl.process(x[a:b]) for a, b in zip(cuts, cuts[1:])])
    assert _same_bits(y, w.real)
    assert s.last_kernel()["name"] == "ssb_demod_kernel"
    if mode == ops.SsbDemod.DSB:
        assert np.array_equal(y, x.real)
    elif volk_gain:
        o = O.Xlator(1.0, 0.0, exact=True, volk_gain=True)
        o.delta[:] = inc
        wo = np.concatenate([o.process(x[a:b]) for a, b in zip(cuts, cuts[1:])])
        assert np.abs(y - wo.real).max() < 6e-7
    # device path, phase carried: the same as the xlator's
    sd, xd = ops.SsbDemod(sr, bw, mode), ops.Xlator(phase_inc=inc)
    xt = torch.from_numpy(x).cuda()
    yd = torch.cat([sd.process(xt[:12_345]), sd.process(xt[12_345:])]).cpu().numpy()
    wd = torch.cat([xd.process(xt[:12_345]), xd.process(xt[12_345:])]).cpu().numpy()
    assert _same_bits(yd, wd.real)
    assert sd.get_phase() == xd.get_phase()


# ---- harness helpers and argument errors ---------------------------------------------------------------------------------------
def test_done_event_and_time(torch):
    L = capi.load()
    ev = C.c_void_p()
    capi.check(L.qdsp_hip_event_create(0, C.byref(ev)))
    xt = ops.synth_iq(1 << 20, seed=1)
    for op, out in ((ops.FmDemod(SR, DEV), torch.empty(1 << 20, device="cuda")),
                    (ops.FmDemod(SR, DEV, stereo=True), torch.empty((1 << 20, 2), device="cuda")),
                    (ops.AmDemod(), torch.empty(1 << 20, device="cuda")),
                    (ops.SsbDemod(48_000.0, 3_000.0, 0), torch.empty(1 << 20, device="cuda"))):
        assert L.qdsp_hip_set_done_event(op._h, ev) == 0
        assert op.time_dev(xt, out, 3) > 0
    capi.check(L.qdsp_hip_event_destroy(ev))


def test_argument_errors(torch):
    L = capi.load()
    h = C.c_void_p()
    assert L.qdsp_hip_demod_create(C.byref(h), 0, 3, 1, 100) == EINVAL       # SSB is not a demod_create kind
    assert L.qdsp_hip_demod_create(C.byref(h), 0, -1, 1, 100) == EINVAL
    assert L.qdsp_hip_demod_create(C.byref(h), 0, 0, 0, 100) == EINVAL
    assert L.qdsp_hip_demod_create(C.byref(h), 0, 0, 1, -5) == EINVAL
    assert L.qdsp_hip_ssb_cf32_create(C.byref(h), 0, 0.0, 0.0, 100) == EINVAL
    fm = ops.FmDemod(SR, DEV, nchan=2, max_block=100)
    one = ops.FmDemod(SR, DEV, max_block=100)
    am = ops.AmDemod(max_block=100)
    x = np.zeros(101, np.complex64)
    y = np.zeros(101, np.float32)
    assert L.qdsp_hip_demod_process(one._h, x.ctypes.data, 101, y.ctypes.data) == ESIZE
    assert L.qdsp_hip_demod_process(fm._h, x.ctypes.data, 10, y.ctypes.data) == EINVAL          # host path: one channel
    assert L.qdsp_hip_demod_process_ex(one._h, x.ctypes.data, 7, 10, y.ctypes.data, 0) == EINVAL
    assert L.qdsp_hip_demod_process_ex(one._h, x.ctypes.data, 0, 10, y.ctypes.data, 3) == EINVAL  # deferred without an event
    assert L.qdsp_hip_demod_set_fm(fm._h, 2, 1.0, 1.0) == EINVAL
    assert L.qdsp_hip_demod_set_fm(fm._h, 0, 1.0, 0.0) == EINVAL
    assert L.qdsp_hip_demod_set_fm(am._h, 0, 1.0, 1.0) == EINVAL
    p = C.c_float()
    assert L.qdsp_hip_demod_get_phase(am._h, 0, C.byref(p)) == EINVAL
    assert L.qdsp_hip_demod_get_phase(fm._h, 2, C.byref(p)) == EINVAL
    ssb = ops.SsbDemod(48_000.0, 3_000.0, 0)
    assert L.qdsp_hip_demod_process_dev(ssb._h, 0, 0, 0, None) == EINVAL                          # handle kinds do not mix
    assert L.qdsp_hip_ssb_cf32_process_dev(one._h, 0, 0, 0, None) == EINVAL
    xt = torch.zeros(1000, dtype=torch.complex64, device="cuda")
    yt = torch.zeros(2000, dtype=torch.float32, device="cuda")
    assert L.qdsp_hip_demod_process_batch_dev(fm._h, xt.data_ptr(), 400, 399, yt.data_ptr(), 400, None) == EINVAL
    assert L.qdsp_hip_demod_process_batch_dev(fm._h, xt.data_ptr(), 400, 400, yt.data_ptr(), 300, None) == EINVAL
    assert L.qdsp_hip_demod_process_batch_dev(fm._h, xt.data_ptr() + 4, 10, 10, yt.data_ptr(), 10, None) == EINVAL
    assert L.qdsp_hip_demod_process_batch_dev(fm._h, xt.data_ptr(), 10, 10, yt.data_ptr() + 2, 10, None) == EINVAL
    ys = torch.zeros((100, 2), dtype=torch.float32, device="cuda")
    st = ops.FmDemod(SR, DEV, stereo=True)
    assert L.qdsp_hip_demod_process_dev(st._h, xt.data_ptr(), 10, ys.data_ptr() + 4, None) == EINVAL
    assert L.qdsp_hip_demod_process_batch_dev(fm._h, xt.data_ptr(), -1, 10, yt.data_ptr(), 10, None) == EINVAL
    torch.cuda.synchronize()
