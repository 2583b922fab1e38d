"""StereoFMDemod on the GPU (qdsp_amd/csrc/stereo_fm.hip): the pilot filter against the FP64 reference under the filter families'
yardstick rule, the determinism rule of its contract bit for bit, the matrix and the AGC level against `stereo_mix_ref`
(tests/test_stereo_fm_cpu.py), state, NaN locality, argument errors, and the C++ block against the operator."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _numerics import FLOOR, K, direct_fma32, fir_ref64, region_check
from qdsp_amd import capi, ops
from test_demod_cpu import fm_ref, phasor_speed
from test_level_cpu import F32, _same_bits, agc_exact_decay, decay_error_ratio
from test_stereo_fm_cpu import (MIN_PEAK_CALL, PEAK_MARGIN, RATES, TAPS, TILE, call_sizes, cfr_of, deviation_of, pilot_taps, recipe,
                                stereo_matrix, stereo_mix_ref)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "demod_check")
EINVAL, ESIZE = -10001, -10003
DECAY_COUNTS = [1, 7]          # appended to every stream: short calls after a long one
REGIME_GAP = 1e-3              # a call whose pilot maximum is within this of the decayed level may go either way on the device


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def sizes_of(T):
    return call_sizes(T) + DECAY_COUNTS


def stream(T, nchan):
    """(iq [nchan, n] complex64, cuts): channel c is the recipe with seed c, cut at the same places."""
    rows = [recipe(T, seed=c, sizes=tuple(sizes_of(T))) for c in range(nchan)]
    return np.stack([r[0] for r in rows]), rows[0][2]


def make(T, nchan=1, **kw):
    return ops.StereoFmDemod(RATES[T], deviation_of(T), nchan=nchan, pilot_taps=pilot_taps(T), **kw)


def run_calls(torch, sfm, xt, cuts, fm=None):
    """The stream through `sfm` call by call (rows of the padded tensor xt): per call (out, pilot, level per channel, m)."""
    res = []
    for a, b in zip(cuts, cuts[1:]):
        y = sfm.process_batch(xt[:, a:b]).cpu().numpy()
        f = sfm.pilot().cpu().numpy()
        lv = np.array([sfm.level(c) for c in range(sfm.nchan)], F32)
        m = fm.process_batch(xt[:, a:b]).cpu().numpy() if fm is not None else None
        res.append((y, f, lv, m))
    return res


# ---- 1. the pilot filter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [1, 3])
@pytest.mark.parametrize("T", TAPS)
def test_pilot_filter_against_the_fp64_reference(torch, T, nchan):
    iq, cuts = stream(T, nchan)
    xt = torch.from_numpy(iq).cuda()
    sfm = make(T, nchan)
    fm = ops.FmDemod(RATES[T], deviation_of(T), nchan=nchan)
    res = run_calls(torch, sfm, xt, cuts, fm)
    assert sfm.last_kernel()["name"] == "stereo_mix_kernel"
    taps = pilot_taps(T)
    pos = np.arange(cuts[-1])
    regions = {f"call {k} ({b - a})": (pos >= a) & (pos < b) for k, (a, b) in enumerate(zip(cuts, cuts[1:])) if b - a >= MIN_PEAK_CALL}
    regions["stream"] = np.ones(cuts[-1], bool)           # (with the calls of 1 to 7 samples, too few for a measure of their own)
    for c in range(nchan):
        m = np.concatenate([r[3][c] for r in res])
        f = np.concatenate([r[1][c] for r in res])
        assert f.shape == m.shape == (cuts[-1],)
        ok, rep = region_check(f, direct_fma32(taps, m), fir_ref64(taps, m), regions, k=K, floor=FLOOR)
        worst = max(rep.values(), key=lambda v: v["ratio"])
        print(f"T={T} nchan={nchan} channel {c}: worst rms ratio to the yardstick {worst['ratio']:.3f} (bound {K})")
        assert ok, {k: v for k, v in rep.items() if not v["ok"]}


# ---- 2. the determinism rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TAPS)
def test_pilot_bits_do_not_depend_on_cuts_channel_alignment_or_stride(torch, T):
    iq3, cuts = stream(T, 3)
    row, n = iq3[0], cuts[-1]
    base = make(T)
    base.process_batch(torch.from_numpy(row).cuda().view(1, -1))
    want = base.pilot().cpu().numpy()[0]                      # one call, one channel, aligned, contiguous
    assert want.shape == (n,)

    def pilot_of(sfm, xt, cs, chan):
        return np.concatenate([r[1][chan] for r in run_calls(torch, sfm, xt, cs)])

    one = torch.from_numpy(row).cuda().view(1, -1)
    assert _same_bits(pilot_of(make(T), one, cuts, 0), want), "the mixed cuts"
    other = sorted({0, 1, 7, 64, T + 64, TILE - 1, TILE + T, 3 * TILE + 1, n})
    assert _same_bits(pilot_of(make(T), one, other, 0), want), "other cuts"
    # channel 2 of 3 (channels 0 and 1 carry other streams)
    x3 = torch.from_numpy(np.stack([iq3[1], iq3[2], row])).cuda()
    assert _same_bits(pilot_of(make(T, 3), x3, cuts, 2), want), "channel 2 of 3"
    # rows that start 8 bytes past a 16-byte boundary, and rows on it: the tensor below holds the stream from complex sample 1
    buf = torch.zeros(n + 5, dtype=torch.complex64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[1:n + 1] = one[0]
    odd = buf[1:n + 1].view(1, -1)
    assert odd.data_ptr() % 16 == 8
    even_cuts = [0] + [c for c in (2048, 4096 + 2 * (T // 2)) if c < n] + [n]
    assert all(c % 2 == 0 for c in even_cuts[:-1])
    assert _same_bits(pilot_of(make(T), odd, even_cuts, 0), want), "every row 8 bytes off"
    assert _same_bits(pilot_of(make(T), one, even_cuts, 0), want), "every row aligned"
    # padded rows (stride n + 5) against contiguous ones (every call its own contiguous copy)
    sfm, got = make(T), []
    for a, b in zip(cuts, cuts[1:]):
        sfm.process_batch(one[:, a:b].contiguous())
        got.append(sfm.pilot().cpu().numpy()[0])
    assert _same_bits(np.concatenate(got), want), "contiguous calls"
    # the same with three rows, where the row stride is used: contiguous slices (stride = count) against the padded ones above,
    # outputs included (the stride terms of fm_demod_kernel and stereo_mix_kernel)
    pad, con = make(T, 3), make(T, 3)
    got = []
    for a, b in zip(cuts, cuts[1:]):
        xc = x3[:, a:b].contiguous()
        assert xc.stride(0) == b - a and (x3[:, a:b].stride(0) == n or b - a == n)
        yc = con.process_batch(xc).cpu().numpy()
        got.append(con.pilot().cpu().numpy()[2])
        assert _same_bits(yc, pad.process_batch(x3[:, a:b]).cpu().numpy()), ("padded and contiguous rows", a, b)
        assert _same_bits(con.pilot().cpu().numpy(), pad.pilot().cpu().numpy())
    assert _same_bits(np.concatenate(got), want), "channel 2 of 3, contiguous calls"


# ---- 3. the matrix and the AGC ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [1, 3])
@pytest.mark.parametrize("T", TAPS)
def test_matrix_and_level_against_the_restatement(torch, T, nchan):
    iq, cuts = stream(T, nchan)
    xt = torch.from_numpy(iq).cuda()
    sfm = make(T, nchan)
    fm = ops.FmDemod(RATES[T], deviation_of(T), nchan=nchan)
    assert all(sfm.level(c) == 0 for c in range(nchan))
    cfr = cfr_of(RATES[T])
    prev = np.zeros(nchan, F32)
    peaks = 0
    for k, (y, f, lv, m) in enumerate(run_calls(torch, sfm, xt, cuts, fm)):
        n = cuts[k + 1] - cuts[k]
        for c in range(nchan):
            want, ref_lvl = stereo_mix_ref(m[c], f[c], prev[c], cfr)
            dec = float(agc_exact_decay(prev[c], cfr, n)[0]) if prev[c] > 0 else 0.0
            peak = float(f[c].max())
            if n >= MIN_PEAK_CALL:
                assert peak >= PEAK_MARGIN * dec * (1 - 1e-4), ("the recipe's peak regime", T, k, n, peak, dec)
            if peak > dec * (1 + REGIME_GAP):                       # peak regime: everything bit for bit
                peaks += 1
                assert _same_bits([lv[c]], [ref_lvl]) and lv[c] == F32(peak), (T, k, c, lv[c], ref_lvl)
                assert _same_bits(y[c], want), (T, k, c)
            else:                                                   # the decayed level stands (or the call is too close to tell)
                near = peak >= dec * (1 - REGIME_GAP)
                ratio = float(decay_error_ratio(lv[c], prev[c], cfr, n))
                assert ratio <= 1.0 or (near and lv[c] == F32(peak)), (T, k, c, n, prev[c], lv[c], ratio)
                assert _same_bits(y[c], stereo_matrix(m[c], f[c], lv[c])), (T, k, c)
        prev = lv
    assert peaks >= nchan * len([s for s in sizes_of(T) if s >= MIN_PEAK_CALL])


@pytest.mark.parametrize("T", [5, 193])
def test_decay_regime_after_a_long_call(torch, T):
    sizes = (3 * TILE + 5, 1, 7, 7, 1)
    iq, _, cuts = recipe(T, seed=3, sizes=sizes)
    xt = torch.from_numpy(iq).cuda().view(1, -1)
    sfm, fm = make(T), ops.FmDemod(RATES[T], deviation_of(T))
    cfr = cfr_of(RATES[T])
    first = run_calls(torch, sfm, xt, cuts[:2], fm)[0]
    assert first[2][0] == F32(first[1][0].max()) > 0
    sfm.set_level(float(first[2][0]) * 8.0)                          # eight times the pilot's crest: what follows can only decay
    prev = sfm.level()
    assert prev == F32(float(first[2][0]) * 8.0)
    for k, (y, f, lv, m) in enumerate(run_calls(torch, sfm, xt, cuts[1:], fm)):
        n = sizes[k + 1]
        assert f[0].max() < 0.5 * lv[0] < lv[0] < prev, "decay regime"
        ratio = float(decay_error_ratio(lv[0], prev, cfr, n))
        print(f"T={T} n={n}: level {prev} -> {lv[0]}, |error| / bound {ratio:.3f}")
        assert ratio <= 1.0, (T, k, prev, lv[0])
        assert _same_bits(y[0], stereo_matrix(m[0], f[0], lv[0])), (T, k)
        prev = lv[0]
    # from level 0 with no positive pilot sample: f * inf
    z = make(T)
    y = z.process(np.ones(40, np.complex64))                          # a constant phase: m = 0 after the first sample, f -> 0
    y = z.process(np.ones(40, np.complex64))
    assert z.level() == 0 and np.all(np.isnan(y)), "0 * inf = NaN in every output"


# ---- 4. state -------------------------------------------------------------------------------------------------------------------
def test_state(torch):
    T = 193
    iq, _, cuts = recipe(T, seed=0, sizes=(500, 700, 300))
    xt = torch.from_numpy(iq).cuda().view(1, -1)
    fs, dev, taps = RATES[T], deviation_of(T), pilot_taps(T)
    fresh = [(r[0], r[1], r[2]) for r in run_calls(torch, make(T), xt, cuts)]
    # reset: phase, history and level back to 0
    sfm = make(T)
    run_calls(torch, sfm, xt, cuts)
    assert sfm.get_phase() != 0 and sfm.level() > 0
    sfm.reset()
    assert sfm.get_phase() == 0 and sfm.level() == 0 and sfm.pilot().shape == (1, 0)
    again = run_calls(torch, sfm, xt, cuts)
    for (y, f, lv, _), (y0, f0, lv0) in zip(again, fresh):
        assert _same_bits(y, y0) and _same_bits(f, f0) and _same_bits(lv, lv0)
    # set_pilot_taps: the history alone
    sfm = make(T)
    a = run_calls(torch, sfm, xt, cuts[:2])[0]
    ph, lv = sfm.get_phase(), sfm.level()
    sfm.set_pilot_taps(taps)
    assert _same_bits([sfm.get_phase()], [ph]) and _same_bits([sfm.level()], [lv])
    fm = ops.FmDemod(fs, dev)
    fm.set_phase(float(ph))
    m = fm.process(xt[0, cuts[1]:cuts[2]]).cpu().numpy()
    y = sfm.process(xt[0, cuts[1]:cuts[2]]).cpu().numpy()
    f = sfm.pilot().cpu().numpy()[0]
    ok, rep = region_check(f, direct_fma32(taps, m), fir_ref64(taps, m), {"all": np.ones(len(m), bool)})     # (zero history)
    assert ok, rep
    assert not _same_bits(f, fresh[1][1][0]), "the carried history would have shown"
    want, lvl = stereo_mix_ref(m, f, lv, cfr_of(fs))
    assert _same_bits(y, want) and _same_bits([sfm.level()], [lvl])
    # other taps, another length
    t5 = pilot_taps(5)
    sfm.set_pilot_taps(t5)
    assert sfm.ntaps == 5
    fm.set_phase(float(sfm.get_phase()))
    m = fm.process(xt[0, :500]).cpu().numpy()
    sfm.process(xt[0, :500])
    ok, rep = region_check(sfm.pilot().cpu().numpy()[0], direct_fma32(t5, m), fir_ref64(t5, m), {"all": np.ones(500, bool)})
    assert ok, rep
    # set_phase / get_phase / set_level / get_level
    p = make(T, 3)
    p.set_phase(0.25)
    p.set_phase(-1.5, 1)
    p.set_level(2.0)
    p.set_level(0.125, 2)
    assert [float(p.get_phase(c)) for c in range(3)] == [0.25, -1.5, 0.25] and [float(p.level(c)) for c in range(3)] == [2.0, 2.0, 0.125]
    q = make(T)
    q.set_phase(-1.5)
    q.set_level(2.0)
    x3 = torch.from_numpy(np.stack([iq[:500]] * 3)).cuda()
    y3 = p.process_batch(x3).cpu().numpy()
    assert _same_bits(y3[1], q.process(xt[0, :500]).cpu().numpy()) and _same_bits([p.level(1), p.get_phase(1)], [q.level(), q.get_phase()])
    # per-channel set_fm: channel 1 at another rate and deviation equals a handle of its own
    p, q = make(T, 2), make(T)
    p.set_fm(96_000.0, 10_000.0, 1)
    q.set_fm(96_000.0, 10_000.0)
    x2 = torch.from_numpy(np.stack([iq, iq])).cuda()
    for a_, b_ in zip(cuts, cuts[1:]):
        y2 = p.process_batch(x2[:, a_:b_]).cpu().numpy()
        y1 = q.process_batch(xt[:, a_:b_]).cpu().numpy()
        assert _same_bits(y2[1], y1[0]) and not _same_bits(y2[0], y1[0])
        assert _same_bits([p.level(1)], [q.level()]) and p.level(0) != p.level(1)
    # the host entry point: the bits of the device entry point
    h = make(T, max_block=1000)
    for (a_, b_), (y0, f0, lv0) in zip(zip(cuts, cuts[1:]), fresh):
        yh = h.process(iq[a_:b_])
        assert yh.shape == (b_ - a_, 2) and _same_bits(yh, y0[0]) and _same_bits([h.level()], lv0)
        assert _same_bits(h.pilot().cpu().numpy(), f0)
    assert len(h.process(np.zeros(0, np.complex64))) == 0 and _same_bits([h.level()], fresh[-1][2])      # count 0: a no-op


def test_done_event_time_and_last_kernel(torch):
    L = capi.load()
    T, n = 193, 1 << 16
    sfm = make(T, 4)
    x = torch.from_numpy(np.tile(recipe(T, sizes=(n,))[0], (4, 1))).cuda()
    out = torch.empty((4, n, 2), dtype=torch.float32, device="cuda")
    assert sfm.time_dev(x, out, 3) > 0
    assert sfm.last_kernel() == {"name": "stereo_mix_kernel", "grid": n // TILE, "block": 256, "lds_bytes": 1024}
    assert sfm.pilot().shape == (4, n)
    ev = C.c_void_p()
    capi.check(L.qdsp_hip_event_create(0, C.byref(ev)))
    one = make(T)
    assert L.qdsp_hip_set_done_event(one._h, ev) == 0
    hx = x[0, :1000].cpu().numpy()
    hy = np.empty((1000, 2), F32)
    one.process_ex(hx.ctypes.data, 0, 1000, hy.ctypes.data, 3)           # host out, deferred
    assert _same_bits(hy, make(T).process(hx))
    capi.check(L.qdsp_hip_event_destroy(ev))


# ---- 5. NaN locality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TAPS)
def test_nan_locality_and_sentinels(torch, T):
    L = capi.load()
    n1 = n2 = TILE + 101 + 4 * T                          # (1 mod 4: three floats of padding behind every scratch row)
    i = n1 - max(3, T - 5)                                # the poisoned span [i, i + T] ends 3 to 6 samples into the second call
    # The level stays what it was only if the poisoned samples do not hold a call's pilot maximum: channel 1 takes the first recipe
    # seed whose maxima (FP64, on the restated demodulator) lie outside the span with 2 % to spare.
    for seed1 in range(1, 40):
        x1 = recipe(T, seed=seed1, sizes=(n1, n2))[0]
        f64 = fir_ref64(pilot_taps(T), fm_ref(x1, phasor_speed(RATES[T], deviation_of(T)))[0])
        if f64[i:n1].max() < 0.98 * f64[:i].max() and f64[n1:i + T + 1].max() < 0.98 * f64[i + T + 1:].max():
            break
    else:
        raise AssertionError("no recipe seed keeps the maxima out of the span")
    iq = np.stack([recipe(T, seed=0, sizes=(n1, n2))[0], x1, recipe(T, seed=50, sizes=(n1, n2))[0]])
    bad = iq.copy()
    bad[1, i] = np.nan + 0j
    SENT = float(np.float32(-7.25e11))
    runs = {}
    for name, x in (("clean", iq), ("nan", bad)):
        sfm = make(T, 3)
        xt = torch.from_numpy(x).cuda()
        outs, pil, lvs = [], [], []
        for k, (a, b) in enumerate(((0, n1), (n1, n1 + n2))):
            guard = torch.full((3, (b - a) + 16, 2), SENT, dtype=torch.float32, device="cuda")
            y = sfm.process_batch(xt[:, a:b], out=guard[:, 8:8 + (b - a)])
            outs.append(y.cpu().numpy())
            g = guard.cpu().numpy()
            assert np.all(g[:, :8] == F32(SENT)) and np.all(g[:, 8 + (b - a):] == F32(SENT)), "sentinels around every output row"
            pil.append(sfm.pilot().cpu().numpy())
            lvs.append([sfm.level(c) for c in range(3)])
            if k == 0:                                    # plant sentinels behind every pilot row; the second call must leave them
                p, stride = sfm.pilot_ptr()
                assert stride == n1 + 3 and p % 16 == 0
                s3 = np.full(3, SENT, F32)
                for c in range(3):
                    capi.check(L.qdsp_hip_memcpy_h2d(0, p + 4 * (c * stride + n1), s3.ctypes.data, 12))
        p2, stride2 = sfm.pilot_ptr()
        assert (p2, stride2) == (p, stride)
        pads = np.empty(3 * stride, F32)
        capi.check(L.qdsp_hip_memcpy_d2h(0, pads.ctypes.data, p, pads.nbytes))
        assert np.all(pads.reshape(3, stride)[:, n2:] == F32(SENT)), "sentinels behind every pilot row"
        runs[name] = (np.concatenate(outs, axis=1), np.concatenate(pil, axis=1), np.array(lvs, F32))
    (yc, fc, lc), (yn, fn, ln) = runs["clean"], runs["nan"]
    assert np.all(np.isfinite(yc)) and np.all(np.isfinite(fc))
    span = np.zeros(n1 + n2, bool)
    span[i:i + T + 1] = True
    assert np.array_equal(~np.isfinite(fn[1]), span), "the pilot is NaN exactly under the two poisoned samples of m"
    assert np.array_equal(~np.isfinite(yn[1]).all(axis=1), span) and np.array_equal(~np.isfinite(yn[1]).any(axis=1), span)
    for c in (0, 2):
        assert _same_bits(yn[c], yc[c]) and _same_bits(fn[c], fc[c])
    assert _same_bits(ln, lc), "a NaN never wins the maximum: every level as in the clean run"
    # outside the span channel 1 differs from the clean run only through nothing at all: same level, same m, same f
    assert _same_bits(yn[1][~span], yc[1][~span])


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors(torch):
    L = capi.load()
    h = C.c_void_p()
    taps = np.ones(4097, F32)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
    for nchan, nt, mb, t in ((1, 0, 10, tp), (1, 4097, 10, tp), (1, -3, 10, tp), (0, 5, 10, tp), (65_536, 5, 10, tp), (1, 5, -1, tp), (1, 5, 10, None)):
        assert L.qdsp_hip_stereo_fm_create(C.byref(h), 0, nchan, t, nt, mb) == EINVAL, (nchan, nt, mb)
        assert not h.value
    assert L.qdsp_hip_stereo_fm_create(None, 0, 1, tp, 5, 10) == EINVAL
    one, two = make(5, max_block=100), make(5, 2, max_block=100)
    x, y = np.zeros((101, 2), F32), np.zeros((101, 2), F32)
    proc, ex = L.qdsp_hip_stereo_fm_process, L.qdsp_hip_stereo_fm_process_ex
    assert proc(one._h, x.ctypes.data, 101, y.ctypes.data) == ESIZE
    assert proc(one._h, x.ctypes.data, -1, y.ctypes.data) == EINVAL
    assert proc(one._h, x.ctypes.data, 0, y.ctypes.data) == 0
    assert proc(two._h, x.ctypes.data, 10, y.ctypes.data) == EINVAL                    # host path: one channel
    assert ex(one._h, x.ctypes.data, 7, 10, y.ctypes.data, 0) == EINVAL
    assert ex(one._h, x.ctypes.data, 0, 10, y.ctypes.data, 3) == EINVAL                  # deferred without an event
    assert L.qdsp_hip_stereo_fm_set_pilot_taps(one._h, tp, 0) == EINVAL and L.qdsp_hip_stereo_fm_set_pilot_taps(one._h, tp, 4097) == EINVAL
    assert L.qdsp_hip_stereo_fm_set_pilot_taps(one._h, None, 5) == EINVAL
    inf, nan = float("inf"), float("nan")
    for sr, dv in ((0.0, 1.0), (-48e3, 1.0), (inf, 1.0), (nan, 1.0), (48e3, nan), (48e3, inf), (48e3, 0.0)):
        assert L.qdsp_hip_stereo_fm_set_fm(one._h, 0, sr, dv) == EINVAL, (sr, dv)
    assert L.qdsp_hip_stereo_fm_set_fm(two._h, 2, 48e3, 5e3) == EINVAL and L.qdsp_hip_stereo_fm_set_fm(two._h, -1, 48e3, 5e3) == 0
    v = C.c_float()
    for get, set_ in ((L.qdsp_hip_stereo_fm_get_phase, L.qdsp_hip_stereo_fm_set_phase), (L.qdsp_hip_stereo_fm_get_level, L.qdsp_hip_stereo_fm_set_level)):
        assert get(two._h, 2, C.byref(v)) == EINVAL and get(two._h, -1, C.byref(v)) == EINVAL and get(two._h, 0, None) == EINVAL
        assert set_(two._h, 2, 1.0) == EINVAL
    pp, st = C.c_void_p(), C.c_int64()
    assert L.qdsp_hip_stereo_fm_pilot_dev(two._h, None, C.byref(st)) == EINVAL and L.qdsp_hip_stereo_fm_pilot_dev(two._h, C.byref(pp), None) == EINVAL
    xt = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    yt = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    bd = L.qdsp_hip_stereo_fm_process_batch_dev
    assert bd(two._h, xt.data_ptr(), 400, 399, yt.data_ptr(), 400, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 400, 400, yt.data_ptr(), 300, None) == EINVAL
    assert bd(two._h, xt.data_ptr() + 4, 10, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 10, 10, yt.data_ptr() + 4, 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), -1, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, None, 10, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 10, 10, None, 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 0, 0, yt.data_ptr(), 0, None) == 0
    # input and output that overlap: in place, and by one sample at either end
    assert bd(two._h, xt.data_ptr(), 100, 100, xt.data_ptr(), 100, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 100, 100, xt.data_ptr() + 8 * 199, 100, None) == EINVAL
    assert bd(two._h, xt.data_ptr() + 8 * 199, 100, 100, xt.data_ptr(), 100, None) == EINVAL
    # nothing was launched: no state moved, no pilot rows, and the next call equals a fresh handle's
    torch.cuda.synchronize()
    assert two.level(0) == 0 and two.get_phase(1) == 0 and two.pilot_ptr() == (0, 0)
    assert bd(two._h, xt.data_ptr(), 100, 100, xt.data_ptr() + 8 * 200, 100, None) == 0        # (adjacent is not overlapping)
    # handle kinds do not mix, in either direction
    fm, agc, fir = ops.FmDemod(250e3, 75e3), ops.Agc(1.0, 48e3), ops.Fir(np.ones(8, np.float32))
    args = (xt.data_ptr(), 10, yt.data_ptr(), None)
    for other in (fm, agc, fir):
        assert L.qdsp_hip_stereo_fm_process_dev(other._h, *args) == EINVAL and L.qdsp_hip_stereo_fm_reset(other._h) == EINVAL
        assert L.qdsp_hip_stereo_fm_set_fm(other._h, 0, 48e3, 5e3) == EINVAL and L.qdsp_hip_stereo_fm_get_level(other._h, 0, C.byref(v)) == EINVAL
    assert L.qdsp_hip_demod_process_dev(one._h, *args) == EINVAL and L.qdsp_hip_agc_process_dev(one._h, *args) == EINVAL
    assert L.qdsp_hip_fir_f32_process_dev(one._h, *args) == EINVAL and L.qdsp_hip_demod_reset(one._h) == EINVAL
    torch.cuda.synchronize()


# ---- 7. the C++ block -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [2048, 4099])
def test_stereo_block_equals_the_operator(torch, tmp_path, block):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST, "build/demod_check"], stdout=subprocess.DEVNULL, timeout=300)
    T = 193
    fs, dev = RATES[T], deviation_of(T)
    iq = recipe(T, seed=5, sizes=(4099, 4099, 4099, 2048, 1000))[0]
    iq.tofile(tmp_path / "x.cf32")
    r = subprocess.run([BIN, "sfm", str(tmp_path / "x.cf32"), str(tmp_path / "y.bin"), str(block), repr(fs), repr(dev)],
                       check=True, timeout=180, capture_output=True, text=True)
    assert "graph ok" in r.stdout and f"{T} pilot taps" in r.stdout, r.stdout
    y = np.fromfile(tmp_path / "y.bin", dtype=F32).reshape(-1, 2)
    op = ops.StereoFmDemod(fs, dev)                              # the default taps: the reference's for this rate
    assert op.ntaps == T
    want = np.concatenate([op.process(iq[a:a + block]) for a in range(0, len(iq), block)])
    assert y.shape == want.shape and _same_bits(y, want)
