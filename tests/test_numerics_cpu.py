"""CPU checks of the numerics helpers (tests/_numerics.py) that tests/test_gpu_numerics.py judges the kernels with.

  * the FP64 restatements agree with the oracle's ACC_F64 arithmetic (up to the oracle's own float32 rounding);
  * the FP32 yardsticks pass their own bounds;
  * deliberately broken CPU models FAIL them -- the region metric and the NaN-span check tell a good kernel from a bad one
    without a GPU: (a) real segments paired (p, p + ceil(nseg / 2)) on one complex transform, (b) twiddles rounded to 16
    mantissa bits, (c) a dot product over zero-padded taps that multiplies samples outside the window."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _numerics as NU  # noqa: E402
import oracle as O  # noqa: E402

N_STREAM = 120_000
LOUD_END = 36_000


def _half_ulp_close(ref64, o32):
    """The oracle rounds its FP64 sums to float32 once: within half an ulp of the FP64 value (plus the subnormal range)."""
    d = np.abs(np.asarray(o32).astype(np.complex128) - ref64)
    return bool(np.all(d <= 2.0 ** -24 * np.abs(ref64) * 1.0000001 + 2.0 ** -149))


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("ntaps", [1, 2, 63, 256, 1024])
def test_fir_ref64_matches_oracle(ntaps, real):
    taps = O.lowpass_taps_f64(ntaps, 0.1) if ntaps > 2 else np.array([0.5, -0.25][:ntaps], np.float32)
    x = NU.to32(NU.blocker_stream(20_000, 7_000, 0.31, 0.02, real=real, seed=ntaps))
    o = O.Fir(taps, complex_data=not real, acc=O.ACC_F64)
    f = NU.fir_ref64(taps, x[:9_000])
    hist = x[9_000 - (ntaps - 1): 9_000] if ntaps > 1 else x[:0]
    f = np.concatenate([f, NU.fir_ref64(taps, x[9_000:], hist=hist)])
    want = np.concatenate([o.process(x[:9_000]), o.process(x[9_000:])])
    assert f.dtype == (np.float64 if real else np.complex128) and _half_ulp_close(f, want)


@pytest.mark.parametrize("L,M,ntaps", [(1, 2, 63), (1, 8, 256), (1, 50, 401), (3, 2, 36), (7, 5, 140), (10, 7, 160), (147, 160, 300)])
@pytest.mark.parametrize("real", [False, True])
def test_resampler64_matches_oracle(L, M, ntaps, real):
    taps = (O.lowpass_taps_f64(ntaps, 0.4 / max(L, M)) * L).astype(np.float32)
    x = NU.to32(NU.blocker_stream(30_000, 9_000, 0.37, 0.004, real=real, seed=L + M))
    sizes = [M * 1001, 7, M * 2000 + 3]
    r = NU.Resampler64(taps, L, M, complex_data=not real)
    o = O.Resampler(taps, L, M, complex_data=not real, acc=O.ACC_F64)
    got = NU.run_calls(r.process, x, sizes)
    want = NU.run_calls(o.process, x, sizes)
    assert got.shape == want.shape and _half_ulp_close(got, want)
    first, last = NU.stream_windows(taps, L, M, NU.call_cuts(len(x), sizes))
    assert len(first) == len(got) and np.all(last - first == r.tpp - 1)


def test_nco_reference_is_the_fp64_phase():
    """The NCO reference is exp(j 2 pi f t) in FP64: the oracle's FP64-phase rotator (without VOLK's gain) rounds it once."""
    f = 0.1234
    x = NU.to32(NU.tone(50_000, 0.01, 0.5))
    xl = O.Xlator(1.0, f, exact=True)
    got = xl.process(x)
    step = np.angle(np.complex128(xl.delta[0] + 1j * xl.delta[1])) / (2 * np.pi)
    want = x.astype(np.complex128) * NU.tone(len(x), step)
    assert np.abs(got - want).max() < 2 ** -22 * 0.5


def _stream(real, n=N_STREAM):
    return NU.to32(NU.blocker_stream(n, LOUD_END, 0.37, 0.011, real=real, seed=5))


def _regions(taps, M, n, span):
    first, last = NU.stream_windows(taps, 1, M, [0, n], fir=True)
    return NU.loud_quiet_masks(first, last, LOUD_END, span, n // M)


@pytest.mark.parametrize("N", [1024, 4096])
@pytest.mark.parametrize("M", [1, 4])
@pytest.mark.parametrize("real", [False, True])
def test_overlap_save_yardsticks_are_fp32_sized(N, M, real):
    """Both overlap-save yardsticks are real FP32 implementations: white-noise relative RMS ~1.3e-7 (numpy) and ~2e-7
    (radix-2), each within K x the other there; on the blocker stream the quiet floor follows the weak tone, not the blocker."""
    taps = O.lowpass_taps_f64(256, 0.4 / max(M, 2))
    w = O.synth_iq(0, 200_000, seed=3)
    w = np.ascontiguousarray(w.real) if real else w
    rw = NU.fir_ref64(taps, w)[::M]
    npy, r2 = NU.os_yardsticks(taps, w, N, M)
    for y in (npy, r2):
        assert np.sqrt(np.mean(np.abs(y - rw) ** 2) / np.mean(np.abs(rw) ** 2)) < 4e-7
    everything = {"all": np.ones(len(rw), bool)}
    assert NU.region_check(r2, npy, rw, everything)[0] and NU.region_check(npy, r2, rw, everything)[0]
    x = _stream(real)
    ref = NU.fir_ref64(taps, x)[::M]
    regions = _regions(taps, M, len(x), 3 * N)
    for y in NU.os_yardsticks(taps, x, N, M):
        loud, quiet = NU.region_err(y, ref, regions["loud"]), NU.region_err(y, ref, regions["quiet"])
        assert quiet[1] < 1e-11 < loud[0] < 1e-6, (loud, quiet)


@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("real", [False, True])
def test_direct_yardsticks_agree(M, real):
    """The oracle's ACC_FMA and ACC_SIMD chains and this module's k-ordered chain: each within K x the others' error,
    region by region, and the quiet floor follows the weak tone."""
    taps = O.lowpass_taps_f64(255, 0.4 / max(M, 2))
    x = _stream(real)
    ref = NU.Resampler64(taps, 1, M, complex_data=not real).process(x)
    fma = O.Resampler(taps, 1, M, complex_data=not real, acc=O.ACC_FMA).process(x)
    simd = O.Resampler(taps, 1, M, complex_data=not real, acc=O.ACC_SIMD).process(x)
    mine = NU.direct_fma32(taps, x, M, resamp=True)
    first, last = NU.stream_windows(taps, 1, M, [0, len(x)])
    regions = NU.loud_quiet_masks(first, last, LOUD_END, 0, len(ref))
    for a, b in ((simd, [fma, mine]), (mine, [fma, simd]), (fma, [simd, mine])):
        ok, rep = NU.region_check(a, b, ref, regions)
        assert ok, rep
        assert rep["quiet"]["max"] < 1e-11 < rep["loud"]["rms"], rep


def test_mutant_half_pairing_fails_quiet_bound():
    """(a) Pairing real segment p with p + ceil(nseg / 2) carries the loud segment's FP32 error floor into a quiet one."""
    taps = O.lowpass_taps_f64(256, 0.05)
    x = _stream(True)
    ref = NU.fir_ref64(taps, x)
    yard = NU.os_yardsticks(taps, x, 4096)
    regions = _regions(taps, 1, len(x), 3 * 4096)
    ok_good, rep_good = NU.region_check(NU.os_model(taps, x, 4096, pair="adjacent"), yard, ref, regions)
    ok_bad, rep_bad = NU.region_check(NU.os_model(taps, x, 4096, pair="half"), yard, ref, regions)
    assert ok_good, rep_good
    assert not ok_bad and not rep_bad["quiet"]["ok"] and rep_bad["quiet"]["ratio"] > 50, rep_bad


@pytest.mark.parametrize("pair,ok", [("adjacent", True), ("half", False)])
def test_mutant_half_pairing_fails_nan_span(pair, ok):
    """(a) ... and a NaN at t poisons a whole segment half a call away."""
    taps = O.lowpass_taps_f64(256, 0.05)
    x = _stream(True)
    t = 10_007
    x[t] = np.nan
    y = NU.os_model(taps, x, 4096, pair=pair)
    first, last = NU.stream_windows(taps, 1, 1, [0, len(x)], fir=True)
    missing, stray = NU.poison_check(~np.isfinite(y), first, last, t, 3 * 4096)
    assert len(missing) == 0
    assert (len(stray) == 0) == ok, (pair, len(stray))


def test_mutant_rounded_twiddles_fail_loud_bound():
    """(b) Twiddles rounded to 16 mantissa bits: a ~1e-5 error on loud data that the yardstick bound catches."""
    taps = O.lowpass_taps_f64(256, 0.05)
    x = _stream(False)
    ref = NU.fir_ref64(taps, x)
    yard = NU.os_yardsticks(taps, x, 1024)
    regions = _regions(taps, 1, len(x), 2 * 1024)
    bad = NU.os_model(taps, x, 1024, fft=lambda a: NU.fft_radix2(a, 16), ifft=lambda a: NU.fft_radix2(a, 16, inverse=True))
    ok, rep = NU.region_check(bad, yard, ref, regions)
    assert not ok and not rep["loud"]["ok"], rep


@pytest.mark.parametrize("real", [False, True])
def test_mutant_zero_padded_taps_fail_span(real):
    """(c) A dot product over zero-padded taps reads samples outside the window: 0 * NaN = NaN, one output too many.
    The k-ordered chain on the true taps passes the same check with span 0."""
    taps = O.lowpass_taps_f64(57, 0.1)       # (padded to 64: seven zero taps, so that some output of the decimation by 4 lands on them)
    x = _stream(real, 20_000)
    t = 5_000
    for v in (np.nan, np.inf, -np.inf):
        xx = x.copy()
        xx[t] = v
        first, last = NU.stream_windows(taps, 1, 4, [0, len(x)], fir=True)
        good = NU.direct_fma32(taps, xx, 4)
        m, s = NU.poison_check(~np.isfinite(good), first, last, t, 0)
        assert len(m) == 0 and len(s) == 0
        bad = NU.padded_dot32(taps, xx, 4)
        m, s = NU.poison_check(~np.isfinite(bad), first, last, t, 0)
        assert len(m) == 0 and len(s) > 0, v


def test_generators():
    n = 4096
    assert np.allclose(np.abs(NU.tone(n, 0.1, 0.5)), 0.5)
    b = NU.bin_tone(n, 17, 4096)
    assert np.argmax(np.abs(np.fft.fft(b))) == 17 and np.abs(np.fft.fft(b))[18] < 1e-9 * n
    assert np.array_equal(NU.nyquist(4, real=True), [1.0, -1.0, 1.0, -1.0])
    assert np.all(NU.dc(8, 2.0) == 2.0) and NU.to32(NU.dc(8, 2.0)).dtype == np.complex64
    g = NU.gate(NU.tone(100, 0.1), 10, 20)
    assert np.count_nonzero(g) == 10 and NU.to32(NU.tone(8, 0.1, real=True)).dtype == np.float32


# ------------------------------------------------------------------------------------------------ uniform channelizer
CH_CUTS = {16: [0, 16 * 325, 16 * 327, 16 * 700], 64: [0, 64 * 325, 64 * 327, 64 * 700]}


def _grid_dphase(sign):
    d0 = NU.fx_of_inc(*NU.inc_of_turns(-sign * 31.5 / 64))
    return [(d0 + sign * c * (1 << 58)) & ((1 << 64) - 1) for c in range(64)]


def _rotate_then_filter(taps, dphase, M, x, cuts, chans):
    out = {}
    t = np.arange(len(x), dtype=np.uint64)
    for c in chans:
        with np.errstate(over="ignore"):
            rot = x.astype(np.complex128) * NU.fx_phasor(t * np.uint64(dphase[c]))
        r = NU.Resampler64(taps, 1, M)
        out[c] = np.concatenate([r.process(rot[a:b]) for a, b in zip(cuts, cuts[1:])])
    return out


def test_fx_of_inc_is_the_angle_of_the_rounded_pair():
    for t in (0.0, 0.1234, 0.5, 0.75, 31.5 / 64, 1e-7):
        re, im = NU.inc_of_turns(t)
        got = NU.fx_of_inc(re, im) * 2.0 ** -64
        want = (np.arctan2(np.float64(np.float32(im)), np.float64(np.float32(re))) / (2 * np.pi)) % 1.0
        assert abs((got - want + 0.5) % 1.0 - 0.5) < 1e-15, (t, got, want)
    inv, delta = NU.chan_uniform_plan([NU.fx_of_inc(*p) for p in NU.chan_grid_incs(-1)])
    assert not inv and delta[0] == 0 and 0 < max(abs(d) for d in delta) * 2.0 ** -64 < 1e-7
    inv, delta = NU.chan_uniform_plan([NU.fx_of_inc(*p) for p in NU.chan_grid_incs(+1, detune=3e-7)])
    assert inv and 2.5e-7 < max(abs(d) for d in delta) * 2.0 ** -64 < 3.5e-7
    assert NU.chan_uniform_plan([NU.fx_of_inc(*p) for p in NU.chan_grid_incs(+1, detune=5e-7)]) is None


@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("M,ntaps", [(16, 100), (64, 255)])
def test_chan_uniform_ref64_without_deviation_is_rotate_then_filter(sign, M, ntaps):
    """(a) With every delta_c = 0 the documented operator IS rotate + PolyphaseResampler, to FP64 rounding -- all 64 channels,
    a stream of three calls (one shorter than the taps)."""
    taps = NU.chan_taps(ntaps)
    dphase = _grid_dphase(sign)
    assert NU.chan_uniform_plan(dphase) == (sign > 0, [0] * 64)
    cuts = CH_CUTS[M]
    x = O.synth_iq(0, cuts[-1], seed=21)
    got = NU.chan_uniform_ref64(taps, None, M, x, cuts, dphase=dphase)
    want = _rotate_then_filter(taps, dphase, M, x, cuts, range(64))
    for c in range(64):
        assert np.abs(got[c] - want[c]).max() <= 1e-12 * np.abs(want[c]).max(), c
    # the per-channel operator of the same class (what a bank off the uniform plan computes) is the same thing
    r = NU.ChanUniform64(taps, None, M, dphase=dphase)
    ex = np.concatenate([r.exact(x[a:b]) for a, b in zip(cuts, cuts[1:])], axis=1)
    assert np.abs(ex - got).max() <= 1e-12 * np.abs(got).max()


@pytest.mark.parametrize("detune", [0.0, 3e-7])
def test_chan_uniform_ref64_deviation_is_the_documented_approximation(detune):
    """(b) With real deviations the restated operator differs from rotate-then-filter by the centre-of-window approximation and
    no more: |e^{j 2pi (kc - k) delta} - 1| <= 2pi |delta| ntaps / 2 per tap."""
    M, ntaps = 16, 255
    taps = NU.chan_taps(ntaps)
    incs = NU.chan_grid_incs(-1, detune=detune)
    r = NU.ChanUniform64(taps, incs, M)
    _, delta = r.plan()
    dmax = max(abs(d) for d in delta) * 2.0 ** -64
    assert (2.5e-7 < dmax < 3.5e-7) if detune else (0 < dmax < 1e-7)
    cuts = CH_CUTS[M]
    x = O.synth_iq(0, cuts[-1], seed=22)
    got = NU.chan_uniform_ref64(taps, incs, M, x, cuts)
    want = _rotate_then_filter(taps, r.dphase, M, x, cuts, range(64))
    bound = 2 * np.pi * dmax * ntaps / 2
    worst = 0.0
    for c in range(64):
        d = np.abs(got[c] - want[c])
        assert d.max() <= bound * np.abs(taps.astype(np.float64)).sum() * np.abs(x).max(), c
        rel = np.sqrt(np.mean(d * d) / np.mean(np.abs(want[c]) ** 2))
        assert rel <= bound, (c, rel, bound)
        worst = max(worst, rel)
    assert worst > 1e-3 * bound          # ... and the deviation is really in there (FP64 rounding alone would sit at 1e-16)


def _chan_check_a(taps, incs, M, y, ref, yard, cuts, loud_end, span):
    first, last = NU.chan_uniform_windows(len(taps), M, cuts)
    regions = NU.loud_quiet_masks(first, last, loud_end, span, ref.shape[1])
    bad = []
    for c in range(64):
        ok, rep = NU.region_check(y[c], yard[c], ref[c], regions)
        if not ok:
            bad.append((c, {k: round(v["ratio"], 1) for k, v in rep.items()}))
    return bad, regions


def test_chan_uniform_three_channels_direct_sum():
    """The matrix form of ChanUniform64 against the operator written out tap by tap, three channels."""
    M, ntaps = 8, 37
    taps = NU.chan_taps(ntaps)
    incs = NU.chan_grid_incs(+1, detune=3e-7)
    x = O.synth_iq(0, 8 * 40, seed=23)
    r = NU.ChanUniform64(taps, incs, M)
    r.advance(12345)
    ph, dph = list(r.phase), list(r.dphase)
    _, delta = r.plan()
    y = r.uniform(x)
    kc = (ntaps - 1) // 2
    buf = np.concatenate([np.zeros(ntaps), x.astype(np.complex128)])
    for c in (1, 17, 63):
        for n in (0, 7, 39):
            j0 = n * M - ntaps
            acc = 0
            for k in range(ntaps):
                turns = ((ph[c] + (j0 + k) * (dph[c] - delta[c])) % (1 << 64)) / 2.0 ** 64
                acc += float(taps[k]) * buf[n * M + k] * np.exp(2j * np.pi * turns)
            acc *= np.exp(2j * np.pi * ((((j0 + kc) * delta[c]) % (1 << 64)) / 2.0 ** 64))
            assert abs(acc - y[c, n]) <= 1e-12 * np.abs(y[c]).max(), (c, n)


@pytest.mark.parametrize("M,ntaps,sign,detune", [(64, 100, -1, 0.0), (16, 255, 1, 3e-7)])
def test_chan_uniform_yardstick_and_broken_models(M, ntaps, sign, detune):
    """(c) Check A on the CPU: the FP32 yardstick sits FP32-close to the FP64 operator -- weak-tone-referred in the quiet region,
    blocker-referred in the loud one, the empty channel 40 included -- and three wrong kernels fail the bound: the window centre
    off by one tap (seen on the detuned plan: 2 pi 3e-7 rad is 30 x the FP32 floor), the DFT's branches numbered without the -P
    (seen when P is no multiple of 64), and the other INV sign."""
    taps = NU.chan_taps(ntaps)
    incs = NU.chan_grid_incs(sign, detune=detune)
    cuts = [0, M * 325, M * 327, M * 967, M * 1168]
    n, loud_end = cuts[-1], cuts[-1] // 3
    dphase = [NU.fx_of_inc(*p) for p in incs]
    x = NU.to32(NU.chan_tones(n, dphase, loud_end))
    ref = NU.chan_uniform_ref64(taps, incs, M, x, cuts)
    yard = NU.chan_uniform_yardstick32(taps, incs, M, x, cuts)
    span = 64 * -(-ntaps // 64) - ntaps
    bad, regions = _chan_check_a(taps, incs, M, yard, ref, yard, cuts, loud_end, span)
    assert not bad and regions["loud"].sum() > 300 and regions["quiet"].sum() > 600
    for c in (17, 16, 40, 63):
        loud, quiet = NU.region_err(yard[c], ref[c], regions["loud"]), NU.region_err(yard[c], ref[c], regions["quiet"])
        assert quiet[1] < 1e-11 and loud[0] < 1e-6, (c, loud, quiet)
    assert NU.region_err(yard[17], ref[17], regions["loud"])[0] > 1e-9          # the blocker's own FP32 floor
    broken = {"inv": dict(flip_inv=True)}
    if detune:
        broken["kc"] = dict(kc_off=1)
    if ntaps % 64:
        broken["mu"] = dict(mu_no_P=True)
    for name, kw in broken.items():
        y = NU.chan_uniform_yardstick32(taps, incs, M, x, cuts, **kw)
        bad, _ = _chan_check_a(taps, incs, M, y, ref, yard, cuts, loud_end, span)
        assert bad, name
        assert any(c == 17 for c, _ in bad), (name, bad[:4])
