"""Numerical semantics of every filter kernel family, judged region by region against FP64 references (tests/_numerics.py).

  A. blocker plus weak signal: a 0 dBFS out-of-band blocker in the first part of the stream, a -100 dB in-band tone
     throughout; the loud and the quiet outputs are each held to K x the FP32 yardstick's error there;
  B. NaN / Inf locality: a bad input sample at t poisons every output whose window holds it and nothing farther than
     the family's span (SPAN below); the rest stays finite and right, and the poisoned set does not depend on the call size;
  C. power-of-two scale invariance: y(2^k x) == 2^k y(x) bit for bit (IEEE arithmetic is exactly scale-equivariant unless
     something underflows, overflows or compares against an absolute constant), FM output unchanged;
  D. subnormal inputs: the direct FIR forms stay bit-identical to the k-ordered fmaf chain at 2^-140;
  E. headroom (a measurement): the first power-of-two amplitude of DC / a bin-centred tone where a family's output stops
     being finite or exactly equivariant.  With NUMERICS_REPORT=<file> the measured ratios and headroom go there as JSON.

The uniform channelizer (chan_uniform_kernel) has its own operator, reference and section at the end: checks A-F in every kernel form.

Every family is pinned the way tests/test_gpu_parity.py pins it, and every call's kernel is asserted."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _numerics as NU  # noqa: E402
import oracle as O  # noqa: E402
from conftest import kname, rel_rms  # noqa: E402

pytestmark = pytest.mark.gpu

_REPORT = {"ratios": {}, "headroom": {}, "subnormal_zero_fraction": {}}

# Largest distance (input samples) between a bad sample and an output it may poison beyond the reference's windows.
SPAN = {
    "direct": lambda L, M, nt, N: 0,            # fir_core, fir_lat, decim_win, resamp_any, resamp_lm: exactly the reference's windows
    # decim_mfma(_real): the A operand holds h[M q + r] in 16 (Q > 16: 32) rows q and K = M rounded up to 8 columns, zero outside the
    # prototype's Q = ceil(nt / M) rows.  The zero taps multiply the Q M - nt samples after the window and the K - M of the next row, and
    # a bad sample in the LAST tile of a call also reaches the outputs of the zero rows Q..15 (measured: 7 outputs = 7 M samples before
    # the window at Q = 9, nowhere else in the call) -- 0 * NaN = NaN
    "mfma_dec": lambda L, M, nt, N: ((16 if -(-nt // M) <= 16 else 32) - -(-nt // M)) * M + (-(-nt // M) * M - nt) + (-(-M // 8) * 8 - M),
    # resamp_mfma(_real): four consecutive outputs share one band of columns (3 M / L + P wide); each meets zero taps over the others' part
    "mfma_rm": lambda L, M, nt, N: -(-3 * M // L),
    "os_complex": lambda L, M, nt, N: 2 * N,    # fir_fft (4096), fir_fft1k (1024), pfb_dec8/4 (4096-point segments)
    "os_real": lambda L, M, nt, N: 3 * N,       # two adjacent real segments per complex transform
    # chan_uniform_kernel: the folded taps lie in a table of four rows of 64, zero behind the prototype.  Both forms multiply Q_eff =
    # ceil(nt / 64) rows -- QF = 4 (193..256 taps) all four without a test, QF = 0 the run-time a.Q = ceil(nt / 64) of them, the rows
    # past it are skipped, not multiplied by zero -- so the zero taps nt .. 64 Q_eff - 1 of the last row meet the samples AFTER the window
    "chan_uniform": lambda L, M, nt, N: 64 * -(-nt // 64) - nt,
}

# name, (interp, decim, ntaps), real data?, env, FFT mode?, expected kernel names, span class, transform length
COMMON_ENV = {"QDSP_HIP_MF_MIN_COUNT": "0", "QDSP_HIP_RM_MIN_COUNT": "0", "QDSP_HIP_NO_LM_SMALL_CALL_RULE": "1", "QDSP_HIP_DECIM_SETTING": "0"}
FAM = [
    ("fir_core", (1, 1, 63), False, {}, "direct_mode", {"fir_core_kernel"}, "direct", None),
    ("fir_core_real", (1, 1, 63), True, {}, "direct_mode", {"fir_core_kernel"}, "direct", None),
    ("fir_lat", (1, 1, 63), False, {"QDSP_HIP_FIR_PICK": "1"}, None, {"fir_lat_kernel"}, "direct", None),
    ("fir_fft1k", (1, 1, 256), False, {"QDSP_HIP_FIR_PICK": "3"}, None, {"fir_fft1k_kernel"}, "os_complex", 1024),
    ("fir_fft1k_real", (1, 1, 256), True, {}, None, {"fir_fft1k_kernel"}, "os_real", 1024),
    ("fir_fft", (1, 1, 256), False, {"QDSP_HIP_FFT1K_MAX_COUNT": "0"}, "fft", {"fir_fft_kernel"}, "os_complex", 4096),
    ("fir_fft_real", (1, 1, 256), True, {"QDSP_HIP_FFT1K_MAX_COUNT": "0", "QDSP_HIP_NO_FFT1K_REAL": "1"}, "fft", {"fir_fft_kernel"}, "os_real", 4096),
    ("fir_fft_dec2", (1, 2, 255), False, {"QDSP_HIP_FFT1K_MAX_COUNT": "0", "QDSP_HIP_NO_FFT1K": "1"}, "fft", {"fir_fft_kernel"}, "os_complex", 4096),
    ("fir_fft_dec3", (1, 3, 1000), False, {"QDSP_HIP_FFT1K_MAX_COUNT": "0", "QDSP_HIP_NO_FFT1K": "1"}, "fft", {"fir_fft_kernel"}, "os_complex", 4096),
    ("pfb_dec8", (1, 8, 256), False, {"QDSP_HIP_PFB_MIN_COUNT": "0"}, "fft", {"pfb_dec8_kernel"}, "os_complex", 4096),
    ("pfb_dec4", (1, 4, 256), False, {"QDSP_HIP_PFB_MIN_COUNT": "0"}, "fft", {"pfb_dec4_kernel"}, "os_complex", 4096),
    ("pfb_dec8_real", (1, 8, 256), True, {"QDSP_HIP_PFB_MIN_COUNT": "0"}, "fft", {"pfb_dec8_real_kernel"}, "os_real", 4096),
    ("pfb_dec4_real", (1, 4, 256), True, {"QDSP_HIP_PFB_MIN_COUNT": "0"}, "fft", {"pfb_dec4_real_kernel"}, "os_real", 4096),
    ("decim_win", (1, 4, 63), False, {}, None, {"decim_win_kernel"}, "direct", None),
    ("decim_win_real", (1, 8, 63), True, {}, None, {"decim_win_kernel"}, "direct", None),
    ("decim_mfma", (1, 50, 401), False, {}, None, {"decim_mfma_kernel"}, "mfma_dec", None),
    ("decim_mfma16", (1, 16, 129), False, {}, None, {"decim_mfma_kernel"}, "mfma_dec", None),
    ("decim_mfma_real", (1, 50, 401), True, {}, None, {"decim_mfma_real_kernel"}, "mfma_dec", None),
    ("resamp_any", (7, 5, 140), False, {"QDSP_HIP_NO_RM": "1"}, None, {"resamp_any_kernel"}, "direct", None),
    ("resamp_any_dec", (1, 50, 401), False, {"QDSP_HIP_NO_MF": "1"}, None, {"resamp_any_kernel"}, "direct", None),
    ("resamp_lm", (3, 2, 36), False, {}, None, {"resamp_lm_kernel"}, "direct", None),
    ("resamp_mfma", (10, 7, 160), False, {}, None, {"resamp_mfma_kernel"}, "mfma_rm", None),
    ("resamp_mfma_real", (10, 7, 160), True, {}, None, {"resamp_mfma_real_kernel"}, "mfma_rm", None),
]
FAM_IDS = [f[0] for f in FAM]


@pytest.fixture(scope="module")
def ops():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from qdsp_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("NUMERICS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_REPORT, f, indent=1, sort_keys=True)


def _fft_mode(op):
    op.set_mode(op.FFT)
    return op


def _taps(L, M, ntaps):
    return (O.lowpass_taps_f64(ntaps, 0.4 / max(L, M, 2)) * L).astype(np.float32)


def _pin(monkeypatch, env):
    for k, v in {**COMMON_ENV, **env}.items():
        monkeypatch.setenv(k, v)


def _make(ops, fam, taps):
    name, (L, M, _), real, _, mode, _, _, _ = fam
    op = ops.Fir(taps, complex_data=not real, max_block=0) if (L, M) == (1, 1) else ops.Resampler(taps, L, M, complex_data=not real, max_block=0)
    if mode == "fft":
        op.set_mode(op.FFT)
    elif mode == "direct_mode":
        op.set_mode(op.DIRECT)
    return op


def _run(op, fam, x, cuts):
    import torch

    ys = []
    for a, b in zip(cuts, cuts[1:]):
        ys.append(op.process(torch.from_numpy(np.ascontiguousarray(x[a:b])).cuda()).cpu().numpy())
        got = kname(op)
        assert got in fam[5], (fam[0], b - a, op.last_kernel())
    return np.concatenate(ys)


def _ref64(fam, taps, x, cuts):
    (L, M, _), real = fam[1], fam[2]
    if (L, M) == (1, 1):
        return NU.fir_ref64(taps, x)
    r = NU.Resampler64(taps, L, M, complex_data=not real)
    return np.concatenate([r.process(x[a:b]) for a, b in zip(cuts, cuts[1:])])


def _windows(fam, taps, cuts):
    L, M, _ = fam[1]
    return NU.stream_windows(taps, L, M, cuts, fir=(L, M) == (1, 1))


def _yardsticks(fam, taps, x, cuts):
    (L, M, _), real, N = fam[1], fam[2], fam[7]
    fir = (L, M) == (1, 1)
    if N is not None:          # (call sizes are multiples of M: the stream is one overlap-save run)
        return NU.os_yardsticks(taps, x, N, M, resamp=not fir)
    out = []
    for acc in (O.ACC_FMA, O.ACC_SIMD):
        o = O.Fir(taps, complex_data=not real, acc=acc) if fir else O.Resampler(taps, L, M, complex_data=not real, acc=acc)
        out.append(np.concatenate([o.process(x[a:b]) for a, b in zip(cuts, cuts[1:])]))
    return out


def _span(fam):
    return SPAN[fam[6]](*fam[1], fam[7])


def _os_layout(fam):
    """(L, shift, N) of an overlap-save family as its launcher lays the call out (qdsp_hip.hip): segment b holds the N
    call-relative input positions from b L - shift on (negative: the history)."""
    name, (_, M, nt), N = fam[0], fam[1], fam[7]
    if name.startswith("pfb"):
        PH = 2 if M == 4 else 1
        Q = -(-(nt + M * (PH - 1)) // 8)
        return 8 * (513 - Q), 8 * Q, 4096
    if name.startswith("fir_fft1k"):
        return 1024 - (nt - 1), nt - 1, 1024
    ov = nt & ~1                                # (nt - 1 rounded up to even)
    if M == 1:
        return 4096 - ov, ov, 4096
    if M in (2, 4, 8, 16):
        ov = -(-(nt - 1) // M) * M
        return 4096 - ov, ov + 1, 4096
    return 4096 - ov, ov + 2, 4096


# ------------------------------------------------------------------------------------------------ A. blocker + weak tone
N_A, LOUD_END = 600_000, 60_000
CUTS_A = [0, 240_000, 441_600, N_A]          # (multiples of 1200 and 64: every decimation here consumes whole calls)


@pytest.mark.parametrize("fam", FAM, ids=FAM_IDS)
def test_blocker_and_weak_tone_regions(ops, monkeypatch, fam):
    _pin(monkeypatch, fam[3])
    L, M, ntaps = fam[1]
    taps = _taps(L, M, ntaps)
    # blocker far out of band (past every cutoff here), weak tone well inside the pass band
    x = NU.to32(NU.blocker_stream(N_A, LOUD_END, 0.43, 0.05 / max(L, M, 2), real=fam[2], seed=len(fam[0])))
    y = _run(_make(ops, fam, taps), fam, x, CUTS_A)
    ref = _ref64(fam, taps, x, CUTS_A)
    assert y.shape == ref.shape
    first, last = _windows(fam, taps, CUTS_A)
    regions = NU.loud_quiet_masks(first, last, LOUD_END, _span(fam), len(ref))
    assert regions["quiet"].sum() > len(ref) // 2
    yards = _yardsticks(fam, taps, x, CUTS_A)
    ok, rep = NU.region_check(y, yards, ref, regions)
    _REPORT["ratios"][fam[0]] = {k: round(v["ratio"], 3) for k, v in rep.items()}
    if fam[7] is not None:     # (on record: the ratio against numpy's complex64 overlap-save alone)
        _REPORT.setdefault("ratios_numpy_only", {})[fam[0]] = {k: round(v["ratio"], 3) for k, v in NU.region_check(y, yards[0], ref, regions)[1].items()}
    assert ok, (fam[0], rep)


def test_fused_vfo_blocker_and_weak_tone(ops, monkeypatch):
    """The fused VFO on the polyphase kernel (pfb_dec8_kernel<ROT>): blocker and weak tone placed around the NCO offset."""
    _pin(monkeypatch, {"QDSP_HIP_PFB_MIN_COUNT": "0"})
    taps = _taps(1, 8, 256)
    f0 = 0.1234
    x = NU.to32(NU.gate(NU.tone(N_A, 0.43, 1.0), 0, LOUD_END) + NU.tone(N_A, -f0 + 0.01, 1e-5) + NU.tone(N_A, f0 + 0.01, 1e-5))
    op = ops.Vfo(taps, 1, 8, ops.phase_delta(1.0, f0), max_block=0)
    op.set_mode(op.FFT)
    fam = ("vfo", (1, 8, 256), False, {}, "fft", {"pfb_dec8_kernel"}, "os_complex", 4096)
    y = _run(op, fam, x, CUTS_A)
    xl = O.Xlator(1.0, f0, exact=True, volk_gain=True)
    xr = np.concatenate([xl.process(x[a:b]) for a, b in zip(CUTS_A, CUTS_A[1:])])
    ref = _ref64(fam, taps, xr, CUTS_A)
    first, last = _windows(fam, taps, CUTS_A)
    regions = NU.loud_quiet_masks(first, last, LOUD_END, _span(fam), len(ref))
    ok, rep = NU.region_check(y, _yardsticks(fam, taps, xr, CUTS_A), ref, regions)
    _REPORT["ratios"]["vfo_pfb_dec8"] = {k: round(v["ratio"], 3) for k, v in rep.items()}
    assert ok, rep


# ------------------------------------------------------------------------------------------------ B. NaN / Inf locality
def _poison_positions(fam, n_call):
    """Call-relative offsets, placed in the second call: its first sample, the last of the call before, a sample inside the
    overlap of the call's segments 1 and 2 (overlap-save forms: it reaches two transforms -- the real forms: two pairs), ~10 %."""
    if fam[7] is not None:
        L, shift, N = _os_layout(fam)
        ov = 2 * L - shift + 3
        assert L - shift <= ov < L - shift + N and 2 * L - shift <= ov < 2 * L - shift + N      # in segment 1 and in segment 2
    else:
        ov = 2 * 3840 + 7                       # (the direct forms have no segments: any interior sample)
    return {"first": n_call, "last": n_call - 1, "overlap": n_call + ov, "tenth": n_call + n_call // 10}


def _poison_input(fam, n_call, where, value, comp):
    x = O.synth_iq(0, 3 * n_call, seed=7)
    x = np.ascontiguousarray(x.real) if fam[2] else x.copy()
    t = _poison_positions(fam, n_call)[where]
    if fam[2]:
        x[t] = value
    elif comp == "re":
        x[t] = complex(value, x[t].imag)
    else:
        x[t] = complex(x[t].real, value)
    return x, t


def _poison_run(ops, fam, taps, n_call, where, value, comp):
    cuts = [0, n_call, 2 * n_call, 3 * n_call]
    x, t = _poison_input(fam, n_call, where, value, comp)
    x0, _ = _poison_input(fam, n_call, where, 0.0, comp)
    y = _run(_make(ops, fam, taps), fam, x, cuts)
    first, last = _windows(fam, taps, cuts)
    return y, x0, t, cuts, first, last


@pytest.mark.parametrize("fam", FAM, ids=FAM_IDS)
def test_nan_inf_locality(ops, monkeypatch, fam):
    _pin(monkeypatch, fam[3])
    L, M, ntaps = fam[1]
    taps = _taps(L, M, ntaps)
    span = _span(fam)
    n_call = 96_000                             # (a multiple of every decimation here: the stream is one overlap-save run)
    cuts = [0, n_call, 2 * n_call, 3 * n_call]
    comps = ["re"] if fam[2] else ["re", "im"]
    for where in ("first", "last", "overlap", "tenth"):
        for comp in comps:
            x0, t = _poison_input(fam, n_call, where, 0.0, comp)
            ref0 = _ref64(fam, taps, x0, cuts)
            yard0 = _yardsticks(fam, taps, x0, cuts)
            for value in (np.nan, np.inf, -np.inf):
                y, _, _, _, first, last = _poison_run(ops, fam, taps, n_call, where, value, comp)
                bad = ~np.isfinite(y)
                missing, stray = NU.poison_check(bad, first, last, t, span)
                assert len(missing) == 0, (fam[0], where, value, comp, missing[:8])
                assert len(stray) == 0, (f"{fam[0]}: {len(stray)} outputs beyond the span {span}, up to "
                                         f"{int(np.max(np.maximum(first[stray] - t, t - last[stray])))} samples away ({where} {value} {comp})")
                # everything farther than the span: finite and inside the region bound against the reference with t set to 0
                far = np.maximum(0, np.maximum(first - t, t - last)) > span
                ok, rep = NU.region_check(y, yard0, ref0, {"far": far})
                assert ok, (fam[0], where, value, comp, rep)
                assert np.isfinite(y[2 * len(y) // 3:]).all()      # the third call has left t behind
    # the poisoned set, relative to t, does not depend on the call size (t at the same offset from its call's start)
    for where in ("first", "overlap"):
        sets = []
        for n in (n_call, 4 * n_call):
            y, _, t, _, first, last = _poison_run(ops, fam, taps, n, where, np.nan, "re")
            sets.append(sorted((last[~np.isfinite(y)] - t).tolist()))
        assert sets[0] == sets[1], (fam[0], where, len(sets[0]), len(sets[1]))


# ------------------------------------------------------------------------------------------------ C. scale invariance
SCALES = (-60, -20, 20, 60, 100)


def _same_scaled(a, b, k):
    """a == 2^k b bit for bit (as float32 arrays)."""
    a = np.asarray(a).view(np.float32) if np.iscomplexobj(a) else np.asarray(a, np.float32)
    b = np.asarray(b).view(np.float32) if np.iscomplexobj(b) else np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a, np.ldexp(b, k).astype(np.float32))


@pytest.mark.parametrize("fam", FAM, ids=FAM_IDS)
def test_power_of_two_scale_invariance(ops, monkeypatch, fam):
    _pin(monkeypatch, fam[3])
    L, M, ntaps = fam[1]
    taps = _taps(L, M, ntaps)
    x = O.synth_iq(0, 200_000, seed=11)
    x = np.ascontiguousarray(x.real) if fam[2] else x
    cuts = [0, 120_000, 200_000]
    y = _run(_make(ops, fam, taps), fam, x, cuts)
    for k in SCALES:
        yk = _run(_make(ops, fam, taps), fam, np.ldexp(x.view(np.float32), k).view(x.dtype), cuts)
        assert _same_scaled(yk, y, k), (fam[0], k, np.flatnonzero(yk.view(np.float32) != np.ldexp(y.view(np.float32), k))[:8])


def test_scale_invariance_nco_channelizer_demod(ops, monkeypatch):
    import torch

    _pin(monkeypatch, {"QDSP_HIP_PFB_MIN_COUNT": "0"})

    x = O.synth_iq(0, 131_072, seed=12)
    inc = ops.phase_delta(1.0, 0.1234)
    taps = _taps(1, 8, 256)
    offs = [(c - 31.5) / 64 for c in range(64)]
    makers = {
        "xlate_kernel": lambda: ops.Xlator(phase_inc=inc, max_block=0),
        "pfb_dec8_kernel": lambda: _fft_mode(ops.Vfo(taps, 1, 8, inc, max_block=0)),
        "chan_uniform_kernel": lambda: ops.Channelizer(taps, 1, 16, [ops.phase_delta(1.0, -f) for f in offs], max_block=len(x)),
        "ssb": lambda: ops.SsbDemod(48_000.0, 3_000.0, 0, max_block=0),
    }
    for name, mk in makers.items():
        op = mk()
        y = np.array(op.process(torch.from_numpy(x).cuda()).cpu()) if "chan" not in name else np.array(op.process(x))
        assert name == "ssb" or kname(op) == name, (name, op.last_kernel())
        for k in SCALES:
            xk = np.ldexp(x.view(np.float32), k).view(np.complex64)
            op = mk()
            yk = np.array(op.process(torch.from_numpy(xk).cuda()).cpu()) if "chan" not in name else np.array(op.process(xk))
            assert name == "ssb" or kname(op) == name, (name, op.last_kernel())
            assert _same_scaled(yk, y, k), (name, k)
    fm = ops.FmDemod(48_000.0, 5_000.0, max_block=0).process(torch.from_numpy(x).cuda()).cpu().numpy()
    for k in SCALES:
        xk = np.ldexp(x.view(np.float32), k).view(np.complex64)
        fk = ops.FmDemod(48_000.0, 5_000.0, max_block=0).process(torch.from_numpy(xk).cuda()).cpu().numpy()
        assert np.array_equal(fk, fm), ("fm", k)


# ------------------------------------------------------------------------------------------------ D. subnormal inputs
@pytest.mark.parametrize("fam", FAM, ids=FAM_IDS)
def test_subnormal_inputs(ops, monkeypatch, fam):
    _pin(monkeypatch, fam[3])
    L, M, ntaps = fam[1]
    taps = _taps(L, M, ntaps)
    x = O.synth_iq(0, 100_000, seed=13)
    x = np.ascontiguousarray(x.real) if fam[2] else x
    xs = np.ldexp(x.view(np.float32), -140).view(x.dtype)
    assert np.count_nonzero(np.abs(xs) < 2.0 ** -126) > len(xs) // 2
    cuts = [0, 60_000, 100_000]
    y = _run(_make(ops, fam, taps), fam, xs, cuts)
    if fam[0] in ("fir_core", "fir_core_real", "fir_lat"):
        o = O.Fir(taps, complex_data=not fam[2], acc=O.ACC_FMA)
        want = np.concatenate([o.process(xs[a:b]) for a, b in zip(cuts, cuts[1:])])
        assert np.array_equal(y, want), fam[0]
    ref = _ref64(fam, taps, xs, cuts)
    assert np.isfinite(y).all()
    assert np.abs(y - ref).max() <= 2.0 ** -120 * np.abs(taps.astype(np.float64)).sum(), fam[0]
    _REPORT["subnormal_zero_fraction"][fam[0]] = float(np.mean(y == 0))
    # a path that flushed denormals would return zeros: the outputs that are zero stay as rare as in the direct forms (< 2 %)
    assert np.mean(y == 0) < 0.05, (fam[0], float(np.mean(y == 0)))


# ------------------------------------------------------------------------------------------------ E. headroom
@pytest.mark.parametrize("fam", FAM, ids=FAM_IDS)
def test_headroom_measurement(ops, monkeypatch, fam):
    """Not an assertion on the figure: the first power of two (log2 amplitude) of DC / a tone on bin 17 of a 4096-point
    transform at which the output stops being finite or exactly equivariant, searched from 2^100 to 2^128 (check C already
    holds every family exact at 2^100 on unit-scale noise); None: exact up to the largest finite input power."""
    _pin(monkeypatch, fam[3])
    L, M, ntaps = fam[1]
    taps = _taps(L, M, ntaps)
    n = 100_000
    cuts = [0, n]
    res = {}
    for sig, x64 in (("dc", NU.dc(n, real=fam[2])), ("bin_tone", NU.bin_tone(n, 17, 4096, real=fam[2]))):
        x = NU.to32(x64)
        y0 = _run(_make(ops, fam, taps), fam, x, cuts)
        first_bad = None
        for e in range(100, 129):
            xe = np.ldexp(x.view(np.float32), e).view(x.dtype) if not fam[2] else np.ldexp(x, e).astype(np.float32)
            if not np.isfinite(xe).all():
                break
            ye = _run(_make(ops, fam, taps), fam, xe, cuts)
            if not (np.isfinite(ye).all() and _same_scaled(ye, y0, e)):
                first_bad = e
                break
        res[sig] = first_bad
    _REPORT["headroom"][fam[0]] = res


# ------------------------------------------------------------------------------------------------ channelizer (batched VFOs)
# Channelizer with arbitrary offsets: all channels in one launch of the MFMA decimator or of the general direct kernel, each
# channel = rotate (FP64 phase) + PolyphaseResampler.  (The uniform polyphase + 64-point DFT form, chan_uniform_kernel, applies
# each channel's NCO deviation at the centre of the tap window -- not the rotate-then-filter operator these references restate:
# it has its own reference and its own section at the end of this file.)
CHAN = [
    ("chan_mfma_batch", {"QDSP_HIP_MF_BATCH_MIN_WORK": "0"}, "decim_mfma_batch_kernel", "mfma_dec"),
    ("chan_any_batch", {"QDSP_HIP_NO_MF_BATCH": "1"}, "resamp_any_batch_kernel", "direct"),
]
CHAN_IDS = [c[0] for c in CHAN]
CHAN_M, CHAN_TAPS = 64, 256
CHAN_F = (0.01, -0.2, 0.3333, 0.125)          # channel 0: blocker; 1, 2: weak tones; 3: guard band (nothing in band)


def _chan_steps(ops):
    return [float(np.angle(complex(*ops.phase_delta(1.0, f)))) / (2 * np.pi) for f in CHAN_F]


def _chan_run(ops, cfg, x, cuts):
    taps = _taps(1, CHAN_M, CHAN_TAPS)
    ch = ops.Channelizer(taps, 1, CHAN_M, [ops.phase_delta(1.0, f) for f in CHAN_F], max_block=max(b - a for a, b in zip(cuts, cuts[1:])))
    ch.set_volk_gain(False)
    ys = []
    for a, b in zip(cuts, cuts[1:]):
        ys.append(np.array(ch.process(np.ascontiguousarray(x[a:b]))))
        assert kname(ch) == cfg[2], (cfg[0], ch.last_kernel())
    return np.concatenate(ys, axis=1)


def _chan_ref64(ops, x, cuts):
    """Per channel: x times exp(j 2 pi step t) in FP64 (t the stream position), then the FP64 resampler call by call."""
    taps = _taps(1, CHAN_M, CHAN_TAPS)
    out = []
    for st in _chan_steps(ops):
        rot = x.astype(np.complex128) * NU.tone(len(x), st)
        r = NU.Resampler64(taps, 1, CHAN_M)
        out.append(np.concatenate([r.process(rot[a:b]) for a, b in zip(cuts, cuts[1:])]))
    return np.array(out)


def _chan_yardsticks(x, cuts):
    """Per channel, the FP32 road: the oracle's FP64-phase rotator rounded to complex64, then the fmaf / SIMD chains."""
    taps = _taps(1, CHAN_M, CHAN_TAPS)
    out = []
    for f in CHAN_F:
        per = []
        for acc in (O.ACC_FMA, O.ACC_SIMD):
            xl, rs = O.Xlator(1.0, f, exact=True), O.Resampler(taps, 1, CHAN_M, acc=acc)
            per.append(np.concatenate([rs.process(xl.process(x[a:b])) for a, b in zip(cuts, cuts[1:])]))
        out.append(per)
    return out


def _chan_span(cfg):
    return SPAN[cfg[3]](1, CHAN_M, CHAN_TAPS, None)


@pytest.mark.parametrize("cfg", CHAN, ids=CHAN_IDS)
def test_channelizer_blocker_and_weak_channels(ops, monkeypatch, cfg):
    _pin(monkeypatch, cfg[1])
    steps = _chan_steps(ops)
    x64 = NU.gate(NU.tone(N_A, -steps[0] + 0.002, 1.0), 0, LOUD_END)
    for c in (1, 2):
        x64 = x64 + NU.tone(N_A, -steps[c] + 0.002 * c, 1e-5)
    x = NU.to32(x64)
    y = _chan_run(ops, cfg, x, CUTS_A)
    ref = _chan_ref64(ops, x, CUTS_A)
    yards = _chan_yardsticks(x, CUTS_A)
    assert y.shape == ref.shape
    first, last = NU.stream_windows(_taps(1, CHAN_M, CHAN_TAPS), 1, CHAN_M, CUTS_A)
    regions = NU.loud_quiet_masks(first, last, LOUD_END, _chan_span(cfg), ref.shape[1])
    for c in range(len(CHAN_F)):
        ok, rep = NU.region_check(y[c], yards[c], ref[c], regions)
        _REPORT["ratios"][f"{cfg[0]}_ch{c}"] = {k: round(v["ratio"], 3) for k, v in rep.items()}
        assert ok, (cfg[0], c, rep)


@pytest.mark.parametrize("cfg", CHAN, ids=CHAN_IDS)
def test_channelizer_nan_inf_locality(ops, monkeypatch, cfg):
    """Span = the channel's tap window (its kernel's span as in SPAN), in every channel; the rest within the region bound."""
    _pin(monkeypatch, cfg[1])
    n_call = 96_000
    cuts = [0, n_call, 2 * n_call, 3 * n_call]
    span = _chan_span(cfg)
    first, last = NU.stream_windows(_taps(1, CHAN_M, CHAN_TAPS), 1, CHAN_M, cuts)
    fam = ("chan", (1, CHAN_M, CHAN_TAPS), False, {}, None, set(), cfg[3], None)
    for where in ("first", "last", "tenth"):
        for comp in ("re", "im"):
            x0, t = _poison_input(fam, n_call, where, 0.0, comp)
            ref0, yard0 = _chan_ref64(ops, x0, cuts), _chan_yardsticks(x0, cuts)
            for value in (np.nan, np.inf, -np.inf):
                x, _ = _poison_input(fam, n_call, where, value, comp)
                y = _chan_run(ops, cfg, x, cuts)
                far = np.maximum(0, np.maximum(first - t, t - last)) > span
                for c in range(len(CHAN_F)):
                    missing, stray = NU.poison_check(~np.isfinite(y[c]), first, last, t, span)
                    assert len(missing) == 0 and len(stray) == 0, (cfg[0], c, where, value, comp, len(missing), len(stray))
                    ok, rep = NU.region_check(y[c], yard0[c], ref0[c], {"far": far})
                    assert ok, (cfg[0], c, where, value, comp, rep)


@pytest.mark.parametrize("cfg", CHAN, ids=CHAN_IDS)
def test_channelizer_scale_and_subnormals(ops, monkeypatch, cfg):
    _pin(monkeypatch, cfg[1])
    x = O.synth_iq(0, 96_000, seed=14)
    cuts = [0, 64_000, 96_000]
    y = _chan_run(ops, cfg, x, cuts)
    for k in SCALES:
        assert _same_scaled(_chan_run(ops, cfg, np.ldexp(x.view(np.float32), k).view(np.complex64), cuts), y, k), (cfg[0], k)
    xs = np.ldexp(x.view(np.float32), -140).view(np.complex64)
    ys = _chan_run(ops, cfg, xs, cuts)
    ref = _chan_ref64(ops, xs, cuts)
    assert np.isfinite(ys).all() and np.abs(ys - ref).max() <= 2.0 ** -120 * np.abs(_taps(1, CHAN_M, CHAN_TAPS).astype(np.float64)).sum()
    _REPORT["subnormal_zero_fraction"][cfg[0]] = float(np.mean(ys == 0))
    assert np.mean(ys == 0) < 0.05, (cfg[0], float(np.mean(ys == 0)))


# ------------------------------------------------------------------------------------------------ coverage
def test_families_covered(ops, monkeypatch):
    """The configurations above reach at least tests/test_gpu_fuzz.py's FAMILIES plus fir_fft_kernel.  Self-contained: one call of
    each configuration, pinned as in checks A-D."""
    from test_gpu_fuzz import FAMILIES

    seen = set()
    x = O.synth_iq(0, 240_000, seed=15)         # (check A's first call size: where every pin above holds)
    pins = {k for f in FAM for k in f[3]} | {k for c in CHAN for k in c[1]}

    def repin(env):           # (one test, many configurations: each starts from the common settings alone)
        for k in pins:
            monkeypatch.delenv(k, raising=False)
        _pin(monkeypatch, env)

    for fam in FAM:
        repin(fam[3])
        xx = np.ascontiguousarray(x.real) if fam[2] else x
        op = _make(ops, fam, _taps(*fam[1]))
        _run(op, fam, xx, [0, len(xx)])
        seen.add(op.last_kernel()["name"])
    for cfg in CHAN:
        repin(cfg[1])
        _chan_run(ops, cfg, x, [0, len(x)])
        seen.add(cfg[2])
    repin({})
    ch = ops.Channelizer(_taps(1, 16, 256), 1, 16, [ops.phase_delta(1.0, -(c - 31.5) / 64) for c in range(64)], max_block=len(x))
    ch.process(x)
    seen.add(ch.last_kernel()["name"])
    seen |= {"fir_fft_kernel" for n in seen if n in ("fir_fft_dma_kernel", "fir_fft_dmapk_kernel")}
    want = set(FAMILIES) | {"fir_fft_kernel"}
    assert want <= seen, sorted(want - seen)


# ------------------------------------------------------------------------------------------------ uniform channelizer
# chan_uniform_kernel<INV, M, QF, ., ., ST4> against ITS operator (NU.ChanUniform64.uniform: each channel's deviation from the grid
# applied at the centre of the tap window) and the FP32 yardstick of its own algorithm (NU.chan_uniform_yard_call), channel by
# channel and region by region.  A form = (M, sign of the grid, taps): INV = sign > 0, QF = 4 for 193..256 taps else 0; every form
# runs with 16-byte stores (aligned output, even row stride), with 8-byte stores (odd row stride) and with QDSP_HIP_CHAN_MAX_WG=1
# (one workgroup: each wave walks a quarter of the call's tiles through the persistent loop and its LDS-DMA re-request).
CU_FORMS = [
    (64, -1, 256), (64, -1, 192), (64, -1, 129), (64, -1, 37),
    (64, +1, 255), (64, +1, 193), (64, +1, 100), (64, +1, 64), (64, +1, 1),
    (32, -1, 193), (32, -1, 100), (32, -1, 1),
    (32, +1, 256), (32, +1, 129),
    (16, -1, 255), (16, -1, 64), (16, -1, 37),
    (16, +1, 193), (16, +1, 192),
    (8, -1, 256), (8, -1, 37),
    (8, +1, 255), (8, +1, 100),
]
CU_TAPS = (256, 255, 193, 192, 129, 100, 64, 37, 1)
CU_DETUNED = [(64, -1, 255), (32, +1, 192), (16, -1, 129), (8, +1, 100)]
CU_QF0 = [(64, -1, 192), (32, -1, 100), (16, -1, 64), (8, -1, 37)]
CU_INV = [(64, +1, 255), (32, +1, 256), (16, +1, 193), (8, +1, 255)]
CU_OUTS = [0, 325, 327, 967, 1168]      # calls in outputs per channel: 20 tiles + 5 outputs (ends inside a tile), 2 outputs (shorter than any
                                        # tile's span of 15 M + 256 samples: guarded staging alone), 40 tiles, 12 tiles + 9 outputs: 73 tiles
CU_WEAK = (16, 18, 49, 0, 63)


def _cu_id(f):
    return f"M{f[0]}_{'asc' if f[1] > 0 else 'desc'}_{f[2]}"


def _cu_qf(ntaps):
    return 4 if ntaps > 192 else 0


def _cu_cuts(M):
    return [o * M for o in CU_OUTS]


def _cu_incs(ops, sign):
    """The plan of the other tests (float theta, libm cosf / sinf) and its mirror image: channel c at sign * (c - 31.5) / 64."""
    return [ops.phase_delta(1.0, sign * (c - 31.5) / 64) for c in range(64)]


def _cu_run(ops, taps, M, incs, x, cuts, stride="even", volk=False, grids=None):
    import torch

    ch = ops.Channelizer(taps, 1, M, incs, max_block=0)
    ch.set_volk_gain(volk)
    ys = []
    for a, b in zip(cuts, cuts[1:]):
        no = (b - a) // M
        out = torch.empty((64, max(2, (no + 1) & ~1) + (stride == "odd")), dtype=torch.complex64, device="cuda")
        assert out.data_ptr() % 16 == 0 and out.shape[1] % 2 == (stride == "odd")      # 16-byte stores exactly when the stride is even
        y = ch.process(torch.from_numpy(np.ascontiguousarray(x[a:b])).cuda(), out)
        lk = ch.last_kernel()
        assert lk["name"] == "chan_uniform_kernel", lk
        if grids is not None:
            grids.append(lk["grid"])
        ys.append(y.cpu().numpy())
    return np.concatenate(ys, axis=1)


def _cu_three_runs(ops, monkeypatch, taps, M, incs, x, cuts, **kw):
    """The call sequence with 16-byte stores, with one workgroup, and with 8-byte stores: (y, y_capped, y_odd_stride)."""
    g0, g1 = [], []
    monkeypatch.delenv("QDSP_HIP_CHAN_MAX_WG", raising=False)
    y = _cu_run(ops, taps, M, incs, x, cuts, grids=g0, **kw)
    yo = _cu_run(ops, taps, M, incs, x, cuts, stride="odd", **kw)
    monkeypatch.setenv("QDSP_HIP_CHAN_MAX_WG", "1")
    yc = _cu_run(ops, taps, M, incs, x, cuts, grids=g1, **kw)
    monkeypatch.delenv("QDSP_HIP_CHAN_MAX_WG", raising=False)
    tiles = [-(-((b - a) // M) // 16) for a, b in zip(cuts, cuts[1:])]
    assert g0 == [max(1, -(-t // 4)) + 1 for t in tiles] and g1 == [2] * len(tiles), (g0, g1)      # (+ 1: the history workgroup)
    return y, yc, yo


def _cu_same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _cu_region_check(y, yard, ref, regions, tag):
    """All 64 rows inside K x the yardstick, region by region; returns the worst ratio per region."""
    worst = {k: 0.0 for k in regions}
    for c in range(64):
        ok, rep = NU.region_check(y[c], yard[c], ref[c], regions)
        assert ok, (tag, c, rep)
        for k, v in rep.items():
            if np.isfinite(v["ratio"]):
                worst[k] = max(worst[k], v["ratio"])
    return {k: round(v, 3) for k, v in worst.items()}


def _cu_check_a(ops, monkeypatch, form, incs, tag):
    M, sign, ntaps = form
    taps = NU.chan_taps(ntaps)
    cuts = _cu_cuts(M)
    loud_end = cuts[-1] // 3
    dphase = [NU.fx_of_inc(*p) for p in incs]
    plan = NU.chan_uniform_plan(dphase)
    assert plan is not None and plan[0] == (sign > 0)
    x = NU.to32(NU.chan_tones(cuts[-1], dphase, loud_end, weak=CU_WEAK, seed=ntaps + M))
    y, yc, yo = _cu_three_runs(ops, monkeypatch, taps, M, incs, x, cuts)
    assert _cu_same_bits(yc, y), (tag, "which wave runs a tile changed a bit", np.argwhere(yc != y)[:4])
    assert _cu_same_bits(yo, y), (tag, "the two store forms differ", np.argwhere(yo != y)[:4])
    ref = NU.chan_uniform_ref64(taps, incs, M, x, cuts)
    yard = NU.chan_uniform_yardstick32(taps, incs, M, x, cuts)
    assert y.shape == ref.shape == (64, CU_OUTS[-1])
    first, last = NU.chan_uniform_windows(ntaps, M, cuts)
    regions = NU.loud_quiet_masks(first, last, loud_end, SPAN["chan_uniform"](1, M, ntaps, None), ref.shape[1])
    assert regions["loud"].sum() > 300 and regions["quiet"].sum() > 600
    # measured first, asserted after: the loud-region floor (RMS error) of the channels that carry no blocker
    quiet_ch = [c for c in range(64) if c != 17]
    floor = max(NU.region_err(y[c], ref[c], regions["loud"])[0] for c in quiet_ch)
    yfloor = max(NU.region_err(yard[c], ref[c], regions["loud"])[0] for c in quiet_ch)
    _REPORT.setdefault("chan_uniform_loud_floor", {})[tag] = {"kernel": float(f"{floor:.3e}"), "yardstick": float(f"{yfloor:.3e}"),
                                                              "blocker_channel": float(f"{NU.region_err(y[17], ref[17], regions['loud'])[0]:.3e}"),
                                                              "quiet_region_worst": float(f"{max(NU.region_err(y[c], ref[c], regions['quiet'])[1] for c in range(64)):.3e}")}
    print(tag, _REPORT["chan_uniform_loud_floor"][tag])
    _REPORT["ratios"][tag] = _cu_region_check(y, yard, ref, regions, tag)
    print(tag, _REPORT["ratios"][tag])
    # the quiet region's floor follows the weak tones (1e-5 x FP32 rounding), not the blocker that has left
    assert max(NU.region_err(y[c], ref[c], regions["quiet"])[1] for c in range(64)) < 1e-10


@pytest.mark.parametrize("form", CU_FORMS, ids=_cu_id)
def test_chan_uniform_forms_blocker_and_weak_channels(ops, monkeypatch, form):
    """Check A in every form: a 0 dBFS tone in channel 17's band for the first third, -100 dB tones throughout in 16, 18, 49 (17's
    radix partner), 0 and 63, channel 40 empty; all 64 rows, loud and quiet region apart.  The capped and the odd-stride run: same bits."""
    _pin(monkeypatch, {})
    _cu_check_a(ops, monkeypatch, form, _cu_incs(ops, form[1]), "chan_uniform_" + _cu_id(form))


@pytest.mark.parametrize("form", CU_DETUNED, ids=_cu_id)
def test_chan_uniform_detuned_plan(ops, monkeypatch, form):
    """Check A': increments 3e-7 turn off the grid, alternating in sign -- still a uniform plan (4e-7 admitted), the second-order
    term of the per-output deviation rotation on (a.quad, chan_launch_uniform's rule restated), the window-centre term 30 x FP32."""
    _pin(monkeypatch, {})
    M = form[0]
    incs = NU.chan_grid_incs(form[1], detune=3e-7)
    _, delta = NU.chan_uniform_plan([NU.fx_of_inc(*p) for p in incs])
    dmax = max(abs(d) for d in delta)
    assert 2.5e-7 < dmax * 2.0 ** -64 < 3.5e-7
    assert 15.0 * float(dmax) * M * 3.4061215800865545e-19 > 1e-4          # a.quad
    _cu_check_a(ops, monkeypatch, form, incs, "chan_uniform_detuned_" + _cu_id(form))


# ---- B
def _cu_poison_positions(M):
    cuts = _cu_cuts(M)
    return {"first": cuts[2], "last": cuts[3] - 1, "history": cuts[1] + 1, "staged": cuts[2] + 20 * 16 * M + 3}


@pytest.mark.parametrize("form", CU_QF0 + CU_INV, ids=_cu_id)
def test_chan_uniform_nan_inf_locality(ops, monkeypatch, form):
    """Check B.  A bad sample at the first / the last sample of the 40-tile call, in the 2-output call before it (it reaches the
    long call through the history alone) and in the middle of the long call (at M = 8: inside the staged span that sixteen
    overlapping windows share): in ALL 64 channels the outputs whose window holds it are bad, nothing beyond the span is, the
    rest is inside the region bound of the clean stream, and one workgroup poisons the same set."""
    _pin(monkeypatch, {})
    M, sign, ntaps = form
    taps, incs, cuts = NU.chan_taps(ntaps), _cu_incs(ops, sign), _cu_cuts(M)
    span = SPAN["chan_uniform"](1, M, ntaps, None)
    _REPORT.setdefault("chan_uniform_span", {})[_cu_id(form)] = {"QF": _cu_qf(ntaps), "Q_eff": -(-ntaps // 64), "span": span}
    first, last = NU.chan_uniform_windows(ntaps, M, cuts)
    xc = O.synth_iq(0, cuts[-1], seed=31)
    for where, t in _cu_poison_positions(M).items():
        x0 = xc.copy()
        x0[t] = 0
        ref0 = NU.chan_uniform_ref64(taps, incs, M, x0, cuts)
        yard0 = NU.chan_uniform_yardstick32(taps, incs, M, x0, cuts)
        far = np.maximum(0, np.maximum(first - t, t - last)) > span
        hold = (first <= t) & (t <= last)
        assert hold.sum() >= -(-ntaps // M) - 1 and far.sum() > 1000
        for value in (np.nan, np.inf, -np.inf):
            for comp in ("re", "im"):
                x = xc.copy()
                x[t] = complex(value, x[t].imag) if comp == "re" else complex(x[t].real, value)
                monkeypatch.delenv("QDSP_HIP_CHAN_MAX_WG", raising=False)
                y = _cu_run(ops, taps, M, incs, x, cuts)
                bad = ~np.isfinite(y)
                for c in range(64):
                    missing, stray = NU.poison_check(bad[c], first, last, t, span)
                    assert len(missing) == 0 and len(stray) == 0, (_cu_id(form), c, where, value, comp, missing[:4], stray[:4])
                _cu_region_check(y, yard0, ref0, {"far": far}, (_cu_id(form), where, value, comp))
                if comp == "re" and not np.isnan(value) or comp == "im" and np.isnan(value):
                    continue
                monkeypatch.setenv("QDSP_HIP_CHAN_MAX_WG", "1")
                assert np.array_equal(~np.isfinite(_cu_run(ops, taps, M, incs, x, cuts)), bad), (_cu_id(form), where, value, comp)
    monkeypatch.delenv("QDSP_HIP_CHAN_MAX_WG", raising=False)


# ---- C / D
@pytest.mark.parametrize("form", CU_QF0 + CU_INV, ids=_cu_id)
def test_chan_uniform_scale_and_subnormals(ops, monkeypatch, form):
    _pin(monkeypatch, {})
    M, sign, ntaps = form
    taps, incs, cuts = NU.chan_taps(ntaps), _cu_incs(ops, sign), _cu_cuts(M)
    x = O.synth_iq(0, cuts[-1], seed=32)
    y = _cu_run(ops, taps, M, incs, x, cuts)
    for k in SCALES:
        yk = _cu_run(ops, taps, M, incs, np.ldexp(x.view(np.float32), k).view(np.complex64), cuts)
        assert _same_scaled(yk, y, k), (_cu_id(form), k)
    xs = np.ldexp(x.view(np.float32), -140).view(np.complex64)
    assert np.count_nonzero(np.abs(xs) < 2.0 ** -126) > len(xs) // 2
    ys = _cu_run(ops, taps, M, incs, xs, cuts)
    ref = NU.chan_uniform_ref64(taps, incs, M, xs, cuts)
    err = np.abs(ys - ref).max()
    print(_cu_id(form), "subnormal max err / bound", err / (2.0 ** -120 * np.abs(taps.astype(np.float64)).sum()), "zeros", float(np.mean(ys == 0)))
    assert np.isfinite(ys).all() and err <= 2.0 ** -120 * np.abs(taps.astype(np.float64)).sum(), _cu_id(form)
    _REPORT["subnormal_zero_fraction"]["chan_uniform_" + _cu_id(form)] = float(np.mean(ys == 0))
    assert np.mean(ys == 0) < 0.05, (_cu_id(form), float(np.mean(ys == 0)))


# ---- E
@pytest.mark.parametrize("form", [(64, +1, 64), (16, -1, 64)], ids=_cu_id)
def test_chan_uniform_volk_gain_against_oracle(ops, monkeypatch, form):
    """Check E: VOLK's magnitude sawtooth on, against the oracle's exact-phase rotator with that gain + the F64 resampler at the
    4e-6 of test_channelizer_64_channels -- an INV and a descending form, both QF = 0.
    The oracle is rotate-then-filter, which the documented operator itself is not: its deviation term sits 2 pi max|delta_c|
    sigma_k away (sigma_k: the taps' RMS distance from the window centre, weighted by h^2 -- white input), whatever computes it.
    On the float-theta plan max|delta_c| = 6.2e-8 turn, so that is 2.8e-6 for these 64 taps (sigma_k 7.3) but 5.3e-6 for the 129
    and 8.2e-6 for the 256 taps of NU.chan_taps (sigma_k 13.7, 21.1): the forms here are those whose operator leaves room under
    4e-6 -- asserted below from the plan and the taps alone -- for the gain's own centre-of-window term (gm1 sigma_k < 3e-7) and FP32.
    Measured: M32_asc_129 5.4e-6 in channel 63 (predicted 5.3e-6) when it was tried here; check A holds that form to its operator."""
    _pin(monkeypatch, {})
    M, sign, ntaps = form
    taps, incs, cuts = NU.chan_taps(ntaps), _cu_incs(ops, sign), _cu_cuts(M)
    _, delta = NU.chan_uniform_plan([NU.fx_of_inc(*p) for p in incs])
    h2, k = taps.astype(np.float64) ** 2, np.arange(ntaps)
    sigma_k = np.sqrt(np.sum(h2 * (k - (ntaps - 1) // 2) ** 2) / np.sum(h2))
    assert 2 * np.pi * max(abs(d) for d in delta) * 2.0 ** -64 * sigma_k < 3e-6
    x = O.synth_iq(0, cuts[-1], seed=33)
    y, yc, yo = _cu_three_runs(ops, monkeypatch, taps, M, incs, x, cuts, volk=True)
    assert _cu_same_bits(yc, y) and _cu_same_bits(yo, y)
    for c in (0, 1, 17, 31, 32, 63):
        xl = O.Xlator(1.0, sign * (c - 31.5) / 64, exact=True, volk_gain=True)
        assert tuple(float(v) for v in xl.delta) == tuple(incs[c])
        rs = O.Resampler(taps, 1, M, acc=O.ACC_F64)
        want = np.concatenate([rs.process(xl.process(x[a:b])) for a, b in zip(cuts, cuts[1:])])
        e = rel_rms(y[c], want)
        print(_cu_id(form), c, "rel_rms", e)
        assert e < 4e-6, (_cu_id(form), c, e)


# ---- F
def _cu_set_inc(ch, c, re, im):
    from qdsp_amd import capi

    capi.check(ch._L.qdsp_hip_chan_cf32_set_phase_inc(ch._h, int(c), float(re), float(im)))


@pytest.mark.parametrize("form", [(16, -1, 100), (64, +1, 255)], ids=_cu_id)
def test_chan_uniform_stream_state(ops, monkeypatch, form):
    """Check F: the stateful ABI on a uniform bank, call by call against NU.ChanUniform64 carrying the same state: reset(),
    advance(n), a retune of all 64 channels to a shifted grid (the folded taps are rebuilt), one channel retuned out of the 4e-7
    tolerance and back and set_mode(DIRECT) for one call (the bank leaves the uniform kernel and comes back: the per-channel
    kernels keep rotated per-channel histories, the uniform one the raw samples -- the first ceil(P / M) outputs after each switch
    are the ones that see the other path's history, and they are checked as a region of their own), and three calls whose length
    is no multiple of M: out_size promises floor(count / M) outputs, each call's windows starting at that call's first sample
    minus P like PolyphaseResampler's, the history always the last P samples of the stream."""
    import torch

    _pin(monkeypatch, {})
    M, sign, ntaps = form
    taps, incs = NU.chan_taps(ntaps), _cu_incs(ops, sign)
    head = -(-ntaps // M)
    ch = ops.Channelizer(taps, 1, M, incs, max_block=0)
    ch.set_volk_gain(False)
    st = NU.ChanUniform64(taps, incs, M)
    x = O.synth_iq(0, M * 2600, seed=34)
    pos = [0]

    def call(count, uniform, tag):
        xs = x[pos[0]: pos[0] + count]
        assert len(xs) == count
        pos[0] += count
        y = ch.process(torch.from_numpy(np.ascontiguousarray(xs)).cuda()).cpu().numpy()
        name = ch.last_kernel()["name"]
        assert (name == "chan_uniform_kernel") == uniform, (tag, name)
        assert y.shape == (64, count // M) and ch.out_size(count) == count // M, (tag, y.shape)
        if uniform:
            assert st.plan() is not None
            yard = NU.chan_uniform_yard_call(st, xs)
            ref = st.uniform(xs)
        else:
            yard = np.array([NU.rotate_direct32(taps, st.dphase[c], st.phase[c], st.hist, xs, M) for c in range(64)])
            ref = st.exact(xs)
        h = np.arange(y.shape[1]) < head
        regions = {"head": h, "rest": ~h} if (~h).any() else {"head": h}
        rep = _cu_region_check(y, yard, ref, regions, (_cu_id(form), tag))
        print(_cu_id(form), tag, name, rep)

    def retune(c, re, im):
        _cu_set_inc(ch, c, re, im)
        st.set_phase_inc(c, re, im)

    call(M * 325, True, "start")
    ch.reset()
    st.reset()
    call(M * 200, True, "after reset")
    ch.advance(12_345)
    st.advance(12_345)
    call(M * 100, True, "after advance")
    shifted = NU.chan_grid_incs(sign, shift=0.0037)
    for c in range(64):
        retune(c, *shifted[c])
    call(M * 150, True, "shifted grid")
    off = NU.inc_of_turns(sign * (5 - 31.5) / 64 + 0.0037 + 1e-5)
    retune(5, *off)
    assert st.plan() is None
    call(M * 120, False, "channel 5 off the grid")
    call(M * 40, False, "still off the grid")
    call(M * 3, False, "off the grid, a call shorter than the taps" if M * 3 < ntaps else "off the grid, a short call")
    retune(5, *shifted[5])
    call(M * 120, True, "back on the grid")
    ch.set_mode(ch.DIRECT)
    call(M * 60, False, "DIRECT for one call")
    ch.set_mode(ch.AUTO)
    call(M * 100, True, "AUTO again")
    for count in (M * 50 + 5, M * 3 + 7, M * 60 + M - 1):
        call(count, True, f"count {count} = {count % M} mod M")
    call(M * 20, True, "whole calls again")


# ---- coverage
def test_chan_uniform_forms_covered(ops, monkeypatch):
    """Every (INV, M, QF) instantiation is in CU_FORMS, each (M, sign) meets a QF = 0 and an odd-P plan, every tap count runs at
    M = 64 and at an oversampled M -- and, one form per instantiation, a 40-tile call launches chan_uniform_kernel with 16-byte
    stores, with 8-byte stores and with a single workgroup (the grid says so)."""
    _pin(monkeypatch, {})
    seen = {}
    for M, sign, ntaps in CU_FORMS:
        seen.setdefault((sign > 0, M, _cu_qf(ntaps)), (M, sign, ntaps))
    assert set(seen) == {(inv, M, qf) for inv in (False, True) for M in (8, 16, 32, 64) for qf in (0, 4)}
    for M in (8, 16, 32, 64):
        for sign in (-1, 1):
            mine = [f[2] for f in CU_FORMS if f[:2] == (M, sign)]
            assert any(_cu_qf(t) == 0 for t in mine) and any(t % 2 for t in mine), (M, sign, mine)
    for t in CU_TAPS:
        assert (64, -1, t) in CU_FORMS or (64, 1, t) in CU_FORMS, t
        assert any(f[2] == t and f[0] != 64 for f in CU_FORMS), t
    assert {f[2] for f in CU_FORMS} == set(CU_TAPS)
    for (inv, M, qf), form in sorted(seen.items()):
        taps, incs = NU.chan_taps(form[2]), _cu_incs(ops, form[1])
        plan = NU.chan_uniform_plan([NU.fx_of_inc(*p) for p in incs])
        assert plan is not None and plan[0] == inv and (4 if -(-form[2] // 64) == 4 else 0) == qf
        x = O.synth_iq(0, 640 * M, seed=35)
        y, yc, yo = _cu_three_runs(ops, monkeypatch, taps, M, incs, x, [0, 640 * M])      # (asserts the kernel, the grids, the strides)
        assert _cu_same_bits(yc, y) and _cu_same_bits(yo, y), form
