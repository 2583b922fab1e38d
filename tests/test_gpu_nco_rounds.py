"""The fused-VFO kernels past each worker's first unit, at test sizes.

Every fused-VFO kernel (NCO and filter in one launch) evaluates an exact fixed-point phase once per worker -- a workgroup or a wave -- and
from the worker's second unit on advances that phasor by a step the host made in FP64.  On the default grids a second unit needs 2^24 and
more samples, so the step, its host side and the order of the LDS slot that carries it ran never, or only inside the 2^27-sample checks.
Here the grids are cut down until every worker goes round:

  kernel                              unit                       worker      grid knob                        step (samples)
  fir_fft_kernel<DEC, true>           segment of L samples       workgroup   QDSP_HIP_FFT_WG_PER_CU=1 (256)   nwg L
  fir_fft_dec_kernel<DEC, true>       group of DEC segments      workgroup   QDSP_HIP_FFT_WG_PER_CU=1 (256)   nwg L DEC
  pfb_dec8_kernel / pfb_dec4_kernel   segment of 8 Lo samples    wave        QDSP_HIP_PFB_WG_PER_CU=0 (1)     8 Lo wpw nwg
  resamp_mfma_kernel<ROT>             tile of 4 G M' samples     wave        QDSP_HIP_RM_WAVES_PER_SIMD=0 (1) nwaves 4 G M'

Geometry, as the launch code (launch_fft, launch_pfb, launch_rm in qdsp_amd/csrc/qdsp_hip.hip; rm_plan in select.cpp) defines it:
  * 4096-point kernels: overlap ov = taps - 1 rounded up to a multiple of DEC (pruned inverse, DEC 2 / 4 / 8 / 16) or to even (full inverse with
    the strided store: every other decimation, 1 included), L = 4096 - ov, segments = ceil(outputs / (L / DEC)) or ceil((count + 2) / L);
    grouped from 1024 groups of DEC segments on; nwg = min(256 per_cu, units), grid = nwg + 1 (the history hand-over workgroup).
  * polyphase kernels: PH = 2 output phases at decimation 4, else 1; Q = ceil((taps + 4 (PH - 1)) / 8) taps per column, Lo = 513 - Q column
    outputs per segment, segments = ceil(columns / Lo); a workgroup has wpw = 4 PH waves, wave w takes segments w, w + wpw nwg, ...;
    nwg = min(256 per_cu / PH, 1024, ceil(segments / wpw)), at least 1; grid = nwg + 1.
  * rational MFMA kernel: J merged periods (L' = J L, M' = J M), G period quads per tile, tiles = ceil(ceil(outputs / L') / (4 G)); wave w takes
    tiles w, w + nwaves, ...; nwaves = min(1024 per_simd, tiles), at least 1; grid = ceil(nwaves / 4) + 1.  rm_plan_py below restates rm_plan
    for complex data; every test checks it against the LDS size and the grid the library reports.

Each case asserts
  (c) first, on the host: the step's phase frac(step x f) lies in [0.05, 0.95] turn for the tuned f, so a dropped, doubled or stale step moves
      every later unit by at least 0.05 turn;
  (a) the run equals the same call(s) on a grid that covers every unit (no later rounds: QDSP_HIP_FFT_WG_PER_CU=8, the other two knobs at their
      defaults), sample by sample: the two runs do the same float arithmetic but for the unit's phasor, which reaches float from an FP64 chain
      instead of one exact evaluation.  Each of its components can move by one ulp and at most two float complex products follow:
      |y_multi - y_single| <= 2^-21 max(|y_single|, 1e-3 rms(y_single)) -- 8 ulp of the sample against ~3 derived;
  (b) the FP64 oracle chain, Xlator(exact) -> Resampler(ACC_F64): on windows of three units at the start, across the boundary between round 1
      and round 2, in the middle and at the ragged end (the single calls of the 4096-point kernels), over the whole stream (the other two and
      the step-cache stream), at the tolerance the existing test of the same kernel uses.  A window's history starts on a multiple of lcm(512, M) with the oracle's NCO advanced to it, so
      the VOLK gain sawtooth and the polyphase counter line up.
and, from last_kernel(), that the intended kernel ran on a grid smaller than its number of units.

Grouped kernel: decimation 4 with 256 taps (15.7 M samples), 8 and 16 at the longest overlap the 4096-point kernels take (2049 taps, L = 2048:
16.8 M and 33.6 M samples, 134 and 268 MB of input).

Step cache (rot_step_ok in launch_fft): one Vfo, four multi-round calls, retuned after the first, re-configured to 129 taps (another L) after the
second, retuned back before the fourth.  The oracle's Resampler has no configure(): the test builds a new one on the 129 taps and hands it the
newest 129 samples of the old one's history, which is what the library's configure() keeps."""
import math

import numpy as np
import pytest

import oracle as O
from conftest import kname, rel_rms
from test_gpu_parity import TOL_FFT, dev, run_blocks

pytestmark = pytest.mark.gpu

GROUPED_LDS = (2 * 4352 + 16 * 17) * 8      # fir_fft_dec_kernel: exchange buffer + staging + pass-B twiddles (tests/test_gpu_fft_tables.py)
F_FFT = 0.1234                              # frac(256 x 3840 x f) = 0.136, grouped decimation 4: 0.544
F_RM = 0.2347                               # frac(640 f) = 0.208 (tiles of 640 samples), frac(672 f) = 0.718 (10/7: 672)
ULP_BOUND = 8.0                             # 2^-21 = 8 x 2^-24


@pytest.fixture(scope="module")
def ops():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from qdsp_amd import ops as _ops

    assert "gfx950" in _ops.device_info(0)["arch"]
    return _ops


@pytest.fixture(autouse=True)
def _pin_kernels(monkeypatch):
    """No measured exception and no one-wave 1024-point form: the rule chain (or set_mode) names the kernel.  The grid knobs and
    QDSP_HIP_NO_PFB are set by each test."""
    monkeypatch.setenv("QDSP_HIP_FFT1K_MAX_COUNT", "0")
    monkeypatch.setenv("QDSP_HIP_DECIM_SETTING", "0")


# ------------------------------------------------------------------------------ geometry of the launch code, restated
def turns_of(inc):
    """The NCO's step in turns, from the float pair the operator is given (launch code: turns_of / fx_of_turns)."""
    return math.atan2(float(inc[1]), float(inc[0])) / (2.0 * math.pi)


def step_phase(samples, inc):
    p = samples * turns_of(inc)
    return p - math.floor(p)


def assert_step_visible(what, samples, inc):
    p = step_phase(samples, inc)
    assert 0.05 <= p <= 0.95, f"{what}: a step of {samples} samples is {p:.3f} turn -- pick another frequency"
    return p


def fft_geometry(ntaps, dec, count):
    """-> (L, units, grouped) of launch_fft for a Vfo / Resampler with interp 1 on complex data."""
    if dec in (2, 4, 8, 16):
        ov = (ntaps - 1 + dec - 1) // dec * dec
        L = 4096 - ov
        per_block = L // dec
        nblocks = (count // dec + per_block - 1) // per_block
    else:
        ov = ntaps & ~1
        L = 4096 - ov
        nblocks = (count + 2 + L - 1) // L
    groups = (nblocks + dec - 1) // dec
    grouped = dec >= 4 and dec in (4, 8, 16) and groups >= 1024
    return L, (groups if grouped else nblocks), grouped


def pfb_geometry(ntaps, dec, count):
    """-> (Lo, wpw, nseg) of launch_pfb."""
    PH = 2 if dec == 4 else 1
    Q = (ntaps + dec * (PH - 1) + 7) // 8
    Lo = 513 - Q
    nout = count // dec
    ncol = nout if PH == 1 else (nout + PH - 2) // PH + 1
    return Lo, 4 * PH, (ncol + Lo - 1) // Lo


def rm_plan_py(L0, M0, P):
    """rm_plan (select.cpp) for complex data -> dict(J, G, ngrp, KB, ext, pitch, lds)."""
    for J in range(1, 65):
        L, M = J * L0, J * M0
        nblk = (L + 3) // 4
        if nblk > 16 * 3 or 4 * M > 64 * 12:
            break
        qpb = 16 // nblk if nblk <= 8 else 1
        ngrp = (nblk + 15) // 16
        c0 = [(4 * b * M0) // L0 for b in range(nblk)]
        KB = 1
        for b in range(nblk):
            i1 = min(4 * b + 3, L - 1)
            KB = max(KB, (i1 * M0) // L0 + P - c0[b])
        if KB > 40:
            break
        reach = max(c + KB for c in c0)
        ext = max(reach - M, 0)
        if ext > M or nblk * qpb / (16.0 * ngrp) < 0.6:
            continue
        pitch = M + ext
        pitch += (pitch & 1) ^ 1
        G = min((64 * 12 - ext) // (4 * M), 16)
        G -= G % qpb
        lds = ((ngrp * KB * 64 + 2 * ngrp * 64 + 3) & ~3) * 4 + 4 * (4 * G * pitch + 64) * 8
        if G < 1 or lds > 64 * 1024:
            continue
        return dict(J=J, G=G, ngrp=ngrp, KB=KB, ext=ext, pitch=pitch, lds=lds)
    return None


def rm_tiles(plan, L0, M0, count):
    nout = count * L0 // M0
    nper = (nout + plan["J"] * L0 - 1) // (plan["J"] * L0)
    return (nper + 4 * plan["G"] - 1) // (4 * plan["G"])


# ------------------------------------------------------------------------------ helpers
def random_taps(ntaps):
    rng = np.random.default_rng(7 + ntaps)
    return (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)


def max_ulp(y_multi, y_single):
    """max |y_multi - y_single| / (2^-24 max(|y_single|, 1e-3 rms)): torch tensors on the device or numpy arrays."""
    assert y_multi.shape == y_single.shape
    if isinstance(y_single, np.ndarray):
        s = y_single.astype(np.complex128)
        mag = np.abs(s)
        ref = np.maximum(mag, 1e-3 * math.sqrt(float(np.mean(mag * mag))))
        return float(np.max(np.abs(y_multi.astype(np.complex128) - s) / ref)) * 2.0 ** 24
    import torch

    s = y_single.to(torch.complex128)
    mag = s.abs()
    ref = torch.clamp(mag, min=1e-3 * math.sqrt(mag.pow(2).mean().item()))
    return ((y_multi.to(torch.complex128) - s).abs() / ref).max().item() * 2.0 ** 24


def oracle_window(seed, a, b, n_total, taps, interp, decim, f, vg):
    """FP64 chain over input samples [a, b) of ONE call of n_total samples that starts the stream -> (index of the first output, outputs).
    The chain starts on a multiple of lcm(512, decim) at least a filter length before a, its NCO advanced to that sample."""
    tpp = -(-len(taps) // interp)
    q = 512 * decim // math.gcd(512, decim)
    lo = max((a - tpp) // q * q, 0)
    a, b = max(a, 0), min(b, n_total)
    xl = O.Xlator(1.0, f, exact=True, volk_gain=vg)
    xl.turns.value = (lo * turns_of(xl.delta)) % 1.0
    y = O.Resampler(taps, interp, decim, acc=O.ACC_F64).process(xl.process(O.synth_iq(lo, b - lo, seed=seed)))
    skip = 0 if lo == 0 else -(-(a - lo) * interp // decim)
    return lo * interp // decim + skip, y[skip:]


def check_windows(tag, y, windows, seed, n, taps, dec, f, vg):
    worst = 0.0
    for a, b in windows:
        o, want = oracle_window(seed, a, b, n, taps, 1, dec, f, vg)
        got = y[o:o + len(want)].cpu().numpy()
        assert len(got) == len(want) and len(want) > 0, (tag, a, b)
        err = rel_rms(got, want)
        print(f"{tag} input [{a}, {b}): rel rms vs FP64 oracle {err:.3e}")
        assert err < TOL_FFT, (tag, a, b, err)
        worst = max(worst, err)
    return worst


def unit_windows(U, nwg, units, n):
    """Three units each: the start, the end of round 1 / start of round 2, the middle, the ragged end."""
    mid = units // 2
    return [(0, 3 * U), ((nwg - 2) * U, (nwg + 1) * U), (mid * U - 100, (mid + 3) * U + 100), (n - 3 * U, n)]


# ------------------------------------------------------------------------------ 1: fir_fft_kernel<DEC, true>, per segment
@pytest.mark.parametrize("vg", [True, False])
@pytest.mark.parametrize("dec", [1, 2, 3, 8, 16])
def test_per_segment_kernel_goes_round(ops, monkeypatch, dec, vg):
    """256 taps, one call of 549 whole segments and 1234 samples on 256 workgroups: two to three segments per workgroup, a guarded first
    segment, a ragged last one, an uneven split.  Decimation 1 and 3: full inverse and strided store; 2, 8, 16: pruned inverse (8 and 16 below
    the grouped threshold, the polyphase kernel switched off)."""
    taps = random_taps(256)
    inc = ops.phase_delta(1.0, F_FFT)
    L = fft_geometry(256, dec, 1 << 20)[0]
    n = L * 549 + 1234
    L, units, grouped = fft_geometry(256, dec, n)
    assert (L, units, grouped) == (3840, 550, False)
    p = assert_step_visible(f"dec {dec}", 256 * L, inc)
    monkeypatch.setenv("QDSP_HIP_NO_PFB", "1")
    seed = 40 + dec
    x = ops.synth_iq(n, seed=seed)
    out = {}
    for per_cu in ("1", "8"):
        monkeypatch.setenv("QDSP_HIP_FFT_WG_PER_CU", per_cu)
        v = ops.Vfo(taps, 1, dec, inc, max_block=0)
        v.set_mode(v.FFT)
        v.set_volk_gain(vg)
        out[per_cu] = v.process(x)
        k = v.last_kernel()
        assert k["name"] == "fir_fft_kernel" and k["lds_bytes"] != GROUPED_LDS, k
        assert k["grid"] == (256 + 1 if per_cu == "1" else units + 1), k
        assert (k["grid"] - 1 < units) == (per_cu == "1")
    ulp = max_ulp(out["1"], out["8"])
    print(f"fir_fft_kernel<{dec if dec in (2, 8, 16) else 1}, true> dec {dec} gain {vg}: grid 257, {units} segments, step {p:.3f} turn, "
          f"max |multi - single| {ulp:.2f} ulp")
    assert ulp <= ULP_BOUND
    check_windows(f"per-segment dec {dec} gain {vg}", out["1"], unit_windows(L, 256, units, n), seed, n, taps, dec, F_FFT, vg)


# ------------------------------------------------------------------------------ 2: fir_fft_dec_kernel<DEC, true>, grouped
@pytest.mark.parametrize("vg", [True, False])
@pytest.mark.parametrize("dec,ntaps", [(4, 256), (8, 2049), (16, 2049)])
def test_grouped_kernel_goes_round(ops, monkeypatch, dec, ntaps, vg):
    """1024 whole groups and a ragged one on 256 workgroups: four to five groups per workgroup.  The grouped kernel never ran with the NCO."""
    taps = random_taps(ntaps)
    inc = ops.phase_delta(1.0, F_FFT)
    L = fft_geometry(ntaps, dec, 1 << 20)[0]
    n = 1024 * dec * L + 4992
    L, units, grouped = fft_geometry(ntaps, dec, n)
    assert grouped and units == 1025 and L == (3840 if ntaps == 256 else 2048)
    p = assert_step_visible(f"grouped dec {dec}", 256 * L * dec, inc)
    monkeypatch.setenv("QDSP_HIP_NO_PFB", "1")
    seed = 60 + dec
    x = ops.synth_iq(n, seed=seed)
    out = {}
    for per_cu in ("1", "8"):      # 8: 2048 workgroup slots >= 1025 groups
        monkeypatch.setenv("QDSP_HIP_FFT_WG_PER_CU", per_cu)
        v = ops.Vfo(taps, 1, dec, inc, max_block=0)
        v.set_mode(v.FFT)
        v.set_volk_gain(vg)
        out[per_cu] = v.process(x)
        k = v.last_kernel()
        assert k["name"] == "fir_fft_kernel" and k["lds_bytes"] == GROUPED_LDS, k
        assert k["grid"] == (256 + 1 if per_cu == "1" else units + 1), k
        assert (k["grid"] - 1 < units) == (per_cu == "1")
    assert out["1"].numel() == n // dec
    ulp = max_ulp(out["1"], out["8"])
    print(f"fir_fft_dec_kernel<{dec}, true> {ntaps} taps gain {vg}: grid 257, {units} groups, step {p:.3f} turn, max |multi - single| {ulp:.2f} ulp")
    assert ulp <= ULP_BOUND
    y = out["1"]
    del out, x
    check_windows(f"grouped dec {dec} gain {vg}", y, unit_windows(dec * L, 256, units, n), seed, n, taps, dec, F_FFT, vg)


# ------------------------------------------------------------------------------ 3: pfb_dec8_kernel<true>, pfb_dec4_kernel<true>
PFB_N = 500_000
PFB_CUTS = [0, 8 * 13001, 8 * 13001 + 8 * 9, 8 * 30000 + 3, 8 * 30000 + 4096 + 3, PFB_N]      # (test_polyphase_overlap_save_decimator_vs_oracle)


@pytest.mark.parametrize("vg", [True, False])
@pytest.mark.parametrize("ntaps", [17, 256, 1024])
@pytest.mark.parametrize("dec", [8, 4])
def test_polyphase_kernels_go_round(ops, monkeypatch, dec, ntaps, vg):
    """One workgroup: 4 waves (decimation 8) or 8 (decimation 4), each walking every 4th or 8th segment -- a ragged stream of calls and the same
    input as one call.  17, 256 and 1024 taps: 3 to 129 taps per column, 510 to 384 outputs per segment, the odd outputs' delay at decimation 4."""
    monkeypatch.setenv("QDSP_HIP_PFB_MIN_COUNT", "0")
    taps = O.lowpass_taps_f64(ntaps, 0.5 / dec).astype(np.float32)
    inc = ops.phase_delta(1.0, F_FFT)
    Lo, wpw, nseg_all = pfb_geometry(ntaps, dec, PFB_N)
    p = assert_step_visible(f"pfb dec {dec} {ntaps} taps", 8 * Lo * wpw * 1, inc)
    x = O.synth_iq(0, PFB_N, seed=800 + ntaps)
    for name, cuts in (("stream", PFB_CUTS), ("one call", [0, PFB_N])):
        spans = list(zip(cuts, cuts[1:]))
        out, went_round = {}, 0
        for per_cu in ("0", None):
            if per_cu is None:
                monkeypatch.delenv("QDSP_HIP_PFB_WG_PER_CU", raising=False)
            else:
                monkeypatch.setenv("QDSP_HIP_PFB_WG_PER_CU", per_cu)
            v = ops.Vfo(taps, 1, dec, inc, max_block=0)
            v.set_mode(v.FFT)
            v.set_volk_gain(vg)
            ys = []
            for a, b in spans:
                ys.append(v.process(dev(x[a:b])).cpu().numpy())
                k = v.last_kernel()
                assert (k["name"] == f"pfb_dec{dec}_kernel") == (b - a >= 4096), (a, b, k)
                if b - a < 4096:
                    continue
                nseg = pfb_geometry(ntaps, dec, b - a)[2]
                if per_cu == "0":
                    assert k["grid"] == 1 + 1, k
                    went_round += nseg > wpw
                else:
                    assert (k["grid"] - 1) * wpw >= nseg, (k, nseg)      # every segment has a wave of its own
            out[per_cu] = np.concatenate(ys)
        assert went_round >= (3 if name == "stream" else 1)
        ulp = max_ulp(out["0"], out[None])
        rs = O.Resampler(taps, 1, dec, acc=O.ACC_F64)
        xl = O.Xlator(1.0, F_FFT, exact=True, volk_gain=vg)
        want = run_blocks(rs, np.concatenate([xl.process(x[a:b]) for a, b in spans]), [b - a for a, b in spans])
        y = out["0"]
        err = rel_rms(y, want)
        print(f"pfb_dec{dec}_kernel<true> {ntaps} taps gain {vg}, {name}: grid 2 ({wpw} waves), {nseg_all} segments in all, step {p:.3f} turn, "
              f"max |multi - single| {ulp:.2f} ulp, rel rms vs FP64 oracle {err:.3e}")
        assert ulp <= ULP_BOUND
        assert len(y) == len(want) and err < 1e-6
        assert np.abs(y - want).max() < 4e-6 * np.abs(want).max()


# ------------------------------------------------------------------------------ 4: resamp_mfma_kernel<ROT>
@pytest.mark.parametrize("vg", [True, False])
@pytest.mark.parametrize("L,M,tpp", [(147, 160, 16), (10, 7, 8), (6, 1, 10), (3, 8, 20)])
def test_rational_mfma_kernel_goes_round(ops, monkeypatch, L, M, tpp, vg):
    """One wave walks every tile: a long period, a merged period, a pure interpolator, a decimating small ratio; the ragged calls of
    test_rational_mfma_resampler, then the whole input as one call (the wave prefetches its next tile with the NCO on)."""
    monkeypatch.setenv("QDSP_HIP_RM_MIN_COUNT", "0")
    ntaps = L * tpp - 3
    taps = (O.lowpass_taps_f64(ntaps, 0.4 / max(L, M)) * L).astype(np.float32)
    plan = rm_plan_py(L, M, -(-ntaps // L))                    # (3 x 20 - 3 taps are 19 per phase)
    assert plan is not None
    tile = 4 * plan["G"] * plan["J"] * M                       # input samples per tile
    inc = ops.phase_delta(1.0, F_RM)
    p = assert_step_visible(f"resamp_mfma {L}/{M}", 1 * tile, inc)
    sizes = [M * 700 + 17, 5, M * 300, max(M - 1, 1), 3 * M + 1, 16 * M, 16 * M + 1, M * 515 + 3]
    if M == 1:
        sizes = [s * 40 for s in sizes]
    x = O.synth_iq(0, sum(sizes), seed=L + M)
    for name, blocks in (("stream", sizes), ("one call", [sum(sizes)])):
        cuts = np.cumsum([0] + blocks)
        out, went_round = {}, 0
        for per_simd in ("0", None):
            if per_simd is None:
                monkeypatch.delenv("QDSP_HIP_RM_WAVES_PER_SIMD", raising=False)
            else:
                monkeypatch.setenv("QDSP_HIP_RM_WAVES_PER_SIMD", per_simd)
            v = ops.Vfo(taps, L, M, inc, max_block=0)
            v.set_volk_gain(vg)
            ys = []
            for a, b in zip(cuts, cuts[1:]):
                ys.append(v.process(dev(x[a:b])).cpu().numpy())
                if (b - a) * L // M == 0:
                    continue
                k = v.last_kernel()
                ntiles = rm_tiles(plan, L, M, b - a)
                assert k["name"] == "resamp_mfma_kernel" and k["lds_bytes"] == plan["lds"], (k, plan)
                if per_simd == "0":
                    assert k["grid"] == 1 + 1, k
                    went_round += ntiles > 1
                else:
                    assert k["grid"] == (ntiles + 3) // 4 + 1, (k, ntiles)      # one wave per tile
            out[per_simd] = np.concatenate(ys)
        assert went_round >= (3 if name == "stream" else 1)
        ulp = max_ulp(out["0"], out[None])
        rs = O.Resampler(taps, L, M, acc=O.ACC_F64)
        xl = O.Xlator(1.0, F_RM, exact=True, volk_gain=vg)
        want = run_blocks(rs, np.concatenate([xl.process(x[a:b]) for a, b in zip(cuts, cuts[1:])]), blocks)
        err = rel_rms(out["0"], want)
        print(f"resamp_mfma_kernel<ROT> {L}/{M} x {tpp} gain {vg}, {name}: grid 2 (1 wave), {rm_tiles(plan, L, M, max(blocks))} tiles in the longest call "
              f"(J {plan['J']}, G {plan['G']}), step {p:.3f} turn, max |multi - single| {ulp:.2f} ulp, rel rms vs FP64 oracle {err:.3e}")
        assert ulp <= ULP_BOUND
        assert out["0"].shape == want.shape and err < 1e-6


# ------------------------------------------------------------------------------ 5: the step cached on the host (launch_fft)
@pytest.mark.parametrize("vg", [True, False])
def test_cached_step_follows_retune_and_new_taps(ops, monkeypatch, vg):
    """launch_fft keeps the FP64 step in the engine, keyed on (dphase, nwg L): four multi-round calls on one Vfo -- f1 / 256 taps, f2 / 256 taps,
    f2 / 129 taps (L 3840 -> 3968), f1 / 129 taps -- so the key changes in its first part, its second and its first again.  A stale step would
    leave every later segment of a workgroup off by the difference of the two steps."""
    dec = 8
    f1, f2 = F_FFT, -0.111
    t256, t129 = random_taps(256), random_taps(129)
    inc1, inc2 = ops.phase_delta(1.0, f1), ops.phase_delta(1.0, f2)
    sizes = [3840 * 300 + 777, 3840 * 257 + 5, 3968 * 290 + 1234, 3968 * 258 + 1]
    plan = [(inc1, 256), (inc2, 256), (inc2, 129), (inc1, 129)]
    steps = []
    for (inc, ntaps), n in zip(plan, sizes):
        L, units, grouped = fft_geometry(ntaps, dec, n)
        assert L == (3840 if ntaps == 256 else 3968) and 256 < units < 1024 and not grouped
        steps.append(assert_step_visible(f"call of {n}", 256 * L, inc))
    for inc in (inc1, inc2):      # both frequencies at both tap counts
        for L in (3840, 3968):
            assert_step_visible("cache key", 256 * L, inc)
    monkeypatch.setenv("QDSP_HIP_NO_PFB", "1")
    cuts = np.cumsum([0] + sizes)
    x = O.synth_iq(0, int(cuts[-1]), seed=77)
    xd = dev(x)
    out = {}
    for per_cu in ("1", "8"):
        monkeypatch.setenv("QDSP_HIP_FFT_WG_PER_CU", per_cu)
        v = ops.Vfo(t256, 1, dec, inc1, max_block=0)
        v.set_mode(v.FFT)
        v.set_volk_gain(vg)
        ys = []
        for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
            if i == 1 or i == 3:
                v.set_phase_inc(*plan[i][0])
            if i == 2:
                v.configure(t129, 1, dec)
            ys.append(v.process(xd[a:b]).cpu().numpy())
            k = v.last_kernel()
            units = fft_geometry(plan[i][1], dec, int(b - a))[1]
            assert kname(v) == "fir_fft_kernel" and k["lds_bytes"] != GROUPED_LDS, k
            assert k["grid"] == (256 + 1 if per_cu == "1" else units + 1), (i, k)
            assert (k["grid"] - 1 < units) == (per_cu == "1")
        out[per_cu] = ys
    # the oracle chain, retuned the way test_rational_mfma_resampler retunes it; new taps: a new resampler on the newest samples of the old history
    xl = O.Xlator(1.0, f1, exact=True, volk_gain=vg)
    rs = O.Resampler(t256, 1, dec, acc=O.ACC_F64)
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        if i == 1 or i == 3:
            O.lib().oracle_xlator_phase_delta(1.0, f2 if i == 1 else f1, O._fp(xl.delta))
        if i == 2:
            old = rs.hist
            rs = O.Resampler(t129, 1, dec, acc=O.ACC_F64)
            rs.hist[:] = old[len(old) - len(rs.hist):]
        want = rs.process(xl.process(x[a:b]))
        ulp = max_ulp(out["1"][i], out["8"][i])
        err = rel_rms(out["1"][i], want)
        print(f"step cache gain {vg}, call {i} ({plan[i][1]} taps, f {'f1' if plan[i][0] is inc1 else 'f2'}): grid 257, "
              f"{fft_geometry(plan[i][1], dec, int(b - a))[1]} segments, step {steps[i]:.3f} turn, max |multi - single| {ulp:.2f} ulp, "
              f"rel rms vs FP64 oracle {err:.3e}")
        assert ulp <= ULP_BOUND, i
        assert len(out["1"][i]) == len(want) and err < TOL_FFT, i
