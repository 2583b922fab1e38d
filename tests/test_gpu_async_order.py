"""Every handle with work still queued on a non-blocking stream.

include/qdsp_hip.h promises that `*_process_dev` is asynchronous on the caller's stream and that state is advanced in stream order;
every setter, getter, reset and lazily rebuilt table of the library waits for what is in flight before it touches device memory.
The rest of the suite runs on torch's default stream (HIP's legacy null stream, ordered against every blocking copy) and
synchronises after each call, so none of those waits, and no launch on the wrong stream, can show there.  Here every scenario -- a
call sequence on fresh handles with host actions in between -- runs three ways (tests/_async.py): on the null stream with a
synchronise after every step, on a non-blocking side stream with a synchronise after every step, and on a side stream with no
synchronisation at all, behind a bounded busy period, so that every host action and every call-time table rebuild finds library
work still queued.  The three runs must agree bit for bit in every output, getter value, count and kernel name (the library has no
device atomics and every kernel's arithmetic order is fixed), and the serial run is anchored to the operator's own reference:

  * engine handles and the channelizer: the FP64 oracle chain (O.Xlator(exact) -> O.Resampler / O.Fir(ACC_F64); the bank:
    _numerics.ChanUniform64), 2e-6 relative RMS per call and 4e-6 x max|want| on the head of each call -- tests/test_gpu_handover.py's
    bounds;
  * the per-row operators and the chains: a model per kind carries the kind's own reference through the steps -- a setter changes
    its parameters, set_state / reset its state -- and every process_batch and every getter of the serial run is compared with
    it: bit for bit for FM, AM (its two candidates), Squelch, Agc, FeedForwardAgc, RowFir, DelayImag, Threshold, Deframer,
    MmClockRecovery and the MSK chain (the numpy definitions of the *_cpu modules, _psk_ref.py, _mmcr_ref.py, _deframer_ref.py);
    at the bound of the kind's own GPU test for Deemp, ComplexAgc (exact recurrence) and CostasLoop (4 x the float loop's
    error); the PSK chains against the composition of the separate device handles, as tests/test_gpu_psk.py does; SsbDemod as the
    real part of the oracle's mixer; StereoFmDemod as its own test does, in three layers (fm_ref, the pilot FIR under the yardstick
    rule, stereo_mix_ref of the handle's own pilot rows bit for bit), every call in the peak regime;
  * the forward error correction handles of qdsp_amd.fec (RsDecoder, FalconRs, and Deframer -> FalconRs through the deframer's
    device counts): _rs_ref.Layout.decode under the maps in force -- set_maps switches the model's layout --, bit for bit over the
    whole output buffer, the counts and the whole errs buffer, each filled with a sentinel by a copy queued in front of the call
    (bytes behind a row's last good frame and errs entries behind a short row included); frames from test_gpu_rs.gen_frames;
  * the NOAA HRPT tail of qdsp_amd.noaa (HrptDemux, TipDemux, HirsDemux, and Deframer -> HrptDemux -> TipDemux -> HirsDemux through
    the device counts): the definition of tests/_noaa_ref.py (hrpt_demux_fast, tip_demux, one HirsFast per row carried through the
    steps: set_state and reset change it as they change the handle), bit for bit over whole sentinel-filled output allocations
    and every getter's value (counts, get_state, tip, aip, qdsp_hip_hrpt_get_frame_slots); every row's HIRS elements climb from
    call to call, so that a line in progress spans every host action.

`test_control_*` proves that the hold holds and that a race shows; `test_scenarios_cover_the_library` (last) that every kernel
family and every public setter / getter / reset / configure of qdsp_amd.ops, qdsp_amd.fec and qdsp_amd.noaa was raced.  With ASYNC_ORDER_REPORT=<file> the measured
host times and the holds used go there (profiles/async_order_windows.txt is one such run)."""
import ctypes as C
import inspect
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _async as A  # noqa: E402
import _deframer_ref as DF  # noqa: E402
import _mmcr_ref as MM  # noqa: E402
import _noaa_ref as NR  # noqa: E402
import _numerics as NU  # noqa: E402
import _rs_ref as RS  # noqa: E402
import oracle as O  # noqa: E402
from _async import Call, H, Host  # noqa: E402
from _psk_ref import delay_imag_ref  # noqa: E402
from conftest import rel_rms  # noqa: E402
from test_cagc_cpu import LD, ROW_TILES as CAGC_ROW_TILES, TILE as CAGC_TILE, cagc_exact  # noqa: E402
from test_cagc_cpu import check_against_truth as cagc_check, gain_bound as cagc_gain_bound, in_domain as cagc_in_domain  # noqa: E402
from test_costas_cpu import costas_gains, costas_ref, costas_truth, deviation as costas_deviation  # noqa: E402
from test_deemp_cpu import ROW_TILES as DEEMP_ROW_TILES, TILE as DEEMP_TILE, deemp_alpha  # noqa: E402
from test_gpu_deemp import meets_bound as deemp_meets_bound  # noqa: E402
from test_demod_cpu import am_candidates, am_row_ok, fm_ref_rows, phasor_speed, phasor_speeds  # noqa: E402
from test_ff_agc_cpu import ffagc_ref  # noqa: E402
from test_gpu_fuzz import FAMILIES  # noqa: E402
from test_gpu_handover import F_A, F_B, TOL_HEAD, TOL_HIST, TOL_PHASE, TOL_RMS, _plans, _steer  # noqa: E402
from test_gpu_numerics import CHAN, CHAN_F, FAM, FAM_IDS, _os_layout, _pin, _taps  # noqa: E402
from test_gpu_rs import Pool, gen_frames  # noqa: E402
from test_gpu_stereo_fm import REGIME_GAP  # noqa: E402
from test_level_cpu import ROW_TILES as LEVEL_ROW_TILES, TILE as LEVEL_TILE, agc_decay, agc_exact_decay, agc_ref, squelch_ref  # noqa: E402
from test_stereo_fm_cpu import cfr_of, modulate, pilot_taps as sfm_pilot_taps, stereo_mix_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, ROWS_WAVE = 5, 17            # 17: past the 16 rows of one wave of costas_kernel / mm_clock_kernel
TILE = 2048                        # kDemodNT * kDemodSpl: the tile of the per-row kernels
N_DIRECT = 3 * 4096 + 37           # direct, MFMA and window kernels: three tiles (of at most 4096 samples) and a tail
_SEEN = set()                      # kernel names of the async runs
_RACED = set()                     # (class name, method) of every host action that ran with its window open
PER_ROW_FAMILIES = {"fm_demod_kernel", "am_sub_kernel", "ssb_demod_kernel", "deemp_row_kernel", "deemp_scan_kernel", "level_row_kernel",
                    "level_apply_kernel", "stereo_mix_kernel", "ff_agc_kernel", "cagc_row_kernel", "cagc_scan_kernel", "costas_kernel",
                    "mm_clock_kernel", "row_fir_kernel", "delay_imag_kernel", "threshold_kernel", "deframe_match_kernel", "rs_decode_kernel",
                    "hrpt_avhrr_kernel", "tip_kernel", "hirs_pack_kernel"}
DMA = {"fir_fft_dma_kernel", "fir_fft_dmapk_kernel"}     # members of the 4096-point overlap-save family (conftest.kname)
OVERLAP_SAVE = DMA | {"fir_fft_kernel", "fir_fft1k_kernel", "pfb_dec8_kernel", "pfb_dec4_kernel", "pfb_dec8_real_kernel", "pfb_dec4_real_kernel"}
DIRECT_FORMS = {"fir_core_kernel", "fir_lat_kernel", "decim_win_kernel", "decim_mfma_kernel", "decim_mfma_real_kernel", "resamp_lm_kernel",
                "resamp_mfma_kernel", "resamp_mfma_real_kernel", "resamp_any_kernel"}      # what set_mode(DIRECT) may run: no overlap-save form


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
    path = os.environ.get("ASYNC_ORDER_REPORT")
    if path:
        A.write_report(path)


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rows(a):
    """A (rows, n) host array as a device tensor whose row stride is n + 1."""
    import torch

    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a)
    buf = torch.zeros((a.shape[0], a.shape[1] + 1) + a.shape[2:], dtype=t.dtype, device="cuda")
    buf[:, :a.shape[1]] = t.cuda()
    return buf[:, :a.shape[1]]


class _In:
    """An input that reaches the operator through a copy queued on the CURRENT stream (behind the hold, in an async run) into a
    buffer that holds zeros until then: a kernel, copy or memset that the library puts on another stream than the caller's runs
    ahead of that copy, reads the zeros and shows in the output.  `rows`: a (rows, n) array with row stride n + 1."""

    def __init__(self, host, rows=False):
        import torch

        self.src = _rows(host) if rows else _dev(host)
        self.dst = _rows(np.zeros_like(host)) if rows else torch.zeros_like(self.src)

    def __call__(self):
        self.dst.copy_(self.src)
        return self.dst


def _family(names):
    return set(names) | (DMA if "fir_fft_kernel" in names else set())


def _three_ways(name, scenario):
    """Run the scenario in the three modes, compare them bit for bit, note what the async run covered; returns the serial Result."""
    null, serial, asy = A.run_modes(name, scenario)
    A.assert_same(name, serial, null, "side stream with a synchronise after every step / null stream")
    A.assert_same(name, asy, serial, "side stream with queued work / the same with a synchronise after every step")
    _SEEN.update(k for _, k in asy.kernels)
    for op, method in asy.raced:
        if op is not None:
            _RACED.add((type(op).__name__, method))      # (a chain's Borrowed* stage view counts under its own name: a public
            #                                              class's method must have been raced on a handle of that very class)
    return serial


def _anchor(serial):
    """Every step's own check of the serial run's value (the reference models live in the steps' closures)."""
    for st, (_, vals) in zip(serial.steps, serial.outputs):
        chk = getattr(st, "check", None)
        if chk is not None:
            chk(vals)


def _checked(step, check):
    step.check = check
    return step


def _close_to(label, got, want, head=0):
    """The handover module's bounds: relative RMS of the call, and the first `head` outputs against max|want|."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    if not want.size:
        return
    rms = rel_rms(got, want)
    assert rms <= TOL_RMS, f"{label}: relative RMS {rms:.3e} against the FP64 oracle"
    if head:
        top = float(np.abs(want).max())
        err = float(np.abs(got[..., :head] - want[..., :head]).max()) / top
        assert err <= TOL_HEAD, f"{label}: head of the call off by {err:.3e} x max|want|"


# ------------------------------------------------------------------------------------------------ control: the harness sees a race
def test_control_a_race_shows_and_the_hold_holds():
    """Behind a hold on stream A a copy dst <- src is queued; stream B, not ordered against A, overwrites src.  Both are in-bounds
    copies of live tensors.  dst must then hold the NEW values -- unlike the serial run's dst: if it does not, the hold is not
    holding and every async scenario of this module would pass vacuously."""
    import torch

    a, b = A.side_stream(), A.side_stream()
    src = torch.arange(1 << 16, dtype=torch.float32, device="cuda")
    other = torch.full((1 << 16,), -1.0, dtype=torch.float32, device="cuda")
    dst_serial, dst_async = torch.zeros_like(src), torch.zeros_like(src)
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        dst_serial.copy_(src)
    a.synchronize()
    with torch.cuda.stream(b):
        src.copy_(other)
    b.synchronize()
    src.copy_(torch.arange(1 << 16, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    A.hold(a, 20.0)
    with torch.cuda.stream(a):
        dst_async.copy_(src)
    w = A.Window(a)
    w.assert_open("the racing overwrite of the control")
    with torch.cuda.stream(b):
        src.copy_(other)
    b.synchronize()
    still_open = w.is_open()
    a.synchronize()
    torch.cuda.synchronize()
    assert still_open, "the hold ended before the racing copy had finished: it is not holding"
    want, got = dst_serial.cpu().numpy(), dst_async.cpu().numpy()
    assert np.array_equal(want, np.arange(1 << 16, dtype=np.float32))
    assert not A.same_bits(got, want), "the racing overwrite did not show in dst: the harness cannot see a race"
    assert np.array_equal(got, np.full(1 << 16, -1.0, np.float32)), "dst holds neither the old nor the new values"


# ------------------------------------------------------------------------------------------------ engine handles
def _rotated(raw, xl):
    """`raw` (the H samples before the next call) times the oracle mixer's phasor at their positions, FP64 phase, no magnitude term."""
    d = math.atan2(float(xl.delta[1]), float(xl.delta[0])) / (2 * math.pi)
    k = np.arange(len(raw), dtype=np.float64) - len(raw)
    return (np.asarray(raw).astype(np.complex128) * np.exp(2j * np.pi * ((xl.turns.value + k * d) % 1.0))).astype(np.complex64)


def _advance(xl, n):
    """*_advance(n): the oracle mixer's phase n samples on."""
    xl.turns.value = (xl.turns.value + n * math.atan2(float(xl.delta[1]), float(xl.delta[0])) / (2 * math.pi)) % 1.0


class _EngineModel:
    """The FP64 oracle of one engine handle and the steps' expectations: Fir / Resampler (cls 0 complex, 2 real) and the fused VFO
    (cls 1: the exact-phase mixer in front)."""

    def __init__(self, L, M, real, taps, vfo):
        self.L, self.M, self.real, self.vfo = L, M, real, vfo
        self.fir = (L, M) == (1, 1) and not vfo
        self.ch = 1 if real else 2
        self.orc = self._oracle(taps)
        self.xl = O.Xlator(1.0, F_A, exact=True, volk_gain=True) if vfo else None

    def _oracle(self, taps):
        if self.fir:
            return O.Fir(taps, complex_data=not self.real, acc=O.ACC_F64)
        return O.Resampler(taps, self.L, self.M, complex_data=not self.real, acc=O.ACC_F64)

    def H(self):
        return (len(self.orc.hist) // self.ch) - (1 if self.fir else 0)

    def retaps(self, taps):
        old, h_old = self.orc.hist, self.H()
        self.orc = self._oracle(taps)
        keep = min(h_old, self.H()) * self.ch      # the newest history_len samples stay (the oracle's FIR buffer holds one more)
        self.orc.hist[len(self.orc.hist) - keep:] = old[len(old) - keep:]

    def history(self):
        h = self.orc.hist[len(self.orc.hist) - self.H() * self.ch:]
        return h.copy() if self.real else h.copy().view(np.complex64)

    def set_history(self, h):
        h = np.ascontiguousarray(h, np.float32 if self.real else np.complex64).view(np.float32)
        self.orc.hist[len(self.orc.hist) - len(h):] = h

    def set_history_raw(self, raw):
        """set_history_dev: the history_len RAW input samples before the next call; a handle with an NCO rotates them with the
        phases they would have had, phase - H dphase onward (qdsp_hip.hip)."""
        self.set_history(_rotated(raw, self.xl) if self.xl is not None else raw)

    def reset(self):
        self.orc.reset()
        if self.xl is not None:
            self.xl.turns.value = 0.0

    def retune(self, f):
        O.lib().oracle_xlator_phase_delta(1.0, f, O._fp(self.xl.delta))

    def set_phase(self, re, im):
        self.xl.turns.value = math.atan2(float(im), float(re)) / (2 * math.pi)

    def process(self, x):
        return self.orc.process(self.xl.process(x) if self.xl is not None else x)

    def phase(self):
        return np.exp(2j * np.pi * self.xl.turns.value)


def _engine_scenario(ops, make, L, M, ntaps, real, n, expect, vfo=False, mode=None, seed=1):
    """The issue's engine sequence; two calls between any two host actions, so that a call that rebuilds a table at call time (and
    so drains the queue) still leaves one queued behind the next hold."""
    taps = _taps(L, M, ntaps)
    taps_b = (_taps(L, M, ntaps) * np.float32(0.75)).astype(np.float32)[::-1].copy()
    taps_long = _taps(L, M, ntaps + 8)
    state = {"pos": 0}

    def block():
        x = O.synth_iq(state["pos"], n, seed=seed)
        state["pos"] += n
        return np.ascontiguousarray(x.real) if real else x

    def scenario():
        state["pos"] = 0
        op = make(taps)
        model = _EngineModel(L, M, real, taps, vfo)
        H0 = op.history_len
        rng = np.random.default_rng(seed)
        hist_a = rng.standard_normal(H0 * (1 if real else 2)).astype(np.float32)
        hist_b = rng.standard_normal(H0 * (1 if real else 2)).astype(np.float32)
        hist_a, hist_b = (hist_a, hist_b) if real else (hist_a.view(np.complex64), hist_b.view(np.complex64))
        hist_b_dev = _dev(hist_b)
        steps = []

        def calls(exp=expect, anchored=True):
            for _ in range(2):
                x = block()
                xd = _In(x)
                k = len(steps)
                st = Call(f"process {k}", lambda xd=xd: op.process(xd()), op, exp)
                if anchored:
                    head = -(-model_H() // M) + 1
                    st.check = lambda v, x=x, k=k, head=head: _close_to(f"call {k}", v[0], model.process(x), head)
                else:
                    st.check = lambda v, x=x: model.process(x)     # (keeps the model's state moving)
                steps.append(st)

        def model_H():
            return H0

        def host(step, act=None, check=None):
            def chk(v):
                if act is not None:
                    act()
                if check is not None:
                    check(v)
            steps.append(_checked(step, chk))

        retap = (lambda t: H(op, "set_taps", t)) if (L, M) == (1, 1) and not vfo else (lambda t: H(op, "configure", t, L, M))
        calls()
        host(retap(taps_b), lambda: model.retaps(taps_b))
        calls()
        host(retap(taps_long), lambda: model.retaps(taps_long))      # another length: the history is resized
        calls(exp=None)
        host(retap(taps), lambda: model.retaps(taps))
        calls()

        def same_history(v):
            want = model.history()
            if vfo:
                assert np.abs(v[0] - want).max() <= TOL_HIST, "get_history: rotated history off the exact-phase mixer"
            else:
                assert np.array_equal(v[0], want), "get_history is not the last history_len input samples"
        host(H(op, "get_history"), None, same_history)
        calls()
        host(H(op, "reset"), model.reset)
        calls()
        host(H(op, "set_history", hist_a), lambda: model.set_history(hist_a))
        calls()
        host(H(op, "set_history_dev", hist_b_dev), lambda: model.set_history_raw(hist_b))
        calls()
        if vfo:
            host(H(op, "set_phase_inc", *ops.phase_delta(1.0, F_B)), lambda: model.retune(F_B))
            calls()
            re, im = np.float32(math.cos(1.37)), np.float32(math.sin(1.37))
            host(H(op, "set_phase", float(re), float(im)), lambda: model.set_phase(re, im))
            calls()
            host(H(op, "set_volk_gain", False), lambda: setattr(model.xl, "volk_gain", False))
            calls()
            host(H(op, "advance", 777), lambda: _advance(model.xl, 777))       # (the NCO moves on, the raw side history is dropped)
            calls()
        host(H(op, "set_mode", op.DIRECT))
        calls(exp=DIRECT_FORMS)
        if vfo:
            host(H(op, "set_mode", op.FFT))
            calls(exp=OVERLAP_SAVE)
        host(H(op, "set_mode", op.AUTO if mode is None else mode))
        calls()
        if vfo:
            host(H(op, "get_phase"), None, lambda v: abs(complex(v[0]) - model.phase()) < TOL_PHASE or pytest.fail(f"get_phase {v[0]} / {model.phase()}"))
        return steps

    return scenario


def _fam_n(fam):
    if fam[7] is None:
        return N_DIRECT
    return 3 * _os_layout(fam)[0] + 37          # overlap-save: three segments of the family's unit and a ragged tail


@pytest.mark.parametrize("fam", FAM, ids=FAM_IDS)
def test_engine_handles(ops, monkeypatch, fam):
    """Fir and Resampler, complex and real data, in every kernel family of tests/test_gpu_numerics.py."""
    _pin(monkeypatch, fam[3])
    name, (L, M, ntaps), real, _, mode, names, _, _ = fam
    fir = (L, M) == (1, 1)
    m = {"fft": 2, "direct_mode": 1, None: 0}[mode]

    def make(taps):
        op = ops.Fir(taps, complex_data=not real, max_block=0) if fir else ops.Resampler(taps, L, M, complex_data=not real, max_block=0)
        op.set_mode(m)
        return op

    sc = _engine_scenario(ops, make, L, M, ntaps, real, _fam_n(fam), _family(names), mode=m, seed=len(name))
    serial = _three_ways(f"engine {name}", sc)
    _anchor(serial)


def _vfo_cases():
    out = []
    for label, cls, M, ntaps, families in _plans():
        if cls == 1:
            out += [(label, M, ntaps, f) for f in families]
    return out


def _vfo_n(M, ntaps, family):
    """Three units of the family and a ragged tail, and at least the 4 500 samples tests/test_gpu_handover.py's steering is made for."""
    if family.startswith("pfb"):
        unit = _os_layout((family, (1, M, ntaps), None, None, None, None, None, 4096))[0]
    elif family == "fir_fft1k_kernel":
        unit = _os_layout(("fir_fft1k", (1, M, ntaps), None, None, None, None, None, 1024))[0]
    elif family == "fir_fft_kernel":
        unit = _os_layout(("fir_fft", (1, M, ntaps), None, None, None, None, None, 4096))[0]
    else:
        return N_DIRECT
    k = 3
    while k * unit + 37 < 4500:
        k += 1
    return k * unit + 37


@pytest.mark.parametrize("case", _vfo_cases(), ids=lambda c: f"{c[0]}-{c[3]}")
def test_fused_vfo_forms(ops, monkeypatch, case):
    """The fused VFO in every kernel form tests/test_gpu_handover.py steers it to, with the NCO's setters and getters on top."""
    label, M, ntaps, family = case
    mode, env = _steer(family)
    for k, v in env.items():
        monkeypatch.setenv("QDSP_HIP_" + k, v)

    def make(taps):
        op = ops.Vfo(taps, 1, M, ops.phase_delta(1.0, F_A), max_block=0)
        op.set_mode(mode)
        return op

    sc = _engine_scenario(ops, make, 1, M, ntaps, False, _vfo_n(M, ntaps, family), _family({family}), vfo=True, mode=mode, seed=M + len(family))
    serial = _three_ways(f"vfo {label} {family}", sc)
    _anchor(serial)


# ------------------------------------------------------------------------------------------------ channelizer
class _ChanChains:
    """Splitter -> N x VFO as the reference runs it: per channel the exact-phase oracle mixer, then the FP64 resampler (each channel's
    history holds ITS mixer's output, so a retune does not reach back into it).  The interface of ChanUniform64 as far as used here."""

    def __init__(self, taps, incs, M):
        self.xl = [O.Xlator(1.0, 0.0, exact=True, volk_gain=False) for _ in incs]
        self.rs = [O.Resampler(taps, 1, M, acc=O.ACC_F64) for _ in incs]
        for c, inc in enumerate(incs):
            self.set_phase_inc(c, *inc)

    def plan(self):
        return None

    def set_phase_inc(self, c, re, im):
        self.xl[c].delta[:] = (re, im)

    def set_volk_gain(self, on):
        for xl in self.xl:
            xl.volk_gain = on

    def advance(self, n):
        for xl in self.xl:
            _advance(xl, n)

    def reset(self):
        for xl, rs in zip(self.xl, self.rs):
            xl.turns.value = 0.0
            rs.reset()

    def set_history_raw(self, raw):
        for xl, rs in zip(self.xl, self.rs):
            rs.hist[:] = _rotated(raw, xl).view(np.float32)

    def exact(self, x):
        return np.stack([rs.process(xl.process(x)) for xl, rs in zip(self.xl, self.rs)])


def _chan_scenario(ops, taps, M, incs, expect, n, retune0, far, direct=False, seed=5):
    """The bank's sequence.  retune0: channel 0's new increment (the folded taps / the batch table are rebuilt); far: (channel, inc)
    of a retune that leaves chan_uniform_plan's tolerance (a path switch for the uniform plan).  The reference is ChanUniform64:
    `uniform` while the library runs the uniform form, `exact` (rotate, then filter) otherwise; volk gain off, as that model has none."""
    from qdsp_amd import capi

    nch = len(incs)
    state = {"pos": 0}

    def block():
        x = O.synth_iq(state["pos"], n, seed=seed)
        state["pos"] += n
        return x

    def scenario():
        state["pos"] = 0
        ch = ops.Channelizer(taps, 1, M, incs, max_block=0)
        ch.set_volk_gain(False)
        if direct:
            ch.set_mode(ch.DIRECT)
        model = NU.ChanUniform64(taps, incs, M) if nch == 64 else _ChanChains(taps, incs, M)
        flags = {"direct": direct, "volk": False}
        hist = O.synth_iq(0, ch.history_len, seed=seed + 1)
        hist_dev = _dev(hist)
        steps = []

        def want(x):
            uni = nch == 64 and not flags["direct"] and model.plan() is not None
            return model.uniform(x) if uni else model.exact(x)

        def calls(exp=expect):
            for _ in range(2):
                x = block()
                xd = _In(x)
                k = len(steps)
                st = Call(f"process {k}", lambda xd=xd: ch.process(xd()), ch, exp)

                def chk(v, x=x, k=k):
                    w = want(x)
                    if flags["volk"] and nch == 64:     # (ChanUniform64 has no magnitude term; the per-channel chains have)
                        return
                    head = -(-len(taps) // M) + 1
                    for c in range(nch):
                        _close_to(f"call {k} channel {c}", v[0][c], w[c], head)
                steps.append(_checked(st, chk))

        def host(step, act=None):
            steps.append(_checked(step, (lambda v: act()) if act else None))

        def set_inc(c, inc):
            L = capi.load()
            return Host(f"chan set_phase_inc({c})", lambda: capi.check(L.qdsp_hip_chan_cf32_set_phase_inc(ch._h, c, *inc)))

        calls()
        host(set_inc(0, retune0), lambda: model.set_phase_inc(0, *retune0))
        calls()
        host(set_inc(*far), lambda: model.set_phase_inc(far[0], *far[1]))
        calls(exp=None if nch == 64 else expect)
        host(set_inc(far[0], incs[far[0]]), lambda: model.set_phase_inc(far[0], *incs[far[0]]))
        calls()
        host(H(ch, "reset"), model.reset)
        calls()

        def set_hist():
            if nch == 64:
                model.hist = hist.astype(np.complex128)
            else:
                model.set_history_raw(hist)
        host(H(ch, "set_history_dev", hist_dev), set_hist)
        calls()
        host(H(ch, "advance", 777), lambda: model.advance(777))
        calls()
        def volk(on):
            flags.update(volk=on)
            if nch != 64:
                model.set_volk_gain(on)
        host(H(ch, "set_volk_gain", True), lambda: volk(True))
        calls()
        host(H(ch, "set_volk_gain", False), lambda: volk(False))
        calls()
        if not direct:
            host(H(ch, "set_mode", ch.DIRECT), lambda: flags.update(direct=True))
            calls(exp=None)
            host(H(ch, "set_mode", ch.AUTO), lambda: flags.update(direct=False))
            calls()
        return steps

    return scenario


def test_channelizer_uniform_plan(ops, monkeypatch):
    """64 channels on the grid, decimation 16, 256 taps: chan_uniform_kernel; a retune of one channel beyond the plan's tolerance
    switches to a batched form (chan_refresh_vfo_hist) and back."""
    _pin(monkeypatch, {})
    taps = _taps(1, 16, 256)
    incs = [ops.phase_delta(1.0, -(c - 31.5) / 64) for c in range(64)]
    t0 = NU.fx_of_inc(*incs[0]) / 2.0 ** 64
    retune0 = NU.inc_of_turns(t0 + 1e-7)            # inside the tolerance of 4e-7 turn: the same plan, new folded taps
    far = (5, ops.phase_delta(1.0, -(5 - 31.5) / 64 + 0.003))
    sc = _chan_scenario(ops, taps, 16, incs, {"chan_uniform_kernel"}, N_DIRECT, retune0, far)
    serial = _three_ways("channelizer uniform", sc)
    _anchor(serial)


@pytest.mark.parametrize("cfg", CHAN, ids=[c[0] for c in CHAN])
def test_channelizer_batched_forms(ops, monkeypatch, cfg):
    """Arbitrary offsets: all channels in one launch of decim_mfma_batch_kernel / resamp_any_batch_kernel."""
    _pin(monkeypatch, cfg[1])
    taps = _taps(1, 64, 256)
    incs = [ops.phase_delta(1.0, f) for f in CHAN_F]
    sc = _chan_scenario(ops, taps, 64, incs, {cfg[2]}, N_DIRECT, ops.phase_delta(1.0, F_B), (1, ops.phase_delta(1.0, 0.4141)))
    serial = _three_ways(f"channelizer {cfg[0]}", sc)
    _anchor(serial)


def test_channelizer_per_channel_loop(ops, monkeypatch):
    """set_mode(DIRECT): one launch per channel on the channels' own engine handles."""
    _pin(monkeypatch, {})
    taps = _taps(1, 64, 256)
    incs = [ops.phase_delta(1.0, f) for f in CHAN_F]
    sc = _chan_scenario(ops, taps, 64, incs, None, N_DIRECT, ops.phase_delta(1.0, F_B), (1, ops.phase_delta(1.0, 0.4141)), direct=True)
    serial = _three_ways("channelizer per-channel loop", sc)
    _anchor(serial)


# ------------------------------------------------------------------------------------------------ per-row operators
def _cx(rng, rows, n, scale=0.5):
    return (scale * (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n)))).astype(np.complex64)


def _re(rng, rows, n, scale=0.5):
    return (scale * rng.standard_normal((rows, n))).astype(np.float32)


def _pb(op, x):
    """process_batch; operators whose output rows are only partly written (a count per row) get zeroed rows to write into."""
    import torch

    from qdsp_amd import ops as P

    if isinstance(op, (P.MmClockRecovery, P.PskDemod, P.MskDemod)):
        real = isinstance(op, P.MskDemod) or (isinstance(op, P.MmClockRecovery) and op.kind == P.MmClockRecovery.REAL)
        dt = torch.float32 if real else torch.complex64
        return op.process_batch(x, out=torch.zeros((op.nchan, max(op.out_size(x.shape[1]), 1)), dtype=dt, device=x.device))
    if isinstance(op, P.StereoFmDemod):            # the outputs, and the handle's own rows of the filtered pilot, copied behind the call
        y = op.process_batch(x)
        ptr, stride = op.pilot_ptr()

        class _Holder:
            pass

        holder = _Holder()
        holder.__cuda_array_interface__ = {"shape": (op.nchan * stride,), "typestr": "<f4", "data": (ptr, False), "version": 2}
        f = torch.as_tensor(holder, device=x.device).view(op.nchan, stride)[:, :x.shape[1]].clone()
        return y, f
    if isinstance(op, P.Deframer):
        nb = op.out_size(x.shape[1]) * op.frame_bytes
        return op.process_batch(x, out=torch.zeros((op.nchan, max(nb, 1)), dtype=torch.uint8, device=x.device))
    return op.process_batch(x)


# ---- the per-row models: the operator's numpy definition carried through the scenario's steps, as _EngineModel carries the oracle.
# A setter changes the model's parameters, set_state / reset its state; `process(x)` is the reference of one process_batch over the
# rows x; `check(got, want, x)` compares the serial run's value with it (bit for bit unless the kind's own GPU test has a bound);
# a getter is compared with the model's method of the same name.
F32 = np.float32


class _RowModel:
    def __init__(self, rows):
        self.rows = rows

    def of(self, chan):
        return range(self.rows) if chan < 0 else [chan]

    def check(self, got, want, x, label):
        assert A.same_bits(np.asarray(got[0]), np.asarray(want)), f"{label}: not the operator's definition bit for bit"


class _FmModel(_RowModel):
    def __init__(self, rows, sr, dev, stereo):
        super().__init__(rows)
        self.speeds = phasor_speeds(sr, np.full(rows, dev, F32))
        self.phases, self.stereo = np.zeros(rows, F32), stereo

    def set_fm(self, sr, dev, chan):
        for r in self.of(chan):
            self.speeds[r] = phasor_speed(sr, dev)

    def set_phase(self, p, chan):
        for r in self.of(chan):
            self.phases[r] = F32(p)

    def get_phase(self, chan):
        return self.phases[chan]

    def reset(self):
        self.phases[:] = 0

    def process(self, x):
        out, self.phases = fm_ref_rows(x, self.speeds, self.phases)
        return np.stack([out, out], axis=-1) if self.stereo else out


class _AmModel(_RowModel):
    def process(self, x):
        return [am_candidates(r) for r in x]

    def check(self, got, want, x, label):
        for r in range(self.rows):
            assert am_row_ok(got[0][r], want[r]), f"{label}: AM row {r}"


class _SquelchModel(_RowModel):
    def __init__(self, rows, level):
        super().__init__(rows)
        self.levels, self.open = [level] * rows, [False] * rows

    def set_level(self, level, chan):
        for r in self.of(chan):
            self.levels[r] = level

    def is_open(self, chan):
        return self.open[chan]

    def reset(self):
        self.open = [False] * self.rows

    def process(self, x):
        res = [squelch_ref(x[r], self.levels[r]) for r in range(self.rows)]
        self.open = [o for _, o in res]
        return np.stack([y for y, _ in res])


class _AgcModel(_RowModel):
    def __init__(self, rows, fall, sr):
        super().__init__(rows)
        self.cfr, self.lvl = [F32(F32(fall) / F32(sr))] * rows, [F32(0)] * rows

    def set(self, fall, sr, chan):
        for r in self.of(chan):
            self.cfr[r] = F32(F32(fall) / F32(sr))

    def set_level(self, level, chan):
        for r in self.of(chan):
            self.lvl[r] = F32(level)

    def level(self, chan):
        return self.lvl[chan]

    def reset(self):
        self.lvl = [F32(0)] * self.rows

    def process(self, x):
        out = []
        for r in range(self.rows):
            assert x[r].max() > 1.01 * agc_decay(self.lvl[r], self.cfr[r], x.shape[1]), "peak regime (where agc_ref is bit-exact)"
            y, self.lvl[r] = agc_ref(x[r], self.lvl[r], self.cfr[r])
            out.append(y)
        return np.stack(out)


class _FfAgcModel(_RowModel):
    def __init__(self, rows, window, dtype):
        super().__init__(rows)
        self.window, self.dt = window, dtype
        self.reset()

    def reset(self):
        self.hist = [np.zeros(0, self.dt) for _ in range(self.rows)]

    def set_history(self, h, chan):
        for r in self.of(chan):
            self.hist[r] = np.asarray(h, self.dt).copy()

    def get_history(self, chan):
        return self.hist[chan]

    def fill(self):
        return len(self.hist[0])

    def process(self, x):
        res = [ffagc_ref(x[r], self.window, self.hist[r]) for r in range(self.rows)]
        self.hist = [h for _, h in res]
        return np.stack([y for y, _ in res])


class _RowFirModel(_RowModel):
    def __init__(self, rows, taps, cplx):
        super().__init__(rows)
        self.cplx, self.ch = cplx, 2 if cplx else 1
        self.f = [O.Fir(taps, complex_data=cplx, acc=O.ACC_FMA) for _ in range(rows)]

    def set_taps(self, taps, chan):
        for r in self.of(chan):
            old = self.f[r].hist
            self.f[r] = O.Fir(taps, complex_data=self.cplx, acc=O.ACC_FMA)
            keep = min(len(old), len(self.f[r].hist)) - self.ch         # the newest ntaps - 1 samples stay
            if keep > 0:
                self.f[r].hist[len(self.f[r].hist) - keep:] = old[len(old) - keep:]

    def set_history(self, h, chan):
        h = np.ascontiguousarray(h, np.complex64 if self.cplx else F32).view(F32)
        for r in self.of(chan):
            self.f[r].hist[len(self.f[r].hist) - len(h):] = h

    def get_history(self, chan):
        h = self.f[chan].hist[self.ch:].copy()
        return h.view(np.complex64) if self.cplx else h

    def reset(self):
        for f in self.f:
            f.reset()

    def process(self, x):
        return np.stack([self.f[r].process(x[r]) for r in range(self.rows)])


class _DelayModel(_RowModel):
    def __init__(self, rows):
        super().__init__(rows)
        self.reset()

    def reset(self):
        self.last = [F32(0)] * self.rows

    def set_state(self, v, chan):
        for r in self.of(chan):
            self.last[r] = F32(v)

    def get_state(self, chan):
        return self.last[chan]

    def process(self, x):
        res = [delay_imag_ref(x[r], self.last[r]) for r in range(self.rows)]
        self.last = [l for _, l in res]
        return np.stack([y for y, _ in res])


class _ThresholdModel(_RowModel):
    def process(self, x):
        return np.stack([DF.threshold_ref(r) for r in x])


class _CountedModel(_RowModel):
    """Kinds that emit a count per row: the value is (rows, counts); a row's slots past its count stay as they were (zero)."""

    def check(self, got, want, x, label):
        rows, counts = got
        for r in range(self.rows):
            w = np.asarray(want[r]).reshape(-1)
            assert counts[r] == self.count_of(want[r]), f"{label}: count of row {r}: {counts[r]} / {self.count_of(want[r])}"
            assert A.same_bits(rows[r, :len(w)], w), f"{label}: row {r} is not the definition bit for bit"
            assert not rows[r, len(w):].any(), f"{label}: row {r} written past its count"

    def counts(self):
        return np.asarray(self.last_counts, np.int32)


class _MmModel(_CountedModel):
    def __init__(self, rows, kind, omega):
        super().__init__(rows)
        self.kind, self.taps = kind, MM.lib_taps()
        self.p = [[omega, 0.01 * 0.01 / 4, 0.01, 0.005] for _ in range(rows)]
        self.reset()

    def count_of(self, w):
        return len(w)

    def reset(self):
        self.st = [MM.new_state(self.kind, MM.params(*p)) for p in self.p]
        self.last_counts = [0] * self.rows

    def set_omega(self, omega, chan):
        for r in self.of(chan):
            self.p[r][0] = omega
            self.st[r]["dyn"] = F32(omega)

    def set_gains(self, go, gm, chan):
        for r in self.of(chan):
            self.p[r][1:3] = [go, gm]

    def set_limit(self, rel, chan):
        for r in self.of(chan):
            self.p[r][3] = rel

    def set_interp_taps(self, taps):
        self.taps = np.asarray(taps, F32)

    def set_state(self, mu, dyn, nxt, chan):
        for r in self.of(chan):
            self.st[r].update(mu=F32(mu), dyn=F32(dyn), next=int(nxt))

    def get_state(self, chan):
        s = self.st[chan]
        return float(s["mu"]), float(s["dyn"]), int(s["next"])

    def process(self, x):
        out = []
        for r in range(self.rows):
            y, self.st[r] = MM.mm_ref(x[r], self.kind, MM.params(*self.p[r]), self.st[r], self.taps)
            out.append(y)
        self.last_counts = [len(y) for y in out]
        return out


class _DeframerModel(_CountedModel):
    def __init__(self, rows, flt, frame=None, sync=None):
        super().__init__(rows)
        self.flt, self.frame, self.sync = flt, FRAME if frame is None else frame, SYNC if sync is None else sync
        self.reset()

    def count_of(self, w):
        return len(w)

    def reset(self):
        self.st = [DF.new_state(self.frame, len(self.sync)) for _ in range(self.rows)]
        self.last_counts = [0] * self.rows

    def set_sync(self, sync):
        self.sync = np.asarray(sync, np.uint8)

    def set_state(self, bits_read, bad, after, chan):
        for r in self.of(chan):
            self.st[r].update(bits_read=bits_read, bad=bad, after=bool(after))

    def get_state(self, chan):
        s = self.st[chan]
        return int(s["bits_read"]), int(s["bad"]), bool(s["after"])

    def process(self, x, counts=None):
        out = []
        for r in range(self.rows):
            row = x[r] if counts is None else x[r][:counts[r]]
            frames, _, self.st[r] = DF.deframe_ref(DF.threshold_ref(row) if self.flt else row, self.frame, self.sync, self.st[r])
            out.append(frames)
        self.last_counts = [len(f) for f in out]
        return out


class _DeempModel(_RowModel):
    """FP64 scan against the exact recurrence: bound 1 of tests/test_gpu_deemp.py (meets_bound), per row, from the exact state."""

    def __init__(self, rows, sr, tau, stereo):
        super().__init__(rows)
        self.al, self.stereo, self.bypassed = [deemp_alpha(sr, tau)] * rows, stereo, False
        self.reset()

    def reset(self):
        z = np.zeros(2, LD) if self.stereo else LD(0)
        self.st, self.rounded = [z] * self.rows, [None] * self.rows

    def set(self, sr, tau, chan):
        for r in self.of(chan):
            self.al[r] = deemp_alpha(sr, tau)

    def bypass(self, on):
        self.bypassed = on

    def alpha(self, chan):
        return self.al[chan]

    def set_state(self, l, r_, chan):
        for r in self.of(chan):
            self.st[r] = np.asarray([F32(l), F32(r_)], LD) if self.stereo else LD(F32(l))
            self.rounded[r] = None

    def process(self, x):
        return None

    def check(self, got, want, x, label):
        y = got[0]
        for r in range(self.rows):
            if self.bypassed:
                assert A.same_bits(y[r], x[r]), f"{label}: bypass is a copy"
            else:
                self.st[r] = deemp_meets_bound(y[r], x[r], self.al[r], self.st[r], f"{label} row {r}")
                self.rounded[r] = y[r][-1]            # the carried output, rounded to float: what the call's last sample shows

    def get_state(self, chan):
        v = self.rounded[chan] if self.rounded[chan] is not None else np.asarray(self.st[chan], F32)
        return (F32(v[0]), F32(v[1])) if self.stereo else F32(v)


class _CagcModel(_RowModel):
    """FP64 clamped scan against the exact recurrence: the bound of tests/test_gpu_cagc.py (check_against_truth, check_gain),
    per row, from the exact gain."""

    def __init__(self, rows, sp, mg, rate):
        super().__init__(rows)
        self.p = [(sp, mg, rate)] * rows
        self.reset()

    def reset(self):
        self.g, self.M, self.extra = [LD(1)] * self.rows, [None] * self.rows, [LD(0)] * self.rows

    def set(self, sp, mg, rate, chan):
        for r in self.of(chan):
            self.p[r] = (sp, mg, rate)

    def set_gain(self, g, chan):
        for r in self.of(chan):
            self.g[r], self.M[r], self.extra[r] = LD(np.float64(g)), None, LD(0)

    def process(self, x):
        return None

    def check(self, got, want, x, label):
        for r in range(self.rows):
            assert cagc_in_domain(x[r], self.p[r][2]), "the scan's domain"
            exact = cagc_exact(x[r], *self.p[r], self.g[r])
            cagc_check(got[0][r], x[r], exact, None, f"{label} row {r}", extra=self.extra[r])
            self.g[r], self.M[r] = exact[4], exact[3][-1]
            self.extra[r] = self.extra[r] + cagc_gain_bound(self.M[r])      # what the device's own starting gain may be off by

    def check_getter(self, method, got, chan):
        assert abs(LD(np.float64(got[0])) - self.g[chan]) <= self.extra[chan], (method, chan, got, float(self.g[chan]))
        return True


class _CostasModel(_RowModel):
    """The bound of tests/test_gpu_costas.py: against the longdouble recurrence (costas_truth) the device may be off by 4 x what the
    reference's own float loop (costas_ref) is off by, in the outputs of every call and in the carried frequency and phase.  Both
    loops are carried through the steps, each from its own state."""

    def __init__(self, rows, order, bw):
        super().__init__(rows)
        self.order, self.bw = order, [bw] * rows
        self.reset()

    def reset(self):
        self.tf, self.tp = np.zeros(self.rows, LD), np.zeros(self.rows, LD)
        self.rf, self.rp = np.zeros(self.rows, F32), np.zeros(self.rows, F32)

    def set_bandwidth(self, bw, chan):
        for r in self.of(chan):
            self.bw[r] = bw

    def set_state(self, f, p, chan):
        for r in self.of(chan):
            self.tf[r], self.tp[r], self.rf[r], self.rp[r] = LD(np.float64(f)), LD(np.float64(p)), F32(f), F32(p)

    def process(self, x):
        al, be = (np.asarray(v, F32) for v in zip(*[costas_gains(b) for b in self.bw]))
        truth = costas_truth(x.T, self.order, al, be, self.tf, self.tp)
        ref, self.rf, self.rp = costas_ref(x.T, self.order, al, be, self.rf, self.rp)
        self.tf, self.tp = truth["freq"], truth["phase"]
        return truth, ref

    def check(self, got, want, x, label):
        truth, ref = want
        for r in range(self.rows):
            e_gpu, e_ref = costas_deviation(got[0][r], truth, r), costas_deviation(ref[:, r], truth, r)
            assert e_gpu <= 4 * e_ref, f"{label} row {r}: off the truth by {e_gpu:.3g}, the float loop by {e_ref:.3g}"

    def check_getter(self, method, got, chan):
        if method == "gains":
            assert tuple(F32(g) for g in got) == costas_gains(self.bw[chan]), (method, got)
            return True
        df, dp = abs(LD(np.float64(got[0])) - self.tf[chan]), abs(LD(np.float64(got[1])) - self.tp[chan])
        rf, rp = abs(LD(self.rf[chan]) - self.tf[chan]), abs(LD(self.rp[chan]) - self.tp[chan])
        assert df <= 4 * rf and dp <= 4 * rp, (method, chan, float(df), float(rf), float(dp), float(rp))
        return True


class _StereoModel(_RowModel):
    """StereoFMDemod as tests/test_gpu_stereo_fm.py judges it, call by call: m is fm_ref with the carried phase, bit for bit (it is
    what the mix is computed from); the filtered pilot f (the handle's own rows, copied behind the call) is held to the filter
    families' yardstick rule against fir_ref64 with the carried history; the outputs and the level are stereo_mix_ref(m, f, level,
    cfr) bit for bit.  Every call of the scenario is in the peak regime (asserted): the level is the pilot's crest there."""

    def __init__(self, rows, sr, dev, taps):
        super().__init__(rows)
        self.fm, self.cfr, self.taps = _FmModel(rows, sr, dev, False), [cfr_of(sr)] * rows, np.asarray(taps, F32)
        self.reset()

    def reset(self):
        self.fm.reset()
        self.prev = [F32(0)] * self.rows
        self.hist = [np.zeros(len(self.taps) - 1, F32) for _ in range(self.rows)]

    def set_fm(self, sr, dev, chan):
        self.fm.set_fm(sr, dev, chan)
        for r in self.of(chan):
            self.cfr[r] = cfr_of(sr)

    def set_pilot_taps(self, taps):
        self.taps = np.asarray(taps, F32)
        self.hist = [np.zeros(len(self.taps) - 1, F32) for _ in range(self.rows)]      # the filter history is zeroed, phase and level stay

    def set_phase(self, p, chan):
        self.fm.set_phase(p, chan)

    def get_phase(self, chan):
        return self.fm.get_phase(chan)

    def set_level(self, v, chan):
        for r in self.of(chan):
            self.prev[r] = F32(v)

    def level(self, chan):
        return self.prev[chan]

    def process(self, x):
        return self.fm.process(x)

    def check(self, got, m, x, label):
        y, f = got
        n = m.shape[1]
        for r in range(self.rows):
            ok, rep = NU.region_check(f[r], NU.direct_fma32(self.taps, m[r], hist=self.hist[r]), NU.fir_ref64(self.taps, m[r], self.hist[r]),
                                      {"call": np.ones(n, bool)}, k=NU.K, floor=NU.FLOOR)
            assert ok, f"{label} row {r}: the filtered pilot against the FP64 reference: {rep}"
            self.hist[r] = np.concatenate([self.hist[r], m[r]])[n:] if len(self.taps) > 1 else self.hist[r]
            dec = float(agc_exact_decay(self.prev[r], self.cfr[r], n)[0]) if self.prev[r] > 0 else 0.0
            assert float(f[r].max()) > dec * (1 + REGIME_GAP), f"{label} row {r}: not in the peak regime ({f[r].max()} / {dec})"
            want, lvl = stereo_mix_ref(m[r], f[r], self.prev[r], self.cfr[r])
            assert A.same_bits(y[r], want), f"{label} row {r}: not stereo_mix_ref of the handle's own pilot bit for bit"
            self.prev[r] = lvl


class _MpxRows:
    """Rows of the composite signal of tests/test_stereo_fm_cpu.py's recipe (1 kHz tone, 19 kHz pilot of 0.1, a 38 kHz subcarrier, a
    little noise), frequency-modulated with `modulate` as one stream per row that runs on from call to call."""
    N = 240_000

    def __init__(self, fs, dev):
        self.fs, self.dev, self.t, self.rows = fs, dev, 0, {}

    def __call__(self, rng, rows, n):
        if rows not in self.rows:
            t = np.arange(self.N, dtype=np.float64) / self.fs
            out = []
            for r in range(rows):
                g = np.random.default_rng(500 + r)
                mpx = (0.4 * np.sin(2 * np.pi * 1_000.0 * t + r) + 0.1 * np.sin(2 * np.pi * 19_000.0 * t + 0.3 * r)
                       + 0.2 * np.sin(2 * np.pi * 700.0 * t) * np.sin(2 * np.pi * 38_000.0 * t) + 0.01 * g.standard_normal(self.N))
                out.append(modulate(mpx, self.dev / self.fs))
            self.rows[rows] = np.stack(out)
        assert self.t + n <= self.N
        x = self.rows[rows][:, self.t:self.t + n]
        self.t += n
        return np.ascontiguousarray(x)


class Kind:
    """One per-row handle kind: how to make it and its input, the call sizes (short rows first; `long` is longer than any call
    before it: the other kernel form where the kind has two, and scratch growth where it has scratch), the kernel of each size, the
    setters (each a (method, args) with the channel argument written out: -1 = every row), the state setters and the getters, and
    the model (above) that carries the kind's reference through the steps; `grow`: every call's input is that factor larger than
    the one before (Agc: every call in the peak regime, where agc_ref is bit-exact)."""

    def __init__(self, name, make, inp, short, long, kernels, setters=(), state=(), getters=(), reset=True, model=None, rows=ROWS, grow=1.0):
        self.name, self.make, self.inp, self.short, self.long, self.kernels = name, make, inp, short, long, kernels
        self.setters, self.state, self.getters, self.reset, self.model, self.rows, self.grow = setters, state, getters, reset, model, rows, grow


SYNC = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
SYNC_B = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.uint8)
FRAME = 64


class _PskRows:
    """Rows of `order`-PSK symbols (one per sample) on a small carrier offset that runs on from call to call, plus a little noise: the
    locked / pull-in cases of tests/test_costas_cpu.py, where the decisions keep their margin."""

    def __init__(self, order):
        self.order, self.t = order, 0

    def __call__(self, rng, rows, n):
        first = {2: 0.0, 4: np.pi / 4, 8: np.pi / 8}[self.order]
        sym = np.exp(1j * (first + 2 * np.pi * rng.integers(0, self.order, (rows, n)) / self.order))
        t = self.t + np.arange(n)
        self.t += n
        noise = 0.02 * (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n)))
        return (sym * np.exp(1j * (0.002 * t + 0.3 + 0.1 * np.arange(rows)[:, None])) + noise).astype(np.complex64)


def _bits_rows(rng, rows, n):
    return np.stack([DF.stream_with_frames(rng, n, FRAME, SYNC) for _ in range(rows)])


def _kinds(ops):
    sr, dev = 250e3, 75e3
    pilot_a = sfm_pilot_taps(1001)                   # the reference's design at 250 kHz
    pilot_b = np.concatenate([np.zeros(8, np.float32), pilot_a * np.float32(1.25)]).astype(np.float32)      # another count, a larger gain
    lv_short, lv_long = 3 * LEVEL_TILE + 5, 3 * LEVEL_ROW_TILES * LEVEL_TILE + 5
    K = [
        Kind("fm", lambda n: ops.FmDemod(sr, dev, nchan=n, max_block=0), _cx, 3 * TILE + 5, 5 * TILE + 7, ("fm_demod_kernel",) * 2,
             setters=[("set_fm", (200e3, 50e3, -1)), ("set_fm", (250e3, 12.5e3, 2))], state=[("set_phase", (0.3, -1)), ("set_phase", (-1.1, 3))],
             getters=[("get_phase", (2,))], model=lambda n: _FmModel(n, sr, dev, False)),
        Kind("fm_stereo", lambda n: ops.FmDemod(sr, dev, stereo=True, nchan=n, max_block=0), _cx, 3 * TILE + 5, 5 * TILE + 7, ("fm_demod_kernel",) * 2,
             setters=[("set_fm", (200e3, 50e3, -1)), ("set_fm", (250e3, 12.5e3, 0))], state=[("set_phase", (0.3, -1)), ("set_phase", (-1.1, 1))],
             getters=[("get_phase", (1,))], model=lambda n: _FmModel(n, sr, dev, True)),
        Kind("am", lambda n: ops.AmDemod(nchan=n, max_block=0), _cx, 3 * TILE + 5, 5 * TILE + 7, ("am_sub_kernel",) * 2, reset=False, model=_AmModel),
        Kind("deemp_mono", lambda n: ops.Deemp(48e3, 50e-6, stereo=False, nchan=n, max_block=0), _re, 3 * DEEMP_TILE + 5,
             (DEEMP_ROW_TILES + 1) * DEEMP_TILE + 5, ("deemp_row_kernel", "deemp_scan_kernel"),
             setters=[("set", (44.1e3, 75e-6, -1)), ("set", (48e3, 50e-6, 2)), ("bypass", (True,)), ("bypass", (False,))],
             state=[("set_state", (0.25, 0.0, -1)), ("set_state", (-0.5, 0.0, 4))], getters=[("get_state", (4,)), ("alpha", (2,))], model=lambda n: _DeempModel(n, 48e3, 50e-6, False)),
        Kind("deemp_stereo", lambda n: ops.Deemp(48e3, 50e-6, stereo=True, nchan=n, max_block=0),
             lambda rng, rows, n: (0.5 * rng.standard_normal((rows, n, 2))).astype(np.float32), 3 * DEEMP_TILE + 5,
             (DEEMP_ROW_TILES + 1) * DEEMP_TILE + 5, ("deemp_row_kernel", "deemp_scan_kernel"),
             setters=[("set", (44.1e3, 75e-6, -1)), ("set", (48e3, 50e-6, 0))], state=[("set_state", (0.25, -0.25, -1)), ("set_state", (-0.5, 0.5, 1))],
             getters=[("get_state", (1,))], model=lambda n: _DeempModel(n, 48e3, 50e-6, True)),
        Kind("squelch", lambda n: ops.Squelch(-50.0, nchan=n, max_block=0), _cx, lv_short, lv_long, ("level_row_kernel", "level_apply_kernel"),
             setters=[("set_level", (10.0, -1)), ("set_level", (-50.0, 2))], getters=[("is_open", (2,)), ("is_open", (0,))],
             model=lambda n: _SquelchModel(n, -50.0)),
        Kind("agc", lambda n: ops.Agc(1.0, 48e3, nchan=n, max_block=0), _re, lv_short, lv_long, ("level_row_kernel", "level_apply_kernel"),
             setters=[("set", (20.0, 44.1e3, -1)), ("set", (1.0, 48e3, 3))], state=[("set_level", (0.5, -1)), ("set_level", (2.0, 1))],
             getters=[("level", (1,))], model=lambda n: _AgcModel(n, 1.0, 48e3), grow=1.3),
        # (every setter leaves the pilot's crest above the decayed level -- a smaller deviation and taps scaled up raise it, the levels
        # set are far below it -- so that every call stays in the peak regime, where stereo_mix_ref is bit-exact)
        Kind("stereo_fm", lambda n: ops.StereoFmDemod(sr, 62.5e3, nchan=n, pilot_taps=pilot_a, max_block=0), _MpxRows(sr, 62.5e3), 3 * TILE + 5,
             5 * TILE + 7, ("stereo_mix_kernel",) * 2,
             setters=[("set_fm", (sr, 55e3, 2)), ("set_fm", (sr, 50e3, -1)), ("set_pilot_taps", (pilot_b,))],
             state=[("set_phase", (0.3, -1)), ("set_phase", (-1.1, 3)), ("set_level", (1e-4, -1)), ("set_level", (2e-4, 0))],
             getters=[("get_phase", (3,)), ("level", (0,))], model=lambda n: _StereoModel(n, sr, 62.5e3, pilot_a)),
    ]
    for kind, gen in (("real", _re), ("complex", _cx)):
        hist = gen(np.random.default_rng(3), 1, 1023)[0]
        K.append(Kind(f"ffagc_{kind}", lambda n, kind=kind: ops.FeedForwardAgc(kind, nchan=n, max_block=0, window=1024), gen, 3 * TILE + 5, 5 * TILE + 7,
                      ("ff_agc_kernel",) * 2, setters=[("set_history", (hist[:500], -1)), ("set_history", (hist[::-1].copy(), 2))],
                      getters=[("fill", ()), ("get_history", (2,))],
                      model=lambda n, kind=kind: _FfAgcModel(n, 1024, np.complex64 if kind == "complex" else np.float32)))
    K.append(Kind("cagc", lambda n: ops.ComplexAgc(1.0, 1e5, 1e-3, nchan=n, max_block=0), _cx, 3 * CAGC_TILE + 5, (CAGC_ROW_TILES + 1) * CAGC_TILE + 5,
                  ("cagc_row_kernel", "cagc_scan_kernel"), setters=[("set", (0.8, 1e4, 2e-3, -1)), ("set", (1.0, 1e5, 1e-3, 2))],
                  state=[("set_gain", (2.0, -1)), ("set_gain", (0.5, 4))], getters=[("get_gain", (4,))],
                  model=lambda n: _CagcModel(n, 1.0, 1e5, 1e-3)))
    for order, rows in ((2, ROWS), (4, ROWS_WAVE), (8, ROWS)):
        K.append(Kind(f"costas{order}", lambda n, order=order: ops.CostasLoop(order, 0.01, nchan=n, max_block=0), _PskRows(order), 512 + 256 + 5,
                      2 * TILE + 7, ("costas_kernel",) * 2,       # (rounds of 512 / 256 / 4096 samples: test_costas_cpu.chunk_of)
                      setters=[("set_bandwidth", (0.02, -1)), ("set_bandwidth", (0.005, 2))],
                      state=[("set_state", (0.01, 0.5, -1)), ("set_state", (-0.02, 1.5, 3))], getters=[("get_state", (3,)), ("gains", (2,))], rows=rows,
                      model=lambda n, order=order: _CostasModel(n, order, 0.01)))
    for kind, rows in ((0, ROWS), (1, ROWS_WAVE)):
        def mm_in(rng, r, n, kind=kind):
            return np.stack([MM.signal(kind, 4.0, n // 4 + 8, int(rng.integers(1 << 30)))[:n] for _ in range(r)])
        K.append(Kind(f"mmcr_{'complex' if kind else 'real'}", lambda n, kind=kind: ops.MmClockRecovery(kind, 4.0, nchan=n, max_block=0), mm_in,
                      TILE + 5, 2 * TILE + 7, ("mm_clock_kernel",) * 2,        # (one row per lane, no tiles; mm_ref is a Python loop)
                      setters=[("set_gains", (1e-5, 0.02, -1)), ("set_gains", (2.5e-5, 0.01, 2)), ("set_limit", (0.004, -1)), ("set_limit", (0.005, 2)),
                               ("set_omega", (4.1, 2)), ("set_omega", (4.0, -1)), ("set_interp_taps", ("scaled",))],
                      state=[("set_state", (0.25, 4.0, 1, -1)), ("set_state", (0.75, 4.01, 3, 4))], getters=[("get_state", (4,)), ("counts", ())],
                      model=lambda n, kind=kind: _MmModel(n, kind, 4.0), rows=rows))
    t33 = _taps(1, 1, 33)
    for kind, gen in ((0, _re), (1, _cx)):
        hk = gen(np.random.default_rng(4), 1, 32)[0]
        K.append(Kind(f"rowfir_{'complex' if kind else 'real'}", lambda n, kind=kind: ops.RowFir(kind, t33, nchan=n, max_block=0), gen, 3 * TILE + 5,
                      5 * TILE + 7, ("row_fir_kernel",) * 2,
                      setters=[("set_taps", (_taps(1, 1, 41), -1)), ("set_taps", (_taps(1, 1, 25), -1)), ("set_taps", (t33, -1)),
                               ("set_taps", ((t33 * np.float32(0.5)).astype(np.float32), 2))],
                      state=[("set_history", (hk, 0)), ("set_history", (hk[::-1].copy(), 3))], getters=[("get_history", (3,))],
                      model=lambda n, kind=kind: _RowFirModel(n, t33, bool(kind))))
    K.append(Kind("delay_imag", lambda n: ops.DelayImag(nchan=n, max_block=0), _cx, 3 * TILE + 5, 5 * TILE + 7, ("delay_imag_kernel",) * 2,
                  state=[("set_state", (0.7, -1)), ("set_state", (-0.3, 2))], getters=[("get_state", (2,))],
                  model=_DelayModel))
    K.append(Kind("threshold", lambda n: ops.Threshold(nchan=n, max_block=0), _re, 3 * TILE + 5, 5 * TILE + 7, ("threshold_kernel",) * 2, reset=False,
                  model=_ThresholdModel))
    for flt in (False, True):
        def df_in(rng, r, n, flt=flt):
            b = _bits_rows(rng, r, n)
            return ((b.astype(np.float32) * 2 - 1) * (0.5 + rng.random(b.shape).astype(np.float32))).astype(np.float32) if flt else b
        K.append(Kind(f"deframer_{'float' if flt else 'bytes'}", lambda n, flt=flt: ops.Deframer(FRAME, SYNC, 1 if flt else 0, nchan=n, max_block=0),
                      df_in, 3 * TILE + 5, 5 * TILE + 7, ("deframe_match_kernel",) * 2, setters=[("set_sync", (SYNC_B,)), ("set_sync", (SYNC,))],
                      state=[("set_state", (0, 1, False, -1)), ("set_state", (-1, 0, True, 2))], getters=[("get_state", (2,)), ("counts", ())],
                      model=lambda n, flt=flt: _DeframerModel(n, flt)))
    return K


KIND_NAMES = ["fm", "fm_stereo", "am", "deemp_mono", "deemp_stereo", "squelch", "agc", "stereo_fm", "ffagc_real", "ffagc_complex", "cagc", "costas2",
              "costas4", "costas8", "mmcr_real", "mmcr_complex", "rowfir_real", "rowfir_complex", "delay_imag", "threshold", "deframer_bytes",
              "deframer_float"]


def _row_scenario(kind):
    def scenario():
        op = kind.make(kind.rows)
        rng = np.random.default_rng(len(kind.name) + 100)
        steps = []
        model = kind.model(kind.rows) if kind.model is not None else None
        ncall = [0]
        if hasattr(kind.inp, "t"):
            kind.inp.t = 0                             # (every run of the scenario sees the same stream)

        def calls(n, kernel):
            for _ in range(2):
                x = kind.inp(rng, kind.rows, n)
                if kind.grow != 1.0:
                    x = (x * np.float32(kind.grow ** ncall[0])).astype(x.dtype)
                ncall[0] += 1
                xd = _In(x, rows=True)
                label = f"process_batch {len(steps)} ({n})"
                st = Call(label, lambda xd=xd: _pb(op, xd()), op, {kernel})
                if model is not None:
                    st.check = lambda v, x=x, label=label: model.check(v, model.process(x), x, f"{kind.name} {label}")
                steps.append(st)

        def host(method, args):
            if method == "set_interp_taps":
                args = ((op.interp_taps() * np.float32(0.99)).astype(np.float32),)
            st = H(op, method, *args)
            if model is not None:
                def chk(v, method=method, args=args):
                    if v and hasattr(model, "check_getter") and model.check_getter(method, v, *args):
                        return
                    want = getattr(model, method)(*args)
                    if v:                              # a getter: the model's value, bit for bit
                        got = v[0] if len(v) == 1 else np.asarray([np.asarray(a) for a in v])
                        want = np.asarray(want)
                        got = np.asarray(got).astype(want.dtype) if np.asarray(got).dtype.kind == want.dtype.kind else np.asarray(got)
                        assert np.array_equal(got.reshape(want.shape), want), f"{kind.name} {method}{args}: {got} / the model's {want}"
                st.check = chk
            steps.append(st)

        calls(kind.short, kind.kernels[0])
        for method, args in list(kind.setters) + list(kind.state) + list(kind.getters):
            host(method, args)
            calls(kind.short, "bypass" if method == "bypass" and args[0] else kind.kernels[0])     # (Deemp.bypass(True): a copy)
        if kind.reset:
            host("reset", ())
            calls(kind.short, kind.kernels[0])
        calls(kind.long, kind.kernels[1])          # longer than any call before
        for method, args in kind.getters:          # the state after ALL queued calls
            host(method, args)
            calls(kind.short, kind.kernels[0])
        return steps

    return scenario


@pytest.mark.parametrize("name", KIND_NAMES)
def test_per_row_operators(ops, name):
    """Every per-row operator over 5 (once 17) rows of stride count + 1: every setter for all rows and for one, every state setter,
    every getter, reset and a call longer than any before, each while the previous process_batch is still held."""
    kind = {k.name: k for k in _kinds(ops)}[name]
    serial = _three_ways(f"per-row {name}", _row_scenario(kind))
    _anchor(serial)


def test_per_row_kinds_are_all_listed(ops):
    assert [k.name for k in _kinds(ops)] == KIND_NAMES


def test_ssb_demod(ops):
    """SsbDemod has one row: the 1-D entry point, the NCO's setters and its getter.  The reference is the one of
    tests/test_gpu_demod.py: the real part of the frequency translator's output, here the FP64 oracle's, at the Xlator's bound."""
    inc = ops.ssb_phase_delta(48_000.0, 2_700.0, ops.SsbDemod.USB)
    inc_b = ops.ssb_phase_delta(48_000.0, 3_000.0, ops.SsbDemod.LSB)

    def scenario():
        op = ops.SsbDemod(phase_inc=inc, max_block=0)
        xl = O.Xlator(1.0, 0.0, exact=True, volk_gain=True)
        xl.delta[:] = inc
        rng = np.random.default_rng(9)
        steps = []

        def calls(n=3 * 256 * 8 + 5):
            for _ in range(2):
                x = _cx(rng, 1, n)[0]
                xd = _In(x)
                st = Call(f"process {len(steps)}", lambda xd=xd: op.process(xd()), op, {"ssb_demod_kernel"})
                st.check = lambda v, x=x: _close_to("ssb", v[0], np.ascontiguousarray(xl.process(x).real))
                steps.append(st)

        def phase(v):
            assert abs(complex(v[0]) - np.exp(2j * np.pi * xl.turns.value)) < TOL_PHASE, ("get_phase", v[0])

        calls()
        steps.append(_checked(H(op, "set_phase_inc", *inc_b), lambda v: xl.delta.__setitem__(slice(None), inc_b)))
        calls()
        steps.append(_checked(H(op, "set_phase", 0.6, 0.8), lambda v: setattr(xl.turns, "value", math.atan2(0.8, 0.6) / (2 * math.pi))))
        calls()
        steps.append(_checked(H(op, "set_volk_gain", False), lambda v: setattr(xl, "volk_gain", False)))
        calls()
        steps.append(_checked(H(op, "get_phase"), phase))
        calls()
        steps.append(_checked(H(op, "advance", 1000), lambda v: setattr(xl.turns, "value", xl.turns.value + 1000 * math.atan2(inc_b[1], inc_b[0]) / (2 * math.pi))))
        calls(5 * 256 * 8 + 7)
        steps.append(_checked(H(op, "get_phase"), phase))
        calls()
        return steps

    _anchor(_three_ways("ssb", scenario))


# ------------------------------------------------------------------------------------------------ chains
class _MskRef:
    """MSKDemod as the numpy definitions of its two stages: fm_ref_rows, then mm_ref on the float rows."""

    def __init__(self, ops):
        self.fm, self.mm = _FmModel(ROWS, 48000.0, 6000.0, False), _MmModel(ROWS, 0, float(F32(48000.0) / F32(12000.0)))

    def setter(self, method, args):
        getattr(self.fm, method)(*args)

    def reset(self):
        self.fm.reset()
        self.mm.reset()

    def process(self, x):
        f = self.fm.process(x)
        return self.mm.process(f), f

    def counts(self):
        return self.mm.counts()


class _PskRef:
    """PSKDemod as tests/test_gpu_psk.py judges it: the composition of the separate device handles (each with its own test and its
    own scenario above), run on the default stream with a synchronise after every call; the Q delay is its numpy definition."""

    def __init__(self, ops, offset):
        self.offset = offset
        self.agc = ops.ComplexAgc(1.0, 65535.0, 10e-4, nchan=ROWS, max_block=0)
        taps = ops.rrc_taps(32, 48000.0, 12000.0, 0.32)
        self.firs = [ops.Fir(taps, max_block=0) for _ in range(ROWS)]
        for f in self.firs:
            f.set_mode(f.DIRECT)
        self.costas = ops.CostasLoop(4, 0.004, nchan=ROWS, max_block=0)
        self.delay = _DelayModel(ROWS)
        self.clock = ops.MmClockRecovery(1, float(F32(48000.0) / F32(12000.0)), nchan=ROWS, max_block=0)
        self.last_counts = np.zeros(ROWS, np.int32)

    def setter(self, method, args):
        getattr(self.costas, method)(*args)

    def reset(self):
        for h in [self.agc, self.costas, self.clock, self.delay] + self.firs:
            h.reset()
        self.last_counts = np.zeros(ROWS, np.int32)

    def process(self, x):
        import torch

        a = self.agc.process_batch(_dev(x))
        f = torch.stack([self.firs[r].process(a[r].contiguous()) for r in range(ROWS)])
        c = self.costas.process_batch(f)
        stage = c.cpu().numpy()
        d = _dev(self.delay.process(stage)) if self.offset else c
        rows, counts = self.clock.process_batch(d)
        torch.cuda.synchronize()
        rows, self.last_counts = rows.cpu().numpy(), counts.cpu().numpy()
        return [rows[r, :self.last_counts[r]] for r in range(ROWS)], stage

    def counts(self):
        return self.last_counts


def _check_counted(label, got, want):
    rows, counts = got
    for r in range(ROWS):
        w = np.asarray(want[r]).reshape(-1)
        assert counts[r] == len(want[r]), f"{label}: count of row {r}: {counts[r]} / {len(want[r])}"
        assert A.same_bits(rows[r, :len(w)], w.astype(rows.dtype)), f"{label}: row {r} is not the reference bit for bit"
        assert not rows[r, len(w):].any(), f"{label}: row {r} written past its count"


def _chain_scenario(ops, make, make_ref, setter, tap_which, seed):
    def scenario():
        chain = make()
        ref = make_ref()
        rng = np.random.default_rng(seed)
        steps, last = [], {}

        def calls(n):
            for _ in range(2):
                x = _cx(rng, ROWS, n, 0.05)
                xd = _In(x, rows=True)
                label = f"process_batch {len(steps)} ({n})"
                st = Call(label, lambda xd=xd: _pb(chain, xd()), chain, {"mm_clock_kernel"})

                def chk(v, x=x, label=label):
                    want, last["stage"] = ref.process(x)
                    _check_counted(label, v, want)
                steps.append(_checked(st, chk))

        def same_counts(v):
            assert np.array_equal(v[0], ref.counts()), ("counts", v[0], ref.counts())

        calls(2053)
        stage, method, args = setter(chain)
        steps.append(_checked(H(stage, method, *args), lambda v: ref.setter(method, args)))      # a setter on a borrowed stage handle
        calls(2053)
        calls(4111)                                  # a larger call: the scratch rows grow
        tap = Host("tap", lambda: chain.tap(tap_which, 4111).clone())
        steps.append(_checked(tap, lambda v: A.same_bits(v[0], last["stage"]) or pytest.fail("tap: not the stage's rows of the last call")))
        calls(2053)
        steps.append(_checked(H(chain, "counts"), same_counts))
        calls(2053)
        steps.append(_checked(H(chain, "reset"), lambda v: ref.reset()))
        calls(2053)
        steps.append(_checked(H(chain, "counts"), same_counts))
        calls(2053)
        return steps

    return scenario


@pytest.mark.parametrize("which", ["psk4", "oqpsk", "msk"])
def test_chains(ops, which):
    """PskDemod (order 4, and offset QPSK) and MskDemod: a setter on a borrowed stage, scratch growth, tap, counts and reset with the
    previous call still held."""
    if which == "msk":
        make = lambda: ops.MskDemod(48000.0, 6000.0, 12000.0, nchan=ROWS, max_block=0)      # noqa: E731
        make_ref = lambda: _MskRef(ops)                                                      # noqa: E731
        setter = lambda c: (c.stage(c.FM), "set_fm", (48000.0, 5000.0, -1))                  # noqa: E731
        tap = ops.MskDemod.FM
    else:
        make = lambda: ops.PskDemod(4, which == "oqpsk", 48000.0, 12000.0, nchan=ROWS, max_block=0)   # noqa: E731
        make_ref = lambda: _PskRef(ops, which == "oqpsk")                                             # noqa: E731
        setter = lambda c: (c.stage(c.COSTAS), "set_bandwidth", (0.006, -1))                          # noqa: E731
        tap = ops.PskDemod.COSTAS
    _anchor(_three_ways(f"chain {which}", _chain_scenario(ops, make, make_ref, setter, tap, seed=len(which))))


def test_msk_to_deframer_count_handover(ops):
    """MskDemod.process_batch -> Deframer.process_batch(in_counts = the chain's device counts) on one stream with no host step in
    between, then Deframer.set_state with both still queued, and both again.  Reference: the chain's numpy stages, then deframe_ref
    over the first counts[r] symbols of every row."""
    def scenario():
        import torch

        msk = ops.MskDemod(48000.0, 6000.0, 12000.0, nchan=ROWS, max_block=0)
        dfr = ops.Deframer(FRAME, SYNC, 1, nchan=ROWS, max_block=0)
        mref, dref = _MskRef(ops), _DeframerModel(ROWS, True)
        rng = np.random.default_rng(21)
        steps, last, want = [], {}, {}

        def pair(n=4111):
            x = _cx(rng, ROWS, n, 0.05)
            xd = _In(x, rows=True)

            def run_msk():
                last["sym"], last["counts"] = _pb(msk, xd())
                return last["sym"], last["counts"]

            def run_dfr():
                sym = last["sym"]
                nb = dfr.out_size(sym.shape[1]) * dfr.frame_bytes
                out = torch.zeros((ROWS, max(nb, 1)), dtype=torch.uint8, device=sym.device)
                return dfr.process_batch(sym, out=out, in_counts=last["counts"])

            def chk_msk(v):
                want["sym"], _ = mref.process(x)
                _check_counted("msk", v, want["sym"])

            def chk_dfr(v):
                _check_counted("deframer", v, dref.process(want["sym"]))
            steps.append(_checked(Call(f"msk {len(steps)}", run_msk, msk, {"mm_clock_kernel"}), chk_msk))
            steps.append(_checked(Call(f"deframer {len(steps)}", run_dfr, dfr, {"deframe_match_kernel"}), chk_dfr))

        pair()
        pair()
        steps.append(_checked(H(dfr, "set_state", 0, 1, False, -1), lambda v: dref.set_state(0, 1, False, -1)))
        pair()
        pair()
        steps.append(_checked(H(dfr, "counts"), lambda v: np.array_equal(v[0], dref.counts()) or pytest.fail("deframer counts")))
        pair()
        steps.append(_checked(H(msk, "counts"), lambda v: np.array_equal(v[0], mref.counts()) or pytest.fail("msk counts")))
        pair()
        return steps

    _anchor(_three_ways("msk -> deframer", scenario))


# ------------------------------------------------------------------------------------------------ forward error correction (qdsp_amd.fec)
RS_SENT, RS_ESENT = 0xA5, -99
FALCON_BITS = 1279 * 8
FALCON_SYNC = np.unpackbits(np.array([0x1A, 0xCF, 0xFC, 0x1D], np.uint8))


@pytest.fixture(scope="module")
def fec(ops):
    from qdsp_amd import fec as _fec

    return _fec


class _RsModel:
    """_rs_ref.Layout.decode carried through the steps: set_maps changes the layout, every call is decoded under the one in force."""

    def __init__(self, lay, rows):
        self.lay, self.last_counts = lay, np.zeros(rows, np.int32)

    def set_maps(self, in_map=None, out_map=None, xor=None):
        self.lay = RS.Layout(self.lay.code, self.lay.depth, self.lay.skip, self.lay.full_out, in_map, out_map, xor)

    def decode(self, frames):
        frames = np.asarray(frames, np.uint8).reshape(-1, self.lay.frame_in)
        if not len(frames):
            return np.zeros((0, self.lay.frame_out), np.uint8), np.zeros((0, self.lay.depth), np.int32)
        out, good, errs = self.lay.decode(frames)
        return out[good], errs

    def check(self, got, per_row, label):
        """got: the whole output buffer (sentinel-filled before the call), the counts and the whole errs buffer (None: not asked
        for); per_row: the frames every row's decoder took.  Every byte and every entry: good frames packed, sentinels behind."""
        out, counts = got[0], got[1]
        want, wc = np.full_like(out, RS_SENT), []
        we = np.full_like(got[2], RS_ESENT) if len(got) > 2 else None
        for r, frames in enumerate(per_row):
            g, e = self.decode(frames)
            want[r, :g.size] = g.ravel()
            wc.append(len(g))
            if we is not None:
                we[r, :e.size] = e.ravel()
        self.last_counts = np.asarray(wc, np.int32)
        assert counts.tolist() == wc, f"{label}: counts {counts.tolist()} / the definition's {wc}"
        assert A.same_bits(out, want), f"{label}: output buffer: {np.argwhere(out != want)[:4].tolist()}"
        assert we is None or np.array_equal(got[2], we), f"{label}: errs: {np.argwhere(got[2] != we)[:4].tolist()}"

    def same_counts(self, v):
        assert np.array_equal(v[0], self.last_counts), ("counts", v[0], self.last_counts)


def _rs_out(op, nframes, with_errs=True):
    """A function that gives a fresh output buffer (7 bytes of slack per row) and errs buffer, each filled with its sentinel by a
    copy queued on the current stream."""
    import torch

    osent = torch.full((op.nchan, nframes * op.frame_out + 7), RS_SENT, dtype=torch.uint8, device="cuda")
    esent = torch.full((op.nchan, max(nframes * (op.frame_in // 255), 1)), RS_ESENT, dtype=torch.int32, device="cuda") if with_errs else None

    def fresh():
        out, errs = torch.empty_like(osent), None if esent is None else torch.empty_like(esent)
        out.copy_(osent)
        if errs is not None:
            errs.copy_(esent)
        return out, errs

    return fresh


def _rs_call(label, op, model, x, nframes, in_counts=None):
    """op.process_batch over the rows x (rows, nframes * frame_in), per-row counts from a device tensor that is itself copied on the
    current stream.  The value: the whole output buffer, the counts, the whole errs buffer."""
    xin, fresh = _In(x, rows=True), _rs_out(op, nframes)
    cin = None if in_counts is None else _In(np.asarray(in_counts, np.int32))
    take = [nframes] * len(x) if in_counts is None else [min(max(int(c), 0), nframes) for c in in_counts]
    per_row = [x[r, :take[r] * op.frame_in] for r in range(len(x))]

    def fn():
        out, errs = fresh()
        _, counts = op.process_batch(xin(), out, nframes=nframes, in_counts=None if cin is None else cin(), errs=errs)
        return out, counts, errs

    return _checked(Call(label, fn, op, {"rs_decode_kernel"}), lambda v: model.check(v, per_row, label))


class _Feed:
    """The frames of a pool dealt out in order: `rows` rows of n frames each, as a (rows, n * frame_in) array."""

    def __init__(self, frames):
        self.frames, self.at = frames, 0

    def __call__(self, rows, n, through=None):
        assert self.at + rows * n <= len(self.frames)
        x = self.frames[self.at:self.at + rows * n].reshape(rows, -1)
        self.at += rows * n
        return np.ascontiguousarray(x if through is None else through[x])


def test_falcon_rs(ops, fec):
    """FalconRs over 5 rows, scratch for 2 frames a row: a 7-frame call (the scratch is freed and reallocated at call time) and
    the same again; set_maps with another output permutation and XOR sequence; counts; per-row counts from a device tensor (0,
    all, more than there are, negative); a 12-frame call while two calls on the scratch it frees are still queued; set_maps back
    to the identity (the frames then come in the decoder's own domain).  A call that drains the queue is followed by one that
    does not, so that every host action finds a library call queued."""
    lay = RS.falcon_layout()
    rng = np.random.default_rng(41)
    pool = Pool(lay, gen_frames(rng, lay, ROWS * 64))
    assert 0.5 < pool.good.mean() < 0.9 and pool.errs.max() == 8
    out_map, xor = rng.permutation(256).astype(np.uint8), rng.integers(0, 256, 100).astype(np.uint8)

    def scenario():
        op = fec.FalconRs(nchan=ROWS, max_block=2)
        model, feed = _RsModel(lay, ROWS), _Feed(pool.frames)
        steps = []

        def call(n, in_counts=None, through=None):
            steps.append(_rs_call(f"process_batch {len(steps)} ({n})", op, model, feed(ROWS, n, through), n, in_counts))

        call(7)                                        # larger than any call before: rs_scratch frees and reallocates
        call(7)
        steps.append(_checked(H(op, "set_maps", lay.in_map, out_map, xor), lambda v: model.set_maps(lay.in_map, out_map, xor)))
        call(4)
        call(4)
        steps.append(_checked(H(op, "counts"), model.same_counts))
        call(5)
        call(7, in_counts=[0, 7, 10, -2, 3])
        call(12)                                       # the second regrowth, the two calls before it still queued
        call(12)
        steps.append(_checked(H(op, "set_maps"), lambda v: model.set_maps()))
        call(6, through=lay.in_map)
        return steps

    _anchor(_three_ways("fec FalconRs", scenario))


def test_rs_decoder_one_row(ops, fec):
    """RsDecoder with one row, three codewords of RS(255, 251) to a frame behind two skipped bytes, scratch for 4 frames: the
    1-D tensor form (launch on the caller's stream, then its own download of the count: it drains the queue, so a process_batch
    call on a (1, n) view goes in front of each and behind it), counts, set_maps, and time_dev (its two calls into one
    sentinel-filled buffer; the time itself is dropped), each with a call still queued."""
    code = RS.Code(0x11d, 1, 1, 4)
    rng = np.random.default_rng(42)
    in_map, out_map = rng.permutation(256).astype(np.uint8), rng.permutation(256).astype(np.uint8)
    xor = rng.integers(0, 256, 300).astype(np.uint8)
    lay_a, lay_b = RS.Layout(code, 3, 2, 0), RS.Layout(code, 3, 2, 0, in_map, out_map, xor)
    pool_a, pool_b = (Pool(lay, gen_frames(rng, lay, 32, p_bad=0.35)) for lay in (lay_a, lay_b))
    assert all(0 < p.good.sum() < 32 and p.errs.max() == 2 for p in (pool_a, pool_b))

    def scenario():
        op = fec.RsDecoder(0x11d, 1, 1, 4, depth=3, skip=2, nchan=1, max_block=4)
        model = _RsModel(lay_a, 1)
        feed = {"f": _Feed(pool_a.frames)}
        steps = []

        def batch(n):
            steps.append(_rs_call(f"process_batch {len(steps)} ({n})", op, model, feed["f"](1, n), n))

        def one_d(n):
            x = feed["f"](1, n)[0]
            xin = _In(x)
            label = f"process {len(steps)} ({n})"

            def chk(v):
                want, _ = model.decode(x)
                model.last_counts = np.asarray([len(want)], np.int32)
                assert A.same_bits(v[0], want), f"{label}: not the definition's good frames"
            steps.append(_checked(Call(label, lambda: op.process(xin()), op, {"rs_decode_kernel"}), chk))

        def timed(n):
            x = feed["f"](1, n)
            xin, fresh = _In(x, rows=True), _rs_out(op, n, with_errs=False)

            def fn():
                out, _ = fresh()
                assert op.time_dev(xin(), out, 2) >= 0.0
                return out, op.counts()
            steps.append(_checked(Host("RsDecoder.time_dev", fn, op, "time_dev"), lambda v: model.check(v, [x[0]], "time_dev")))

        batch(3)
        one_d(6)                                       # past max_block: the scratch grows
        batch(4)
        one_d(5)
        batch(2)
        steps.append(_checked(H(op, "counts"), model.same_counts))
        batch(4)

        def to_b(v):
            model.set_maps(in_map, out_map, xor)
        steps.append(_checked(H(op, "set_maps", in_map, out_map, xor), to_b))
        feed_b = _Feed(pool_b.frames)
        feed["f"] = feed_b
        batch(3)
        timed(4)
        batch(2)
        return steps

    _anchor(_three_ways("fec RsDecoder", scenario))


def test_deframer_to_falcon_rs_count_handover(ops, fec):
    """Deframer.process_batch(bits) -> FalconRs.process_batch(frames, nframes = the deframer's capacity, in_counts = its device
    counts) on one stream with no host step in between; Deframer.set_state (the next call starts a frame in the middle of one,
    which the decoder drops), FalconRs.set_maps and counts with a pair still queued.  Falcon frames with the real sync word back
    to back behind a short gap, a call boundary every 2.39 frames, so that one frame straddles every boundary.  Reference:
    deframe_ref carried over the calls, then Layout.decode over each row's frames."""
    import torch

    lay = RS.falcon_layout()
    rng = np.random.default_rng(43)
    npair, n = 7, 2 * FALCON_BITS + 4000
    per_row = -(-npair * n // FALCON_BITS) + 1
    frames = gen_frames(rng, lay, ROWS * per_row, p_bad=0.3)
    frames[:, :4] = [0x1A, 0xCF, 0xFC, 0x1D]
    pool = Pool(lay, frames)
    assert 0.4 < pool.good.mean() < 0.9
    bits = np.zeros((ROWS, npair * n), np.uint8)
    for r in range(ROWS):
        gap = int(rng.integers(0, 300))
        assert all((j * n - gap) % FALCON_BITS for j in range(1, npair))          # a frame straddles every call boundary
        row = np.concatenate([rng.integers(0, 2, gap).astype(np.uint8), np.unpackbits(frames[r * per_row:(r + 1) * per_row].ravel())])
        bits[r] = row[:npair * n]
    out_map, xor = rng.permutation(256).astype(np.uint8), rng.integers(0, 256, 100).astype(np.uint8)

    def scenario():
        dfr = ops.Deframer(FALCON_BITS, FALCON_SYNC, 0, nchan=ROWS, max_block=0)
        cap = dfr.out_size(n)
        rs = fec.FalconRs(nchan=ROWS, max_block=cap)
        dref, rref = _DeframerModel(ROWS, False, FALCON_BITS, FALCON_SYNC), _RsModel(lay, ROWS)
        fresh = _rs_out(rs, cap)
        steps, last, want, at = [], {}, {}, [0]

        def pair():
            x = np.ascontiguousarray(bits[:, at[0]:at[0] + n])
            at[0] += n
            xd = _In(x, rows=True)

            def run_dfr():
                out = torch.zeros((ROWS, cap * dfr.frame_bytes), dtype=torch.uint8, device="cuda")
                last["frames"], last["counts"] = dfr.process_batch(xd(), out=out)
                return last["frames"], last["counts"]

            def run_rs():
                out, errs = fresh()
                _, counts = rs.process_batch(last["frames"], out, nframes=cap, in_counts=last["counts"], errs=errs)
                return out, counts, errs

            def chk_dfr(v):
                want["frames"] = dref.process(x)
                _check_counted("deframer", v, want["frames"])
            steps.append(_checked(Call(f"deframer {len(steps)}", run_dfr, dfr, {"deframe_match_kernel"}), chk_dfr))
            steps.append(_checked(Call(f"rs {len(steps)}", run_rs, rs, {"rs_decode_kernel"}), lambda v: rref.check(v, want["frames"], "rs")))

        pair()
        pair()
        steps.append(_checked(H(dfr, "set_state", 0, 4, False, -1), lambda v: dref.set_state(0, 4, False, -1)))
        pair()                                         # (frames cut from the middle of others, all dropped; then it searches again)
        pair()
        steps.append(_checked(H(rs, "set_maps", lay.in_map, out_map, xor), lambda v: rref.set_maps(lay.in_map, out_map, xor)))
        pair()
        pair()
        steps.append(_checked(H(rs, "counts"), rref.same_counts))
        pair()
        return steps

    serial = _three_ways("deframer -> FalconRs", scenario)
    _anchor(serial)
    good = sum(int(v[1].sum()) for (_, v), st in zip(serial.outputs, serial.steps) if st.label.startswith("rs "))
    taken = sum(int(v[1].sum()) for (_, v), st in zip(serial.outputs, serial.steps) if st.label.startswith("deframer "))
    assert 0 < good < taken, (good, taken)


# ------------------------------------------------------------------------------------------------ the NOAA HRPT tail (qdsp_amd.noaa)
NOAA_S16, NOAA_S8 = 0xA5C3, 0x5A               # sentinels: no AVHRR or HIRS value (> 0x1FFF), and a byte


@pytest.fixture(scope="module")
def noaa(ops):
    from qdsp_amd import noaa as _noaa

    return _noaa


def _fresh(shape, value, dtype):
    """A function that gives a new device tensor filled with the sentinel `value` by a copy queued on the current stream."""
    import torch

    src = _dev(np.full(shape, value, dtype))

    def fresh():
        out = torch.empty_like(src)
        out.copy_(src)
        return out

    return fresh


def _eff(in_counts, n, rows):
    return [n] * rows if in_counts is None else [min(max(int(c), 0), n) for c in in_counts]


def _is(v, want, what):
    assert np.array_equal(np.asarray(v), np.asarray(want)), f"{what}: {v} / the model's {want}"


class _HirsModel:
    """One _noaa_ref.HirsFast per row, carried through the steps as the handle carries its state and its line in progress."""

    def __init__(self, rows, stride):
        self.refs, self.stride, self.last_counts = [NR.HirsFast() for _ in range(rows)], stride, np.zeros(rows, np.int32)

    def set_state(self, last_element, new_image_data, chan=-1):
        for r in (range(len(self.refs)) if chan < 0 else [chan]):
            self.refs[r].set_state(last_element, new_image_data)

    def reset(self):
        for ref in self.refs:
            ref.reset()

    def get_state(self, chan):
        return self.refs[chan].last_element, self.refs[chan].new_image_data

    def lines(self, x, eff):
        out = [ref.process(x[r][:eff[r] * self.stride], self.stride) for r, ref in enumerate(self.refs)]
        self.last_counts = np.asarray([ln.shape[1] for ln in out], np.int32)
        return out

    def check(self, got, x, eff, label):
        """got: the whole output allocation (sentinel-filled in front of the call) and the counts."""
        out, counts = got
        want = np.full_like(out, NOAA_S16)
        for r, ln in enumerate(self.lines(x, eff)):
            want[r, :, :ln.shape[1]] = ln
        assert counts.tolist() == self.last_counts.tolist(), f"{label}: counts {counts.tolist()} / the definition's {self.last_counts.tolist()}"
        assert A.same_bits(out, want), f"{label}: output allocation: {np.argwhere(out != want)[:4].tolist()}"


def _hirs_call(label, op, model, x, n, in_counts=None):
    """op.process_batch over the rows x (rows, n * packet_stride bytes; row stride + 1) into a sentinel-filled allocation with one
    line of slack, per-row counts from a device tensor that is itself copied on the current stream."""
    rows = len(x)
    xin, fresh = _In(x, rows=True), _fresh((rows, 20, n + 2, 56), NOAA_S16, np.uint16)
    cin = None if in_counts is None else _In(np.asarray(in_counts, np.int32))

    def fn():
        out = fresh()
        _, counts = op.process_batch(xin(), out[:, :, :n + 1], count=n, in_counts=None if cin is None else cin())
        return out, counts

    return _checked(Call(label, fn, op, {"hirs_pack_kernel"}), lambda v: model.check(v, x, _eff(in_counts, n, rows), label))


def _state_is(model, chan):
    return lambda v: _is((int(v[0]), bool(v[1])), model.get_state(chan), f"get_state({chan})")


@pytest.mark.parametrize("rows,stride", [(ROWS, 36), (ROWS_WAVE, 74)])
def test_noaa_hirs(ops, noaa, rows, stride):
    """HirsDemux: get_state, set_state for all rows and for one, counts, reset, a count == 0 call and a call longer than any before
    (hirs_scratch frees and reallocates the map while the call before it is queued), each with a call still held.  Every row's
    elements climb by one from call to call, so a line in progress spans every action: set_state(60 .., True) makes the next
    packet flush it, reset drops it, and a setter that wrote the state buffers early would be overwritten by the held calls.
    Runs of two and of three calls in front of the actions: both of the double-buffered state slots are the current one."""
    from test_gpu_noaa import Climb

    def scenario():
        op = noaa.HirsDemux(packet_stride=stride, nchan=rows, max_block=8)
        model, gen = _HirsModel(rows, stride), Climb(rows, 360, stride)
        steps = []

        def call(n, in_counts=None):
            eff = _eff(in_counts, n, rows)
            x = np.stack([gen.packets(r, n, eff[r]) for r in range(rows)])
            steps.append(_hirs_call(f"process_batch {len(steps)} ({n})", op, model, x, n, in_counts))

        def host(method, *args, act=None, check=None):
            steps.append(_checked(H(op, method, *args), (lambda v: act()) if act else check))

        def same_counts(v):
            _is(v[0], model.last_counts, "counts")

        mixed = [(6, 0, 9, -1, 3)[r % 5] for r in range(rows)]
        call(6), call(6)
        host("get_state", 2, check=_state_is(model, 2))
        call(6), call(6), call(6)
        host("set_state", 60, True, act=lambda: model.set_state(60, True))
        call(6), call(6)
        host("set_state", 62, True, 3, act=lambda: model.set_state(62, True, 3))
        call(6), call(6, mixed)
        host("counts", check=same_counts)
        call(6), call(0, mixed)
        host("counts", check=same_counts)
        call(6), call(6), call(6)
        host("reset", act=model.reset)
        call(6), call(6)
        host("get_state", rows - 1, check=_state_is(model, rows - 1))
        call(6), call(40), call(40)                   # longer than any call before
        host("counts", check=same_counts)
        call(6), call(6, mixed), call(6)
        host("set_state", 61, True, rows - 2, act=lambda: model.set_state(61, True, rows - 2))
        call(6), call(6)
        host("get_state", rows - 2, check=_state_is(model, rows - 2))
        return steps

    serial = _three_ways(f"noaa hirs {rows} rows", scenario)
    _anchor(serial)
    lines = sum(int(v[1].sum()) for (_, v), st in zip(serial.outputs, serial.steps) if st.label.startswith("process_batch"))
    assert lines >= 3 * rows                              # the setters' flushes, and the lines that end by themselves


def test_noaa_hirs_one_row(ops, noaa):
    """HirsDemux with one row: the 1-D tensor form (launch on the caller's stream, then its own download of the line count: it
    drains the queue, so a process_batch call on a (1, n) view goes in front of each and behind it; the first is longer than
    max_block), get_state and counts."""
    from test_gpu_noaa import Climb

    def scenario():
        op = noaa.HirsDemux(nchan=1, max_block=8)
        model, gen = _HirsModel(1, 36), Climb(1, 361, 36)
        steps = []

        def batch(n):
            steps.append(_hirs_call(f"process_batch {len(steps)} ({n})", op, model, gen.packets(0, n)[None, :], n))

        def one_d(n):
            x = gen.packets(0, n)
            xin, label = _In(x), f"process {len(steps)} ({n})"
            steps.append(_checked(Call(label, lambda: op.process(xin()), op, {"hirs_pack_kernel"}),
                                  lambda v: A.same_bits(v[0], model.lines([x], [n])[0]) or pytest.fail(f"{label}: not the definition's lines")))

        batch(6)
        one_d(45)
        batch(6)
        one_d(7)
        batch(6)
        steps.append(_checked(H(op, "get_state", 0), _state_is(model, 0)))
        batch(6), batch(6)
        steps.append(_checked(H(op, "counts"), lambda v: _is(v[0], model.last_counts, "counts")))
        batch(6)
        return steps

    _anchor(_three_ways("noaa hirs one row", scenario))


def _hrpt_frames(rng, rows, n):
    """(rows, n, 13863) random bytes, the `minor` values 1, 3, 0, 1, 2, 3, 1 in turn, each row from another place in the cycle."""
    fr = rng.integers(0, 256, (rows, n, NR.FRAME_BYTES)).astype(np.uint8)
    for r in range(rows):
        m = np.array([(1, 3, 0, 1, 2, 3, 1)[(f + 2 * r) % 7] for f in range(n)], np.uint8)
        fr[r, :, 7] = (fr[r, :, 7] & 0xF9) | (m << 1)
    return fr


def _slot_ranks(minors):
    want = np.full(len(minors), -1, np.int32)
    want[minors == 1] = np.arange((minors == 1).sum())
    want[minors == 3] = np.arange((minors == 3).sum()) | (1 << 30)
    return want


class _HrptModel:
    """_noaa_ref.hrpt_demux_fast per row and call (no state between frames); what the getters report is the last call's."""

    def __init__(self, rows):
        self.rows, self.last_counts, self.minors, self.tip, self.aip = rows, np.zeros((3, rows), np.int32), [np.zeros(0, np.int64)] * rows, None, None

    def run(self, fr, eff):
        res = [NR.hrpt_demux_fast(fr[r, :eff[r]]) for r in range(self.rows)]
        self.last_counts = np.asarray([eff, [len(q[1]) for q in res], [len(q[2]) for q in res]], np.int32)
        self.minors, self.tip, self.aip = [q[3] for q in res], [q[1] for q in res], [q[2] for q in res]
        return res

    def check(self, got, fr, eff, label):
        av, tip, tc, aip, ac = got
        w_av, w_tip, w_aip = np.full_like(av, NOAA_S16), np.full_like(tip, NOAA_S8), np.full_like(aip, NOAA_S8)
        for r, (a, t, p, _) in enumerate(self.run(fr, eff)):
            w_av[r, :, :eff[r]] = a
            w_tip[r, :t.size], w_aip[r, :p.size] = t.ravel(), p.ravel()
        assert tc.tolist() == self.last_counts[1].tolist() and ac.tolist() == self.last_counts[2].tolist(), f"{label}: TIP / AIP counts"
        for name, g, w in (("avhrr", av, w_av), ("tip", tip, w_tip), ("aip", aip, w_aip)):
            assert A.same_bits(g, w), f"{label}: {name} allocation: {np.argwhere(g != w)[:4].tolist()}"


def _frame_slots(op, chan, cap):
    from qdsp_amd import capi

    L = capi.load()

    def fn():
        buf = np.full(cap, -7, np.int32)
        return np.int32(capi.check(L.qdsp_hip_hrpt_get_frame_slots(op._h, chan, buf.ctypes.data, cap))), buf

    return Host(f"HrptDemux.get_frame_slots({chan})", fn, op, "get_frame_slots")


def _slots_are(model, chan, cap):
    def chk(v):
        want = _slot_ranks(model.minors[chan])
        m = min(len(want), cap)
        assert int(v[0]) == len(want) and np.array_equal(v[1][:m], want[:m]) and (v[1][m:] == -7).all(), ("get_frame_slots", chan, v, want)
    return chk


def test_noaa_hrpt(ops, noaa):
    """HrptDemux over 5 rows, process_batch into sentinel-filled torch-owned outputs: counts, qdsp_hip_hrpt_get_frame_slots, an
    nframes == 0 call, per-row device counts, and a 5-frame call on a handle made for 2 (hrpt_scratch frees the slots and the
    library's own TIP / AIP rows while the call before it is queued; that call's outputs are checked after the growth, like
    every other), each host action with a call still held; own_dev at the end (host only: the stride of the grown rows)."""
    rng = np.random.default_rng(44)

    def scenario():
        op = noaa.HrptDemux(nchan=ROWS, max_block=2)
        model, steps = _HrptModel(ROWS), []

        def call(n, in_counts=None):
            fr, m, label = _hrpt_frames(rng, ROWS, n), max(n, 1), f"process_batch {len(steps)} ({n})"
            xin, cin = _In(fr.reshape(ROWS, n * NR.FRAME_BYTES), rows=True), None if in_counts is None else _In(np.asarray(in_counts, np.int32))
            fa, ft = _fresh((ROWS, 5, m + 1, 2048), NOAA_S16, np.uint16), _fresh((ROWS, m * 520 + 7), NOAA_S8, np.uint8)

            def fn():
                a, t, p = fa(), ft(), ft()
                _, _, tc, _, ac = op.process_batch(xin(), nframes=n, in_counts=None if cin is None else cin(), avhrr=a[:, :, :m], tip=t, aip=p)
                return a, t, tc, p, ac

            steps.append(_checked(Call(label, fn, op, {"hrpt_avhrr_kernel"}), lambda v: model.check(v, fr, _eff(in_counts, n, ROWS), label)))

        def same_counts(v):
            _is(v[0], model.last_counts, "counts")

        call(2), call(2)
        steps.append(_checked(H(op, "counts"), same_counts))
        call(2), call(2, [2, 0, 5, -1, 1])
        steps.append(_checked(_frame_slots(op, 2, 4), _slots_are(model, 2, 4)))
        call(2), call(0)
        steps.append(_checked(H(op, "counts"), same_counts))
        call(2), call(5), call(5)                     # more frames than any call before
        steps.append(_checked(_frame_slots(op, 4, 3), _slots_are(model, 4, 3)))
        call(3), call(3, [3, 1, 0, 3, 2])
        steps.append(_checked(H(op, "counts"), same_counts))
        call(2)
        steps.append(_checked(Host("HrptDemux.own_dev", lambda: np.int64(op.own_dev("tip")[1]), op, "own_dev"), lambda v: _is(v[0], 5 * 520, "own_dev stride")))
        return steps

    rng_state = rng.bit_generator.state

    def same_every_run():
        rng.bit_generator.state = rng_state           # (every run of the scenario sees the same frames)
        return scenario()

    _anchor(_three_ways("noaa hrpt", same_every_run))


def test_noaa_hrpt_one_row(ops, noaa):
    """HrptDemux's single-output entry point (qdsp_hip_hrpt_process_dev: AVHRR to the caller, TIP and AIP into the library's own
    rows) with tip(chan), aip(chan), get_frame_slots and counts as racing getters, and a 4-frame call on a handle made for 2: the
    rows the getters read are freed and reallocated with the call before still queued."""
    import torch

    from qdsp_amd import capi

    rng = np.random.default_rng(45)
    frames = {k: _hrpt_frames(rng, 1, n) for k, n in enumerate([2, 2, 2, 2, 2, 2, 2, 4, 4, 3, 3])}

    def scenario():
        op = noaa.HrptDemux(nchan=1, max_block=2)
        model, steps = _HrptModel(1), []

        def single():
            fr = frames[sum(not s.racing for s in steps)]
            n = fr.shape[1]
            xin, fresh, label = _In(fr.ravel()), _fresh(5 * n * 2048 + 16, NOAA_S16, np.uint16), f"process_dev {len(steps)} ({n})"

            def fn():
                out = fresh()
                capi.check(int(op._fn("process_dev")(op._h, xin().data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)))
                return out

            def chk(v):
                av = model.run(fr, [n])[0][0]
                assert A.same_bits(v[0][:av.size], av.ravel()) and (v[0][av.size:] == NOAA_S16).all(), f"{label}: AVHRR lines"
            steps.append(_checked(Call(label, fn, op, {"hrpt_avhrr_kernel"}), chk))

        single(), single()
        steps.append(_checked(H(op, "tip", 0), lambda v: A.same_bits(v[0], model.tip[0]) or pytest.fail("tip(0)")))
        single(), single()
        steps.append(_checked(H(op, "aip", 0), lambda v: A.same_bits(v[0], model.aip[0]) or pytest.fail("aip(0)")))
        single(), single()
        steps.append(_checked(_frame_slots(op, 0, 8), _slots_are(model, 0, 8)))
        single(), single(), single()                  # 2, 4 and 4 frames
        steps.append(_checked(H(op, "tip", 0), lambda v: A.same_bits(v[0], model.tip[0]) or pytest.fail("tip(0) after the growth")))
        single(), single()
        steps.append(_checked(H(op, "counts"), lambda v: _is(v[0], model.last_counts, "counts")))
        return steps

    serial = _three_ways("noaa hrpt one row", scenario)
    _anchor(serial)
    got = [v[0] for (_, v), st in zip(serial.outputs, serial.steps) if st.racing and (".tip" in st.label or ".aip" in st.label)]
    assert len(got) == 3 and all(len(g) for g in got), "a getter that read no minor frame checked nothing"


def test_noaa_tip(ops, noaa):
    """TipDemux over 5 rows: counts, a count == 0 call, per-row device counts and a call longer than any before (two workgroups a
    row), each getter with a call still held."""
    rng = np.random.default_rng(46)
    blocks = [rng.integers(0, 256, (ROWS, n, 104)).astype(np.uint8) for n in (5, 5, 5, 0, 5, 70, 70, 5)]
    counts_of = {2: [5, 0, 9, -2, 3], 6: [70, 64, 65, 0, 1]}

    def scenario():
        op = noaa.TipDemux(nchan=ROWS, max_block=5)
        steps, last = [], {}

        def call():
            k = sum(not s.racing for s in steps)
            mf, in_counts = blocks[k], counts_of.get(k)
            n = mf.shape[1]
            eff, label = _eff(in_counts, n, ROWS), f"process_batch {len(steps)} ({n})"
            xin, cin, fresh = _In(mf.reshape(ROWS, n * 104), rows=True), None if in_counts is None else _In(np.asarray(in_counts, np.int32)), _fresh((ROWS, n * 74 + 7), NOAA_S8, np.uint8)

            def fn():
                out = fresh()
                _, counts = op.process_batch(xin(), out, count=n, in_counts=None if cin is None else cin())
                return out, counts

            def chk(v):
                want = np.full_like(v[0], NOAA_S8)
                for r in range(ROWS):
                    want[r, :eff[r] * 74] = NR.tip_demux(mf[r, :eff[r]]).ravel()
                last["counts"] = eff
                assert v[1].tolist() == eff and A.same_bits(v[0], want), f"{label}: not the definition's records, or written past a row's count"
            steps.append(_checked(Call(label, fn, op, {"tip_kernel"}), chk))

        def counts():
            steps.append(_checked(H(op, "counts"), lambda v: _is(v[0], last["counts"], "counts")))

        call(), call()
        counts()
        call(), call()                                # device counts, then count == 0
        counts()
        call(), call(), call()                        # 5, then 70 twice: longer than any call before
        counts()
        call()
        return steps

    _anchor(_three_ways("noaa tip", scenario))


def test_noaa_chain_with_a_racing_setter_and_growth(ops, noaa):
    """Deframer(110900, the 60-bit sync) -> HrptDemux -> TipDemux -> HirsDemux(stride 74) over 2 rows, every stage reading the one
    before's device counts, three rounds on one stream: HirsDemux.set_state(60, True) races the first round's held calls (the
    next round's first packet then ends every row's line); the third round has 4 frames a row on an HrptDemux made for 2, so
    hrpt_scratch frees the slots with the second round's kernels still queued.  A fresh Deframer per round (a round's bits end
    inside the noise behind its last frame).  Reference: the rows' own frames, then the definition chain with one HirsFast per
    row carried over the rounds."""
    import torch

    from test_noaa_cpu import noaa_check_input

    frames, _ = noaa_check_input(9, min_lines=1)       # minors 1, 1, 3, 0, 1, 2, 1, 3, 1
    rounds = [[frames[0:1], frames[6:7]], [frames[1:2], frames[8:9]], [frames[2:5], frames[[5, 7]]]]
    sync = NR.sync_bits()

    def round_bits(rows):
        nf = max(len(fr) for fr in rows)
        width = 41 + nf * NR.FRAME_BITS + 100
        bits = np.zeros((2, width), np.uint8)
        for r, fr in enumerate(rows):
            b = np.unpackbits(fr, axis=1)[:, :NR.FRAME_BITS].ravel()
            bits[r, 41 - 4 * r:41 - 4 * r + b.size] = b
        return bits, np.array([width, 37 + len(rows[1]) * NR.FRAME_BITS + 80], np.int32)

    inputs = [round_bits(rows) for rows in rounds]

    def scenario():
        hr, tp, hi = noaa.HrptDemux(nchan=2, max_block=2), noaa.TipDemux(nchan=2, max_block=20), noaa.HirsDemux(74, nchan=2, max_block=20)
        model, steps = _HirsModel(2, 74), []

        def one_round(k):
            bits, nbits = inputs[k]
            width = bits.shape[1]
            df = ops.Deframer(NR.FRAME_BITS, sync, nchan=2, max_block=width)
            cap = df.out_size(width)
            x, xn, s = _In(bits), _In(nbits), {}
            zeros = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")              # noqa: E731
            zeros16 = lambda *shape: zeros(*shape[:-1], 2 * shape[-1]).view(torch.uint16)              # noqa: E731

            def deframe():
                s["frames"], s["nf"] = df.process_batch(x(), out=zeros(2, cap * NR.FRAME_BYTES), in_counts=xn())
                return s["frames"], s["nf"]

            def hrpt():
                s["hr"] = hr.process_batch(s["frames"], nframes=cap, in_counts=s["nf"], avhrr=zeros16(2, 5, cap, 2048),
                                           tip=zeros(2, cap * 520), aip=zeros(2, cap * 520))
                return s["hr"]

            def tip():
                s["rec"], s["nr"] = tp.process_batch(s["hr"][1], zeros(2, 5 * cap * 74), count=5 * cap, in_counts=s["hr"][2])
                return s["rec"], s["nr"]

            def hirs():
                return hi.process_batch(s["rec"], zeros16(2, 20, 5 * cap + 1, 56), count=5 * cap, in_counts=s["nr"])

            ref = {}

            def chk_deframe(v):
                for r, fr in enumerate(rounds[k]):
                    assert int(v[1][r]) == len(fr) and np.array_equal(v[0][r, :fr.size], fr.ravel()) and not v[0][r, fr.size:].any(), ("deframer", k, r)

            def chk_hrpt(v):
                a, t, tc, p, pc = v
                ref["hr"] = [NR.hrpt_demux_fast(fr) for fr in rounds[k]]
                for r, (av, tip_, aip_, _) in enumerate(ref["hr"]):
                    nf = av.shape[1]
                    assert np.array_equal(a[r][:, :nf], av) and not a[r][:, nf:].any() and int(tc[r]) == len(tip_) and int(pc[r]) == len(aip_), ("hrpt", k, r)
                    assert np.array_equal(t[r, :tip_.size], tip_.ravel()) and not t[r, tip_.size:].any(), ("tip rows", k, r)
                    assert np.array_equal(p[r, :aip_.size], aip_.ravel()) and not p[r, aip_.size:].any(), ("aip rows", k, r)

            def chk_tip(v):
                ref["rec"] = [NR.tip_demux(q[1]) for q in ref["hr"]]
                for r, rec in enumerate(ref["rec"]):
                    assert int(v[1][r]) == len(rec) and np.array_equal(v[0][r, :rec.size], rec.ravel()) and not v[0][r, rec.size:].any(), ("tip", k, r)

            def chk_hirs(v):
                x_rows = [rec.ravel() for rec in ref["rec"]]
                for r, ln in enumerate(model.lines(x_rows, [len(rec) for rec in ref["rec"]])):
                    assert int(v[1][r]) == ln.shape[1] and np.array_equal(v[0][r][:, :ln.shape[1]], ln) and not v[0][r][:, ln.shape[1]:].any(), ("hirs", k, r)

            steps.extend([_checked(Call(f"deframe {k}", deframe, df), chk_deframe), _checked(Call(f"hrpt {k}", hrpt, hr, {"hrpt_avhrr_kernel"}), chk_hrpt),
                          _checked(Call(f"tip {k}", tip, tp, {"tip_kernel"}), chk_tip), _checked(Call(f"hirs {k}", hirs, hi, {"hirs_pack_kernel"}), chk_hirs)])

        one_round(0)
        steps.append(_checked(H(hi, "set_state", 60, True), lambda v: model.set_state(60, True)))
        one_round(1)
        one_round(2)
        steps.append(_checked(H(hi, "counts"), lambda v: _is(v[0], model.last_counts, "hirs counts")))
        return steps

    serial = _three_ways("noaa chain", scenario)
    _anchor(serial)
    out = dict(serial.outputs)
    assert all(int(c) >= 1 for c in out["hirs 1"][1]), "set_state(60, True) ends every row's line in progress at the next packet"
    assert sum(int(out[f"hrpt {k}"][2].sum() + out[f"hrpt {k}"][4].sum()) for k in range(3)) >= 25 and int(out["hirs 0"][1].sum()) >= 1


# ------------------------------------------------------------------------------------------------ Math, Xlator alone, the sine source
def test_math_xlator_and_sine_source(ops):
    from qdsp_amd import capi

    L = capi.load()
    n = N_DIRECT

    def math_scenario():
        ma, mm = ops.Math(ops.Math.ADD, max_block=0), ops.Math(ops.Math.MUL, complex_data=False, max_block=0)
        ha, hb = O.synth_iq(0, n, seed=1), O.synth_iq(0, n, seed=2)
        a, b = _In(ha), _In(hb)
        ar, br = _In(np.ascontiguousarray(O.synth_iq(0, n, seed=3).real)), _In(np.ascontiguousarray(O.synth_iq(0, n, seed=4).imag))
        steps = [Call("add", lambda: ma.process(a(), b())), Call("mul", lambda: mm.process(ar(), br()))]
        har, hbr = np.ascontiguousarray(O.synth_iq(0, n, seed=3).real), np.ascontiguousarray(O.synth_iq(0, n, seed=4).imag)
        steps[0].check = lambda v: A.same_bits(v[0], O.math_op(0, ha, hb)) or pytest.fail("Math ADD")
        steps[1].check = lambda v: A.same_bits(v[0], O.math_op(2, har, hbr)) or pytest.fail("Math MUL")
        return steps

    _anchor(_three_ways("math", math_scenario))

    def xlate_scenario():
        op = ops.Xlator(phase_inc=ops.phase_delta(1.0, F_A), max_block=0)
        xl = O.Xlator(1.0, F_A, exact=True, volk_gain=True)
        steps, pos = [], [0]

        def calls():
            for _ in range(2):
                x = O.synth_iq(pos[0], n, seed=8)
                pos[0] += n
                xd = _In(x)
                st = Call(f"process {len(steps)}", lambda xd=xd: op.process(xd()), op, None)
                st.check = lambda v, x=x: _close_to("xlator", v[0], xl.process(x))
                steps.append(st)

        calls()
        steps.append(_checked(H(op, "set_phase_inc", *ops.phase_delta(1.0, F_B)), lambda v: O.lib().oracle_xlator_phase_delta(1.0, F_B, O._fp(xl.delta))))
        calls()
        steps.append(_checked(H(op, "set_phase", 0.6, 0.8), lambda v: setattr(xl.turns, "value", math.atan2(0.8, 0.6) / (2 * math.pi))))
        calls()
        steps.append(_checked(H(op, "set_volk_gain", False), lambda v: setattr(xl, "volk_gain", False)))
        calls()
        steps.append(_checked(H(op, "get_phase"), lambda v: abs(complex(v[0]) - np.exp(2j * np.pi * xl.turns.value)) < TOL_PHASE or pytest.fail("get_phase")))
        calls()
        steps.append(_checked(H(op, "advance", 777), lambda v: _advance(xl, 777)))
        calls()
        return steps

    _anchor(_three_ways("xlator", xlate_scenario))

    def sine_scenario():
        import torch

        h = C.c_void_p()
        capi.check(L.qdsp_hip_sine_cf32_create(C.byref(h), 0, *ops.phase_delta(1.0, F_A), 0))
        keep = {"h": h}
        steps = []

        def gen():
            out = torch.zeros(n, dtype=torch.complex64, device="cuda")
            capi.check(L.qdsp_hip_sine_cf32_generate_dev(keep["h"], n, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
            return out

        def phase():
            re, im = C.c_float(), C.c_float()
            capi.check(L.qdsp_hip_sine_cf32_get_phase(keep["h"], C.byref(re), C.byref(im)))
            return complex(re.value, im.value)

        steps += [Call("generate 0", gen), Call("generate 1", gen)]
        steps.append(Host("sine set_phase_inc", lambda: capi.check(L.qdsp_hip_sine_cf32_set_phase_inc(keep["h"], *ops.phase_delta(1.0, F_B)))))
        steps += [Call("generate 2", gen), Call("generate 3", gen)]
        steps.append(Host("sine get_phase", phase))
        steps += [Call("generate 4", gen), Call("generate 5", gen)]
        steps.append(Host("sine destroy", lambda: L.qdsp_hip_sine_cf32_destroy(keep.pop("h"))))
        return steps

    _three_ways("sine source", sine_scenario)


# ------------------------------------------------------------------------------------------------ release
def _close_noaa():
    """HirsDemux (its destroy frees the most: both state and partial-line slots, the map, the pinned count), HrptDemux (the slots
    and its own TIP / AIP rows) and TipDemux, each closed behind two held calls into sentinel-filled torch-owned outputs."""
    from qdsp_amd import noaa
    from test_gpu_noaa import Climb

    rng, gen, steps = np.random.default_rng(32), Climb(ROWS, 362, 36), []
    hi, hr, tp = noaa.HirsDemux(nchan=ROWS, max_block=12), noaa.HrptDemux(nchan=ROWS, max_block=2), noaa.TipDemux(nchan=ROWS, max_block=9)
    hmodel, rmodel = _HirsModel(ROWS, 36), _HrptModel(ROWS)
    for k in range(2):
        x = np.stack([gen.packets(r, 12) for r in range(ROWS)])
        steps.append(_hirs_call(f"hirs {k}", hi, hmodel, x, 12))
    steps.append(H(hi, "close"))
    for k in range(2):
        fr = _hrpt_frames(rng, ROWS, 2)
        xin, fa, ft = _In(fr.reshape(ROWS, -1), rows=True), _fresh((ROWS, 5, 3, 2048), NOAA_S16, np.uint16), _fresh((ROWS, 2 * 520 + 7), NOAA_S8, np.uint8)

        def fn(xin=xin, fa=fa, ft=ft):
            a, t, p = fa(), ft(), ft()
            _, _, tc, _, ac = hr.process_batch(xin(), nframes=2, avhrr=a[:, :, :2], tip=t, aip=p)
            return a, t, tc, p, ac
        steps.append(_checked(Call(f"hrpt {k}", fn, hr), lambda v, fr=fr, k=k: rmodel.check(v, fr, [2] * ROWS, f"hrpt {k}")))
    steps.append(H(hr, "close"))
    for k in range(2):
        mf = rng.integers(0, 256, (ROWS, 9, 104)).astype(np.uint8)
        xin, fresh = _In(mf.reshape(ROWS, -1), rows=True), _fresh((ROWS, 9 * 74 + 7), NOAA_S8, np.uint8)

        def fn(xin=xin, fresh=fresh):
            out = fresh()
            return out, tp.process_batch(xin(), out, count=9)[1]

        def chk(v, mf=mf):
            want = np.full_like(v[0], NOAA_S8)
            want[:, :9 * 74] = np.stack([NR.tip_demux(mf[r]).ravel() for r in range(ROWS)])
            assert v[1].tolist() == [9] * ROWS and A.same_bits(v[0], want), "tip records behind a close"
        steps.append(_checked(Call(f"tip {k}", fn, tp), chk))
    steps.append(H(tp, "close"))
    return steps


@pytest.mark.parametrize("which", ["engine", "per_row", "chain", "fec", "noaa"])
def test_close_while_the_last_call_is_held(ops, monkeypatch, which):
    """process into a torch-owned output, then close() while that call is still queued: every *_destroy waits for the device
    before its first hipFree (Engine destroy, level_free, chain_free and the stages' own, rs_free, hirs_free / hrpt_free /
    tip_free), so the output is the serial run's (and, for the NOAA handles, the definition's)."""
    _pin(monkeypatch, {})
    if which == "noaa":
        _anchor(_three_ways("close noaa", _close_noaa))
        return

    def scenario():
        import torch

        rng = np.random.default_rng(31)
        if which == "engine":
            op = ops.Fir(_taps(1, 1, 63), max_block=0)
            xs = [_In(O.synth_iq(i * N_DIRECT, N_DIRECT, seed=6)) for i in range(2)]
            outs = [torch.zeros(N_DIRECT, dtype=torch.complex64, device="cuda") for _ in xs]
            call = lambda i: op.process(xs[i](), outs[i])                                              # noqa: E731
        elif which == "per_row":
            op = ops.Squelch(-50.0, nchan=ROWS, max_block=0)
            xs = [_In(_cx(rng, ROWS, 3 * TILE + 5), rows=True) for _ in range(2)]
            outs = [torch.zeros((ROWS, 3 * TILE + 5), dtype=torch.complex64, device="cuda") for _ in xs]
            call = lambda i: op.process_batch(xs[i](), outs[i])                                        # noqa: E731
        elif which == "fec":
            from qdsp_amd import fec

            lay = RS.falcon_layout()
            op = fec.FalconRs(nchan=ROWS, max_block=3)
            xs = [_In(gen_frames(rng, lay, ROWS * 3).reshape(ROWS, -1), rows=True) for _ in range(2)]
            outs = [torch.zeros((ROWS, 3 * op.frame_out), dtype=torch.uint8, device="cuda") for _ in xs]
            call = lambda i: op.process_batch(xs[i](), outs[i])                                        # noqa: E731
        else:
            op = ops.MskDemod(48000.0, 6000.0, 12000.0, nchan=ROWS, max_block=0)
            xs = [_In(_cx(rng, ROWS, 4111, 0.05), rows=True) for _ in range(2)]
            call = lambda i: _pb(op, xs[i]())                                                          # noqa: E731
        return [Call("process 0", lambda: call(0), op), Call("process 1", lambda: call(1), op), H(op, "close")]

    _three_ways(f"close {which}", scenario)


# ------------------------------------------------------------------------------------------------ coverage (keep last)
# public set_* / get_* / reset / configure methods that no scenario races, each with its reason
NOT_RACED = {
    ("*", "set_done_event"): "only read by process_ex's deferred link, i.e. on the handle's own or the library's shared stream: out of this module's reach",
    ("*", "set_history_ptr"): "the raw-pointer spelling of set_history_dev (same C entry point, which is raced), for the C ring",
    ("Threshold", "reset"): "Threshold has no state: the method does nothing",
    ("RsDecoder", "reset"): "no state between frames: the method does nothing",
    ("FalconRs", "reset"): "no state between frames: the method does nothing",
    ("HrptDemux", "reset"): "no state between frames: the method does nothing",
    ("TipDemux", "reset"): "no state between minor frames: the method does nothing",
}
# getters of qdsp_amd.noaa that the name filter below does not find: raced all the same
NOAA_GETTERS = {("HirsDemux", "counts"), ("HrptDemux", "counts"), ("HrptDemux", "tip"), ("HrptDemux", "aip"), ("HrptDemux", "get_frame_slots"),
                ("TipDemux", "counts")}


def test_scenarios_cover_the_library(ops):
    """Every kernel family of tests/test_gpu_fuzz.py's FAMILIES and every per-row kernel family ran in an async scenario, and every
    public setter, getter, reset and configure of every operator class of qdsp_amd.ops, qdsp_amd.fec and qdsp_amd.noaa was a
    racing host action (or is excluded above, with a reason)."""
    from qdsp_amd import fec, noaa

    seen = set(_SEEN)
    if seen & DMA:
        seen.add("fir_fft_dma_kernel")
    missing = (FAMILIES | PER_ROW_FAMILIES) - seen
    assert not missing, f"kernel families no async scenario ran: {sorted(missing)} (seen: {sorted(seen)})"
    assert NOAA_GETTERS <= _RACED, f"never a racing host action: {sorted(NOAA_GETTERS - _RACED)}"
    unraced, public, raced_methods = [], set(), set()
    classes = [(n, c, m) for m in (ops, fec, noaa) for n, c in inspect.getmembers(m, inspect.isclass)]
    assert {"RsDecoder", "FalconRs"} <= {n for n, c, m in classes if c.__module__ == fec.__name__}
    assert {"HrptDemux", "TipDemux", "HirsDemux"} <= {n for n, c, m in classes if c.__module__ == noaa.__name__}
    for name, cls, mod in classes:
        if cls.__module__ != mod.__name__ or name.startswith("_"):
            continue
        for m in dir(cls):
            if not (m.startswith("set_") or m.startswith("get_") or m in ("reset", "configure", "advance")) or not callable(getattr(cls, m)):
                continue
            public.add((name, m))
            if (name, m) in _RACED:
                assert (name, m) not in NOT_RACED, f"{name}.{m} is raced: its exclusion is stale"
                raced_methods.add(m)
            elif (name, m) not in NOT_RACED and ("*", m) not in NOT_RACED:
                unraced.append(f"{name}.{m}")
    assert not unraced, f"never a racing host action, and not excluded: {unraced}"
    for cls_name, m in NOT_RACED:
        if cls_name == "*":
            assert any(pm == m for _, pm in public) and m not in raced_methods, f"the exclusion of {m} for every class is stale"
        else:
            assert (cls_name, m) in public, f"the exclusion of {cls_name}.{m} names no public method"
