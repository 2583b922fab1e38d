"""One kernel family taking over the stream another one left, and a dispatch that does not depend on the handle's past.

`process_dev` (qdsp_amd/csrc/qdsp_hip.hip) picks one of about a dozen kernel families per call of a decimator, a fused VFO or a real-data
filter, and every family leaves the stream state in its own way: the direct kernels write the rotated history d_hist[cur ^ 1], the
overlap-save kernels keep a raw side copy as well (d_hist_raw, raw_valid, raw_history()), and each family reads plan-time tables of its own
(d_taps_lm, d_taps_mf, the spectra keyed by the tap count and the NCO increment, the NCO tables).  The rest of the suite judges each family
alone or a whole call by relative RMS, where the few outputs that depend on the handed-over history drown among thousands that do not.

  1. the transition matrix: ONE handle per plan, created under the defaults, walks every ordered pair of the plan's families (an Euler circuit
     of the complete digraph, built and checked here), then meets a short call, an empty call, new taps of the same length and -- the VFO -- a
     retune and a phase jump between any two families.  After every call: the call's outputs against the FP64 oracle, the HEAD of the call
     (the ceil(H / M) + 1 outputs that read the handed-over history) on its own, get_history() and get_phase();
  2. a handle that has served a call in a cell of the measured table (decim_table.inc) that vetoes the strided-window kernel, and then got
     new taps, must dispatch, launch and compute exactly like a fresh handle (first item);
  3. every (class, decimation, setting) of the committed table under the shipped defaults, against the oracle with the checks of part 1.

The families are steered per call with switches the library reads per call (the `_STEER` table) and with set_mode; the handle itself is
never recreated.  Bounds: relative RMS per call 2e-6 (DESIGN.md's overlap-save bound, the loosest per-family bound the project states), head
of a call 4e-6 x max|want| (test_polyphase_overlap_save_decimator_vs_oracle), VFO history 6e-7 against the exact-phase oracle mixer
(test_xlator_long_stream_exact_phase, same synth_iq scale), NCO phase 1e-6."""
import contextlib
import math
import os
import re

import numpy as np
import pytest

import oracle as O
from conftest import kname, rel_rms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_RMS = 2e-6        # per call, every family
TOL_HEAD = 4e-6       # x max|want| of the call, on the outputs that read the handed-over history
TOL_HIST = 6e-7       # fused VFO: rotated history against the exact-phase oracle mixer
TOL_PHASE = 1e-6
F_A, F_B = 0.1234, -0.0777      # NCO offsets (fs = 1): every VFO starts on F_A, a retune toggles

WIN, CORE, ANY, F1K, F4K = "decim_win_kernel", "fir_core_kernel", "resamp_any_kernel", "fir_fft1k_kernel", "fir_fft_kernel"
AUTO, DIRECT, FFT = 0, 1, 2

# Worst figures seen, by (plan, family of the call): [head error / max|want|, history deviation, relative RMS].  Printed by every stream.
_WORST = {}


@pytest.fixture(scope="module")
def ops():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from qdsp_amd import ops as _ops

    return _ops


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _lp(ntaps, fc, gain=1.0):
    return (O.lowpass_taps_f64(ntaps, fc) * gain).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the table's mirror
def _load_decim_table():
    inc = open(os.path.join(ROOT, "qdsp_amd", "csrc", "decim_table.inc")).read()
    k = {name: int(v) for name, v in re.findall(r"(kDecimTab\w+) = (\d+)", inc)}
    ms = [int(v) for v in re.search(r"kDecimTabM\[kDecimTabMs\] = \{([^}]*)\}", inc).group(1).split(",")]
    taps = [int(v) for v in re.search(r"kDecimTabTaps\[kDecimTabCols\] = \{([^}]*)\}", inc).group(1).split(",")]
    rows = [[int(v) for v in m.group(1).split(",")] for m in re.finditer(r"\*/ \{([^}]*)\},", inc)]
    tab = np.array(rows, dtype=np.int64).reshape(k["kDecimTabClasses"], k["kDecimTabMs"], k["kDecimTabRows"], k["kDecimTabCols"])
    assert len(ms) == k["kDecimTabMs"] and len(taps) == k["kDecimTabCols"]
    return {"lmin": k["kDecimTabLog2Min"], "M": ms, "taps": taps, "tab": tab}


_T = _load_decim_table()


def _m_index(M):
    ms = _T["M"]
    if M < ms[0] or M > ms[-1]:
        return -1
    if M in ms:
        return ms.index(M)
    for i in range(1, len(ms)):
        if ms[i - 1] >= 10 and ms[i - 1] < M < ms[i]:
            return i if M * M >= ms[i - 1] * ms[i] else i - 1
    return -1


def _row(count):
    lg = int(count).bit_length() - 1
    if count - (1 << lg) > (1 << lg) * 0.41421356:
        lg += 1
    return min(max(lg - _T["lmin"], 0), _T["tab"].shape[2] - 1)


def _col(ntaps):
    col, taps = 0, _T["taps"]
    for c in range(1, len(taps)):
        if float(ntaps) * ntaps >= float(taps[c - 1]) * taps[c]:
            col = c
    return col


def decim_setting(cls, M, ntaps, count):
    """decim_table_setting() of qdsp_hip.hip on the committed decim_table.inc: class 0 complex decimator, 1 fused VFO, 2 real data."""
    if count <= 0 or cls >= _T["tab"].shape[0] or ntaps < _T["taps"][0] / 2:
        return 0
    mi = _m_index(M)
    return 0 if mi < 0 else int(_T["tab"][cls, mi, _row(count), _col(ntaps)])


_WIN_LIMIT = [0, 7, 150, 150, 160, 200, 256, 160, 200, 0, 192, 0, 224, 0, 0, 0, 256]      # win_limit() of qdsp_hip.hip


def _win_is_the_rules_choice(cls, M, ntaps, count):
    """The rule chain of process_dev, as far as calls of up to 2^16 samples need it: the strided-window kernel serves the shape (use_win),
    no MFMA table outranks it (mf_plan: from 6 taps per unit of decimation, decimation >= 9) and it does not hand the call to the one-wave
    overlap-save form (win_yields_to_fft1k: complex data, >= 96 taps, <= 2^19 samples).  The tests assert the kernel a fresh handle
    takes on top of this, so a rule that moves makes them fail, not pass."""
    if M > 16 or _WIN_LIMIT[M] == 0 or ntaps > _WIN_LIMIT[M]:
        return False
    if M >= 9 and ntaps >= 6 * M and (M >= 14 or ntaps >= 12 * M):
        return False
    if cls != 2 and ntaps >= 96 and count <= (1 << 19):
        return False
    return True


def history_pairs():
    """(class, decimation, taps, row of a cell that vetoes the window kernel, row of a setting-0 cell where that kernel is the rules' choice),
    one per (class, decimation, taps) column that has both: veto rows up to 2^13, plain rows up to 2^17 (the largest call this module makes;
    the real-data column at decimation 2, 48 taps has its first plain cell there)."""
    out, lmin = [], _T["lmin"]
    for cls in range(_T["tab"].shape[0]):
        for mi, M in enumerate(_T["M"]):
            for col, ntaps in enumerate(_T["taps"]):
                veto = [r for r in range(0, 13 - lmin + 1) if _T["tab"][cls, mi, r, col] in (1, 3)]
                plain = [r for r in range(0, 17 - lmin + 1)
                         if _T["tab"][cls, mi, r, col] == 0 and _win_is_the_rules_choice(cls, M, ntaps, 1 << (r + lmin))]
                if veto and plain:
                    out.append((cls, M, ntaps, veto[0] + lmin, plain[0] + lmin))
    return out


def table_triples():
    """Every distinct (class, decimation, setting != 0) of the table with the first cell (smallest row, then column) that holds it."""
    out = []
    for cls in range(_T["tab"].shape[0]):
        for mi, M in enumerate(_T["M"]):
            first = {}
            for r in range(_T["tab"].shape[2]):
                for col in range(_T["tab"].shape[3]):
                    s = int(_T["tab"][cls, mi, r, col])
                    if s and s not in first:
                        first[s] = (r + _T["lmin"], _T["taps"][col])
            out += [(cls, M, s, lg, ntaps) for s, (lg, ntaps) in sorted(first.items())]
    return out


def _in_cell(lg, M, salt=37):
    """A ragged call size in the table row 2^lg: no multiple of the decimation."""
    n = (1 << lg) + salt
    while M > 1 and n % M == 0:
        n += 1
    return n


# ------------------------------------------------------------------------------------------------------------ steering
@contextlib.contextmanager
def _switches(op, mode, env):
    """set_mode + QDSP_HIP_* variables for one call; everything back to the defaults afterwards."""
    from qdsp_amd import capi

    try:
        for k, v in env.items():
            capi.setenv("QDSP_HIP_" + k, v)
        op.set_mode(mode)
        yield
    finally:
        op.set_mode(AUTO)
        for k in env:
            capi.setenv("QDSP_HIP_" + k, None)


def _steer(family):
    """(mode, switches) that send a call of 4 500 .. 40 000 samples of the module's plans to `family` (process_dev's chain, top to bottom:
    MFMA table, overlap-save, strided window, de-interleaved direct, general direct).  DECIM_SETTING=0 keeps the measured table out of the
    AUTO calls; a set_mode call never consults it."""
    rules = {"DECIM_SETTING": "0"}
    if family == WIN:
        return AUTO, dict(rules, NO_MF="1", NO_FFT1K="1")
    if family == CORE:
        return DIRECT, {}
    if family == ANY:
        return DIRECT, {"FORCE_ANY": "1"}
    if family == F1K:      # (FFT_MIN_TAPS_DECIM: the rule keeps filters below 112 taps off the overlap-save forms at decimation 2-6 -- the 96-tap plan)
        return AUTO, dict(rules, NO_MF="1", FFT_MIN_TAPS_DECIM="2")
    if family == F4K:
        return FFT, {"NO_PFB": "1"}
    if family.startswith("pfb_dec"):
        return FFT, {"PFB_MIN_COUNT": "0"}
    if family.startswith("decim_mfma"):
        return AUTO, dict(rules, MF_MIN_COUNT="0")
    raise AssertionError(family)


# ------------------------------------------------------------------------------------------------------------ one stream, device and oracle
class _Stream:
    """One device handle and its oracle, fed the same blocks.  cls: the table's class (0 complex decimator, 1 fused VFO, 2 real data;
    real data at decimation 1 is FIR<float>)."""

    def __init__(self, ops, cls, M, ntaps, seed, label):
        self.ops, self.cls, self.M, self.ntaps, self.seed, self.label = ops, cls, M, ntaps, seed, label
        self.tap_sets = [_lp(ntaps, 0.45 / M), (_lp(ntaps, 0.30 / M) * np.float32(0.75)).astype(np.float32)]
        self.which = 0
        self.freq = F_A
        self.op = self.make(self.tap_sets[0])
        self.orc = self._oracle(self.tap_sets[0])
        self.xl = O.Xlator(1.0, F_A, exact=True, volk_gain=True) if cls == 1 else None
        self.H = self.op.history_len
        self.dtype = np.float32 if cls == 2 else np.complex64
        self.tail = np.zeros(self.H, self.dtype)      # what get_history() must return: raw input (mixer output for the VFO), zeros before the start
        self.pos = 0
        self.index = 0

    def make(self, taps):
        ops, M = self.ops, self.M
        if self.cls == 1:
            return ops.Vfo(taps, 1, M, ops.phase_delta(1.0, self.freq), max_block=0)
        if self.cls == 2 and M == 1:
            return ops.Fir(taps, complex_data=False, max_block=0)
        return ops.Resampler(taps, 1, M, complex_data=self.cls != 2, max_block=0)

    def _oracle(self, taps):
        if self.cls == 2 and self.M == 1:
            return O.Fir(taps, complex_data=False, acc=O.ACC_F64)
        return O.Resampler(taps, 1, self.M, complex_data=self.cls != 2, acc=O.ACC_F64)

    # -- the events between two calls --------------------------------------------------------------------------------------------
    def new_taps(self):
        """Other tap values, same length: configure / set_taps on the device, a new oracle that inherits the history."""
        self.which ^= 1
        taps = self.tap_sets[self.which]
        if self.cls == 2 and self.M == 1:
            self.op.set_taps(taps)
        else:
            self.op.configure(taps, 1, self.M)
        hist = self.orc.hist
        self.orc = self._oracle(taps)
        self.orc.hist[:] = hist

    def retune(self):
        self.freq = F_B if self.freq == F_A else F_A
        self.op.set_phase_inc(*self.ops.phase_delta(1.0, self.freq))
        O.lib().oracle_xlator_phase_delta(1.0, self.freq, O._fp(self.xl.delta))

    def phase_jump(self):
        ang = 1.0 + 0.37 * self.index
        re, im = np.float32(math.cos(ang)), np.float32(math.sin(ang))
        self.op.set_phase(float(re), float(im))
        self.xl.turns.value = math.atan2(float(im), float(re)) / (2 * math.pi)

    # -- one call --------------------------------------------------------------------------------------------------------------
    def block(self, n):
        x = O.synth_iq(self.pos, n, seed=self.seed) if n else np.zeros(0, np.complex64)
        return np.ascontiguousarray(x.real) if self.cls == 2 else x

    def call(self, n, ctx):
        """Process the next n samples on both sides and check everything the hand-over can spoil.  Returns the kernel family."""
        x = self.block(n)
        got = self.op.process(_dev(x)).cpu().numpy()
        name = kname(self.op)
        ctx = f"{self.label} call {self.index} ({ctx}, {n} samples at {self.pos}) -> {name}"
        mixed = (self.xl.process(x) if self.xl is not None else x) if n else x
        want = self.orc.process(mixed) if n else np.zeros(0, self.dtype)
        self.pos += n
        self.index += 1
        assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, want.shape)
        w = _WORST.setdefault((self.label, name), [0.0, 0.0, 0.0])
        if len(want):
            top = float(np.abs(want).max())
            k = min(len(want), -(-self.H // self.M) + 1)
            head = float(np.abs(got[:k] - want[:k]).max()) / top
            rms = rel_rms(got, want)
            w[0], w[2] = max(w[0], head), max(w[2], rms)
            assert head <= TOL_HEAD, f"{ctx}: head of the call (first {k} of {len(want)} outputs) off by {head:.3e} x max|want|"
            assert rms <= TOL_RMS, f"{ctx}: relative RMS {rms:.3e} over {len(want)} outputs"
        self.tail = np.concatenate([self.tail, mixed.astype(self.dtype)])[len(mixed):] if self.H else self.tail
        hist = self.op.get_history()
        if self.cls == 1:
            d = float(np.abs(hist - self.tail).max()) if self.H else 0.0
            w[1] = max(w[1], d)
            assert d <= TOL_HIST, f"{ctx}: rotated history off the exact-phase mixer by {d:.3e}"
            ph = self.op.get_phase()
            dp = abs(ph - np.exp(2j * np.pi * self.xl.turns.value))
            assert dp < TOL_PHASE, f"{ctx}: NCO phase off by {dp:.3e}"
        else:
            assert np.array_equal(hist, self.tail), f"{ctx}: history is not the last {self.H} input samples"
        return name

    def twin(self):
        """A fresh handle with this one's plan and stream state: same taps, history and -- through advance(), exact in the 64-bit phase --
        NCO phase.  Only valid while the NCO has not been retuned or jumped (the callers see to that)."""
        t = self.make(self.tap_sets[self.which])
        t.set_history(self.op.get_history())
        return t


# ------------------------------------------------------------------------------------------------------------ 1. the transition matrix
def pair_walk(families):
    """A closed walk over `families` in which every ordered pair (A, B), A = B included, is consecutive exactly once: an Euler circuit of
    the complete digraph with loops (Hierholzer)."""
    n = len(families)
    unused = {a: list(range(n)) for a in range(n)}
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop())
        else:
            circuit.append(stack.pop())
    return [families[i] for i in reversed(circuit)]


def _sizes(count, M, seed):
    """Ragged call sizes of 4 500 .. 40 000 samples (mostly small: the oracle and the walk stay quick): no multiple of the decimation, of 4096
    or of the 481 outputs a polyphase segment yields."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(4500, 9000)) if i % 6 else int(rng.integers(20_000, 40_000))
        while n % M == 0 or n % 4096 == 0 or (n // M) % 481 == 0 or n % 2 == 0:
            n += 1
        out.append(n)
    return out


def _plans():
    cx = {8: [WIN, CORE, ANY, F1K, F4K, "pfb_dec8_kernel"], 4: [WIN, CORE, ANY, F1K, F4K, "pfb_dec4_kernel"], 3: [WIN, CORE, ANY, F1K, F4K],
          16: [WIN, ANY, F1K, F4K, "decim_mfma_kernel"]}
    taps = {8: 128, 4: 160, 3: 96, 16: 128}
    plans = []
    for cls, what in ((0, "decim"), (1, "vfo")):
        for M in (8, 4, 3, 16):
            plans.append((f"{what}_{M}_{taps[M]}", cls, M, taps[M], cx[M]))
    plans.append(("real_8_128", 2, 8, 128, [WIN, CORE, ANY, F4K, "pfb_dec8_real_kernel"]))
    plans.append(("real_16_128", 2, 16, 128, [WIN, ANY, F4K, "decim_mfma_real_kernel"]))
    return plans


@pytest.mark.parametrize("plan", _plans(), ids=lambda p: p[0])
def test_every_family_takes_over_from_every_other(ops, plan):
    """The transition matrix of one plan on one handle (module docstring, part 1).

    Families left out because the code shows the plan cannot reach them at any call size:
      * fir_core_kernel at decimation 16: use_core() serves decimations up to 8;
      * fir_fft1k_kernel on real data with 128 taps at decimation 8 / 16: the one-wave form only runs in AUTO mode (fft1k_eligible: mode 0),
        where fft_eligible() asks real data for 32 taps per unit of decimation (256 / 512 here; 384 / 257 from 2^22 samples), a floor that
        QDSP_HIP_FFT_MIN_TAPS_REAL can raise but not lower; the table's mode-2 settings force the 4096-point form.  The overlap-save forms
        that serve these plans are the 4096-point kernel and, at decimation 8, pfb_dec8_real_kernel;
      * the polyphase kernels at decimation 3 / 16 (pfb_eligible: decimation 8 or 4) and the MFMA decimator below decimation 9 (mf_plan).
    resamp_any_kernel at decimation <= 8 is reached through QDSP_HIP_FORCE_ANY on a handle whose taps were uploaded branch-major for
    fir_core_kernel: the launch gives it the phase table it reads (Engine::taps_core / plain_taps)."""
    label, cls, M, ntaps, families = plan
    assert not [k for k in os.environ if k.startswith("QDSP_HIP_") and k not in ("QDSP_HIP_LIB", "QDSP_HIP_NO_AUTOBUILD", "QDSP_HIP_DEVICE")]
    st = _Stream(ops, cls, M, ntaps, seed=1000 * cls + 10 * M + 1, label=label)
    H = st.H
    assert H == ntaps

    walk = pair_walk(families)
    pairs = set(zip(walk, walk[1:]))
    assert pairs == {(a, b) for a in families for b in families} and len(walk) == len(families) ** 2 + 1, "the walk misses a pair"
    events = [("short", lambda: st.call(H - 29, "a call shorter than the history")),
              ("empty", lambda: st.call(0, "an empty call")),
              ("taps", st.new_taps)]
    if cls == 1:
        events += [("retune", st.retune), ("jump", st.phase_jump)]
    # pairs first (nothing in between), then around every event f0 E f1 E ... f(n-1) E f0: each family once before and once after it
    steps = [(f, None) for f in walk]
    for ev in events:
        steps.append((families[0], None))
        steps += [(f, ev) for f in families[1:] + families[:1]]
    sizes = _sizes(len(steps), M, seed=M * 7 + cls)
    assert all(4500 <= n <= 40_050 for n in sizes)

    seen, around, took = [], {name: {"before": set(), "after": set()} for name, _ in events}, {"short": set(), "empty": set()}
    prev = None
    for (fam, ev), n in zip(steps, sizes):
        between = None
        if ev is not None:
            between, act = ev
            r = act()
            if between in took:
                took[between].add(r)
            around[between]["before"].add(prev)
        mode, env = _steer(fam)
        with _switches(st.op, mode, env):
            name = st.call(n, f"{prev} -> {fam}, in between: {between}")
        assert name == fam, f"{label} call {st.index - 1}: asked for {fam}, ran {st.op.last_kernel()} ({n} samples)"
        if between:
            around[between]["after"].add(fam)
        seen.append(fam)
        prev = fam
    assert seen[:len(walk)] == walk
    for name, _ in events:
        assert around[name]["before"] == set(families) == around[name]["after"], (label, name, around[name])

    # the handle's past must not show in its dispatch: one more call under the defaults against a fresh handle's.  (The VFO's twin is
    # created on the increment the walk ended on; its phase has not jumped: it is there for the kernel and its geometry, not for the bits.)
    twin = st.twin()
    x = _dev(st.block(20_011))
    twin.process(x)
    st.call(20_011, "the last call, defaults")
    assert st.op.last_kernel() == twin.last_kernel(), f"{label}: after the walk {st.op.last_kernel()}, a fresh handle {twin.last_kernel()}"
    print(f"\n{label}: {len(seen)} steered calls over {sorted(set(seen))}; short calls ran {sorted(took['short'])}, empty calls {sorted(took['empty'])}")
    for (lab, fam), (head, hist, rms) in sorted(_WORST.items()):
        if lab == label:
            print(f"  {lab:12s} {fam:24s} head {head:.2e} x max|want|   rms {rms:.2e}   history {hist:.2e}")


# ------------------------------------------------------------------------------------------------------------ 2. dispatch and the handle's past
def _pair_id(p):
    return f"class{p[0]}_dec{p[1]}_{p[2]}taps"


def test_table_still_has_the_cells_the_history_test_needs():
    """A regenerated table that loses every (veto cell, plain window cell) column fails here: the history test below would be vacuous."""
    found = {(c, M, t) for c, M, t, _, _ in history_pairs()}
    assert (0, 3, 64) in found, sorted(found)
    assert _veto_cells_dec16()          # (decimation 16, 64 taps: the MFMA-table test below; its plain cells start at 2^19 samples)
    assert (2, 2, 48) in found, sorted(found)


@pytest.mark.parametrize("pair", history_pairs(), ids=_pair_id)
def test_dispatch_does_not_depend_on_the_handles_past(ops, pair):
    """A call in a cell whose setting vetoes decim_win_kernel, new taps of the same length, a call in a setting-0 cell where that kernel is
    the rules' choice -- no QDSP_HIP_* variable set -- against a fresh handle that only makes the last call from the same history and NCO
    phase: same kernel, same launch geometry, same output bits.  Before the fix the vetoed call left Engine::auto_veto set, configure()
    planned under it and dropped d_taps_lm (decimation 16: built an MFMA table instead), and the handle never ran decim_win_kernel again."""
    cls, M, ntaps, lg_veto, lg_plain = pair
    assert not [k for k in os.environ if k.startswith("QDSP_HIP_") and k not in ("QDSP_HIP_LIB", "QDSP_HIP_NO_AUTOBUILD", "QDSP_HIP_DEVICE")]
    st = _Stream(ops, cls, M, ntaps, seed=77 + M, label=_pair_id(pair))
    n1, n2 = _in_cell(lg_veto, M), _in_cell(lg_plain, M, salt=101)
    assert decim_setting(cls, M, ntaps, n1) in (1, 3) and decim_setting(cls, M, ntaps, n2) == 0
    first = st.call(n1, "the vetoed cell")
    assert first != WIN, (pair, first)
    st.new_taps()
    fresh = st.twin()
    if cls == 1:
        fresh.advance(n1)
    x = _dev(st.block(n2))
    want = fresh.process(x).cpu().numpy()
    got = st.op.process(x).cpu().numpy()
    old, new = st.op.last_kernel(), fresh.last_kernel()
    assert new["name"] == WIN, f"{_pair_id(pair)}: the mirror expects decim_win_kernel in the plain cell, a fresh handle ran {new}"
    assert old == new, f"{_pair_id(pair)}: a handle that served a vetoed call and got new taps ran {old}, a fresh handle {new}"
    assert np.array_equal(got, want), _pair_id(pair)


def _veto_cells_dec16():
    """(class, row) of the cells up to 2^13 samples at decimation 16, 64 taps whose setting vetoes the window kernel, complex data."""
    mi, col, lmin = _T["M"].index(16), _T["taps"].index(64), _T["lmin"]
    return [(cls, r + lmin) for cls in (0, 1) for r in range(0, 13 - lmin + 1) if _T["tab"][cls, mi, r, col] in (1, 3)][:2]


def test_no_mfma_table_appears_after_a_vetoed_call_at_decimation_16(ops):
    """The same for d_taps_mf at decimation 16, 64 taps: mf_plan() leaves such short filters to the window kernel (`use_win(e) && P < 6 * M`),
    so a configure() that sees a stale window veto builds an MFMA table the rules would not have built, and every later call runs
    decim_mfma_kernel.  This column's first setting-0 cell sits at 2^19 / 2^20 samples, beyond the sizes this module runs, so the call after
    the new taps is made in a vetoed cell again (2^13 samples): the defect shows there just as well -- the fresh handle has no MFMA table."""
    cells = _veto_cells_dec16()
    assert cells, "no cell that vetoes the window kernel at decimation 16, 64 taps, up to 2^13 samples, in decim_table.inc"
    assert not [k for k in os.environ if k.startswith("QDSP_HIP_") and k not in ("QDSP_HIP_LIB", "QDSP_HIP_NO_AUTOBUILD", "QDSP_HIP_DEVICE")]
    for cls, lg in cells:
        st = _Stream(ops, cls, 16, 64, seed=5, label=f"mfma_table_class{cls}")
        n1, n2 = _in_cell(lg, 16), _in_cell(13, 16, salt=101)
        assert decim_setting(cls, 16, 64, n1) in (1, 3)
        st.call(n1, "the vetoed cell")
        st.new_taps()
        fresh = st.twin()
        if cls == 1:
            fresh.advance(n1)
        x = _dev(st.block(n2))
        want = fresh.process(x).cpu().numpy()
        got = st.op.process(x).cpu().numpy()
        old, new = st.op.last_kernel(), fresh.last_kernel()
        assert new["name"] != "decim_mfma_kernel", (cls, new)
        assert old == new, f"class {cls}: after a vetoed call and new taps the handle ran {old}, a fresh handle {new}"
        assert np.array_equal(got, want), cls


# ------------------------------------------------------------------------------------------------------------ 3. the exception cells, shipped defaults
@pytest.mark.parametrize("cell", table_triples(), ids=lambda c: f"class{c[0]}_dec{c[1]}_setting{c[2]}")
def test_exception_cells_under_the_shipped_defaults(ops, monkeypatch, cell):
    """Every (class, decimation, setting) of decim_table.inc against the oracle with the per-call checks of part 1: two calls in the first cell
    that holds the setting with a call shorter than the history between them, no switch set; a setting that only occurs above 2^16 samples
    is forced with QDSP_HIP_DECIM_SETTING on 2^16-sample calls of its cell's filter."""
    cls, M, setting, lg, ntaps = cell
    assert not [k for k in os.environ if k.startswith("QDSP_HIP_") and k not in ("QDSP_HIP_LIB", "QDSP_HIP_NO_AUTOBUILD", "QDSP_HIP_DEVICE")]
    assert decim_setting(cls, M, ntaps, 1 << lg) == setting
    st = _Stream(ops, cls, M, ntaps, seed=300 + 17 * M + setting, label=f"cell_{cls}_{M}_{setting}")
    if lg <= 16:
        n1, n2 = _in_cell(lg, M), _in_cell(lg, M, salt=101)
    else:
        n1, n2 = _in_cell(16, M), _in_cell(16, M, salt=101)
        monkeypatch.setenv("QDSP_HIP_DECIM_SETTING", str(setting))
    assert lg > 16 or (decim_setting(cls, M, ntaps, n1) == setting and decim_setting(cls, M, ntaps, n2) == setting)
    names = [st.call(n1, f"setting {setting}, first call"),
             st.call(max(1, st.H - 5), "a call shorter than the history"),
             st.call(n2, f"setting {setting}, second call")]
    print(f"\nclass {cls} decimation {M} setting {setting} ({ntaps} taps, row 2^{lg}): {names}")
