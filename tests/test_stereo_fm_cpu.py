"""StereoFMDemod (src/dsp/demodulator.h:189-330) without a GPU: the C ABI exports the entry points, capi binds them and the header
compiles as C; the C++ block mirror carries the reference's surface and build() makes the graph harness with its `sfm` mode -- and
the numpy helpers the GPU tests stand on are checked here: `stereo_mix_ref` (pinned bit for bit to a C++ restatement of run()'s VOLK
lines behind AGC::run) and the input recipe, whose every call of at least 64 samples lifts the AGC level by its own pilot maximum."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
from _numerics import fir_ref64
from qdsp_amd import capi
from test_demod_cpu import fm_ref, phasor_speed
from test_level_cpu import F32, _same_bits, agc_exact_decay, agc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
CSRC = os.path.join(ROOT, "qdsp_amd", "csrc")
TILE = 2048            # kDemodNT * kDemodSpl (qdsp_amd/csrc/demod.hip.h): outputs per workgroup of pilot_fir_kernel
MAX_TAPS = 4096        # kPilotMaxTaps (qdsp_amd/csrc/stereo_fm.hip.h)
RATES = {5: 48_000.0, 193: 48_000.0, 1001: 250_000.0}      # the sample rate each tap count is run at
TAPS = tuple(RATES)


def deviation_of(T):
    """A quarter of the sample rate: the composite signal (|mpx| < 1.3) moves the phase by less than 0.65 pi per sample."""
    return RATES[T] / 4.0
PEAK_MARGIN = 1.1      # every call of at least MIN_PEAK_CALL samples: pilot maximum >= PEAK_MARGIN x the decayed level
MIN_PEAK_CALL = 64


# ---- the restatement --------------------------------------------------------------------------------------------------------
def stereo_mix_ref(m, f, level, cfr):
    """One StereoFMDemod::run behind the demodulator and the filter: AGC::run on the filtered pilot f from `level`
    (p = f * (1.0f / level)), then d = p * p, s = m * d, out = {m + s, m - s}, every operation rounded to float.
    Returns (out [n, 2], level after the call)."""
    m, f = np.ascontiguousarray(m, F32), np.ascontiguousarray(f, F32)
    p, lvl = agc_ref(f, level, cfr)
    return stereo_matrix(m, f, lvl), lvl


def stereo_matrix(m, f, level):
    """The element-wise lines alone, at a given level of the call."""
    m, f = np.ascontiguousarray(m, F32), np.ascontiguousarray(f, F32)
    with np.errstate(all="ignore"):
        p = f * F32(F32(1.0) / F32(level))
        d = p * p
        s = m * d
        return np.stack([m + s, m - s], axis=1)


def cfr_of(sample_rate):
    """AGC::init's _CorrectedFallRate for StereoFMDemod's agc.init(&filter.out, 20.0f, sampleRate)."""
    return F32(F32(20.0) / F32(sample_rate))


# ---- the shapes and the input recipe of the GPU tests -------------------------------------------------------------------------
def pilot_taps(T):
    """193 and 1001: the reference's window design at 48 kHz (its own tap count there) and at 250 kHz (where its float tap-count
    formula gives 999; 1001 is the nominal 4 fs / 1000 + 1).  5: the shortest filter that still isolates the pilot of the recipe --
    zeros on the 1 kHz tone and on the 38 kHz carrier (10 kHz after aliasing at 48 kHz), unit gain at 19 kHz."""
    fs = RATES[T]
    if T == 5:
        z = np.exp(2j * np.pi * np.array([1_000.0, -1_000.0, 38_000.0, -38_000.0]) / fs)
        h = np.real(np.poly(z))
        g = abs(np.polyval(h[::-1], np.exp(-2j * np.pi * 19_000.0 / fs)))
        return (h / g).astype(F32)
    return O.blackman_bandpass_taps(1000.0, 19000.0, fs, T)


def call_sizes(T):
    """The call sizes of the GPU tests in the order they are run (mixed: long and short calls alternate, the 64-sample call
    first, where the level is still 0)."""
    sizes = [64, 2048 + T - 1, T - 1, 2049, T - 2, 3 * 2048 + 5, T, 2047, 2048]
    assert sorted(sizes) == sorted([64, T - 2, T - 1, T, 2047, 2048, 2049, 2048 + T - 1, 3 * 2048 + 5])
    return sizes


@functools.lru_cache(maxsize=None)
def recipe(T, seed=0, sizes=None):
    """(iq complex64, mpx float64, cuts) of one stream for tap count T: the composite signal
         0.4 sin(1 kHz) + g_k sin(19 kHz) + 0.2 sin(700 Hz) sin(38 kHz) + 0.01 noise,   g_k = 0.1 * 1.2^k in call k,
    frequency-modulated with deviation_of(T) at RATES[T] (`modulate`)."""
    fs = RATES[T]
    sizes = list(sizes) if sizes is not None else call_sizes(T)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    n = int(cuts[-1])
    t = np.arange(n, dtype=np.float64) / fs
    g = np.repeat(0.1 * 1.2 ** np.arange(len(sizes)), sizes)
    rng = np.random.default_rng(1000 * T + seed)
    mpx = (0.4 * np.sin(2 * np.pi * 1_000.0 * t) + g * np.sin(2 * np.pi * 19_000.0 * t)
           + 0.2 * np.sin(2 * np.pi * 700.0 * t) * np.sin(2 * np.pi * 38_000.0 * t) + 0.01 * rng.standard_normal(n))
    return modulate(mpx, deviation_of(T) / fs), mpx, [int(c) for c in cuts]


def modulate(mpx, dev_over_fs):
    """IQ samples whose phase UNDER THE REFERENCE'S fast_arctan2 is 2 pi dev / fs * cumsum(mpx): the sample of phase phi lies on the
    diamond |re| + |im| = 1, where fast_arctan2 (demodulator.h:14-30: pi/4 - pi/4 * (x - |y|) / (x + |y|) for x >= 0, and
    3 pi/4 - pi/4 * (x + |y|) / (|y| - x) for x < 0) is linear in the coordinates.  On the unit circle that approximation is off by up to
    0.07 rad, and the demodulated signal would carry the composite plus a distortion that hides a 0.1 pilot; with these samples m is the
    composite to float rounding, so the level of every call is the pilot's."""
    phi = 2 * np.pi * dev_over_fs * np.cumsum(np.asarray(mpx, np.float64))
    phi = (phi + np.pi) % (2 * np.pi) - np.pi
    a, c1 = np.abs(phi), np.pi / 4
    right = a <= np.pi / 2
    r = np.where(right, 1.0 - a / c1, (3 * c1 - a) / c1)
    x = np.where(right, (1.0 + r) / 2, (r - 1.0) / 2)
    y = np.where(right, (1.0 - r) / 2, (1.0 + r) / 2) * np.where(phi < 0, -1.0, 1.0)
    return (x + 1j * y).astype(np.complex64)


def pilot_ratios(T, seed=0, sizes=None):
    """Per call: (count, FP64 pilot maximum / decayed level) along the FP64 level recursion; inf for the first call."""
    iq, _, cuts = recipe(T, seed, tuple(sizes) if sizes is not None else None)
    m, _ = fm_ref(iq, phasor_speed(RATES[T], deviation_of(T)))
    f = fir_ref64(pilot_taps(T), m)
    cfr, level, out = cfr_of(RATES[T]), 0.0, []
    for a, b in zip(cuts, cuts[1:]):
        dec = float(agc_exact_decay(F32(level), cfr, b - a)[0]) if level > 0 else 0.0
        peak = float(f[a:b].max())
        out.append((b - a, peak / dec if dec > 0 else np.inf))
        level = max(dec, peak)
    return out


@pytest.mark.parametrize("T", TAPS)
def test_every_long_enough_call_of_the_recipe_is_in_the_peak_regime(T):
    assert len(pilot_taps(T)) == T
    for seed in (0, 1, 2):                                   # (the GPU tests run three channels: seeds 0 to 2)
        rs = pilot_ratios(T, seed)
        print(f"T={T} seed {seed}: " + ", ".join(f"{n}: {r:.3f}" for n, r in rs))
        assert [n for n, _ in rs] == call_sizes(T)
        assert all(r >= PEAK_MARGIN for n, r in rs if n >= MIN_PEAK_CALL), rs
    # the shapes the issue names: calls around a tile and around the filter length, at the reference's two rates
    if T != 5:
        for sizes in ((2048, 2047, 2049, 2048, 2050), (T, T + 1, T - 1, T, T + 3) if T >= 256 else (2 * T, 2 * T + 1, 2 * T - 1)):
            rs = pilot_ratios(T, 0, sizes)
            assert all(r >= PEAK_MARGIN for _, r in rs), (sizes, rs)


@pytest.mark.parametrize("T", TAPS)
def test_the_demodulated_recipe_is_the_composite_signal(T):
    iq, mpx, _ = recipe(T)
    m, _ = fm_ref(iq, phasor_speed(RATES[T], deviation_of(T)))
    err = np.abs(m[1:].astype(np.float64) - mpx[1:])
    print(f"T={T}: max |m - mpx| = {err.max():.2e}")
    assert err.max() < 1e-5 and np.abs(mpx).max() < 1.3


def test_calls_shorter_than_a_pilot_period_may_fall_short():
    """... which is why counts 1 and 7 belong to the decay-regime test only: a call that holds no pilot crest decays."""
    rs = pilot_ratios(193, 0, (4096, 1, 1, 1))
    assert min(r for _, r in rs[1:]) < 1.0


def test_constants_are_the_kernels():
    sf = open(os.path.join(CSRC, "stereo_fm.hip.h")).read()
    dm = open(os.path.join(CSRC, "demod.hip.h")).read()
    assert int(re.search(r"constexpr int kPilotMaxTaps = (\d+);", sf).group(1)) == MAX_TAPS
    nt = int(re.search(r"constexpr int kDemodNT = (\d+);", dm).group(1))
    spl = int(re.search(r"constexpr int kDemodSpl = (\d+);", dm).group(1))
    assert nt * spl == TILE
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^stereo_fm\.o:.*\n\t(.*)$", mk, re.M).group(1)
    assert "fast-math" not in rule and "-O3" not in rule.replace("$(CXXFLAGS)", ""), "the demodulators' flags"
    assert re.search(r"^libqdsp_hip\.so:.*\bstereo_fm\.o\b", mk, re.M)


# ---- the C ABI and the mirror -------------------------------------------------------------------------------------------------
SFM_SYMBOLS = ["qdsp_hip_stereo_fm_" + s for s in (
    "create", "set_fm", "set_pilot_taps", "process", "process_ex", "process_dev", "process_batch_dev", "get_phase", "set_phase",
    "get_level", "set_level", "pilot_dev", "reset", "destroy")]


def test_stereo_fm_symbols_declared_exported_and_bound(tmp_path):
    declared = set(capi.declared_symbols())
    assert set(SFM_SYMBOLS) <= declared, sorted(set(SFM_SYMBOLS) - declared)
    L = capi.load()
    assert all(hasattr(L, s) for s in SFM_SYMBOLS)
    assert all(getattr(L, s).argtypes is not None for s in SFM_SYMBOLS), "declared in capi.py"
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(SFM_SYMBOLS) <= exported
    assert L.qdsp_hip_abi_version() == 1
    from qdsp_amd import ops

    for name in ("process", "process_batch", "process_ex", "set_fm", "get_phase", "set_phase", "level", "set_level", "pilot", "reset",
                 "last_kernel", "time_dev", "set_pilot_taps"):
        assert callable(getattr(ops.StereoFmDemod, name)), name
    # the header is a C header
    (tmp_path / "c.c").write_text('#include "qdsp_hip.h"\nint main(void) { return qdsp_hip_stereo_fm_reset(0) == 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / "c.c")])


def test_default_taps_are_the_references():
    from qdsp_amd import ops

    for fs, about in ((48_000.0, 193), (250_000.0, 1001), (1_000_000.0, 4001)):
        t = ops.stereo_pilot_taps(fs)
        T = O.blackman_tap_count(1000.0, 1000.0, fs)         # (int)(4.0f / (1000.0f / fs)) in float, made odd: 193, 999, 3999
        assert len(t) == T <= MAX_TAPS and T % 2 == 1 and 0 <= about - T <= 2 and t.dtype == np.float32
        assert _same_bits(t, O.blackman_bandpass_taps(1000.0, 19000.0, fs, T))


_SURFACE_SRC = r"""
#include <type_traits>
#include "dsp/stereo_demod.h"
using namespace dsp;
static_assert(std::is_same<decltype(StereoFMDemod::out), stream<stereo_t>>::value, "StereoFMDemod::out");
static_assert(std::is_base_of<generic_unnamed_block, StereoFMDemod>::value, "a block");
float use(stream<complex_t>* iq) {
    StereoFMDemod a(iq, 250000.0f, 75000.0f);
    a.setSampleRate(240000.0f); a.setDeviation(50000.0f); a.setInput(iq);
    StereoFMDemod b;
    b.init(iq, 48000.0f, 5000.0f);
    b.start(); b.stop();
    generic_unnamed_block* blocks[] = {&a, &b};
    (void)blocks;
    return a.getSampleRate() + a.getDeviation();
}
"""


def test_stereo_block_compiles_with_the_reference_surface(tmp_path):
    (tmp_path / "s.cpp").write_text(_SURFACE_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.cpp")])
    src = open(os.path.join(HOST, "dsp", "stereo_demod.h")).read()
    for name in ("class StereoFMDemod", "BlackmanBandpassWindow", "win.init(1000, 1000, 19000, sampleRate)", "qdsp_hip_stereo_fm_process_ex",
                 "qdsp_hip_stereo_fm_set_pilot_taps"):
        assert name in src, name
    # nothing that is built against dsp/demodulator.h alone needs the new entry points
    assert "#include \"stereo_demod.h\"" not in open(os.path.join(HOST, "dsp", "demodulator.h")).read()
    assert "qdsp_hip_stereo_fm_" not in re.sub(r"//[^\n]*", "", open(os.path.join(HOST, "dsp", "demodulator.h")).read())
    # (the sanitizer tests' stand-in library has them, so that demod_check runs against it)
    assert "qdsp_hip_stereo_fm_process_ex" in open(os.path.join(ROOT, "tests", "fake_hip", "fake_qdsp_hip.cpp")).read()


def test_build_makes_the_stereo_harness():
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert re.search(r"^all:.*build/demod_check", mk, re.M)
    src = open(os.path.join(HOST, "examples", "demod_check.cpp")).read()
    assert '"sfm"' in src and "dsp/stereo_demod.h" in src
    subprocess.check_call(["make", "-C", HOST, "build/demod_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "demod_check")
    assert os.access(exe, os.X_OK)
    out = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    assert "qdsp_hip_stereo_fm_process_ex" in out and "qdsp_hip_stereo_fm_create" in out


# ---- stereo_mix_ref against a C++ restatement of the reference lines ----------------------------------------------------------
_CHECK_SRC = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
// argv: m.bin f.bin out.bin sampleRate cut...
// m: the demodulated signal (decodeInput), f: the filtered pilot (filter.out); processed in calls that end at the cuts.
// out.bin: the interleaved stereo samples, then the AGC level after every call.
static std::vector<float> load(const char* path) {
    std::vector<float> x;
    FILE* fp = fopen(path, "rb");
    float v;
    while (fread(&v, sizeof(v), 1, fp) == 1) x.push_back(v);
    fclose(fp);
    return x;
}
int main(int argc, char** argv) {
    const std::vector<float> m = load(argv[1]), f = load(argv[2]);
    const size_t total = m.size();
    const float sampleRate = (float)atof(argv[4]);
    const float fallRate = 20.0f;
    const float correctedFallRate = fallRate / sampleRate;
    std::vector<float> agcOut(total), doubled(total), diff(total), left(total), right(total), inter(2 * total), levels;
    float level = 0.0f;
    size_t pos = 0;
    for (int k = 5; k <= argc; k++) {
        const size_t end = k < argc ? (size_t)atol(argv[k]) : total;
        if (end <= pos) continue;
        const int count = (int)(end - pos);
        // AGC::run on the filter's output
        level = pow(10, ((10.0f * log10f(level)) - (correctedFallRate * count)) / 10.0f);
        for (int i = 0; i < count; i++) {
            if (f[pos + i] > level) { level = f[pos + i]; }
        }
        const float gain = 1.0f / level;
        for (int i = 0; i < count; i++) agcOut[pos + i] = f[pos + i] * gain;
        // StereoFMDemod::run: multiply, multiply, add, subtract, interleave
        for (int i = 0; i < count; i++) doubled[pos + i] = agcOut[pos + i] * agcOut[pos + i];
        for (int i = 0; i < count; i++) diff[pos + i] = m[pos + i] * doubled[pos + i];
        for (int i = 0; i < count; i++) left[pos + i] = m[pos + i] + diff[pos + i];
        for (int i = 0; i < count; i++) right[pos + i] = m[pos + i] - diff[pos + i];
        for (int i = 0; i < count; i++) { inter[2 * (pos + i)] = left[pos + i]; inter[2 * (pos + i) + 1] = right[pos + i]; }
        levels.push_back(level);
        pos = end;
    }
    FILE* o = fopen(argv[3], "wb");
    fwrite(inter.data(), 4, inter.size(), o);
    fwrite(levels.data(), 4, levels.size(), o);
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def cpp_mix(tmp_path_factory):
    d = tmp_path_factory.mktemp("sfmref")
    (d / "c.cpp").write_text(_CHECK_SRC)
    exe = d / "c"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", str(d / "c.cpp"), "-o", str(exe)])

    def run(m, f, sample_rate, cuts=()):
        np.ascontiguousarray(m, F32).tofile(d / "m.bin")
        np.ascontiguousarray(f, F32).tofile(d / "f.bin")
        subprocess.check_call([str(exe), str(d / "m.bin"), str(d / "f.bin"), str(d / "y.bin"), repr(float(sample_rate))] + [str(c) for c in cuts])
        y = np.fromfile(d / "y.bin", dtype=F32)
        return y[:2 * len(m)].reshape(-1, 2), y[2 * len(m):]

    return run


@pytest.mark.parametrize("which", ["recipe", "edges"])
def test_stereo_mix_ref_is_bit_identical_to_the_cpp_restatement(cpp_mix, which):
    if which == "recipe":
        T = 193
        iq, _, cuts = recipe(T)
        m, _ = fm_ref(iq, phasor_speed(RATES[T], deviation_of(T)))
        f = fir_ref64(pilot_taps(T), m).astype(F32)
        cuts = cuts[1:-1] + [cuts[-1] - 7, cuts[-1] - 6]            # two short calls at the end: the decayed level stands
        fs = RATES[T]
    else:
        v = [0.0, -0.0, 1e-45, -1e-40, 1e30, -1e30, 3e38, 1e-30, 1.0, -1.0, 0.5, 2.0, np.nan, 1.0, -2.0, np.inf, 3.0, -np.inf]
        f = np.asarray(v * 3, F32)
        m = np.asarray((v[5:] + v[:5]) * 3, F32)
        cuts = [2, 6, 14, 16, 19, 23, 30]                           # the first call: zeros only (f * inf); later ones reach NaN and Inf
        fs = 100.0
    want, levels = cpp_mix(m, f, fs, cuts)
    cfr, lvl, got, a = cfr_of(fs), F32(0), [], 0
    for k, b in enumerate(list(cuts) + [len(m)]):
        y, lvl = stereo_mix_ref(m[a:b], f[a:b], lvl, cfr)
        assert _same_bits([lvl], [levels[k]]), (k, lvl, levels[k])
        assert _same_bits(y, stereo_matrix(m[a:b], f[a:b], lvl))
        got.append(y)
        a = b
    assert _same_bits(np.concatenate(got), want)
    if which == "edges":
        assert np.isinf(lvl) and np.all(np.isnan(got[0])), "0 * inf in the first call, and an Inf that pins the level"
