"""Squelch and AGC (src/dsp/processing.h:424-489, :83-145) without a GPU: the C ABI exports the entry points and capi binds them, the
C++ block mirror carries the reference's surface, build() makes the graph harness -- and the numpy helpers the GPU tests stand on
are checked here: `squelch_ref` and `agc_ref` (pinned bit for bit to a C++ restatement of the reference lines), the bound
`agc_decay_bound` on the decayed level, and the case table of the squelch test, whose every level keeps its distance from the mean."""
import ctypes as C
import ctypes.util
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from qdsp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
CSRC = os.path.join(ROOT, "qdsp_amd", "csrc")
LD = np.longdouble
F32 = np.float32
TILE = 2048            # kDemodNT * kDemodSpl (qdsp_amd/csrc/demod.hip.h)
ROW_TILES = 4          # kLevelRowTiles: rows of at most this many tiles take one launch (qdsp_amd/csrc/level.hip.h)
SIZES = (1, 7, TILE - 1, TILE, TILE + 1, ROW_TILES * TILE, ROW_TILES * TILE + 1, 3 * ROW_TILES * TILE + 5, 1024 * TILE + TILE + 3)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.log10f.restype = C.c_float
_libm.log10f.argtypes = [C.c_float]


def log10f(v):
    """The C library's float log10 (what the C++ restatement below calls), per element."""
    a = np.asarray(v, F32)
    out = np.fromiter((_libm.log10f(float(t)) for t in a.reshape(-1)), dtype=F32, count=a.size)
    return out.reshape(a.shape) if a.ndim else F32(out[0])


def _same_bits(a, b):
    """Equal as float32 bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


# ---- the two restatements ---------------------------------------------------------------------------------------------------
def squelch_mean_db(x):
    """10.0f * log10f(mean |x|) of one call: |x| = sqrtf(re*re + im*im) with every operation rounded to float, the sum in
    float64 (sequential), divided by the count and rounded once to float."""
    x = np.ascontiguousarray(x, np.complex64)
    with np.errstate(all="ignore"):
        re, im = x.real, x.imag
        mag = np.sqrt(re * re + im * im)
        total = np.add.accumulate(mag.astype(np.float64))[-1] if len(x) else np.float64(0)
        mean = F32(total / np.float64(len(x)))
        return F32(F32(10.0) * log10f(mean))


def squelch_ref(x, level):
    """Squelch::run over one call: (output, open)."""
    x = np.ascontiguousarray(x, np.complex64)
    is_open = bool(squelch_mean_db(x) >= F32(level))
    return (x.copy() if is_open else np.zeros_like(x)), is_open


def agc_decay(level, cfr, count):
    """The first line of AGC::run: float32 throughout, pow(10, float) in float64, rounded to float32."""
    with np.errstate(all="ignore"):
        e = F32(F32(F32(10.0) * log10f(level) - F32(F32(cfr) * F32(count))) / F32(10.0))
        return F32(np.power(10.0, np.float64(e)))


def agc_ref(x, level, cfr):
    """AGC::run over one call from `level`: (output, level after it)."""
    x = np.ascontiguousarray(x, F32)
    lvl = agc_decay(level, cfr, len(x))
    with np.errstate(all="ignore"):
        peak = x[~np.isnan(x)]
        if peak.size and peak.max() > lvl:          # `if (x[i] > level) level = x[i]`: a NaN never wins, a NaN level stays
            lvl = F32(peak.max())
        return x * F32(F32(1.0) / lvl), lvl


# ---- the bound on the decayed level -----------------------------------------------------------------------------------------
def ulp32(t):
    return np.spacing(np.abs(np.asarray(t, LD)).astype(F32)).astype(LD)


def agc_exact_decay(level, cfr, count):
    """L * 10^(-f / 10) in np.longdouble, f = cfr * count exactly: (value, f)."""
    f = np.asarray(cfr, F32).astype(LD) * np.asarray(count, LD)
    return np.asarray(level, F32).astype(LD) * LD(10.0) ** (-f / LD(10.0)), f


def agc_decay_bound(L, f, k=6):
    """Relative to the exact L * 10^(-f / 10):  (ln 10 / 10) * k * ulp32(m) + 2^-24,  m = max(|10 log10 L|, f, |10 log10 L - f|).
    The expression has four float roundings in dB units (10.0f * log10f(L) counts two, the product cfr * count and the difference
    one each; the division by 10.0f rounds at a tenth of that scale), two more ulp are what a device log10f may add to a correctly
    rounded one (k = 6), and an error of d dB moves the level by ln(10) / 10 * d relative.  2^-24: the final rounding to float."""
    db = LD(10.0) * np.log10(np.asarray(L, F32).astype(LD))
    m = np.maximum(np.maximum(np.abs(db), np.asarray(f, LD)), np.abs(db - f))
    return np.log(LD(10.0)) / LD(10.0) * LD(k) * ulp32(m) + LD(2.0) ** -24


def decay_error_ratio(got, L, cfr, count, k=6):
    """|got - exact| over the bound.  A result below FLT_MIN carries the absolute rounding of the subnormal grid, half its spacing
    2^-149, which no relative bound covers: that is added for those."""
    truth, f = agc_exact_decay(L, cfr, count)
    bound = agc_decay_bound(L, f, k) * truth + np.where(truth < LD(np.finfo(F32).tiny), LD(2.0) ** -150, LD(0))
    return np.abs(np.asarray(got, F32).astype(LD) - truth) / bound


def test_agc_ref_decay_meets_the_bound():
    rng = np.random.default_rng(3)
    n = 100_000
    L = (10.0 ** rng.uniform(-6, 6, n)).astype(F32)
    cfr = (10.0 ** rng.uniform(-7, -2, n)).astype(F32)
    count = np.floor(10.0 ** rng.uniform(0, 6, n)).astype(np.int64)
    with np.errstate(all="ignore"):
        e = ((F32(10.0) * log10f(L) - cfr * count.astype(F32)) / F32(10.0)).astype(F32)
        got = np.power(10.0, e.astype(np.float64)).astype(F32)
    assert _same_bits(got[:50], [agc_decay(L[i], cfr[i], count[i]) for i in range(50)])
    r6, r4 = decay_error_ratio(got, L, cfr, count), decay_error_ratio(got, L, cfr, count, k=4)
    print(f"worst |error| / bound over {n} cases: {float(r6.max()):.3f} (k = 6), {float(r4.max()):.3f} (k = 4)")
    assert r6.max() <= 1.0


# ---- the cases of the GPU squelch test --------------------------------------------------------------------------------------
SQUELCH_INPUTS = ("gauss_-40dB", "gauss_-6dB", "gauss_+30dB", "tone_in_noise")
MARGIN_DB = 1e-3       # the device's mean_db differs from squelch_mean_db by < 1e-4 dB: 2^-24 relative in the mean (4e-7 dB), 2 ulp of
#                        a log10f below 16 (2 * 2^-20 = 2e-6) times 10


def squelch_input(kind, n, seed=21):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
    if kind.startswith("gauss"):
        return (z * 10.0 ** (float(kind.split("_")[1][:-2]) / 20.0)).astype(np.complex64)
    t = np.arange(n)
    return (0.7 * np.exp(2j * np.pi * 0.0371 * t) + 0.05 * z).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def squelch_cases(n):
    """[(name, x, mean_db, level, open)]: every input with a level 0.01 dB below (open) and 0.01 dB above (closed) its own mean."""
    out = []
    for kind in SQUELCH_INPUTS:
        x = squelch_input(kind, n)
        db = squelch_mean_db(x)
        for d, is_open in ((-0.01, True), (0.01, False)):
            out.append((f"{kind} {d:+}", x, db, F32(float(db) + d), is_open))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_every_squelch_case_keeps_its_distance(n):
    cases = squelch_cases(n)
    assert len(cases) == 2 * len(SQUELCH_INPUTS)
    for name, x, db, level, is_open in cases:
        assert np.isfinite(db) and abs(float(db) - float(level)) >= MARGIN_DB, (n, name, db, level)
        assert squelch_ref(x, level)[1] == is_open, (n, name)
        assert abs(float(db)) < 160, "log10f below 16"


def test_constants_are_the_kernels():
    lv = open(os.path.join(CSRC, "level.hip.h")).read()
    dm = open(os.path.join(CSRC, "demod.hip.h")).read()
    assert int(re.search(r"constexpr int kLevelRowTiles = (\d+);", lv).group(1)) == ROW_TILES
    nt = int(re.search(r"constexpr int kDemodNT = (\d+);", dm).group(1))
    spl = int(re.search(r"constexpr int kDemodSpl = (\d+);", dm).group(1))
    assert nt * spl == TILE


# ---- the C ABI and the mirror -------------------------------------------------------------------------------------------------
COMMON = ("create", "process", "process_ex", "process_dev", "process_batch_dev", "reset", "destroy")
LEVEL_SYMBOLS = (["qdsp_hip_squelch_" + s for s in COMMON + ("set_level", "get_open")] +
                 ["qdsp_hip_agc_" + s for s in COMMON + ("set", "get_level", "set_level")])


def test_level_symbols_declared_exported_and_bound():
    declared = set(capi.declared_symbols())
    assert set(LEVEL_SYMBOLS) <= declared, sorted(set(LEVEL_SYMBOLS) - declared)
    L = capi.load()
    assert all(hasattr(L, s) for s in LEVEL_SYMBOLS)
    assert all(getattr(L, s).argtypes is not None for s in LEVEL_SYMBOLS), "declared in capi.py"
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(LEVEL_SYMBOLS) <= exported
    assert L.qdsp_hip_abi_version() == 1
    from qdsp_amd import ops

    for name in ("process", "process_batch", "set_level", "is_open", "reset", "time_dev", "last_kernel"):
        assert callable(getattr(ops.Squelch, name)), name
    for name in ("process", "process_batch", "set", "level", "set_level", "reset", "time_dev", "last_kernel"):
        assert callable(getattr(ops.Agc, name)), name


_SURFACE_SRC = r"""
#include <type_traits>
#include "dsp/processing.h"
#include "dsp/demodulator.h"
using namespace dsp;
static_assert(std::is_same<decltype(Squelch::out), stream<complex_t>>::value, "Squelch::out");
static_assert(std::is_same<decltype(AGC::out), stream<float>>::value, "AGC::out");
static_assert(std::is_base_of<detail::hip_block<complex_t, complex_t>, Squelch>::value, "the shared base of the HIP-backed blocks");
static_assert(std::is_base_of<detail::hip_block<float, float>, AGC>::value, "the shared base of the HIP-backed blocks");
float use(stream<complex_t>* iq, stream<float>* in) {
    Squelch a(iq, -30.0f);
    a.setLevel(-42.5f); a.setInput(iq);
    Squelch b;
    b.init(iq, -50.0f);
    AGC c(in, 20.0f, 48000.0f);
    c.setSampleRate(44100.0f); c.setFallRate(10.0f); c.setInput(in);
    AGC d;
    d.init(in, 20.0f, 24000.0f);
    AMDemod am(&a.out);
    AGC e(&am.out, 20.0f, 24000.0f);
    generic_unnamed_block* blocks[] = {&a, &b, &c, &d, &e};
    (void)blocks;
    return a.getLevel();
}
"""


def test_squelch_and_agc_blocks_compile_with_the_reference_surface(tmp_path):
    (tmp_path / "s.cpp").write_text(_SURFACE_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.cpp")])
    src = open(os.path.join(HOST, "dsp", "processing.h")).read() + open(os.path.join(HOST, "dsp", "hip_block.h")).read()    # (the link protocol is the base's)
    for name in ("class Squelch", "class AGC", "claimConsumer", "done.arm", "qdsp_hip_squelch_process_ex", "qdsp_hip_agc_process_ex",
                 "linkIn()"):
        assert name in src, name


def test_build_makes_the_level_harness():
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert re.search(r"^all:.*build/demod_check", mk, re.M)
    src = open(os.path.join(HOST, "examples", "demod_check.cpp")).read()
    assert '"squelch"' in src and '"agc"' in src and "dsp/processing.h" in src
    subprocess.check_call(["make", "-C", HOST, "build/demod_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "demod_check")
    assert os.access(exe, os.X_OK)
    out = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    assert "qdsp_hip_squelch_process_ex" in out and "qdsp_hip_agc_process_ex" in out


# ---- the restatements against a C++ restatement of the reference lines ------------------------------------------------------
_CHECK_SRC = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
// argv: squelch in.bin out.bin level 0 cut...  |  agc in.bin out.bin fallRate sampleRate cut...
// the float samples of in.bin (squelch: re, im pairs; the cuts count complex samples) processed in calls that end at the cuts
int main(int argc, char** argv) {
    const bool sq = !strcmp(argv[1], "squelch");
    FILE* f = fopen(argv[2], "rb");
    std::vector<float> x;
    float v;
    while (fread(&v, sizeof(v), 1, f) == 1) x.push_back(v);
    fclose(f);
    const size_t nc = sq ? 2 : 1, total = x.size() / nc;
    const float _level = (float)atof(argv[4]);
    const float _fallRate = (float)atof(argv[4]), _sampleRate = (float)atof(argv[5]);
    const float _CorrectedFallRate = _fallRate / _sampleRate;
    std::vector<float> y(x.size()), calls;
    float level = 0.0f;
    size_t pos = 0;
    for (int k = 6; k <= argc; k++) {
        const size_t end = k < argc ? (size_t)atol(argv[k]) : total;
        if (end <= pos) continue;
        const int count = (int)(end - pos);
        const float* in = x.data() + pos * nc;
        float* out = y.data() + pos * nc;
        if (sq) {
            double acc = 0.0;   // (the reference: volk_32f_accumulator_s32f, a float sum in the order of the host's SIMD width)
            for (int i = 0; i < count; i++) acc += (double)sqrtf(in[2 * i] * in[2 * i] + in[2 * i + 1] * in[2 * i + 1]);
            float sum = (float)(acc / (double)count);
            const float db = 10.0f * log10f(sum);
            if (db >= _level) { memcpy(out, in, count * 2 * sizeof(float)); }
            else { memset(out, 0, count * 2 * sizeof(float)); }
            calls.push_back(db);
            calls.push_back(db >= _level ? 1.0f : 0.0f);
        } else {
            level = pow(10, ((10.0f * log10f(level)) - (_CorrectedFallRate * count)) / 10.0f);
            for (int i = 0; i < count; i++) {
                if (in[i] > level) { level = in[i]; }
            }
            const float scalar = 1.0f / level;
            for (int i = 0; i < count; i++) out[i] = in[i] * scalar;   // volk_32f_s32f_multiply_32f
            calls.push_back(level);
        }
        pos = end;
    }
    FILE* o = fopen(argv[3], "wb");
    fwrite(y.data(), 4, y.size(), o);
    fwrite(calls.data(), 4, calls.size(), o);
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def cpp_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("levelref")
    (d / "c.cpp").write_text(_CHECK_SRC)
    exe = d / "c"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", str(d / "c.cpp"), "-o", str(exe)])

    def run(mode, x, p1, p2=0.0, cuts=()):
        x = np.ascontiguousarray(x)
        x.tofile(d / "x.bin")
        subprocess.check_call([str(exe), mode, str(d / "x.bin"), str(d / "y.bin"), repr(float(p1)), repr(float(p2))] + [str(c) for c in cuts])
        y = np.fromfile(d / "y.bin", dtype=F32)
        nf = x.size * (2 if mode == "squelch" else 1)
        return (y[:nf].view(np.complex64) if mode == "squelch" else y[:nf]), y[nf:]

    return run


def edge_vector():
    v = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1e30, -1e30, 3e38, 1e-30, -1e-30, 1.0, -1.0, 0.5, 2.0, 0.25, np.nan, 1.0, -2.0, np.inf, 3.0, -np.inf]
    return np.asarray(v * 3, F32)


def test_squelch_ref_is_bit_identical_to_the_cpp_restatement(cpp_check):
    n = 50_000
    x = np.concatenate([squelch_input("tone_in_noise", n), squelch_input("gauss_-40dB", n), squelch_input("gauss_-6dB", n // 2)])
    x[2 * n + 100] = np.nan + 0j                   # the last call holds a NaN: closed whatever the level
    cuts = (7, n, 2 * n, 2 * n + 1)
    for level in (-50.0, -20.0, 5.0):
        want, calls = cpp_check("squelch", x, level, cuts=cuts)
        got, a = [], 0
        for k, b in enumerate(cuts + (len(x),)):
            y, is_open = squelch_ref(x[a:b], level)
            assert _same_bits([squelch_mean_db(x[a:b])], [calls[2 * k]]) and is_open == bool(calls[2 * k + 1]), (level, k)
            got.append(y)
            a = b
        assert _same_bits(np.concatenate(got).view(F32), want.view(F32))
        assert calls[-1] == 0 and np.isnan(calls[-2])
    z = np.zeros(10, np.complex64)
    want, calls = cpp_check("squelch", z, -1e30)
    assert calls[0] == -np.inf and calls[1] == 0 and not squelch_ref(z, -1e30)[1]      # a mean of 0: closed at every finite level


@pytest.mark.parametrize("which", ["random", "edges"])
def test_agc_ref_is_bit_identical_to_the_cpp_restatement(cpp_check, which):
    if which == "random":
        rng = np.random.default_rng(9)
        x = (rng.standard_normal(200_000) * np.repeat([0.01, 3.0, 0.2, 0.001, 50.0], 40_000)).astype(F32)
        cuts = (1, 8, 4104, 40_000, 90_000, 130_000, 170_000)
        fall, rate = 300.0, 48_000.0
    else:
        x = edge_vector()
        cuts = (2, 6, 14, 16, 19, 23, 30)           # the first call: zeros only (x * inf); later ones reach the NaN and the Inf
        fall, rate = 1000.0, 100.0
    want, levels = cpp_check("agc", x, fall, rate, cuts=cuts)
    cfr = F32(F32(fall) / F32(rate))
    lvl, got, a = F32(0), [], 0
    for k, b in enumerate(cuts + (len(x),)):
        y, lvl = agc_ref(x[a:b], lvl, cfr)
        assert _same_bits([lvl], [levels[k]]), (k, lvl, levels[k])
        got.append(y)
        a = b
    assert _same_bits(np.concatenate(got), want)
    if which == "edges":
        assert np.all(np.isnan(got[0])) and np.isinf(lvl)
