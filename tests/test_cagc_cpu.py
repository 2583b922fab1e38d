"""ComplexAGC (src/dsp/processing.h:235-298) without a GPU: the C ABI exports the entry points, the C++ block mirror carries the
reference's surface, build() makes the graph harness -- and the numpy helpers the GPU tests stand on are checked here: `cagc_ref`
(the reference's float loop, pinned bit for bit to a C++ restatement), `cagc_exact` (the same float parameters and samples run
sequentially in np.longdouble: the truth), the bound `cagc_bound`, which a numpy emulation of the kernel's blocked FP64 scan has to
meet for every case of the GPU accuracy test, and the composition law of the clamped affine maps the scan rests on."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from qdsp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
LD = np.longdouble
F32 = np.float32
TILE = 2048            # kDemodNT * kDemodSpl (qdsp_amd/csrc/demod.hip.h)
ROW_TILES = 16         # kCagcRowTiles: rows of at most this many tiles take one launch
MAX_PARTS = 1024       # kAmMaxParts
BIG = np.finfo(np.float64).max      # the c of the identity map (cagc.hip.h)


# ---- the restatement, the truth and the bound -------------------------------------------------------------------------------
def _columns(x):
    x = np.asarray(x, np.complex64)
    ncol = int(np.prod(x.shape[1:], dtype=np.int64))
    return x.reshape(len(x), ncol), x.shape


def _per_column(v, dtype, ncol):
    return np.broadcast_to(np.asarray(v, dtype), (ncol,)).copy()


def cagc_ref(x, set_point, max_gain, rate, gain=1.0):
    """ComplexAGC::run over one call, float32 throughout, every product and sum rounded: (outputs complex64, carried gain float32).
    x: (n,) or (n, k), every column on its own; parameters and `gain` scalars or one value per column."""
    xc, shape = _columns(x)
    k = xc.shape[1]
    sp, mg, rt, g = (_per_column(v, F32, k) for v in (set_point, max_gain, rate, gain))
    re, im = np.ascontiguousarray(xc.real), np.ascontiguousarray(xc.imag)
    yr, yi = np.empty_like(re), np.empty_like(im)
    with np.errstate(all="ignore"):
        for i in range(len(xc)):
            a, b = re[i] * g, im[i] * g
            yr[i], yi[i] = a, b
            amp = np.sqrt(a * a + b * b)
            g = g + (sp - amp) * rt
            g = np.where(g > mg, mg, g)
    y = np.empty(xc.shape, np.complex64)
    y.real, y.imag = yr, yi
    return y.reshape(shape), (g if len(shape) > 1 else g[0])


def cagc_exact(x, set_point, max_gain, rate, gain=1.0):
    """The truth: the float parameters and samples, g' = min(g + (S - |x| |g|) r, max) run sequentially in np.longdouble with
    exact |x|, from `gain` (longdouble, or anything exactly convertible).  Returns (yr, yi, G, M, g): x.re g and x.im g per sample,
    G[i] the gain sample i was scaled by, M[i] = max(1, G[0..i]) with one more entry for the gain after the last sample, and that
    gain.  Shapes follow x; G, M have n + 1 rows."""
    xc, shape = _columns(x)
    n, k = xc.shape
    sp, mg, rt = (_per_column(F32(1) * np.asarray(v, F32), LD, k) for v in (set_point, max_gain, rate))
    g = _per_column(gain, LD, k)
    re, im = xc.real.astype(LD), xc.imag.astype(LD)
    with np.errstate(all="ignore"):
        mag = np.sqrt(re * re + im * im)
        G = np.empty((n + 1, k), LD)
        for i in range(n):
            G[i] = g
            g = np.minimum(g + (sp - mag[i] * np.abs(g)) * rt, mg)
        G[n] = g
        M = np.maximum.accumulate(np.maximum(G, 1), axis=0)
        yr, yi = re * G[:n], im * G[:n]
    tail = shape[1:]
    out = (yr.reshape((n,) + tail), yi.reshape((n,) + tail), G.reshape((n + 1,) + tail), M.reshape((n + 1,) + tail))
    return out + ((g.reshape(tail) if tail else g[0]),)


def ulp32(t):
    """The float32 spacing at |t|; where |t| rounds up to the next binade the larger spacing is taken."""
    return np.spacing(np.abs(np.asarray(t, LD)).astype(F32)).astype(LD)


def cagc_bound(truth, xcomp, M):
    """For one output component y = x g: 0.5 ulp32(x g_truth), the one final rounding, plus |x| 2^-40 M_i, the gain's bound
    |g - g_truth| <= 2^-40 M_i carried through the product.  2^-40 is 2^13 FP64 epsilons: a lane fold of 8, a scan tree of 6 + 2
    levels, the tiles of a chunk and up to 1023 chunk totals in turn, two roundings each (the clamp adds none), relative to the
    largest gain so far; the FP64 product in front of the final rounding adds 2^-53 of it."""
    return LD(0.5) * ulp32(truth) + np.abs(np.asarray(xcomp, LD)) * LD(2.0) ** -40 * np.asarray(M, LD)


def gain_bound(M):
    return LD(2.0) ** -40 * np.asarray(M, LD)


def _same_bits(a, b):
    """Equal as float32 bit patterns (complex64: both components), any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if np.iscomplexobj(a) or np.iscomplexobj(b):
        a = np.ascontiguousarray(a, np.complex64).view(F32)
        b = np.ascontiguousarray(b, np.complex64).view(F32)
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def in_domain(x, rate):
    """Every sample finite with a = 1 - r |x| >= 0, computed as the kernel computes it (FP64, the product exact to one rounding)."""
    x = np.asarray(x, np.complex64)
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    with np.errstate(all="ignore"):
        a = 1.0 - np.float64(F32(rate)) * np.sqrt(re * re + im * im)
    return bool(np.all(a >= 0))


def check_against_truth(y, x, exact, ref=None, label="", extra=0):
    """The bound for both components of every output; with `ref` (the float loop's outputs) also |y - ref| <= |ref - truth| + bound.
    `exact` = cagc_exact(x, ...); `extra`: what the truth's own starting gain may be off by, as a gain (it reaches an output
    through |x|).  Returns (worst error / bound, max |y - truth|, max |ref - truth|) and prints them."""
    yr, yi, G, M, _ = exact
    x = np.asarray(x, np.complex64)
    y = np.asarray(y, np.complex64)
    n = len(x)
    worst, e_y, e_ref = 0.0, 0.0, 0.0
    for comp, truth in (("real", yr), ("imag", yi)):
        got = getattr(y, comp).astype(LD)
        bound = cagc_bound(truth, getattr(x, comp), M[:n]) + np.abs(getattr(x, comp).astype(LD)) * extra
        err = np.abs(got - truth)
        ok = err <= bound
        if n:
            worst = max(worst, float(np.max(err / bound)))
            e_y = max(e_y, float(np.max(err)))
        assert np.all(ok), (label, comp, int(np.argmin(ok)), worst)
        if ref is not None:
            r = getattr(np.asarray(ref, np.complex64), comp).astype(LD)
            if n:
                e_ref = max(e_ref, float(np.max(np.abs(r - truth))))
            assert np.all(np.abs(got - r) <= np.abs(r - truth) + bound), (label, comp)
    print(f"{label}: worst error / bound {worst:.3f}, max |y - truth| {e_y:.3g}, max |float loop - truth| {e_ref:.3g}")
    return worst, e_y, e_ref


def check_gain(g, exact, label="", extra=0):
    """|g - truth| <= 2^-40 M after the last sample."""
    _, _, _, M, gt = exact
    err = np.abs(np.asarray(g, LD) - gt)
    assert np.all(err <= gain_bound(M[-1]) + extra), (label, float(np.max(err / gain_bound(M[-1]))))


# ---- the cases of the accuracy test -------------------------------------------------------------------------------------------
PARAMS = {"ref_defaults": (1.0, 65535.0, 1e-3), "tight_clamp": (0.5, 4.0, 0.02), "fast_x4": (1.0, 3.0, 0.125)}
SCALE = {"ref_defaults": 1.0, "tight_clamp": 1.0, "fast_x4": 4.0}
INPUTS = ("gauss", "tone", "step", "silence", "gauss30", "pattern")
SIZES = (1, 7, TILE, TILE + 1, ROW_TILES * TILE, ROW_TILES * TILE + 1, 40 * TILE + 1001)


def make_input(kind, n, seed=11):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    if kind in ("gauss", "gauss30"):        # complex Gaussian of unit variance x 0.7 (x 30)
        z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
        return (z * (0.7 if kind == "gauss" else 30.0)).astype(np.complex64)
    if kind == "tone":                      # amplitude 0.01: the gain climbs
        return (0.01 * np.exp(2j * np.pi * 0.01 * t)).astype(np.complex64)
    if kind == "step":                      # 60 dB up half way
        amp = np.where(t < n // 2, 1e-3, 1.0)
        return (amp * np.exp(2j * np.pi * 0.003 * t)).astype(np.complex64)
    if kind == "silence":                   # the gain ramps into the clamp
        return np.zeros(n, np.complex64)
    if kind == "pattern":                   # |x| = 2, 0.25, 0, 0, 0: under fast_x4 (x 4) a == 0 exactly on every fifth sample
        p = np.asarray([2.0, 0.25j, 0.0, 0.0, 0.0], np.complex64)
        return np.resize(p, n)
    raise ValueError(kind)


def limit_to_domain(x, rate):
    """Samples with rate |x| > 1 shrunk onto |x| = 0.999 / rate: only the fast_x4 Gaussian has any (about 3 in 10 000)."""
    x = np.asarray(x, np.complex64).copy()
    mag = np.abs(x.astype(np.complex128))
    over = mag * float(F32(rate)) > 1.0
    x[over] = (x[over].astype(np.complex128) * (0.999 / float(F32(rate)) / mag[over])).astype(np.complex64)
    return x


def case_list():
    """(parameter set, input) of every column of the accuracy test: gauss30 under the reference's defaults only."""
    return [(p, k) for p in PARAMS for k in INPUTS if k != "gauss30" or p == "ref_defaults"]


@functools.lru_cache(maxsize=None)
def case_table(n):
    """For one size: x (n, 16) complex64, one column per case_list() entry, the per-column parameters (3, 16) float32, the float
    loop's outputs and final gain, and the truth, all from gain 1.  The two sequential loops run once over all columns."""
    cols, par = [], []
    for p, k in case_list():
        sp, mg, rt = PARAMS[p]
        cols.append(limit_to_domain(make_input(k, n) * F32(SCALE[p]), rt))
        par.append((sp, mg, rt))
    x = np.stack(cols, axis=1)
    par = np.asarray(par, F32).T.copy()
    ref, gref = cagc_ref(x, par[0], par[1], par[2])
    exact = cagc_exact(x, par[0], par[1], par[2])
    return x, par, ref, gref, exact


def column(exact, k):
    yr, yi, G, M, g = exact
    return yr[:, k], yi[:, k], G[:, k], M[:, k], g[k]


def test_cases_are_in_the_domain_and_do_what_they_are_there_for():
    n = SIZES[-1]
    x, par, ref, gref, exact = case_table(n)
    G = exact[2]
    for k, (p, kind) in enumerate(case_list()):
        assert in_domain(x[:, k], par[2, k]), (p, kind)
        assert np.all(G[:, k] >= 0)
        if p == "tight_clamp" and kind in ("tone", "silence"):
            assert np.mean(G[1:, k] == LD(par[1, k])) > 0.99, (p, kind)
        if p == "fast_x4" and kind == "pattern":
            a = 1.0 - np.float64(par[2, k]) * np.abs(x[:, k].astype(np.complex128))
            assert abs(np.mean(a == 0.0) - 0.2) < 1e-3
        if kind == "tone" and p == "ref_defaults":
            assert G[-1, k] > 10 * G[0, k]


# ---- the C ABI and the mirror ---------------------------------------------------------------------------------------------------
CAGC_SYMBOLS = ["qdsp_hip_cagc_" + s for s in (
    "create", "set", "get_gain", "set_gain", "process", "process_ex", "process_dev", "process_batch_dev", "reset", "destroy")]


def test_cagc_symbols_declared_and_exported():
    declared = set(capi.declared_symbols())
    assert set(CAGC_SYMBOLS) <= declared, sorted(set(CAGC_SYMBOLS) - declared)
    L = capi.load()
    assert all(hasattr(L, s) for s in CAGC_SYMBOLS)
    assert all(getattr(L, s).argtypes is not None for s in CAGC_SYMBOLS), "declared in capi.py"
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(CAGC_SYMBOLS) <= exported
    assert L.qdsp_hip_abi_version() == 1


def test_ops_complex_agc_surface():
    from qdsp_amd import ops

    for name in ("process", "process_batch", "set", "get_gain", "set_gain", "reset", "time_dev", "last_kernel", "set_done_event",
                 "process_ex"):
        assert callable(getattr(ops.ComplexAgc, name)), name
    assert "ComplexAgc" in ops.__all__


_SURFACE_SRC = r"""
#include <type_traits>
#include "dsp/processing.h"
#include "dsp/vfo.h"
using namespace dsp;
static_assert(std::is_same<decltype(ComplexAGC::out), stream<complex_t>>::value, "ComplexAGC::out");
static_assert(std::is_base_of<detail::hip_block<complex_t, complex_t>, ComplexAGC>::value, "the shared base of the HIP-backed blocks");
void use(stream<complex_t>* in) {
    ComplexAGC a(in, 1.0f, 65535, 0.001f);
    a.setSetPoint(0.5f); a.setMaxGain(10.0f); a.setRate(0.01f); a.setInput(in);
    ComplexAGC agc;
    float _agcRate = 0.02f;
    agc.init(in, 1.0f, 65535, _agcRate);        // demodulator.h:585
    stream<complex_t>* next = &agc.out;
    generic_unnamed_block* blocks[] = {&a, &agc};
    (void)blocks; (void)next;
}
"""


def test_complex_agc_block_compiles_with_the_reference_usage(tmp_path):
    (tmp_path / "s.cpp").write_text(_SURFACE_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.cpp")])
    src = open(os.path.join(HOST, "dsp", "processing.h")).read() + open(os.path.join(HOST, "dsp", "hip_block.h")).read()    # (the link protocol is the base's)
    for name in ("claimConsumer", "done.arm", "qdsp_hip_cagc_process_ex", "qdsp_hip_cagc_set"):
        assert name in src, name


def test_build_makes_the_cagc_harness():
    assert re.search(r'mode == "cagc"', open(os.path.join(HOST, "examples", "demod_check.cpp")).read())
    subprocess.check_call(["make", "-C", HOST, "build/demod_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "demod_check")
    assert os.access(exe, os.X_OK)
    out = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    assert "qdsp_hip_cagc_process_ex" in out


# ---- the restatement against a C++ restatement ----------------------------------------------------------------------------------
_CHECK_SRC = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
struct complex_t {
    complex_t operator*(const float b) { return complex_t{re * b, im * b}; }
    inline float amplitude() { return std::sqrt((re * re) + (im * im)); }
    float re;
    float im;
};
// argv: in.bin out.bin setPoint maxGain rate gain cut...: the samples of in.bin run in calls that end at the cuts
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    std::vector<complex_t> x;
    complex_t v;
    while (fread(&v, sizeof(v), 1, f) == 1) x.push_back(v);
    fclose(f);
    const float _setPoint = (float)atof(argv[3]), _maxGain = (float)atof(argv[4]), _rate = (float)atof(argv[5]);
    float _gain = (float)atof(argv[6]);
    std::vector<complex_t> y(x.size());
    size_t pos = 0;
    for (int k = 7; k <= argc; k++) {
        const size_t end = k < argc ? (size_t)atol(argv[k]) : x.size();
        if (end <= pos) continue;
        const complex_t* readBuf = x.data() + pos;
        complex_t* writeBuf = y.data() + pos;
        const int count = (int)(end - pos);
        complex_t val;
        for (int i = 0; i < count; i++) {
            val = complex_t(readBuf[i]) * _gain;
            writeBuf[i] = val;
            _gain += (_setPoint - val.amplitude()) * _rate;
            if (_gain > _maxGain) { _gain = _maxGain; }
        }
        pos = end;
    }
    FILE* o = fopen(argv[2], "wb");
    fwrite(y.data(), 8, y.size(), o);
    fwrite(&_gain, 4, 1, o);
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def cpp_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("cagcref")
    (d / "c.cpp").write_text(_CHECK_SRC)
    exe = d / "c"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", str(d / "c.cpp"), "-o", str(exe)])

    def run(x, par, gain=1.0, cuts=()):
        np.asarray(x, np.complex64).tofile(d / "x.bin")
        args = [repr(float(F32(v))) for v in par] + [repr(float(F32(gain)))]
        subprocess.check_call([str(exe), str(d / "x.bin"), str(d / "y.bin")] + args + [str(c) for c in cuts])
        raw = np.fromfile(d / "y.bin", dtype=F32)
        return raw[:-1].view(np.complex64), raw[-1]

    return run


def edge_vector():
    v = [0.0, -0.0, 1e-45, -1e-45j, 1e-40 + 1e-40j, -3e-39, 1e30, -1e30j, 3e38, 1e-30, 1 + 1j, -1.0, 0.5j, np.inf, 1.0, 2.0j,
         complex(0, -np.inf), 0.25, np.nan, 1.0, -2.0]
    return np.asarray(v * 3, np.complex64)


@pytest.mark.parametrize("which", ["random", "edges", "negative_gain"])
@pytest.mark.parametrize("case", list(PARAMS))
def test_restatement_is_bit_identical_to_the_cpp_restatement(cpp_check, which, case):
    par = PARAMS[case]
    g0 = 1.0
    if which == "random":
        x = make_input("gauss", 100_000, seed=5) * F32(SCALE[case])
        x[::97] *= F32(1e-20)
        x[5::89] *= F32(1e3)           # out of the scan's domain: the gain turns negative now and then
    elif which == "edges":
        x = edge_vector()
    else:
        x, g0 = make_input("gauss", 5000, seed=6) * F32(SCALE[case]), -0.75
    want, last = cpp_check(x, par, g0)
    y, g = cagc_ref(x, *par, gain=g0)
    assert _same_bits(y, want) and _same_bits([g], [last])
    if which == "edges":
        assert np.isnan(g)
    # ... and in three calls with the gain carried
    k1, k2 = (len(x) // 3, 2 * len(x) // 3) if which != "edges" else (7, 20)
    want3, last3 = cpp_check(x, par, g0, (k1, k2))
    y1, s1 = cagc_ref(x[:k1], *par, gain=g0)
    y2, s2 = cagc_ref(x[k1:k2], *par, gain=s1)
    y3, s3 = cagc_ref(x[k2:], *par, gain=s2)
    assert _same_bits(np.concatenate([y1, y2, y3]), want3) and _same_bits([s3], [last3]) and _same_bits(want3, want)


def test_ref_columns_are_independent_and_state_shapes():
    x = make_input("gauss", 1000).reshape(500, 2)
    y, g = cagc_ref(x, (1.0, 0.5), 4.0, (1e-3, 0.02), (0.5, 2.0))
    y0, g0 = cagc_ref(x[:, 0], 1.0, 4.0, 1e-3, 0.5)
    y1, g1 = cagc_ref(x[:, 1], 0.5, 4.0, 0.02, 2.0)
    assert _same_bits(y[:, 0], y0) and _same_bits(y[:, 1], y1) and _same_bits(g, [g0, g1])
    yr, yi, G, M, gt = cagc_exact(x, (1.0, 0.5), 4.0, (1e-3, 0.02), (0.5, 2.0))
    assert yr.dtype == LD and G.shape == (501, 2) and gt.shape == (2,) and np.all(M >= 1) and np.all(np.diff(M, axis=0) >= 0)
    assert np.max(np.abs(yr - y.real)) < 1e-4 and np.max(np.abs(gt - g)) < 1e-4
    assert cagc_ref(x[:0], 1.0, 4.0, 1e-3, 0.25)[1][0] == F32(0.25)
    assert cagc_exact(x[:0, 0], 1.0, 4.0, 1e-3, 0.25)[4] == LD(0.25)


# ---- the composition law ------------------------------------------------------------------------------------------------------------
def compose(later, earlier):
    """(a2, b2, c2) o (a1, b1, c1) = (a2 a1, a2 b1 + b2, min(a2 c1 + b2, c2)) on float64 arrays, every operation rounded."""
    a2, b2, c2 = later
    a1, b1, c1 = earlier
    return a2 * a1, a2 * b1 + b2, np.minimum(a2 * c1 + b2, c2)


def apply_map(m, g):
    return np.minimum(m[0] * g + m[1], m[2])


def identity_map(shape=()):
    return np.ones(shape), np.zeros(shape), np.full(shape, BIG)


def test_composition_law_against_applying_the_maps_in_turn():
    """On eighths every operation is exact, so the composed map and the maps applied one after the other agree to the bit."""
    rng = np.random.default_rng(3)
    k, trials = 6, 4000
    a = rng.integers(0, 9, (k, trials)) / 8.0           # a in [0, 1]: a == 0 on a ninth of the maps
    b = rng.integers(0, 33, (k, trials)) / 8.0
    c = rng.integers(0, 41, (k, trials)) / 8.0          # small enough for the clamp to act most of the time
    ident = rng.integers(0, k, trials)                  # one of the maps is the identity, at either end or inside
    for j in range(k):
        sel = ident == j
        a[j, sel], b[j, sel], c[j, sel] = 1.0, 0.0, BIG
    assert np.any(a == 0) and np.any(ident == 0) and np.any(ident == k - 1)
    clamped = 0
    for g0 in (0.0, 0.125, 1.0, 7.5, 1e6, BIG):
        g = np.full(trials, g0)
        left = identity_map((trials,))                  # ((m5 o m4) o ...): folded from the left
        for j in range(k):
            m = (a[j], b[j], c[j])
            clamped += int(np.sum(m[0] * g + m[1] > m[2]))
            g = apply_map(m, g)
            left = compose(m, left)
        right = (a[k - 1], b[k - 1], c[k - 1])          # (m5 o (m4 o ...)): folded from the right
        for j in range(k - 2, -1, -1):
            right = compose(right, (a[j], b[j], c[j]))
        pair = compose(compose((a[5], b[5], c[5]), compose((a[4], b[4], c[4]), (a[3], b[3], c[3]))),
                       compose((a[2], b[2], c[2]), compose((a[1], b[1], c[1]), (a[0], b[0], c[0]))))
        for m in (left, right, pair):
            assert np.all(np.isfinite(m[0]) & np.isfinite(m[1]) & np.isfinite(m[2]))
            assert np.array_equal(apply_map(m, np.full(trials, g0)), g), g0
    assert clamped > trials
    # the identity on either side leaves the map's action alone, a == 0 next to it included (0 * inf with c = +inf)
    m = (np.asarray([0.0, 0.5, 1.0]), np.asarray([0.25, 0.25, 0.0]), np.asarray([3.0, 0.125, 2.0]))
    for g0 in (0.0, 1.0, 1e300):
        g = np.full(3, g0)
        assert np.array_equal(apply_map(compose(m, identity_map((3,))), g), apply_map(m, g))
        assert np.array_equal(apply_map(compose(identity_map((3,)), m), g), apply_map(m, g))
    with np.errstate(all="ignore"):
        assert np.isnan(compose(m, (np.ones(3), np.zeros(3), np.full(3, np.inf)))[2][0])


# ---- the bound against an emulation of the kernel's scan ------------------------------------------------------------------------
def emulate_scan(x, set_point, max_gain, rate, gain=1.0):
    """numpy stand-in for the kernel (qdsp_amd/csrc/cagc.hip), FP64: lanes fold 8 samples, Hillis-Steele over the 64 lanes of a
    wave, the four wave totals in turn, tiles carried in turn inside a chunk, the chunk totals applied in turn, each lane replaying
    its samples from its exclusive prefix; every output the FP64 product rounded to float32.  Every operation is rounded
    separately here; the kernel fuses a x + b into one rounding.  Returns (outputs, the gain after the last sample)."""
    x = np.asarray(x, np.complex64)
    n = len(x)
    r = np.float64(F32(rate))
    b = np.float64(F32(set_point)) * np.float64(F32(rate))
    c = min(np.float64(F32(max_gain)), BIG)
    tiles = -(-n // TILE)
    re, im = np.zeros(tiles * TILE), np.zeros(tiles * TILE)
    re[:n], im[:n] = x.real, x.imag
    valid = (np.arange(tiles * TILE) < n).reshape(tiles, 256, 8)
    re, im = re.reshape(tiles, 256, 8), im.reshape(tiles, 256, 8)
    aj = 1.0 - r * np.sqrt(re * re + im * im)
    assert np.all(aj[valid] >= 0), "out of the scan's domain"
    A, B, C = identity_map((tiles, 256))
    for j in range(8):
        v = valid[:, :, j]
        C = np.where(v, np.minimum(aj[:, :, j] * C + b, c), C)
        B = np.where(v, aj[:, :, j] * B + b, B)
        A = np.where(v, A * aj[:, :, j], A)
    m = tuple(t.reshape(tiles, 4, 64) for t in (A, B, C))
    d = 1
    while d < 64:                               # inclusive scan of every wave
        new = compose(tuple(t[:, :, d:] for t in m), tuple(t[:, :, :-d] for t in m))
        m = tuple(np.concatenate([t[:, :, :d], u], axis=2) for t, u in zip(m, new))
        d *= 2
    ex = tuple(np.concatenate([i[:, :, None], t[:, :, :-1]], axis=2) for i, t in zip(identity_map((tiles, 4)), m))
    pre = identity_map((tiles,))
    ex_w = []
    for w in range(4):                          # the waves before, then the tile total
        ex_w.append(compose(tuple(t[:, w] for t in ex), tuple(t[:, None] for t in pre)))
        pre = compose(tuple(t[:, w, 63] for t in m), pre)
    ex = tuple(np.stack([e[i] for e in ex_w], axis=1).reshape(tiles, 256) for i in range(3))
    tile = pre
    # carries: tile by tile inside a chunk, the chunk totals in front applied in turn
    if tiles <= ROW_TILES:
        T = max(tiles, 1)
    else:
        T = -(-tiles // min(tiles, MAX_PARTS))
    G = -(-tiles // T)
    chunk = []
    for g in range(G - 1):
        acc = identity_map()
        for t in range(g * T, (g + 1) * T):
            acc = compose(tuple(u[t] for u in tile), acc)
        chunk.append(acc)
    carry = np.empty(tiles)
    for g in range(G):
        cur = np.float64(gain)
        for k in range(g):
            cur = apply_map(chunk[k], cur)
        for t in range(g * T, min(tiles, (g + 1) * T)):
            carry[t] = cur
            cur = apply_map(tuple(u[t] for u in tile), cur)
    g_lane = apply_map(ex, carry[:, None])
    yr, yi, after = np.empty((tiles, 256, 8)), np.empty((tiles, 256, 8)), np.empty((tiles, 256, 8))
    for j in range(8):
        yr[:, :, j], yi[:, :, j] = re[:, :, j] * g_lane, im[:, :, j] * g_lane
        g_lane = np.where(valid[:, :, j], np.minimum(aj[:, :, j] * g_lane + b, c), g_lane)
        after[:, :, j] = g_lane
    y = np.empty(n, np.complex64)
    with np.errstate(all="ignore"):
        y.real, y.imag = yr.reshape(-1)[:n].astype(F32), yi.reshape(-1)[:n].astype(F32)
    return y, (after.reshape(-1)[n - 1] if n else np.float64(gain))


@pytest.mark.parametrize("n", SIZES)
def test_emulated_scan_meets_the_bound_of_the_gpu_test(n):
    x, par, ref, gref, exact = case_table(n)
    for k, (p, kind) in enumerate(case_list()):
        label = f"n={n} {p} {kind}"
        y, g = emulate_scan(x[:, k], *par[:, k])
        ex = column(exact, k)
        ratio, e_scan, e_ref = check_against_truth(y, x[:, k], ex, ref[:, k], label)
        check_gain(g, ex, label)
        assert ratio <= 1.0
        if n >= 4096:
            assert e_scan <= e_ref, label


def test_emulated_scan_with_more_than_one_tile_per_chunk():
    n = (MAX_PARTS + 3) * TILE + 77                     # T = 2
    sp, mg, rt = PARAMS["fast_x4"]
    x = limit_to_domain(make_input("gauss", n, seed=8) * F32(4), rt)
    w = slice(n - 6000, n)
    y, g = emulate_scan(x, sp, mg, rt)
    # the truth of the last samples from any gain a run-in before them: the loop forgets (tests/test_gpu_cagc.py, case 8)
    s = n - 12_000
    exact = cagc_exact(x[s:], sp, mg, rt, 2.0)
    a = 1.0 - float(F32(rt)) * np.abs(x[s:w.start].astype(np.complex128))
    assert np.sum(np.log2(np.maximum(a, 1e-300))) < -60
    tail = tuple(t[w.start - s:] for t in exact[:4]) + (exact[4],)
    check_against_truth(y[w], x[w], tail, None, "T = 2", extra=LD(2.0) ** -60 * LD(mg))
    check_gain(g, tail, "T = 2", extra=LD(2.0) ** -60 * LD(mg))


def test_float_loop_alone_is_outside_the_bound_on_the_silent_row():
    """Why the bound is set against the exact recurrence and not against the reference's loop: on silence the float loop adds
    set_point * rate = 1e-3 to a gain of thousands 80 000 times, every sum rounded to float."""
    x, par, ref, gref, exact = case_table(SIZES[-1])
    k = case_list().index(("ref_defaults", "silence"))
    yr, yi, G, M, gt = column(exact, k)
    err = abs(LD(gref[k]) - gt)
    assert err > 100 * gain_bound(M[-1]) and err / gt > 1e-4
    # (its outputs are all 0 * g = 0 on this row; on the tone the same drift reaches the outputs)
    kt = case_list().index(("ref_defaults", "tone"))
    yr, yi, G, M, gt = column(exact, kt)
    e = np.abs(ref[:, kt].real.astype(LD) - yr)
    assert np.max(e / cagc_bound(yr, x[:, kt].real, M[:-1])) > 10
