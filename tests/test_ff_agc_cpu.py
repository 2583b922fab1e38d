"""FeedForwardAGC (src/dsp/processing.h:147-233) without a GPU: the C ABI exports the entry points and capi binds them, the C++ block
mirror carries the reference's surface, build() makes the graph harness -- and the numpy helper the GPU tests stand on is checked
here: `ffagc_ref`, pinned bit for bit to the block's equations written out in C++ over a flat stream (a W-compare loop per output), and the property
the kernel leans on: the amplitude a(r) is non-decreasing in r = |re|, so the maximum may be taken before a is applied."""
import os
import re
import subprocess

import numpy as np
import pytest

from qdsp_amd import capi
from test_level_cpu import F32, _same_bits, edge_vector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
CSRC = os.path.join(ROOT, "qdsp_amd", "csrc")
TILE = 2048            # kFfAgcTile = kDemodNT * kDemodSpl (qdsp_amd/csrc/ff_agc.hip.h)
MAX_WINDOW = 4096      # kFfAgcMaxWindow
FLOOR = F32(1e-4)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def amplitude(x):
    """a(v) of every sample: fabsf(v) for float rows; for complex rows fastAmplitude as the reference has it (types.h:58-63), both
    magnitudes from re: r + 0.4f * r with the product and the sum each rounded to float."""
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        if np.iscomplexobj(x):
            r = np.abs(x.real.astype(F32))
            return (r + (F32(0.4) * r).astype(F32)).astype(F32)
        return np.abs(x.astype(F32))


def window_max(v, window):
    """max over [p, p + window) for every p that has a whole window, under `val > level`: a NaN never wins (v >= 0 or NaN)."""
    v = np.where(np.isnan(v), F32(0), v).astype(F32)
    if len(v) < window:
        return np.zeros(0, F32)
    return np.lib.stride_tricks.sliding_window_view(v, window).max(axis=1)


def divide(x, level):
    with np.errstate(all="ignore"):
        if np.iscomplexobj(x):
            y = np.empty(len(x), np.complex64)
            y.real = x.real / level                 # two true divisions, no complex arithmetic
            y.imag = x.imag / level
            return y
        return (x / level).astype(F32)


def ffagc_ref(x, window, hist=None):
    """One call of FeedForwardAGC over `x` with the `hist` samples not yet output before it: (outputs, samples not yet output).
    The amplitude of every sample first, then the maximum: the reference's order."""
    x = np.ascontiguousarray(x)
    dt = np.complex64 if np.iscomplexobj(x) else F32
    buf = np.concatenate([np.zeros(0, dt) if hist is None else np.asarray(hist, dt), x.astype(dt)])
    level = np.maximum(FLOOR, window_max(amplitude(buf), window))
    n = len(level)
    return divide(buf[:n], level), buf[n:].copy()


def ffagc_max_first(x, window):
    """The kernel's order: the window maximum of r = |re| (a NaN as 0), then a once per output."""
    x = np.ascontiguousarray(x)
    r = np.abs(x.real.astype(F32)) if np.iscomplexobj(x) else np.abs(x.astype(F32))
    m = window_max(r, window)
    a = amplitude(m.astype(np.complex64)) if np.iscomplexobj(x) else m
    return divide(x[:len(m)], np.maximum(FLOOR, a))


def test_constants_are_the_kernels():
    ff = open(os.path.join(CSRC, "ff_agc.hip.h")).read()
    dm = open(os.path.join(CSRC, "demod.hip.h")).read()
    assert re.search(r"constexpr int kFfAgcTile = kDemodNT \* kDemodSpl;", ff)
    nt = int(re.search(r"constexpr int kDemodNT = (\d+);", dm).group(1))
    spl = int(re.search(r"constexpr int kDemodSpl = (\d+);", dm).group(1))
    assert nt * spl == TILE
    assert int(re.search(r"constexpr int kFfAgcMaxWindow = (\d+);", ff).group(1)) == MAX_WINDOW


# ---- a is monotone, so max-then-a is a-then-max -----------------------------------------------------------------------------------
def test_amplitude_is_monotone_in_r():
    every = np.arange(0, 0x7F800001, 509, dtype=np.uint32)           # every 509th non-negative float, +0 to the last finite ones
    dense = [np.arange(lo, lo + 70_000, dtype=np.uint32) for lo in
             (0, 0x00800000 - 35_000,                                   # +0 and the subnormals; around FLT_MIN
              F32(1e-4).view(np.uint32) - 35_000, F32(1.0).view(np.uint32) - 35_000,
              F32(3.4028235e38 / 1.4).view(np.uint32) - 35_000,        # where r + 0.4f * r starts to overflow
              0x7F800000 - 69_999)]                                     # up to +Inf
    r = np.unique(np.concatenate([every] + dense)).view(F32)
    assert r[0] == 0 and r[-1] == np.inf and np.all(r[1:] > r[:-1])
    a = amplitude(r.astype(np.complex64))
    assert np.all(a[1:] >= a[:-1]) and a[0] == 0 and a[-1] == np.inf and not np.any(np.isnan(a))
    assert _same_bits(amplitude(-r.astype(np.complex64) + 7j), a), "im never enters, the sign of re neither"
    assert _same_bits(amplitude(r), r)


def stream_input(kind, which, n=20_000):
    if which == "random":
        rng = np.random.default_rng(17)
        amp = np.repeat([0.01, 3.0, 0.2, 1e-6, 50.0], n // 5)
        re_, im_ = (rng.standard_normal(n) * amp).astype(F32), (rng.standard_normal(n) * amp * 2).astype(F32)
    else:
        re_ = edge_vector()
        im_ = np.roll(re_, 5)
    if kind == "real":
        return re_
    z = np.empty(len(re_), np.complex64)             # (re + 1j * im would turn an Inf in im into a NaN in re)
    z.real, z.imag = re_, im_
    return z


@pytest.mark.parametrize("which", ["random", "edges"])
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_max_then_amplitude_equals_amplitude_then_max(kind, which):
    x = stream_input(kind, which)
    for window in ((1, 2, 7, 1024) if which == "random" else (1, 2, 5, 22)):
        assert _same_bits(ffagc_max_first(x, window).view(F32), ffagc_ref(x, window)[0].view(F32)), (kind, which, window)


# ---- the restatement against the equations in C++, a W-compare loop per output --------------------------------------------------
_CHECK_SRC = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
// argv: real|complex in.bin out.bin W cut...
// x = the floats of in.bin as one flat stream (complex: re, im pairs; cuts count samples).  Output p exists once x[p + W - 1] does:
//   level[p] = max(1e-4f, max over j in [0, W) of a(x[p + j])) under `val > level`,   y[p] = x[p] / level[p]
//   a = fabsf(x) (real);  r = fabsf(re), a = r + 0.4f * r (complex: im never enters), y = {re / level, im / level}
// A call that ends at cut e emits the outputs p with p + W - 1 < e that no earlier call emitted.  out.bin: y, then one float per
// call, the number of outputs it emitted.
int main(int argc, char** argv) {
    const bool cx = !strcmp(argv[1], "complex");
    const size_t nc = cx ? 2 : 1;
    std::vector<float> x;
    FILE* f = fopen(argv[2], "rb");
    for (float v; fread(&v, sizeof(v), 1, f) == 1;) x.push_back(v);
    fclose(f);
    const size_t total = x.size() / nc, W = (size_t)atol(argv[4]);
    std::vector<float> y, calls;
    size_t done = 0, prev = 0;      // outputs emitted so far; where the previous call ended
    for (int k = 5; k <= argc; k++) {
        const size_t end = k < argc ? (size_t)atol(argv[k]) : total;
        if (end <= prev) continue;
        const size_t have = end + 1 > W ? end + 1 - W : 0;      // outputs whose whole window lies below `end`
        for (size_t p = done; p < have; p++) {
            float level = 1e-4f;
            for (size_t j = 0; j < W; j++) {
                const float r = fabsf(x[(p + j) * nc]);
                float val = r;
                if (cx) {
                    const float t = 0.4f * r;
                    val = r + t;
                }
                if (val > level) level = val;
            }
            for (size_t e = 0; e < nc; e++) y.push_back(x[p * nc + e] / level);
        }
        calls.push_back((float)(have > done ? have - done : 0));
        if (have > done) done = have;
        prev = end;
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
    d = tmp_path_factory.mktemp("ffagcref")
    (d / "c.cpp").write_text(_CHECK_SRC)
    exe = d / "c"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", str(d / "c.cpp"), "-o", str(exe)])

    def run(kind, x, window, cuts=()):
        x = np.ascontiguousarray(x)
        x.tofile(d / "x.bin")
        subprocess.check_call([str(exe), kind, str(d / "x.bin"), str(d / "y.bin"), str(window)] + [str(c) for c in cuts])
        y = np.fromfile(d / "y.bin", dtype=F32)
        ncalls = len([c for c in cuts if 0 < c < len(x)]) + 1
        outs, calls = y[:len(y) - ncalls], y[len(y) - ncalls:]
        return (outs.view(np.complex64) if kind == "complex" else outs), calls.astype(np.int64)

    return run


@pytest.mark.parametrize("which", ["random", "edges"])
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_ffagc_ref_is_bit_identical_to_the_cpp_restatement(cpp_check, kind, which):
    x = stream_input(kind, which)
    n = len(x)
    if which == "random":
        cases = ((1024, (1, 5, 1022, 1023, 1024, 1030, 3000, 3001, 3500, 12_000)),        # five calls before the first output
                 (7, (2, 5, 6, 7, 8, 100, 101, 15_000)), (1, (1, 2, 700)), (2, (1, 2, 3, 9000)))
    else:
        cases = ((5, (1, 2, 4, 5, 9, 10, 30, 31)), (22, (3, 20, 21, 22, 23, 40)), (1, (1, 7)), (2, (1, 2)))
    for window, cuts in cases:
        want, emitted = cpp_check(kind, x, window, cuts)
        assert len(want) == n - (window - 1) and emitted.sum() == len(want)
        hist, got = None, []
        bounds = (0,) + cuts + (n,)
        for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
            fill = 0 if hist is None else len(hist)
            y, hist = ffagc_ref(x[a:b], window, hist)
            assert len(y) == emitted[k] == max(0, fill + (b - a) - (window - 1)), (window, k)
            assert len(hist) == fill + (b - a) - len(y) <= window - 1
            got.append(y)
        assert emitted[0] == 0 or window <= cuts[0]
        assert _same_bits(np.concatenate(got).view(F32), want.view(F32)), (kind, which, window)
        assert _same_bits(ffagc_ref(x, window)[0].view(F32), want.view(F32)), "one call"
    if which == "edges":                             # what the edge vector is there for
        y = ffagc_ref(x, 5)[0]
        re_ = y.real if kind == "complex" else y
        k_nan, k_inf = 16, 19
        assert np.isnan(re_[k_nan]) and not np.any(np.isnan(re_[k_nan - 4:k_nan])), "a NaN is a NaN at its own index only"
        assert np.isnan(re_[k_inf]) and not np.any(re_[[15, 17, 18]]), "+Inf: 0 under the windows that see it, NaN at the Inf"


# ---- the C ABI and the mirror -------------------------------------------------------------------------------------------------
FFAGC_SYMBOLS = ["qdsp_hip_ffagc_" + s for s in ("create", "process", "process_ex", "process_dev", "process_batch_dev", "out_size", "window",
                                                  "fill", "get_history", "set_history", "reset", "destroy")]


def test_ffagc_symbols_declared_exported_and_bound():
    declared = set(capi.declared_symbols())
    assert set(FFAGC_SYMBOLS) <= declared, sorted(set(FFAGC_SYMBOLS) - declared)
    L = capi.load()
    assert all(hasattr(L, s) for s in FFAGC_SYMBOLS)
    assert all(getattr(L, s).argtypes is not None for s in FFAGC_SYMBOLS), "declared in capi.py"
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(FFAGC_SYMBOLS) <= exported
    assert L.qdsp_hip_abi_version() == 1
    hdr = open(capi.HEADER_PATH).read()
    assert re.search(r"#define QDSP_HIP_FFAGC_REAL 0\b", hdr) and re.search(r"#define QDSP_HIP_FFAGC_COMPLEX 1\b", hdr)
    from qdsp_amd import ops

    for name in ("process", "process_batch", "out_size", "fill", "reset", "time_dev", "last_kernel", "get_history", "set_history"):
        assert callable(getattr(ops.FeedForwardAgc, name)), name
    assert "FeedForwardAgc" in ops.__all__
    kinds = [ops.FeedForwardAgc._kind_of(k) for k in (0, 1, "real", "complex", np.float32, np.complex64, np.dtype("complex64"))]
    assert kinds == [0, 1, 0, 1, 0, 1, 1]
    with pytest.raises(ValueError):
        ops.FeedForwardAgc._kind_of(np.float64)


_SURFACE_SRC = r"""
#include <type_traits>
#include "dsp/processing.h"
#include "dsp/demodulator.h"
using namespace dsp;
static_assert(std::is_same<decltype(FeedForwardAGC<float>::out), stream<float>>::value, "FeedForwardAGC<float>::out");
static_assert(std::is_same<decltype(FeedForwardAGC<complex_t>::out), stream<complex_t>>::value, "FeedForwardAGC<complex_t>::out");
static_assert(std::is_base_of<detail::hip_block<float, float>, FeedForwardAGC<float>>::value, "the shared base of the HIP-backed blocks");
static_assert(std::is_base_of<detail::hip_block<complex_t, complex_t>, FeedForwardAGC<complex_t>>::value, "the shared base of the HIP-backed blocks");
static_assert(std::is_default_constructible<FeedForwardAGC<float>>::value, "FeedForwardAGC()");
static_assert(std::is_constructible<FeedForwardAGC<complex_t>, stream<complex_t>*>::value, "FeedForwardAGC(stream<T>*)");
static_assert(std::is_same<decltype(std::declval<FeedForwardAGC<float>&>().run()), int>::value, "int run()");
void use(stream<complex_t>* iq, stream<float>* in) {
    FeedForwardAGC<complex_t> a(iq);
    a.setInput(iq);
    FeedForwardAGC<float> b;
    b.init(in);
    b.setInput(in);
    AMDemod am(&a.out);
    FeedForwardAGC<float> c(&am.out);
    generic_unnamed_block* blocks[] = {&a, &b, &c};
    (void)blocks;
}
"""


def test_feed_forward_agc_block_compiles_with_the_reference_surface(tmp_path):
    (tmp_path / "s.cpp").write_text(_SURFACE_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.cpp")])
    src = open(os.path.join(HOST, "dsp", "processing.h")).read() + open(os.path.join(HOST, "dsp", "hip_block.h")).read()    # (the link protocol is the base's)
    body = src[src.index("class FeedForwardAGC"):]
    for name in ("claimConsumer", "done.arm", "qdsp_hip_ffagc_process_ex", "qdsp_hip_ffagc_out_size", "linkIn()", "sampleCount = 1024"):
        assert name in body, name


def test_build_makes_the_ffagc_harness():
    src = open(os.path.join(HOST, "examples", "demod_check.cpp")).read()
    assert '"ffagc"' in src and "FeedForwardAGC<complex_t>" in src
    subprocess.check_call(["make", "-C", HOST, "build/demod_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "demod_check")
    assert os.access(exe, os.X_OK)
    out = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    assert "qdsp_hip_ffagc_process_ex" in out and "qdsp_hip_ffagc_create" in out
    # a block whose VFO output is below the window would never complete: refused before anything starts
    r = subprocess.run([exe, "ffagc", "dev", "none.cf32", "none.out", "10000", "0", "2400000", "240000", "200000"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "at least 1024" in r.stderr, (r.returncode, r.stderr)
