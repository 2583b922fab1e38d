"""BFMDeemp (src/dsp/filter.h:90-173) without a GPU: the C ABI exports the de-emphasis entry points, the C++ block mirror carries
the reference's surface, build() makes the graph harness -- and the three numpy helpers the GPU tests stand on are checked here:
`deemp_ref` (the reference's float loop, pinned bit for bit to a C++ restatement), `deemp_exact` (the same float coefficients run
sequentially in np.longdouble: the truth) and the bound `deemp_bound`, which a numpy emulation of the kernel's blocked FP64 scan has to
meet for every case of the GPU accuracy test."""
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
TILE = 2048            # kDemodNT * kDemodSpl (qdsp_amd/csrc/demod.hip.h)
ROW_TILES = 16         # kDeempRowTiles: rows of at most this many tiles take one launch
MAX_PARTS = 1024       # kAmMaxParts


# ---- the restatement, the truth and the bound -------------------------------------------------------------------------------
def deemp_alpha(sample_rate, tau):
    """alpha of BFMDeemp::init (filter.h:102-103), in float."""
    dt = np.float32(1.0) / np.float32(sample_rate)
    return np.float32(dt / np.float32(np.float32(tau) + dt))


def _columns(x, dtype):
    x = np.asarray(x, dtype)
    ncol = int(np.prod(x.shape[1:], dtype=np.int64))
    return x.reshape(len(x), ncol), x.shape


def deemp_ref(x, alpha, state=0.0):
    """BFMDeemp::run over one call, float32 throughout, products rounded before the add: (outputs, carried state).  x: (n,) or
    (n, k), every column filtered on its own; `state` a scalar or one value per column.  A NaN state reads as 0."""
    xc, shape = _columns(x, np.float32)
    alpha = np.float32(alpha)
    b = np.float32(np.float32(1.0) - alpha)
    prev = np.broadcast_to(np.asarray(state, np.float32), xc.shape[1:]).copy()
    prev[np.isnan(prev)] = 0
    y = np.empty_like(xc)
    with np.errstate(all="ignore"):
        ax = alpha * xc
        for i in range(len(xc)):
            prev = ax[i] + b * prev
            y[i] = prev
    return y.reshape(shape), (prev if len(shape) > 1 else prev[0])


def deemp_exact(x, alpha, state=0.0):
    """The exact recurrence of the reference's float coefficients a = alpha, b = (float)(1 - alpha), run sequentially in
    np.longdouble from `state` (longdouble, or anything exactly convertible): (outputs, state), both longdouble.  A state that
    is not finite reads as 0 (include/qdsp_hip.h)."""
    xc, shape = _columns(x, LD)
    a = LD(np.float32(alpha))
    b = LD(np.float32(np.float32(1.0) - np.float32(alpha)))
    prev = np.broadcast_to(np.asarray(state, LD), xc.shape[1:]).copy()
    prev[~np.isfinite(prev)] = 0
    y = np.empty_like(xc)
    with np.errstate(all="ignore"):
        ax = a * xc
        for i in range(len(xc)):
            prev = ax[i] + b * prev
            y[i] = prev
    return y.reshape(shape), (prev if len(shape) > 1 else prev[0])


def deemp_envelope(x, alpha, state=0.0):
    """E = deemp_exact(|x|, alpha, |state|): the sum of the absolute terms of every output."""
    st = np.abs(np.asarray(state, LD))
    st = np.where(np.isfinite(st), st, 0)
    return deemp_exact(np.abs(np.asarray(x, LD)), alpha, st)[0]


def ulp32(t):
    """The float32 spacing at |t|; where |t| rounds up to the next binade the larger spacing is taken."""
    return np.spacing(np.abs(np.asarray(t, LD)).astype(np.float32)).astype(LD)


def deemp_bound(truth, env):
    """0.5 ulp32(truth): the one final rounding; 2^-40 E: 2^13 FP64 epsilons of reassociation relative to the sum of the absolute
    terms (a scan tree of about 3 + 6 + 2 levels plus the fold of the chunk totals, a few roundings each)."""
    return LD(0.5) * ulp32(truth) + LD(2.0) ** -40 * np.asarray(env, LD)


# ---- the cases of the accuracy test -------------------------------------------------------------------------------------------
ALPHAS = {"48k_50us": (48_000.0, 50e-6), "240k_75us": (240_000.0, 75e-6), "2400k_75us": (2_400_000.0, 75e-6), "tiny": (200_000.0, 50e-3)}
INPUTS = ("gauss", "tone", "step")
SIZES = (1, 7, TILE, TILE + 1, 1 << 20, 3_000_001)


def make_input(kind, n, sample_rate, seed=11):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "tone":          # 1 kHz, with a DC offset
        t = np.arange(n, dtype=np.float64) / sample_rate
        return (0.5 * np.sin(2 * np.pi * 1000.0 * t) + 0.25).astype(np.float32)
    if kind == "step":          # 1e6 : 1 amplitude step half way: the outputs after it are what is left of a cancellation
        x = rng.standard_normal(n)
        x[: n // 2] *= 1e6
        return x.astype(np.float32)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case_table(n):
    """For one size: x (n, 12) float32, one column per (alpha, input) in ALPHAS x INPUTS order, and per column the float loop's
    outputs, the truth and the envelope from state 0.  The three sequential loops run once over all columns."""
    cols, alphas = [], []
    for sr, tau in ALPHAS.values():
        for kind in INPUTS:
            cols.append(make_input(kind, n, sr))
            alphas.append(deemp_alpha(sr, tau))
    x = np.stack(cols, axis=1)
    al = np.asarray(alphas, np.float32)
    ref, _ = deemp_ref(x, al)
    both, _ = deemp_exact(np.concatenate([x.astype(LD), np.abs(x.astype(LD))], axis=1), np.concatenate([al, al]))
    return x, al, ref, both[:, :12], both[:, 12:]


def test_alphas_are_the_ones_the_cases_name():
    a = [float(deemp_alpha(*v)) for v in ALPHAS.values()]
    assert abs(a[0] - 0.294) < 1e-3 and abs(a[1] - 0.0526) < 1e-4 and abs(a[2] - 0.00552) < 1e-5 and abs(a[3] - 1e-4) < 1e-6


# ---- the C ABI and the mirror ---------------------------------------------------------------------------------------------------
DEEMP_SYMBOLS = ["qdsp_hip_deemp_" + s for s in (
    "create", "set", "set_bypass", "process", "process_ex", "process_dev", "process_batch_dev", "get_state", "set_state", "get_alpha",
    "reset", "destroy")]


def test_deemp_symbols_declared_and_exported():
    declared = set(capi.declared_symbols())
    assert set(DEEMP_SYMBOLS) <= declared, sorted(set(DEEMP_SYMBOLS) - declared)
    L = capi.load()
    assert all(hasattr(L, s) for s in DEEMP_SYMBOLS)
    assert all(getattr(L, s).argtypes is not None for s in DEEMP_SYMBOLS), "declared in capi.py"
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(DEEMP_SYMBOLS) <= exported
    hdr = open(capi.HEADER_PATH).read()
    for k, v in (("QDSP_HIP_DEEMP_MONO", 0), ("QDSP_HIP_DEEMP_STEREO", 1)):
        assert re.search(rf"#define {k}\s+{v}\b", hdr), k
    assert L.qdsp_hip_abi_version() == 1
    from qdsp_amd import ops

    for name in ("process", "process_batch", "set", "bypass", "get_state", "set_state", "alpha", "reset", "time_dev", "last_kernel"):
        assert callable(getattr(ops.Deemp, name)), name


_SURFACE_SRC = r"""
#include <type_traits>
#include "dsp/deemp.h"
#include "dsp/demodulator.h"
using namespace dsp;
static_assert(std::is_same<decltype(BFMDeemp::out), stream<stereo_t>>::value, "BFMDeemp::out");
static_assert(std::is_same<decltype(BFMDeemp::bypass), bool>::value, "BFMDeemp::bypass");
static_assert(std::is_base_of<detail::hip_block<stereo_t, stereo_t>, BFMDeemp>::value, "the shared base of the HIP-backed blocks");
void use(stream<complex_t>* iq, stream<stereo_t>* in) {
    BFMDeemp a(in, 48000.0f, 50e-6f);
    a.setSampleRate(44100.0f); a.setTau(75e-6f); a.setInput(in); a.bypass = true;
    BFMDeemp b;
    b.init(in, 240e3f, 75e-6f);
    FMDemod fm(iq, 240e3f, 75e3f);
    BFMDeemp c(&fm.out, 240e3f, 50e-6f);
    generic_unnamed_block* blocks[] = {&a, &b, &c};
    (void)blocks;
}
"""


def test_bfmdeemp_block_compiles_with_the_reference_types(tmp_path):
    (tmp_path / "s.cpp").write_text(_SURFACE_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.cpp")])
    src = open(os.path.join(HOST, "dsp", "deemp.h")).read() + open(os.path.join(HOST, "dsp", "hip_block.h")).read()    # (the link protocol is the base's)
    for name in ("claimConsumer", "done.arm", "qdsp_hip_deemp_process_ex", "qdsp_hip_deemp_set_bypass"):
        assert name in src, name
    # graph_check is linked against the fake library of the sanitizer test, which has no de-emphasis symbols
    assert not re.search(r"#include\s*[<\"]dsp/deemp\.h", open(os.path.join(HOST, "examples", "graph_check.cpp")).read())
    assert "BFMDeemp" not in open(os.path.join(HOST, "dsp", "filter.h")).read()


def test_build_makes_the_deemp_harness():
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert re.search(r"^all:.*build/demod_check", mk, re.M)
    assert "dsp/deemp.h" in open(os.path.join(HOST, "examples", "demod_check.cpp")).read()
    subprocess.check_call(["make", "-C", HOST, "build/demod_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "demod_check")
    assert os.access(exe, os.X_OK)
    out = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    assert "qdsp_hip_deemp_process_ex" in out


# ---- the restatement against a C++ restatement ----------------------------------------------------------------------------------
_CHECK_SRC = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
// argv: in.bin out.bin sampleRate tau cut...: the float samples of in.bin filtered in calls that end at the cuts
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    std::vector<float> x;
    float v;
    while (fread(&v, sizeof(v), 1, f) == 1) x.push_back(v);
    fclose(f);
    const float sampleRate = (float)atof(argv[3]), tau = (float)atof(argv[4]);
    const float dt = 1.0f / sampleRate;
    const float alpha = dt / (tau + dt);
    std::vector<float> y(x.size());
    float lastOut = 0.0f;
    size_t pos = 0;
    for (int k = 5; k <= argc; k++) {
        const size_t end = k < argc ? (size_t)atol(argv[k]) : x.size();
        if (end <= pos) continue;
        if (std::isnan(lastOut)) lastOut = 0.0f;
        y[pos] = (alpha * x[pos]) + ((1 - alpha) * lastOut);
        for (size_t i = pos + 1; i < end; i++) y[i] = (alpha * x[i]) + ((1 - alpha) * y[i - 1]);
        lastOut = y[end - 1];
        pos = end;
    }
    FILE* o = fopen(argv[2], "wb");
    fwrite(y.data(), 4, y.size(), o);
    fwrite(&lastOut, 4, 1, o);
    fwrite(&alpha, 4, 1, o);
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def cpp_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("deempref")
    (d / "c.cpp").write_text(_CHECK_SRC)
    exe = d / "c"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", str(d / "c.cpp"), "-o", str(exe)])

    def run(x, sr, tau, cuts=()):
        np.asarray(x, np.float32).tofile(d / "x.bin")
        subprocess.check_call([str(exe), str(d / "x.bin"), str(d / "y.bin"), repr(float(sr)), repr(float(tau))] + [str(c) for c in cuts])
        y = np.fromfile(d / "y.bin", dtype=np.float32)
        return y[:-2], y[-2], y[-1]

    return run


def _same_bits(a, b):
    """Equal as float32 bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def edge_vector():
    v = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1e30, -1e30, 3e38, 1e-30, -1e-30, 1.0, -1.0, 0.5, np.inf, 1.0, 2.0, -np.inf, 0.25, np.nan, 1.0, -2.0]
    return np.asarray(v * 3, np.float32)


@pytest.mark.parametrize("which", ["random", "edges"])
@pytest.mark.parametrize("case", list(ALPHAS))
def test_restatement_is_bit_identical_to_the_cpp_restatement(cpp_check, which, case):
    sr, tau = ALPHAS[case]
    if which == "random":
        x = make_input("gauss", 200_000, sr, seed=5)
        x[::97] *= np.float32(1e-20)
        x[5::89] *= np.float32(1e20)
    else:
        x = edge_vector()
    al = deemp_alpha(sr, tau)
    want, last, al_cpp = cpp_check(x, sr, tau)
    assert _same_bits([al], [al_cpp])
    y, st = deemp_ref(x, al)
    assert _same_bits(y, want) and _same_bits([st], [last])
    # ... and in three calls with the state carried; in the edge vector the second call ends on the NaN (the reset)
    k1, k2 = (len(x) // 3, 2 * len(x) // 3) if which == "random" else (7, 20)
    want3, last3, _ = cpp_check(x, sr, tau, (k1, k2))
    y1, s1 = deemp_ref(x[:k1], al)
    y2, s2 = deemp_ref(x[k1:k2], al, s1)
    y3, s3 = deemp_ref(x[k2:], al, s2)
    assert _same_bits(np.concatenate([y1, y2, y3]), want3) and _same_bits([s3], [last3])
    if which == "edges":
        assert np.isnan(s2) and np.isfinite(y3[0]) and not _same_bits(want3, want)
        assert _same_bits(y3[:10], deemp_ref(x[k2:k2 + 10], al, 0.0)[0])


def test_ref_columns_are_independent_and_state_shapes():
    x = make_input("gauss", 1000, 48_000.0).reshape(500, 2)
    al = deemp_alpha(48_000.0, 50e-6)
    y, st = deemp_ref(x, al, (0.5, np.nan))
    yl, sl = deemp_ref(x[:, 0], al, 0.5)
    yr, sr_ = deemp_ref(x[:, 1], al, 0.0)
    assert _same_bits(y[:, 0], yl) and _same_bits(y[:, 1], yr) and _same_bits(st, [sl, sr_])
    t, ts = deemp_exact(x, al, (0.5, np.nan))
    assert t.dtype == LD and np.max(np.abs(t - y)) < 1e-6 and ts.shape == (2,)
    assert deemp_ref(x[:0], al, 0.25)[1][0] == np.float32(0.25)


# ---- the bound against an emulation of the kernel's scan ------------------------------------------------------------------------
def emulate_scan(x, alpha, state=0.0):
    """numpy stand-in for the kernel (qdsp_amd/csrc/deemp.hip.h), FP64, every operation rounded separately: lanes fold 8 samples,
    Hillis-Steele over the 64 lanes of a wave, the four wave totals in turn, tiles carried in turn inside a chunk, the chunk totals
    folded by Horner, each lane replaying its samples from its exclusive prefix; one final rounding to float32."""
    x = np.asarray(x, np.float32)
    n = len(x)
    a = np.float64(np.float32(alpha))
    b = np.float64(np.float32(np.float32(1.0) - np.float32(alpha)))
    tiles = -(-n // TILE)
    xp = np.zeros(tiles * TILE, np.float64)
    xp[:n] = x
    valid = (np.arange(tiles * TILE) < n).reshape(tiles, 256, 8)
    xs = xp.reshape(tiles, 256, 8)
    A = np.ones((tiles, 256))
    B = np.zeros((tiles, 256))
    for j in range(8):
        B = np.where(valid[:, :, j], b * B + a * xs[:, :, j], B)
        A = np.where(valid[:, :, j], A * b, A)
    A = A.reshape(tiles, 4, 64)
    B = B.reshape(tiles, 4, 64)
    d = 1
    while d < 64:                               # inclusive scan of every wave
        An, Bn = A.copy(), B.copy()
        Bn[:, :, d:] = A[:, :, d:] * B[:, :, :-d] + B[:, :, d:]
        An[:, :, d:] = A[:, :, d:] * A[:, :, :-d]
        A, B, d = An, Bn, 2 * d
    exA = np.concatenate([np.ones((tiles, 4, 1)), A[:, :, :-1]], axis=2)
    exB = np.concatenate([np.zeros((tiles, 4, 1)), B[:, :, :-1]], axis=2)
    preA, preB = np.ones(tiles), np.zeros(tiles)
    for w in range(4):                          # the waves before, then the tile total
        exB[:, w], exA[:, w] = exA[:, w] * preB[:, None] + exB[:, w], exA[:, w] * preA[:, None]
        preB, preA = A[:, w, 63] * preB + B[:, w, 63], A[:, w, 63] * preA
    # carries: tile by tile inside a chunk, Horner over the chunk totals in front
    if tiles <= ROW_TILES:
        T = tiles
    else:
        g0 = min(tiles, MAX_PARTS)
        T = -(-tiles // g0)
    carry = np.empty(tiles)
    s0 = np.float64(state) if np.isfinite(state) else np.float64(0)
    G = -(-tiles // T)
    cA, cB = np.ones(G), np.zeros(G)
    for g in range(G - 1):
        for t in range(g * T, (g + 1) * T):
            cB[g], cA[g] = preA[t] * cB[g] + preB[t], preA[t] * cA[g]
    for g in range(G):
        c = s0
        for k in range(g):
            c = cA[k] * c + cB[k]
        for t in range(g * T, min(tiles, (g + 1) * T)):
            carry[t] = c
            c = preA[t] * c + preB[t]
    y = exA.reshape(tiles, 256) * carry[:, None] + exB.reshape(tiles, 256)
    out = np.empty((tiles, 256, 8))
    for j in range(8):
        y = b * y + a * xs[:, :, j]
        out[:, :, j] = y
    with np.errstate(all="ignore"):
        return out.reshape(-1)[:n].astype(np.float32)


def check_against_truth(y, truth, env, ref=None, label=""):
    """Bound 1 for every output; with `ref` (the float loop's outputs) also |y - ref| <= |ref - truth| + bound.  Returns
    (worst error / bound, max |y - truth|, max |ref - truth|) and prints them."""
    y = np.asarray(y, np.float32).astype(LD)
    bound = deemp_bound(truth, env)
    err = np.abs(y - truth)
    ratio = float(np.max(err / bound))
    e_gpu = float(np.max(err))
    e_ref = float(np.max(np.abs(np.asarray(ref, np.float32).astype(LD) - truth))) if ref is not None else float("nan")
    print(f"{label}: worst error / bound {ratio:.3f}, max |y - truth| {e_gpu:.3g}, max |float loop - truth| {e_ref:.3g}")
    assert np.all(err <= bound), (label, ratio)
    if ref is not None:
        r = np.asarray(ref, np.float32).astype(LD)
        assert np.all(np.abs(y - r) <= np.abs(r - truth) + bound), label
    return ratio, e_gpu, e_ref


@pytest.mark.parametrize("n", SIZES)
def test_emulated_scan_meets_the_bound_of_the_gpu_test(n):
    x, al, ref, truth, env = case_table(n)
    for k in range(x.shape[1]):
        label = f"n={n} {list(ALPHAS)[k // 3]} {INPUTS[k % 3]}"
        y = emulate_scan(x[:, k], al[k])
        ratio, e_scan, e_ref = check_against_truth(y, truth[:, k], env[:, k], ref[:, k], label)
        assert ratio <= 1.0
        if n >= 4096:
            assert e_scan <= e_ref, label


def test_float_loop_alone_is_outside_the_bound():
    """Why the bound is set against the exact recurrence and not against the reference's loop."""
    x, al, ref, truth, env = case_table(1 << 20)
    k = 3 * 3 + 1                                   # tiny alpha, tone
    err = np.abs(ref[:, k].astype(LD) - truth[:, k])
    assert np.max(err / deemp_bound(truth[:, k], env[:, k])) > 100
