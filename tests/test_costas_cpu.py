"""CostasLoop<2 / 4 / 8> (src/dsp/pll.h:47-102) without a GPU: the C ABI exports the entry points, the C++ block mirror carries the
reference's surface, build() makes the graph harness -- and the numpy helpers the GPU tests stand on are checked here:
`costas_gains` (alpha and beta by the reference's mixed float / double formula), `costas_truth` (the recurrence on the float alpha,
beta and samples, run sequentially in np.longdouble with exact decisions), `costas_ref` (the reference's loop in float32, every
product and sum rounded, the VCO the float32 of an FP64 cosine and sine), which is held against a C++ restatement that calls
cosf / sinf, and the cases of the accuracy test, each of which is shown to do what it is there for.

The decision margin.  The error detectors of orders 4 and 8 decide on the signs of the de-rotated sample (order 8 also on
|re| >= |im|), and the phase wrap decides on |phase| > T.  Two correct loops that differ by rounding part company where such a
decision flips, so the inputs are chosen (by seed) such that over the whole truth trajectory min(|re|, |im|), for order 8 also
||re| - |im||, stays >= 1e-4, and the unwrapped phase stays 1e-6 away from +-T.  Order 2 decides nothing about the sample
(error = re im is continuous), so only the wrap margin applies to it.  This is a condition on the inputs, not a tolerance."""
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
F64 = np.float64
ROWS = 16                                   # kCostasRows: rows per wave, one per lane of its first quarter (qdsp_amd/csrc/costas.hip.h)
SLOTS = 64                                  # kCostasSlots: staging instructions per round
WRAP32 = F32(2.0) * F32(3.1415926535)       # 2.0f * FL_M_PI
K32 = np.sqrt(F32(2.0)) - F32(1.0)          # (float)(sqrtf(2.0) - 1)
N = 20_000
MARGIN, WRAP_MARGIN = 1e-4, 1e-6


def chunk_of(rows):
    """Samples per row and round of a wave that holds `rows` (<= 16) rows: 64 S, S the largest power of two with rows S <= 64."""
    assert 1 <= rows <= ROWS
    s = 1
    while rows * s * 2 <= SLOTS:
        s *= 2
    return 64 * s


def chunks_of(nchan):
    """The round lengths in a launch of `nchan` rows: full waves of 16 rows, and the last wave's."""
    return sorted({chunk_of(min(nchan, ROWS)), chunk_of(nchan % ROWS or ROWS)})


# ---- alpha, beta --------------------------------------------------------------------------------------------------------------
def costas_gains(bw):
    """pll.h:20-23: dampningFactor, alpha and beta are floats; the denominator is summed in double and rounded to float."""
    bw = F32(bw)
    damp = np.sqrt(F32(2.0)) / F32(2.0)
    with np.errstate(all="ignore"):
        den = F32(F64(1.0) + F64(2.0) * F64(damp) * F64(bw) + F64(bw * bw))
        alpha = (F32(4) * damp * bw) / den
        beta = (F32(4) * bw * bw) / den
    return F32(alpha), F32(beta)


def _columns(x):
    x = np.asarray(x, np.complex64)
    ncol = int(np.prod(x.shape[1:], dtype=np.int64))
    return x.reshape(len(x), ncol), x.shape


def _per_column(v, dtype, ncol):
    return np.broadcast_to(np.asarray(v, dtype), (ncol,)).copy()


def _error(order, ore, oim, K):
    """The three detectors on arrays, selected per column by `order`; operations in the arrays' own precision."""
    a = np.where(ore > 0, oim, -oim)            # DSP_STEP(re) * im
    b = np.where(oim > 0, ore, -ore)            # DSP_STEP(im) * re
    e8 = np.where(np.abs(ore) >= np.abs(oim), a - b * K, a * K - b)
    return np.where(order == 2, ore * oim, np.where(order == 4, a - b, e8))


# ---- the truth ------------------------------------------------------------------------------------------------------------------
def costas_truth(x, order, alpha, beta, freq=0.0, phase=0.0):
    """The recurrence on the float alpha, beta and samples, sequential in np.longdouble, decisions exact.  x: (n,) or (n, k), every
    column on its own; order, alpha, beta, freq, phase scalars or one value per column.  Returns a dict: yr, yi (n, k) longdouble,
    freq, phase (k,) after the last sample, and what the trajectory did per column: margin (min over samples of min(|re|, |im|) and,
    order 8, ||re| - |im||), wrap_margin (min | |unwrapped phase| - T |), wraps_up / wraps_down, e_clamped, f_clamped (counts)."""
    xc, shape = _columns(x)
    n, k = xc.shape
    order = _per_column(order, np.int64, k)
    al, be = (_per_column(np.asarray(v, F32), LD, k) for v in (alpha, beta))
    f, p = _per_column(freq, LD, k), _per_column(phase, LD, k)
    T, K = LD(WRAP32), LD(K32)
    xr, xi = xc.real.astype(LD), xc.imag.astype(LD)
    yr, yi = np.empty((n, k), LD), np.empty((n, k), LD)
    margin, wmargin = np.full(k, np.inf), np.full(k, np.inf)
    up, down, ecl, fcl = (np.zeros(k, np.int64) for _ in range(4))
    one = LD(1)
    with np.errstate(all="ignore"):
        for i in range(n):
            vre, vim = np.cos(p), -np.sin(p)
            ore = vre * xr[i] - vim * xi[i]
            oim = vim * xr[i] + vre * xi[i]
            yr[i], yi[i] = ore, oim
            m = np.minimum(np.abs(ore), np.abs(oim))
            m = np.where(order == 8, np.minimum(m, np.abs(np.abs(ore) - np.abs(oim))), m)
            margin = np.minimum(margin, np.where(order == 2, np.inf, m).astype(F64))
            e = _error(order, ore, oim, K)
            ecl += np.abs(e) > one
            e = np.clip(e, -one, one)
            f = f + be * e
            fcl += np.abs(f) > one
            f = np.clip(f, -one, one)
            p = p + (f + al * e)
            wmargin = np.minimum(wmargin, np.abs(np.abs(p) - T).astype(F64))
            hi, lo = p > T, p < -T
            up += hi
            down += lo
            p = np.where(hi, p - T, np.where(lo, p + T, p))
    tail = shape[1:]
    r = dict(yr=yr.reshape((n,) + tail), yi=yi.reshape((n,) + tail), freq=f, phase=p, margin=margin, wrap_margin=wmargin, wraps_up=up,
             wraps_down=down, e_clamped=ecl, f_clamped=fcl)
    return r


# ---- the reference's float loop ---------------------------------------------------------------------------------------------------
def costas_ref(x, order, alpha, beta, freq=0.0, phase=0.0):
    """CostasLoop::run over one call in float32, every product and sum rounded separately; lastVCO = float32 of the FP64 cosine and
    sine of the phase (libm's cosf / sinf differ from that in the last bit now and then: test_ref_against_the_cpp_restatement).
    Returns (outputs complex64, freq float32 (k,), phase float32 (k,))."""
    xc, shape = _columns(x)
    n, k = xc.shape
    order = _per_column(order, np.int64, k)
    al, be, f, p = (_per_column(v, F32, k) for v in (alpha, beta, freq, phase))
    xr, xi = np.ascontiguousarray(xc.real), np.ascontiguousarray(xc.imag)
    yr, yi = np.empty_like(xr), np.empty_like(xi)
    one = F32(1)
    with np.errstate(all="ignore"):
        for i in range(n):
            vre, vim = np.cos(-p.astype(F64)).astype(F32), np.sin(-p.astype(F64)).astype(F32)
            ore = (vre * xr[i]) - (vim * xi[i])
            oim = (vim * xr[i]) + (vre * xi[i])
            yr[i], yi[i] = ore, oim
            e = _error(order, ore, oim, K32)
            e = np.where(e > one, one, np.where(e < -one, -one, e))
            f = f + be * e
            f = np.where(f > one, one, np.where(f < -one, -one, f))
            p = p + (f + (al * e))
            for _ in range(3):                  # the reference's while: |phase| < 3 T here
                p = np.where(p > WRAP32, p - WRAP32, p)
                p = np.where(p < -WRAP32, p + WRAP32, p)
    y = np.empty(xc.shape, np.complex64)
    y.real, y.imag = yr, yi
    return y.reshape(shape), f, p


def _same_bits(a, b):
    """Equal as float32 bit patterns (complex64: both components), any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if np.iscomplexobj(a) or np.iscomplexobj(b):
        a = np.ascontiguousarray(a, np.complex64).view(F32)
        b = np.ascontiguousarray(b, np.complex64).view(F32)
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def deviation(y, truth, col=None):
    """max |y - truth| over both components (of column `col`)."""
    y = np.asarray(y, np.complex64)
    yr, yi = truth["yr"], truth["yi"]
    if col is not None:
        yr, yi = yr[:, col], yi[:, col]
    if len(y) == 0:
        return 0.0
    return float(max(np.max(np.abs(y.real.astype(LD) - yr)), np.max(np.abs(y.imag.astype(LD) - yi))))


# ---- the cases --------------------------------------------------------------------------------------------------------------------
# name: (order, loop bandwidth, carrier offset rad / sample, noise sigma per component, amplitude, samples per symbol, phase at 0, seed)
CASES = {
    "locked2": (2, 0.004, 0.002, 0.02, 1.0, 1, 0.3, 1),
    "locked4": (4, 0.004, 0.002, 0.03, 1.0, 1, 0.3, 2),
    "locked8": (8, 0.004, 0.002, 0.02, 1.0, 1, 0.1, 3),
    "pull_in2": (2, 0.004, -0.006, 0.05, 1.0, 1, 0.5, 4),
    "pull_in4": (4, 0.004, -0.006, 0.03, 1.0, 1, 0.5, 5),
    "pull_in8": (8, 0.004, -0.004, 0.02, 1.0, 1, 0.2, 6),
    "wide4": (4, 0.05, 0.05, 0.03, 1.0, 1, 0.0, 7),
    "noisy4": (4, 0.004, 0.0, 0.3, 1.0, 1, 0.2, 8),
    "slow_pull_in8": (8, 0.004, 0.02, 0.03, 1.0, 1, 0.0, 22),
    "freq_clamp2": (2, 1.0, 0.9, 0.02, 1.0, 1, 0.0, 10),
    "error_clamp4": (4, 0.004, 0.002, 0.03, 3.0, 1, 0.4, 11),
    "sps4_4": (4, 0.004, 0.002, 0.03, 1.0, 4, 0.3, 12),
}


def make_case(name, n=N):
    order, bw, off, sigma, amp, sps, ph0, seed = CASES[name]
    rng = np.random.default_rng(1000 + seed)
    nsym = -(-n // sps)
    k = rng.integers(0, order, nsym)
    first = {2: 0.0, 4: np.pi / 4, 8: np.pi / 8}[order]         # where the order's detector is zero
    sym = np.repeat(np.exp(1j * (first + 2 * np.pi * k / order)), sps)[:n]
    t = np.arange(n, dtype=F64)
    noise = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return (amp * sym * np.exp(1j * (off * t + ph0)) + noise).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def case_table():
    """Every case as one column: names, x (N, 12) complex64, orders, bandwidths, alpha, beta, the truth, the float loop's outputs and
    final state, and e_ref[k] = max |costas_ref - truth| of column k.  The two sequential loops run once over all columns."""
    names = list(CASES)
    x = np.stack([make_case(c) for c in names], axis=1)
    order = np.asarray([CASES[c][0] for c in names])
    bw = np.asarray([CASES[c][1] for c in names], F32)
    ab = np.asarray([costas_gains(b) for b in bw], F32)
    truth = costas_truth(x, order, ab[:, 0], ab[:, 1])
    ref, fref, pref = costas_ref(x, order, ab[:, 0], ab[:, 1])
    e_ref = np.asarray([deviation(ref[:, k], truth, k) for k in range(len(names))])
    return dict(names=names, x=x, order=order, bw=bw, alpha=ab[:, 0], beta=ab[:, 1], truth=truth, ref=ref, fref=fref, pref=pref, e_ref=e_ref)


def test_gains_follow_the_reference_formula():
    a, b = costas_gains(0.004)
    d = np.sqrt(2.0) / 2.0
    den = 1 + 2 * d * 0.004 + 0.004 ** 2
    assert abs(float(a) / (4 * d * 0.004 / den) - 1) < 1e-6 and abs(float(b) / (4 * 0.004 ** 2 / den) - 1) < 1e-6      # (0.004f is 1e-7 off)
    assert a.dtype == F32 and b.dtype == F32
    assert max(float(costas_gains(w)[0]) for w in np.linspace(0, 50, 5001)) < 0.83        # |freq + alpha e| < 1.83 < 2 pi
    assert float(WRAP32) == 6.2831854820251465 and float(K32) == 0.41421353816986083984375
    assert [chunk_of(r) for r in (1, 2, 3, 4, 5, 8, 9, 15, 16)] == [4096, 2048, 1024, 1024, 512, 512, 256, 256, 256]
    assert chunks_of(1) == [4096] and chunks_of(64) == [256] and chunks_of(65) == [256, 4096] and chunks_of(130) == [256, 2048]


def test_cases_hold_the_decision_margin_and_do_what_they_are_there_for():
    t = case_table()
    tr, names = t["truth"], t["names"]
    col = {c: names.index(c) for c in names}
    print("margin", dict(zip(names, tr["margin"])), "wrap margin", dict(zip(names, tr["wrap_margin"])))
    print("e_ref", dict(zip(names, t["e_ref"])))
    assert np.all(tr["margin"] >= MARGIN), dict(zip(names, tr["margin"]))
    assert np.all(tr["wrap_margin"] >= WRAP_MARGIN), dict(zip(names, tr["wrap_margin"]))
    # the float loop stays far inside the margin
    assert np.all(t["e_ref"] < 1e-5) and np.all(t["e_ref"] > 1e-8), t["e_ref"]

    def on_constellation(c, lo, hi):
        """rms over samples [lo, hi) of the de-rotated samples' phase error against the nearest constellation point."""
        k = col[c]
        order = CASES[c][0]
        y = (tr["yr"][lo:hi, k] + 1j * tr["yi"][lo:hi, k]).astype(np.complex128)
        first = {2: 0.0, 4: np.pi / 4, 8: np.pi / 8}[order]
        resid = np.angle((y * np.exp(-1j * first)) ** order) / order
        return float(np.sqrt(np.mean(resid ** 2))) < 0.25 / np.sqrt(order) * (1 + 10 * CASES[c][3])

    def locked(c):
        """At the end the loop's frequency is the carrier offset and the last 2000 de-rotated samples sit on the constellation."""
        return abs(float(tr["freq"][col[c]]) - CASES[c][2]) < 2e-3 and on_constellation(c, N - 2000, N)

    for c in ("locked2", "locked4", "locked8", "pull_in2", "pull_in4", "pull_in8", "wide4", "sps4_4", "error_clamp4", "noisy4"):
        assert locked(c), c
    for c in ("locked2", "locked4", "locked8"):
        assert on_constellation(c, 1000, 3000), c
    for o in (2, 4, 8):
        assert tr["wraps_up"][col[f"locked{o}"]] >= 3 and tr["wraps_down"][col[f"locked{o}"]] == 0, o
        assert tr["wraps_down"][col[f"pull_in{o}"]] >= 3, o
    # bandwidth 0.004 against an offset of 0.02.  A second-order loop with a perfect integrator has no pull-in limit, only a
    # pull-in time, about offset^2 / (2 zeta bw^3) = 4400 samples: the order-8 loop slips cycles for some 6000 samples (the case
    # is there for that: an unlocked loop's decisions) and is locked at the end of the 20 000.
    assert not on_constellation("slow_pull_in8", 500, 4500) and locked("slow_pull_in8")
    print({c: (int(tr["wraps_up"][k]), int(tr["wraps_down"][k]), int(tr["e_clamped"][k]), int(tr["f_clamped"][k])) for c, k in col.items()})
    assert tr["f_clamped"][col["freq_clamp2"]] >= 10
    assert tr["e_clamped"][col["error_clamp4"]] > 10
    assert tr["wraps_up"][col["wide4"]] > 100


# ---- the float loop against a C++ restatement that calls cosf / sinf ---------------------------------------------------------
_CHECK_SRC = r"""
// A float32 Costas loop for tests/test_costas_cpu.py, written for this test: the arithmetic of costas_ref, operation by operation,
// with libm's cosf / sinf for the oscillator.  argv: in.bin out.bin order bandwidth cut
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static const float TWO_PI_F = 2.0f * 3.1415926535f;

struct State {
    float a, b;             // proportional and integral coefficients
    float w = 0.0f;         // frequency
    float th = 0.0f;        // phase
    float c = 1.0f;         // oscillator = (cos(-th), sin(-th))
    float s = 0.0f;
};

static float sgn(float v) { return v > 0.0f ? 1.0f : -1.0f; }

static float detect(int order, float re, float im) {
    if (order == 2) return re * im;
    const float p = sgn(re) * im, q = sgn(im) * re;
    if (order == 4) return p - q;
    const float k = sqrtf(2.0f) - 1.0f;
    return fabsf(re) >= fabsf(im) ? p - q * k : p * k - q;
}

static float limit1(float v) { return v > 1.0f ? 1.0f : (v < -1.0f ? -1.0f : v); }

static void advance(State& z, int order, const float* x, float* y, int n) {
    for (int i = 0; i < n; i++) {
        const float xr = x[2 * i], xi = x[2 * i + 1];
        const float re = z.c * xr - z.s * xi;
        const float im = z.s * xr + z.c * xi;
        y[2 * i] = re;
        y[2 * i + 1] = im;
        const float e = limit1(detect(order, re, im));
        z.w = limit1(z.w + z.b * e);
        z.th = z.th + (z.w + z.a * e);
        while (z.th > TWO_PI_F) z.th -= TWO_PI_F;
        while (z.th < -TWO_PI_F) z.th += TWO_PI_F;
        z.c = cosf(-z.th);
        z.s = sinf(-z.th);
    }
}

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    std::vector<float> x;
    FILE* f = fopen(argv[1], "rb");
    float v[2];
    while (fread(v, sizeof(float), 2, f) == 2) { x.push_back(v[0]); x.push_back(v[1]); }
    fclose(f);
    const int n = (int)(x.size() / 2), order = atoi(argv[3]), cut = atoi(argv[5]);
    const float bw = (float)atof(argv[4]);
    State z;
    const float zeta = sqrtf(2.0f) / 2.0f;
    const float den = (float)(1.0 + 2.0 * (double)zeta * (double)bw + (double)(bw * bw));   // summed in double, kept as float
    z.a = (4.0f * zeta * bw) / den;
    z.b = (4.0f * bw * bw) / den;
    std::vector<float> y(x.size());
    advance(z, order, x.data(), y.data(), cut);                            // two calls: the state carries over
    advance(z, order, x.data() + 2 * cut, y.data() + 2 * cut, n - cut);
    const float st[4] = {z.a, z.b, z.w, z.th};
    FILE* o = fopen(argv[2], "wb");
    fwrite(y.data(), sizeof(float), y.size(), o);
    fwrite(st, sizeof(float), 4, o);
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def cpp_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("costasref")
    (d / "c.cpp").write_text(_CHECK_SRC)
    exe = d / "c"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", str(d / "c.cpp"), "-o", str(exe)])

    def run(x, order, bw, cut=0):
        np.asarray(x, np.complex64).tofile(d / "x.bin")
        subprocess.check_call([str(exe), str(d / "x.bin"), str(d / "y.bin"), str(int(order)), repr(float(F32(bw))), str(int(cut))])
        raw = np.fromfile(d / "y.bin", dtype=F32)
        return raw[:-4].view(np.complex64), raw[-4:]

    return run


def test_ref_against_the_cpp_restatement(cpp_check):
    """The two float loops differ only in the last bit of the cosine and sine (float32 of the FP64 value against libm's cosf /
    sinf), so they cannot be bit-identical over 20 000 samples.  Per case: |ref - cpp| <= the sum of the two loops' own deviations
    from the truth (sample by sample and as maxima), each loop is within 4 x the other's deviation (two such loops stood up to
    1.8 x apart), alpha and beta are the same floats, and the first outputs, before any rounding has been fed back, are the
    same bits."""
    t = case_table()
    for k, c in enumerate(t["names"]):
        order, bw = CASES[c][0], CASES[c][1]
        y, st = cpp_check(t["x"][:, k], order, bw, cut=N // 3)
        assert _same_bits(st[:2], [t["alpha"][k], t["beta"][k]]), c
        assert _same_bits(y[:1], t["ref"][:1, k]), c
        tr = t["truth"]
        truth = (tr["yr"][:, k] + 1j * tr["yi"][:, k])
        d_ref = np.abs(t["ref"][:, k].astype(np.clongdouble) - truth)
        d_cpp = np.abs(y.astype(np.clongdouble) - truth)
        delta = np.abs(y.astype(np.clongdouble) - t["ref"][:, k].astype(np.clongdouble))
        assert np.all(delta <= (d_ref + d_cpp) * (1 + 1e-12)), c
        e_cpp, e_ref = deviation(y, tr, k), t["e_ref"][k]
        print(f"{c}: max |ref - truth| {e_ref:.3g}, max |cpp - truth| {e_cpp:.3g}, max |ref - cpp| {float(np.max(delta)):.3g}")
        assert float(np.max(delta)) <= e_ref + e_cpp and e_cpp <= 4 * e_ref and e_ref <= 4 * e_cpp, c
        assert abs(float(st[2]) - float(t["fref"][k])) <= 1e-5 and abs(float(st[3]) - float(t["pref"][k])) <= 1e-4, c


def test_ref_and_truth_columns_are_independent_and_carry_their_state():
    t = case_table()
    for k in (0, 5, 9):
        x, o, a, b = t["x"][:3000, k], t["order"][k], t["alpha"][k], t["beta"][k]
        y, f, p = costas_ref(x, o, a, b)
        assert _same_bits(y, t["ref"][:3000, k])
        y1, f1, p1 = costas_ref(x[:1000], o, a, b)
        y2, f2, p2 = costas_ref(x[1000:], o, a, b, f1, p1)
        assert _same_bits(np.concatenate([y1, y2]), y) and _same_bits([f2[0], p2[0]], [f[0], p[0]])
        tr = costas_truth(x, o, a, b)
        t1 = costas_truth(x[:1000], o, a, b)
        t2 = costas_truth(x[1000:], o, a, b, t1["freq"], t1["phase"])
        assert np.array_equal(np.concatenate([t1["yr"], t2["yr"]]), tr["yr"]) and t2["phase"][0] == tr["phase"][0]
        assert np.array_equal(tr["yr"], t["truth"]["yr"][:3000, k])
    e = costas_truth(t["x"][:0, 0], 2, 0.1, 0.1, 0.25, -0.5)
    assert e["freq"][0] == LD(0.25) and e["phase"][0] == LD(-0.5) and e["yr"].shape == (0,)


# ---- the C ABI and the mirror ---------------------------------------------------------------------------------------------------
COSTAS_SYMBOLS = ["qdsp_hip_costas_" + s for s in (
    "create", "set_bandwidth", "get_gains", "get_state", "set_state", "process", "process_ex", "process_dev", "process_batch_dev", "reset",
    "destroy")]


def test_costas_symbols_declared_and_exported():
    declared = set(capi.declared_symbols())
    assert set(COSTAS_SYMBOLS) <= declared, sorted(set(COSTAS_SYMBOLS) - declared)
    L = capi.load()
    assert all(hasattr(L, s) for s in COSTAS_SYMBOLS)
    assert all(getattr(L, s).argtypes is not None for s in COSTAS_SYMBOLS), "declared in capi.py"
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(COSTAS_SYMBOLS) <= exported
    assert L.qdsp_hip_abi_version() == 1


def test_ops_costas_loop_surface():
    from qdsp_amd import ops

    for name in ("process", "process_batch", "set_bandwidth", "get_state", "set_state", "reset", "gains", "time_dev", "last_kernel",
                 "set_done_event", "process_ex"):
        assert callable(getattr(ops.CostasLoop, name)), name
    assert "CostasLoop" in ops.__all__


_SURFACE_SRC = r"""
#include <type_traits>
#include "dsp/processing.h"
#include "dsp/pll.h"
using namespace dsp;
static_assert(std::is_same<decltype(CostasLoop<4>::out), stream<complex_t>>::value, "CostasLoop::out");
static_assert(std::is_base_of<detail::hip_block<complex_t, complex_t>, CostasLoop<8>>::value, "the shared base of the HIP-backed blocks");
template <int ORDER> struct Demod {           // demodulator.h:566-682, the members and calls that touch the loop
    void init(stream<complex_t>* input, float agcRate, float costasLoopBw) {
        agc.init(input, 1.0f, 65535, agcRate);
        demod.init(&agc.out, costasLoopBw);
        blocks[0] = &agc; blocks[1] = &demod;
        out = &demod.out;
    }
    void setCostasLoopBw(float costasLoopBw) { demod.setLoopBandwidth(costasLoopBw); }
    ComplexAGC agc;
    CostasLoop<ORDER> demod;
    generic_unnamed_block* blocks[2];
    stream<complex_t>* out = NULL;
};
void use(stream<complex_t>* in) {
    CostasLoop<2> a(in, 0.004f);
    a.setLoopBandwidth(0.01f); a.setInput(in);
    Demod<2> d2; Demod<4> d4; Demod<8> d8;
    d2.init(in, 0.001f, 0.004f); d4.init(in, 0.001f, 0.004f); d8.init(in, 0.001f, 0.004f);
    d8.setCostasLoopBw(0.002f);
}
"""


def test_costas_block_compiles_with_the_reference_usage(tmp_path):
    (tmp_path / "s.cpp").write_text(_SURFACE_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.cpp")])
    src = open(os.path.join(HOST, "dsp", "pll.h")).read() + open(os.path.join(HOST, "dsp", "hip_block.h")).read()    # (the link protocol is the base's)
    for name in ("claimConsumer", "done.arm", "qdsp_hip_costas_process_ex", "qdsp_hip_costas_set_bandwidth"):
        assert name in src, name


def test_build_makes_the_costas_harness():
    assert re.search(r'mode == "costas"', open(os.path.join(HOST, "examples", "demod_check.cpp")).read())
    subprocess.check_call(["make", "-C", HOST, "build/demod_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "demod_check")
    assert os.access(exe, os.X_OK)
    out = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    assert "qdsp_hip_costas_process_ex" in out and "qdsp_hip_costas_create" in out
