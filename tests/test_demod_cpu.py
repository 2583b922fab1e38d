"""The demodulators (src/dsp/demodulator.h: FloatFMDemod, FMDemod, AMDemod, SSBDemod) without a GPU: the C ABI exports them,
the C++ block mirror carries the reference's names, build() makes the graph harness -- and the numpy float32 restatement of
the FM and AM arithmetic that the GPU tests compare against is pinned, bit for bit, to the C++ host code it restates
(complex_t::fastPhase of qdsp_amd/host/dsp/types.h, the FM loop of demodulator.h:86-95, VOLK's generic magnitude)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from qdsp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")

PI = np.float32(3.1415926535)          # FL_M_PI, and the literal of the wrap (demodulator.h:89-90)
TWO_PI = np.float32(2) * PI
C1 = PI / np.float32(4)                 # FAST_ATAN2_COEF1
C2 = np.float32(np.float32(3) * PI) / np.float32(4)   # FAST_ATAN2_COEF2 = 3.0f * FL_M_PI / 4.0f


# ---- the restatement (float32 throughout; each numpy operation is one correctly rounded IEEE operation) -------------------
def fast_arctan2(y, x):
    """fast_arctan2 (demodulator.h:14-30) over arrays."""
    y = np.asarray(y, np.float32)
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        ay = np.abs(y)
        right = x >= 0
        r = np.where(right, (x - ay) / (x + ay), (x + ay) / (ay - x)).astype(np.float32)
        angle = np.where(right, C1, C2).astype(np.float32) - (C1 * r).astype(np.float32)
        angle = np.where(y < 0, -angle, angle)
        return np.where((x == 0) & (y == 0), np.float32(0), angle).astype(np.float32)


def phasor_speed(sample_rate, deviation):
    """(2 * FL_M_PI) / (sampleRate / deviation) in float (FloatFMDemod::init)."""
    return np.float32(TWO_PI / np.float32(np.float32(sample_rate) / np.float32(deviation)))


def fm_ref(x, speed, phase=np.float32(0)):
    """FloatFMDemod::run over one call: (outputs, carried phase)."""
    x = np.asarray(x, np.complex64)
    cp = fast_arctan2(x.imag, x.real)
    prev = np.concatenate([np.asarray([phase], np.float32), cp[:-1]])
    with np.errstate(all="ignore"):
        d = (cp - prev).astype(np.float32)
        d = np.where(d > PI, d - TWO_PI, np.where(d <= -PI, d + TWO_PI, d)).astype(np.float32)
        out = (d / np.float32(speed)).astype(np.float32)
    return out, (cp[-1] if len(cp) else np.float32(phase))


def am_mag(x):
    """volk_32fc_magnitude_32f, generic: sqrtf(re*re + im*im), every operation rounded."""
    x = np.asarray(x, np.complex64)
    re, im = x.real, x.imag
    with np.errstate(all="ignore"):
        return np.sqrt((re * re) + (im * im)).astype(np.float32)


def am_ref(x):
    """AMDemod::run with the mean taken in FP64 and rounded once: (outputs, avg)."""
    m = am_mag(x)
    avg = np.float32(np.sum(m.astype(np.float64)) / len(m)) if len(m) else np.float32(0)
    return (m - avg).astype(np.float32), avg


def fm_ref_rows(x, speeds, phases=None):
    """fm_ref over the rows of a batch, row c with its own phasorSpeed and carried phase: (outputs, carried phases)."""
    x = np.asarray(x, np.complex64)
    speeds = np.asarray(speeds, np.float32).reshape(-1, 1)
    phases = np.zeros(len(x), np.float32) if phases is None else np.asarray(phases, np.float32)
    cp = fast_arctan2(x.imag, x.real)
    prev = np.concatenate([phases.reshape(-1, 1), cp[:, :-1]], axis=1)
    with np.errstate(all="ignore"):
        d = (cp - prev).astype(np.float32)
        d = np.where(d > PI, d - TWO_PI, np.where(d <= -PI, d + TWO_PI, d)).astype(np.float32)
        out = (d / speeds).astype(np.float32)
    return out, (cp[:, -1].copy() if x.shape[1] else phases.copy())


def phasor_speeds(sample_rate, deviations):
    """phasor_speed for an array of deviations."""
    return (TWO_PI / (np.float32(sample_rate) / np.asarray(deviations, np.float32))).astype(np.float32)


def am_candidates_of_mag(m):
    """What the AM kernels' header allows for a row of magnitudes `m`: m - a in float32 for a = the float32 just below the
    FP64 mean of m (math.fsum: the exact sum, rounded once) and the float32 just above it; one candidate where the mean is
    a float32 itself (or not finite: a NaN or infinite mean poisons the row as it does in the reference).  -> [(a, m - a)]"""
    m = np.asarray(m, np.float32)
    with np.errstate(all="ignore"):
        mu = math.fsum(m.tolist()) / len(m)
        a = np.float32(mu)
        if not np.isfinite(a) or float(a) == mu:
            return [(a, (m - a).astype(np.float32))]
        lo = a if float(a) < mu else np.nextafter(a, np.float32(-np.inf))
        hi = np.nextafter(lo, np.float32(np.inf))
        assert float(lo) < mu < float(hi)
        return [(c, (m - c).astype(np.float32)) for c in (lo, hi)]


def am_candidates(x):
    """am_candidates_of_mag of a row of complex samples: |x| is VOLK's generic magnitude, bit for bit."""
    return am_candidates_of_mag(am_mag(x))


def am_row_ok(y, candidates):
    """The whole row `y` has the bits of one candidate (the same mean subtracted from every sample)."""
    return any(_same_bits(y, c) for _, c in candidates)


def am_cancellation_row(n, seed):
    """|x| = 4096 (1 + 2^-12 u), u uniform in [-1, 1], uniform argument: a mean of 4096 under samples that differ from it
    by less than 1, so that m - avg keeps only the low bits of m and a mean that is off by one ulp (2^-12 below 4096) shows everywhere."""
    rng = np.random.default_rng(seed)
    r = 4096.0 * (1.0 + 2.0 ** -12 * rng.uniform(-1.0, 1.0, n))
    return (r * np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, n))).astype(np.complex64)


def am_ref_f32_sequential(x):
    """AMDemod::run with the mean accumulated in one float, sample after sample (what the reference's VOLK accumulator does)."""
    m = am_mag(x)
    avg = np.float32(np.cumsum(m, dtype=np.float32)[-1] / np.float32(len(m)))
    return (m - avg).astype(np.float32), avg


def am_ref_f32_tree(x, parts=1024):
    """... with `parts` float partial sums (each over a contiguous share of the row, sample after sample) added in a pairwise tree."""
    m = am_mag(x)
    share = -(-len(m) // parts)
    padded = np.zeros(parts * share, np.float32)
    padded[:len(m)] = m
    p = np.cumsum(padded.reshape(parts, share), axis=1, dtype=np.float32)[:, -1]
    while len(p) > 1:
        p = (p[0::2] + p[1::2]).astype(np.float32)
    avg = np.float32(p[0] / np.float32(len(m)))
    return (m - avg).astype(np.float32), avg


def edge_vectors():
    """Signed zeros, subnormals, infinities, NaN, magnitudes of 1e+-30, and neighbours whose phases differ by exactly
    +-pi (+-j: fast_arctan2 = +-pi/2 exactly)."""
    v = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, np.inf, -np.inf, np.nan, 1e30, -1e30, 1e-30, -1e-30, 1.0, -1.0, 0.5]
    pairs = [complex(a, b) for a in v for b in v]
    pairs += [1j, -1j, 1j, 1, -1, 1, -1, -1j, 1j, -1j, complex(-1, -0.0), complex(-1, 0.0), complex(-1, -1e-38)]
    return np.asarray(pairs, np.complex64)


def random_vectors(n=1_000_000, seed=7):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    x[::97] *= np.float32(1e-20)
    x[5::89] *= np.float32(1e20)
    return x


# ---- the C ABI and the mirror ---------------------------------------------------------------------------------------------
DEMOD_SYMBOLS = [
    "qdsp_hip_demod_create", "qdsp_hip_demod_set_fm", "qdsp_hip_demod_process", "qdsp_hip_demod_process_ex",
    "qdsp_hip_demod_process_dev", "qdsp_hip_demod_process_batch_dev", "qdsp_hip_demod_get_phase", "qdsp_hip_demod_set_phase",
    "qdsp_hip_demod_reset", "qdsp_hip_demod_destroy",
    "qdsp_hip_ssb_cf32_create", "qdsp_hip_ssb_cf32_process", "qdsp_hip_ssb_cf32_process_dev", "qdsp_hip_ssb_cf32_process_ex",
    "qdsp_hip_ssb_cf32_set_phase_inc", "qdsp_hip_ssb_cf32_get_phase", "qdsp_hip_ssb_cf32_set_phase", "qdsp_hip_ssb_cf32_advance",
    "qdsp_hip_ssb_cf32_set_volk_gain", "qdsp_hip_ssb_cf32_destroy",
]


def test_demod_symbols_declared_and_exported():
    declared = set(capi.declared_symbols())
    assert set(DEMOD_SYMBOLS) <= declared, sorted(set(DEMOD_SYMBOLS) - declared)
    L = capi.load()
    assert all(hasattr(L, s) for s in DEMOD_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(DEMOD_SYMBOLS) <= exported
    hdr = open(capi.HEADER_PATH).read()
    for k, v in (("QDSP_HIP_DEMOD_FM", 0), ("QDSP_HIP_DEMOD_FM_STEREO", 1), ("QDSP_HIP_DEMOD_AM", 2)):
        assert re.search(rf"#define {k}\s+{v}\b", hdr), k
    assert L.qdsp_hip_abi_version() == 1


def test_demodulator_header_keeps_the_reference_surface():
    src = open(os.path.join(HOST, "dsp", "demodulator.h")).read() + open(os.path.join(HOST, "dsp", "hip_block.h")).read()    # (the link protocol is the base's)
    for cls in ("FloatFMDemod", "FMDemod", "AMDemod", "SSBDemod"):
        assert re.search(rf"class {cls}\b", src), cls
    for name in ("init", "setInput", "setSampleRate", "getSampleRate", "setDeviation", "getDeviation", "setBandWidth", "setMode", "run"):
        assert re.search(rf"\b{name}\(", src), name
    for name in ("MODE_USB", "MODE_LSB", "MODE_DSB", "claimConsumer", "done.arm", "qdsp_hip_demod_process_ex", "qdsp_hip_ssb_cf32_process_ex"):
        assert name in src, name
    # graph_check is linked against the fake library of the sanitizer test, which has no demodulator symbols
    assert not re.search(r"#include\s*[<\"]dsp/demodulator\.h", open(os.path.join(HOST, "examples", "graph_check.cpp")).read())


_SURFACE_SRC = r"""
#include <type_traits>
#include "dsp/demodulator.h"
using namespace dsp;
static_assert(std::is_same<decltype(FloatFMDemod::out), stream<float>>::value, "FloatFMDemod::out");
static_assert(std::is_same<decltype(FMDemod::out), stream<stereo_t>>::value, "FMDemod::out");
static_assert(std::is_same<decltype(AMDemod::out), stream<float>>::value, "AMDemod::out");
static_assert(std::is_same<decltype(SSBDemod::out), stream<float>>::value, "SSBDemod::out");
static_assert(SSBDemod::MODE_USB == 0 && SSBDemod::MODE_LSB == 1 && SSBDemod::MODE_DSB == 2, "modes");
void use(stream<complex_t>* in) {
    FloatFMDemod a(in, 250e3f, 75e3f);
    a.setSampleRate(200e3f); a.setDeviation(5e3f); (void)a.getSampleRate(); (void)a.getDeviation(); a.setInput(in);
    FMDemod b;
    b.init(in, 250e3f, 75e3f);
    AMDemod c(in);
    c.setInput(in);
    SSBDemod d(in, 48e3f, 3e3f, SSBDemod::MODE_LSB);
    d.setSampleRate(24e3f); d.setBandWidth(2.7e3f); d.setMode(SSBDemod::MODE_USB); d.setInput(in);
    generic_unnamed_block* blocks[] = {&a, &b, &c, &d};
    (void)blocks;
}
"""


def test_demodulator_blocks_compile_with_the_reference_types(tmp_path):
    (tmp_path / "s.cpp").write_text(_SURFACE_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.cpp")])


def test_build_makes_the_demod_harness():
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert re.search(r"^all:.*build/demod_check", mk, re.M)
    if not os.path.exists(os.path.join(HOST, "build", "demod_check")):
        subprocess.check_call(["make", "-C", HOST, "build/demod_check"], stdout=subprocess.DEVNULL, timeout=300)
    assert os.access(os.path.join(HOST, "build", "demod_check"), os.X_OK)


# ---- the restatement against the C++ it restates --------------------------------------------------------------------------
_CHECK_SRC = r"""
#include <cstdio>
#include <cmath>
#include <vector>
#include "dsp/types.h"
// in: n complex_t; out: fastPhase, the FM loop of demodulator.h:86-95 (phasorSpeed of argv[3] / argv[4]), |x|
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    std::vector<dsp::complex_t> x;
    dsp::complex_t v;
    while (fread(&v, sizeof(v), 1, f) == 1) x.push_back(v);
    fclose(f);
    const float sr = (float)atof(argv[3]), dev = (float)atof(argv[4]);
    const float phasorSpeed = (2 * FL_M_PI) / (sr / dev);
    std::vector<float> cp(x.size()), fm(x.size()), mag(x.size());
    float phase = 0, diff, currentPhase;
    for (size_t i = 0; i < x.size(); i++) {
        cp[i] = x[i].fastPhase();
        currentPhase = cp[i];
        diff = currentPhase - phase;
        if (diff > 3.1415926535f)        { diff -= 2 * 3.1415926535f; }
        else if (diff <= -3.1415926535f) { diff += 2 * 3.1415926535f; }
        fm[i] = diff / phasorSpeed;
        phase = currentPhase;
        mag[i] = sqrtf(x[i].re * x[i].re + x[i].im * x[i].im);
    }
    FILE* o = fopen(argv[2], "wb");
    fwrite(cp.data(), 4, cp.size(), o);
    fwrite(fm.data(), 4, fm.size(), o);
    fwrite(mag.data(), 4, mag.size(), o);
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def cpp_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("demodref")
    (d / "c.cpp").write_text(_CHECK_SRC)
    exe = d / "c"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", HOST, str(d / "c.cpp"), "-o", str(exe)])

    def run(x, sr, dev):
        x.astype(np.complex64).tofile(d / "x.bin")
        subprocess.check_call([str(exe), str(d / "x.bin"), str(d / "y.bin"), repr(float(sr)), repr(float(dev))])
        y = np.fromfile(d / "y.bin", dtype=np.float32).reshape(3, -1)
        return y[0], y[1], y[2]

    return run


def _same_bits(a, b):
    """Equal as float32 bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


@pytest.mark.parametrize("which", ["random", "edges"])
def test_restatement_is_bit_identical_to_the_cpp_reference(cpp_check, which):
    x = random_vectors() if which == "random" else edge_vectors()
    sr, dev = 250_000.0, 75_000.0
    cp, fm, mag = cpp_check(x, sr, dev)
    assert _same_bits(fast_arctan2(x.imag, x.real), cp)
    y, last = fm_ref(x, phasor_speed(sr, dev))
    assert _same_bits(y, fm)
    assert _same_bits([last], [cp[-1]])
    assert _same_bits(am_mag(x), mag)
    # ... and in two calls with the phase carried
    k = len(x) // 3
    y1, p1 = fm_ref(x[:k], phasor_speed(sr, dev))
    y2, _ = fm_ref(x[k:], phasor_speed(sr, dev), p1)
    assert _same_bits(np.concatenate([y1, y2]), fm)


def test_edge_vectors_reach_the_wrap_on_both_sides():
    x = edge_vectors()
    cp = fast_arctan2(x.imag, x.real)
    d = np.diff(cp)
    assert np.any(d == PI) and np.any(d == -PI)
    y, _ = fm_ref(x, np.float32(1))
    assert np.sum(~np.isfinite(y)) > 0


def test_am_restatement():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(10_000) + 1j * rng.standard_normal(10_000)).astype(np.complex64)
    y, avg = am_ref(x)
    m = am_mag(x)
    assert avg == np.float32(np.mean(m.astype(np.float64)))
    assert np.array_equal(y, m - avg)
    assert am_ref(x[:1])[0][0] == 0


# ---- the restatements the GPU edge tests (tests/test_gpu_demod_edges.py) are built on ----------------------------------------
def test_fm_ref_rows_is_fm_ref_row_by_row():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((5, 300)) + 1j * rng.standard_normal((5, 300))).astype(np.complex64)
    x[3, 17] = complex(np.nan, 1.0)
    x[4, 299] = complex(1.0, -np.inf)
    devs = np.asarray([75_000.0, 12_500.0, 3_000.0, 1_001.0, 65_535.0], np.float32)
    sp = phasor_speeds(250_000.0, devs)
    ph = np.asarray([0.0, 1.5, -3.0, 0.25, np.nan], np.float32)
    y, last = fm_ref_rows(x, sp, ph)
    for c in range(5):
        assert _same_bits([sp[c]], [phasor_speed(250_000.0, devs[c])])
        want, p = fm_ref(x[c], sp[c], ph[c])
        assert _same_bits(y[c], want) and _same_bits([last[c]], [p]), c
    y0, last0 = fm_ref_rows(x[:, :0], sp, ph)
    assert y0.shape == (5, 0) and _same_bits(last0, ph)
    assert _same_bits(fm_ref_rows(x, sp)[0][:, 0], fm_ref_rows(x, sp, np.zeros(5))[0][:, 0])


AM_CANCEL_N, AM_CANCEL_SEED = 1_000_003, 9


def test_am_candidates_take_the_fp64_mean_and_refuse_float_accumulators():
    """The candidate rule on the cancellation row: the FP64-mean restatement is one of the candidates; a mean accumulated in
    float32 -- one running sum, or 1024 running sums added as a tree -- is neither.  A float running sum of this row stops
    taking in the samples' offsets from 4096 once it has grown past 2^25, so its mean is off by about the mean of those
    offsets, 1 / sqrt(3 n): of the order of one ulp of 4096 at n = 10^6, not many.  Which draws of the row a float
    accumulator misses on is therefore chance: of seeds 0..15 at this count the running sum misses the candidates on nine
    (by up to 3 ulp) and the 1024-partial tree on two (seeds 9 and 15, by 1 ulp); seed 9 is used because both miss there.
    (A float accumulation that is pairwise all the way down stays within the candidates on this input at these sizes.)"""
    x = am_cancellation_row(AM_CANCEL_N, AM_CANCEL_SEED)
    m = am_mag(x)
    assert 4094.99 < m.min() < 4095.01 and 4096.99 < m.max() < 4097.01
    cands = am_candidates(x)
    assert len(cands) == 2 and np.nextafter(cands[0][0], np.float32(np.inf)) == cands[1][0]
    y, avg = am_ref(x)
    assert am_row_ok(y, cands) and avg in (cands[0][0], cands[1][0])
    assert np.abs(y).max() < 1.01                        # 12 of the 24 significant bits of m are gone in m - avg
    for name, model in (("sequential", am_ref_f32_sequential), ("tree of 1024", am_ref_f32_tree)):
        yf, af = model(x)
        ulps = (float(af) - float(avg)) / float(np.spacing(avg))
        print(f"{name}: mean {af!r}, {ulps:+.0f} ulp from the FP64 mean {avg!r}")
        assert not am_row_ok(yf, cands), name
        assert af not in (cands[0][0], cands[1][0]), name


def test_am_candidates_edges():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(4097) + 1j * rng.standard_normal(4097)).astype(np.complex64)
    # unit noise: the FP64 restatement is a candidate (at every count the GPU tests use below the partials cap)
    for n in (1, 2, 7, 8, 9, 2047, 2048, 2049, 4097):
        y, avg = am_ref(x[:n])
        cands = am_candidates(x[:n])
        assert am_row_ok(y, cands) and any(_same_bits([avg], [a]) for a, _ in cands), n
    # one sample, or a mean that is a float32: one candidate
    assert len(am_candidates(x[:1])) == 1 and not np.any(am_candidates(x[:1])[0][1])
    (a, c), = am_candidates(np.asarray([3 + 4j, 3 + 4j, 6 + 8j, 0], np.complex64))
    assert a == np.float32(5) and np.array_equal(c, np.asarray([0, 0, 5, -5], np.float32))
    # a candidate differs from the other in about every sample, and from a row with a sample off by an ulp
    lo, hi = am_candidates(x)
    assert not am_row_ok(np.where(np.arange(4097) < 2000, lo[1], hi[1]), [lo, hi]), "one mean for the whole row"
    off = lo[1].copy()
    off[4096] = np.nextafter(off[4096], np.float32(9))
    assert not am_row_ok(off, [lo, hi])
    # non-finite: the mean is NaN or infinite, and the row is the reference's
    for bad in (complex(np.nan, 1), complex(1, np.inf), complex(-np.inf, 0)):
        xb = x[:100].copy()
        xb[37] = bad
        (a, c), = am_candidates(xb)
        with np.errstate(all="ignore"):
            assert not np.isfinite(a) and _same_bits(c, am_ref(xb)[0])
        assert np.all(np.isnan(c)) if np.isnan(a) else (np.isnan(c[37]) and np.all(c[np.arange(100) != 37] == -np.inf))
