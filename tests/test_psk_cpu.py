"""RowFir, DelayImag, PSKDemod and MSKDemod without a GPU: the library's surface, the C++ mirror against the reference's usage, the
RRC taps of ops.rrc_taps against the mirror's, psk_check over the real chain code under the sanitizers on a fake library, and the
numpy chain (tests/_psk_ref.py) against the convergence condition the GPU test asserts on the operator."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _psk_ref as P
from qdsp_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "qdsp_amd", "host")
CSRC = os.path.join(ROOT, "qdsp_amd", "csrc")
FAKE = os.path.join(HERE, "fake_hip")

PROCESS = ["process", "process_ex", "process_dev", "process_batch_dev", "reset", "destroy"]
ENTRY = {
    "rowfir": ["create", "set_taps", "ntaps", "get_history", "set_history", "tile", "tap_group"] + PROCESS,
    "delay_imag": ["create", "get_state", "set_state"] + PROCESS,
    "psk": ["create", "stage", "tap_dev", "out_size", "get_counts"] + PROCESS,
    "msk": ["create", "stage", "tap_dev", "out_size", "get_counts"] + PROCESS,
}


# ---- surface ----
@pytest.mark.parametrize("family", sorted(ENTRY))
def test_symbols_declared_and_exported(family):
    want = {f"qdsp_hip_{family}_{n}" for n in ENTRY[family]}
    assert want <= set(capi.declared_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    have = set(re.findall(rf"\bT (qdsp_hip_{family}_\w+)", out))
    assert have == want, (sorted(want - have), sorted(have - want))


def test_stage_constants():
    hdr = open(capi.HEADER_PATH).read()
    for k, v in (("PSK_AGC", 0), ("PSK_RRC", 1), ("PSK_COSTAS", 2), ("PSK_DELAY", 3), ("PSK_CLOCK", 4), ("MSK_FM", 0), ("MSK_CLOCK", 1)):
        assert re.search(rf"#define QDSP_HIP_{k}\s+{v}\b", hdr), k
    assert "BORROWED" in hdr and "never processed on and never destroyed" in hdr


def test_ops_surface():
    from qdsp_amd import ops

    common = ("process", "process_batch", "process_ex", "reset", "last_kernel", "time_dev", "set_done_event")
    for name in common + ("set_taps", "get_history", "set_history", "tile", "tap_group"):
        assert callable(getattr(ops.RowFir, name)), name
    for name in common + ("get_state", "set_state"):
        assert callable(getattr(ops.DelayImag, name)), name
    for cls in (ops.PskDemod, ops.MskDemod):
        for name in common + ("stage", "tap", "out_size", "counts"):
            assert callable(getattr(cls, name)), (cls, name)
    assert (ops.PskDemod.AGC, ops.PskDemod.RRC, ops.PskDemod.COSTAS, ops.PskDemod.DELAY, ops.PskDemod.CLOCK) == (0, 1, 2, 3, 4)
    assert (ops.MskDemod.FM, ops.MskDemod.CLOCK) == (0, 1)
    for name in ("RowFir", "DelayImag", "PskDemod", "MskDemod"):
        assert name in ops.__all__, name


def test_stream_op_takes_the_new_kinds():
    """The kinds of RowFir, DelayImagOp and the chain exist in the one enum of handle kinds, their handles name them, and
    as_stream_op takes every kind of the enum (it asks the table for the address alone); the fourteen kinds' values all differ."""
    hdr = open(os.path.join(CSRC, "stream_op.h")).read()
    src = open(os.path.join(CSRC, "stream_op.cpp")).read()
    enum = re.search(r"enum class OpKind : int \{(.*?)\n\};", hdr, re.S).group(1)
    entries = re.findall(r"^\s*(\w+)(?:\s*=\s*(\d+))?,", enum, re.M)
    values, nxt = {}, 0
    for name, explicit in entries:                      # the values as the compiler counts them
        nxt = int(explicit) if explicit else nxt
        values[name] = nxt
        nxt += 1
    for kind, where in (("RowFir", "rowfir.hip.h"), ("DelayImag", "rowfir.hip.h"), ("Chain", "psk_chain.cpp")):
        assert kind in values, kind
        assert f"static constexpr OpKind kKind = OpKind::{kind};" in open(os.path.join(CSRC, where)).read(), kind
    body = src[src.index("StreamOp* as_stream_op"):src.index("int stream_op_check")]
    assert "lookup(h" in body and "OpKind::" not in body and "->" not in body       # any kind, and h is not read
    assert not re.search(r"k\w+Magic\s*=", hdr) and "magic" not in src
    assert len(values) == len(set(values.values())) == 14 and 0 not in values.values()


# ---- build ----
def test_build_makes_psk_check():
    subprocess.check_call(["make", "-C", HOST, "build/psk_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "psk_check")
    assert os.access(exe, os.X_OK)
    und = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    for name in ("qdsp_hip_psk_create", "qdsp_hip_psk_process_ex", "qdsp_hip_msk_create", "qdsp_hip_msk_process_ex"):
        assert name in und, name
    assert re.search(r"^all:.*\bbuild/psk_check\b", open(os.path.join(HOST, "Makefile")).read(), re.M)
    # none of the older harnesses has come to need the new entry points (they link against the tests' older fake libraries)
    for other in ("graph_check", "demod_check", "clock_check"):
        subprocess.check_call(["make", "-C", HOST, "build/" + other], stdout=subprocess.DEVNULL, timeout=600)
        und = subprocess.check_output(["nm", "-D", "--undefined-only", os.path.join(HOST, "build", other)], text=True)
        assert not re.search(r"qdsp_hip_(rowfir|delay_imag|psk|msk)_", und), other
    # the chain is host code: built without an offload architecture, with no kernel in it
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^psk_chain\.o:.*\n\t(.*)$", mk, re.M).group(1)
    assert "--offload-arch" not in rule
    chain = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "psk_chain.cpp")).read())
    assert "__global__" not in chain and "hipLaunchKernelGGL" not in chain and "<<<" not in chain
    # ... and reaches its stages through the public C ABI
    for name in ("qdsp_hip_cagc_process_batch_dev", "qdsp_hip_rowfir_process_batch_dev", "qdsp_hip_costas_process_batch_dev",
                 "qdsp_hip_delay_imag_process_batch_dev", "qdsp_hip_mmcr_process_batch_dev", "qdsp_hip_demod_process_batch_dev"):
        assert name in chain, name
    assert not re.search(r'#include\s+"(?!stream_op\.h)[a-z_]+\.h(ip\.h)?"', chain), "no stage's private header"


# ---- the mirror ----
_USAGE = r"""
#include <type_traits>
#include <dsp/psk_demod.h>
using namespace dsp;
static_assert(std::is_same<decltype(PSKDemod<4, false>::out), stream<complex_t>*>::value, "PSKDemod::out is a pointer");
static_assert(std::is_same<decltype(MSKDemod::out), stream<float>*>::value, "MSKDemod::out is a pointer");
static_assert(std::is_same<decltype(DelayImag::out), stream<complex_t>>::value, "DelayImag::out");
static_assert(std::is_base_of<detail::hip_block<complex_t, complex_t>, DelayImag>::value, "the shared base of the HIP-backed blocks");
int use(stream<complex_t>* in) {
    PSKDemod<4, false> qpsk(in, 48000.0f, 12000.0f);
    PSKDemod<4, true> oqpsk;
    oqpsk.init(in, 48000.0f, 12000.0f, 31, 0.35f, 1e-3f, 0.004f, 1e-5f, 0.01f, 0.005f);
    qpsk.setInput(in); qpsk.setSampleRate(96000.0f); qpsk.setBaudRate(24000.0f); qpsk.setRRCParams(33, 0.3f); qpsk.setAgcRate(2e-3f);
    qpsk.setCostasLoopBw(0.002f); qpsk.setMMGains(1e-5f, 0.02f); qpsk.setOmegaRelLimit(0.01f);
    qpsk.start(); qpsk.stop();
    stream<complex_t>* a = qpsk.out;
    stream<complex_t>* b = oqpsk.out;
    MSKDemod msk(in, 48000.0f, 6000.0f, 12000.0f, 1e-5f, 0.01f, 0.005f);
    MSKDemod msk2;
    msk2.init(in, 48000.0f, 6000.0f, 12000.0f);
    msk.setSampleRate(96000.0f); msk.setDeviation(3000.0f); msk.setBaudRate(24000.0f, 0.01f); msk.setMMGains(1e-5f, 0.02f);
    msk.setOmegaRelLimit(0.01f); msk.start(); msk.stop();
    stream<float>* c = msk.out;
    DelayImag d(in), d2;
    d2.init(in); d.setInput(in); d.start(); d.stop();
    return a != nullptr && b != nullptr && c != nullptr && d.out.writeBuf != nullptr;
}
"""


def test_mirror_compiles_with_the_reference_usage(tmp_path):
    (tmp_path / "use.cpp").write_text(_USAGE)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "use.cpp")])
    src = open(os.path.join(HOST, "dsp", "psk_demod.h")).read()
    for name in ("class DelayImag", "class PSKDemod", "class MSKDemod", "qdsp_hip_psk_stage", "qdsp_hip_msk_stage"):
        assert name in src, name
    # what is built against the older headers alone needs no new entry point
    for hdr in ("demodulator.h", "processing.h"):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(HOST, "dsp", hdr)).read())
        assert "psk_demod.h" not in text and not re.search(r"qdsp_hip_(rowfir|delay_imag|psk|msk)_", text), hdr


_TAPS_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <dsp/window.h>
int main(int argc, char** argv) {        // <count> <sampleRate> <baudRate> <alpha>: the taps FIR<T>::loadTaps keeps, as raw floats
    const int n = atoi(argv[1]);
    dsp::RRCTaps w(n, (float)atof(argv[2]), (float)atof(argv[3]), (float)atof(argv[4]));
    std::vector<float> t((size_t)n + 1, 0.0f);
    w.createTaps(t.data(), n);
    fwrite(t.data(), sizeof(float), (size_t)n, stdout);
    return 0;
}
"""


def test_rrc_taps_equal_the_mirrors(tmp_path):
    """ops.rrc_taps is what dsp::FIR<complex_t> keeps of dsp::RRCTaps, bit for bit: `count | 1` computed and normalised, the first
    `count` used (so an even count's taps do not sum to 1)."""
    from qdsp_amd import ops

    (tmp_path / "t.cpp").write_text(_TAPS_SRC)
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", HOST, "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "t.cpp")])
    for n, sr, baud, alpha in ((32, 4.0, 1.0, 0.32), (31, 4.0, 1.0, 0.32), (32, 48000.0, 9600.0, 0.35), (361, 3.0, 1.0, 0.32), (25, 4.0, 1.0, 0.5),
                               (1, 4.0, 1.0, 0.32), (32, 50000.0, 10700.0, 1.0)):
        want = np.frombuffer(subprocess.check_output([exe, str(n), repr(sr), repr(baud), repr(alpha)]), np.float32)
        got = ops.rrc_taps(n, sr, baud, alpha)
        assert got.dtype == np.float32 and got.shape == (n,)
        assert got.tobytes() == want.tobytes(), (n, sr, baud, alpha, np.abs(got - want).max())
    odd, even = ops.rrc_taps(33, 4.0, 1.0, 0.32), ops.rrc_taps(32, 4.0, 1.0, 0.32)
    assert even.tobytes() == odd[:32].tobytes() and abs(float(odd.sum()) - 1.0) < 1e-6 and float(even.sum()) < 0.999


# ---- the harness under the sanitizers ----
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_psk_check_is_clean_under_asan_ubsan(tmp_path):
    """psk_check, the real stream_op.cpp and the real psk_chain.cpp with -fsanitize=address,undefined, as one program of its own, on
    the fake HIP runtime, the tests' fake library and fake_mmcr.cpp (all unchanged) and fake_rowfir.cpp.  The fake stages copy, the
    fake clock stage emits every floor(omega)-th sample: every mode and both links run to completion, silently, and hand over the
    expected number of symbols."""
    hip_inc = "/opt/rocm/include"
    if not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("needs the HIP headers")
    out = os.path.join(FAKE, "build", "address_psk")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "psk_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-Wall", "-pthread",
                        "-D__HIP_PLATFORM_AMD__", "-DFAKE_HIP", f"-I{hip_inc}", f"-I{HOST}", f"-I{os.path.join(ROOT, 'include')}", "-o", exe,
                        os.path.join(HOST, "examples", "psk_check.cpp"), os.path.join(CSRC, "stream_op.cpp"), os.path.join(CSRC, "psk_chain.cpp"),
                        os.path.join(FAKE, "fake_hip_runtime.cpp"), os.path.join(FAKE, "fake_qdsp_hip.cpp"), os.path.join(FAKE, "fake_mmcr.cpp"),
                        os.path.join(FAKE, "fake_rowfir.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    n = 20_000
    x = np.arange(n, dtype=np.float32)
    (x - 1j * x).astype(np.complex64).tofile(tmp_path / "x.cf32")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1 exitcode=68")
    for mode, dt in (("psk2", np.complex64), ("psk4", np.complex64), ("psk8", np.complex64), ("oqpsk", np.complex64), ("msk", np.float32)):
        for link in ("dev", "host"):
            for block, sr, baud in ((4096, "43", "10"), (5, "2", "1"), (3, "10.7", "1")):
                y = tmp_path / f"y_{mode}_{link}.bin"
                p = subprocess.run([exe, mode, link, "x.cf32", str(y), str(block), sr, baud], cwd=tmp_path, env=env, capture_output=True, text=True,
                                   timeout=300)
                bad = [ln for ln in p.stderr.splitlines() if any(k in ln for k in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:"))]
                assert p.returncode == 0 and not bad and "graph ok" in p.stdout, (mode, link, block, p.stderr[-3000:])
                step = int(np.float32(sr) / np.float32(baud))
                assert len(np.fromfile(y, dtype=dt)) == len(range(0, n, step)), (mode, link, block, sr)


def test_create_that_fails_half_way_leaves_nothing(tmp_path):
    """The chain's creates over the fake runtime, whose n-th hipMalloc can be made to fail: for every n until a create succeeds,
    the failing create returns an error, a null handle and everything it had allocated (the runtime counts what is live)."""
    hip_inc = "/opt/rocm/include"
    if shutil.which("g++") is None or not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("needs g++ and the HIP headers")
    (tmp_path / "t.cpp").write_text(r"""
#include <cstdio>
#include <qdsp_hip.h>
extern "C" int fake_hip_live(void);
extern "C" void fake_hip_fail_malloc(int nth);
int main() {
    const float taps[3] = {0.25f, 0.5f, 0.25f};
    for (int kind = 0; kind < 3; kind++) {
        int n = 1;
        for (;; n++) {
            if (n > 200) { printf("kind %d never succeeded\n", kind); return 1; }
            void* h = (void*)16;
            fake_hip_fail_malloc(n);
            const int rc = kind == 2 ? qdsp_hip_msk_create(&h, 0, 1, 64, 48000.0f, 6000.0f, 4.0f, 2.5e-5f, 0.01f, 0.005f)
                                     : qdsp_hip_psk_create(&h, 0, 4, kind, 1, 64, taps, 3, 1e-3f, 0.004f, 4.0f, 2.5e-5f, 0.01f, 0.005f);
            fake_hip_fail_malloc(0);
            if (rc == 0) {
                if (!h) { printf("kind %d: success without a handle\n", kind); return 1; }
                if (kind == 2) qdsp_hip_msk_destroy(h); else qdsp_hip_psk_destroy(h);
                if (fake_hip_live() != 0) { printf("kind %d: %d live after destroy\n", kind, fake_hip_live()); return 1; }
                break;
            }
            if (h || fake_hip_live() != 0) { printf("kind %d, malloc %d: rc %d handle %p live %d\n", kind, n, rc, h, fake_hip_live()); return 1; }
        }
        printf("kind %d: %d failing creates\n", kind, n - 1);
        if (n < 4) { printf("kind %d: too few allocations seen\n", kind); return 1; }
    }
    void* bad = (void*)16;
    if (qdsp_hip_psk_create(&bad, 0, 4, 0, 1, 64, taps, 3, 1e-3f, 0.004f, 0.5f, 2.5e-5f, 0.01f, 0.005f) == 0 || bad || fake_hip_live() != 0) {
        printf("a refused symbol period left something\n"); return 1;
    }
    puts("ok");
    return 0;
}
""")
    exe = str(tmp_path / "t")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-pthread", "-D__HIP_PLATFORM_AMD__", "-DFAKE_HIP",
                        f"-I{hip_inc}", f"-I{os.path.join(ROOT, 'include')}", "-o", exe, str(tmp_path / "t.cpp"), os.path.join(CSRC, "stream_op.cpp"),
                        os.path.join(CSRC, "psk_chain.cpp"), os.path.join(FAKE, "fake_hip_runtime.cpp"), os.path.join(FAKE, "fake_qdsp_hip.cpp"),
                        os.path.join(FAKE, "fake_mmcr.cpp"), os.path.join(FAKE, "fake_rowfir.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="halt_on_error=1 exitcode=68"))
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout[-2000:], p.stderr[-3000:])


# ---- the definitions ----
def test_delay_imag_ref_does_not_depend_on_the_cuts():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(300) + 1j * rng.standard_normal(300)).astype(np.complex64)
    x[17] = complex(np.nan, -0.0)
    x[18] = complex(-0.0, np.inf)
    whole, last = P.delay_imag_ref(x)
    assert whole.real.tobytes() == x.real.tobytes() and whole.imag[1:].tobytes() == x.imag[:-1].tobytes()
    assert whole.imag[0] == 0 and not np.signbit(whole.imag[0]) and last.tobytes() == x.imag[-1].tobytes()
    for cut in (1, 2, 7, 299):
        st, parts = 0.0, []
        for i in range(0, len(x), cut):
            y, st = P.delay_imag_ref(x[i:i + cut], st)
            parts.append(y)
        assert np.concatenate(parts).tobytes() == whole.tobytes() and np.float32(st).tobytes() == last.tobytes(), cut
    y, st = P.delay_imag_ref(x[:0], np.float32(2.5))
    assert len(y) == 0 and st == np.float32(2.5)


@pytest.mark.parametrize("ntaps", [31, 32])
@pytest.mark.parametrize("order", [4, 2])
def test_numpy_chain_meets_the_convergence_condition(order, ntaps):
    """The condition of tests/test_gpu_psk.py's convergence test on the reference's own float loops (cagc_ref, the k-ordered FIR,
    costas_ref, mm_ref): 6000 symbols at 4 samples per symbol, RMS 0.05, a carrier of 2e-3 rad per sample, a fractional timing
    offset, noise at 0.05 of the RMS, default loop parameters.  Every decision over the second half less the last 250 symbols
    equals the sent symbol for one rotation and one delay, and the loop's frequency ends within 5e-4 of the carrier."""
    from qdsp_amd import ops

    x, sent = P.psk_signal(order, 6000)
    assert abs(float(np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2))) - 0.05) < 0.05 * 0.01
    y, freq, _ = P.psk_chain_ref(x, order, False, ops.rrc_taps(ntaps, 4.0, 1.0, 0.32))
    ok, rep = P.converged(y, freq, sent, order)
    print(order, ntaps, rep)
    assert rep["compared"] == 2750 and ok, rep
