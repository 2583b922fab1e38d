"""Threshold and Deframer without a GPU: the library's surface, the numpy definition the GPU tests compare against
(tests/_deframer_ref.py: the reference's per-bit loop and the event form, which must agree), a recorded run of the reference's own
Deframer, the out_size bound, the parameter errors, and the C++ mirror's harness on a fake library, plain and under the sanitizers.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _deframer_ref as D
from qdsp_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "qdsp_amd", "host")
FAKE = os.path.join(HERE, "fake_hip")
EINVAL = -10001

THR_ENTRY = ["create", "process", "process_ex", "process_dev", "process_batch_dev", "destroy", "span"]
DF_ENTRY = ["create", "set_sync", "get_state", "set_state", "out_size", "frame_bytes", "process", "process_ex", "process_dev",
            "process_batch_dev", "get_counts", "reset", "destroy", "tile", "pack_span"]


def test_symbols_declared_and_exported():
    want = {"qdsp_hip_threshold_" + n for n in THR_ENTRY} | {"qdsp_hip_deframer_" + n for n in DF_ENTRY}
    assert want <= set(capi.declared_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    have = set(re.findall(r"\bT (qdsp_hip_(?:threshold|deframer)_\w+)", out))
    assert have == want, (sorted(want - have), sorted(have - want))
    L = capi.load()
    assert all(getattr(L, s).argtypes is not None for s in want), "declared in capi.py"


def test_ops_surface():
    from qdsp_amd import ops

    for cls in (ops.Threshold, ops.Deframer):
        for name in ("process", "process_batch", "process_ex", "out_size", "reset", "last_kernel", "time_dev"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("get_state", "set_state", "set_sync", "counts", "tile", "pack_span"):
        assert callable(getattr(ops.Deframer, name)), name
    assert "Threshold" in ops.__all__ and "Deframer" in ops.__all__


# ---- the definition ----

def _random_case(rng):
    L = int(rng.integers(1, 17))
    fl = int(rng.integers(1, 41))
    style = int(rng.integers(0, 4))
    if style == 0:
        sync = np.zeros(L, np.uint8)                       # matches through the zero prefix
    elif style == 1:
        sync = np.ones(L, np.uint8)                        # overlapping matches in a run of ones
    else:
        sync = rng.integers(0, 2, L).astype(np.uint8)
    values = [(0, 1), (0, 1), (0, 1, 3), (0, 1, 255)][int(rng.integers(0, 4))]
    if 3 in values and style >= 2:
        sync[int(rng.integers(0, L))] = 3
    n = int(rng.integers(0, 400))
    x = D.stream_with_frames(rng, n, fl, sync, gap=(0, 3 * L + 5), p_sync=0.6, values=values)
    return x, fl, sync


def _random_cuts(rng, n, with_zero=True):
    cuts = []
    while sum(cuts) < n:
        c = int(rng.integers(0 if with_zero else 1, 30))
        cuts.append(min(c, n - sum(cuts)))
    return cuts


def test_event_form_equals_the_per_bit_loop():
    """400 random cases, sync lengths 1-16, frame lengths 1-40, overlapping and prefix-zero matches, bytes 0/1, 3 and 255: frames,
    frame starts, per-call counts and the final state agree, in one call and in random cuts that include 0."""
    rng = np.random.default_rng(1)
    nframes = 0
    for _ in range(400):
        x, fl, sync = _random_case(rng)
        for cuts in ([len(x)], _random_cuts(rng, len(x))):
            fa, ca, sa, sta = D.run_cuts(D.deframe_bits, x, fl, sync, cuts)
            fb, cb, sb, stb = D.run_cuts(D.deframe_ref, x, fl, sync, cuts)
            assert fa.tobytes() == fb.tobytes() and ca == cb and sa == sb
            assert D.public_state(sta) == D.public_state(stb) and sta["tail"].tobytes() == stb["tail"].tobytes()
            if sta["bits_read"] > 0:
                nb = (sta["bits_read"] + 7) // 8
                assert sta["cur"][:nb].tobytes() == stb["cur"][:nb].tobytes()
            nframes += len(fa)
    assert nframes > 2000


def test_the_definition_does_not_depend_on_the_cuts():
    rng = np.random.default_rng(2)
    for _ in range(60):
        x, fl, sync = _random_case(rng)
        whole, _, starts, st = D.run_cuts(D.deframe_bits, x, fl, sync, [len(x)])
        for cuts in ([1] * len(x), _random_cuts(rng, len(x))):
            f, counts, s, st2 = D.run_cuts(D.deframe_bits, x, fl, sync, cuts)
            assert f.tobytes() == whole.tobytes() and s == starts and D.public_state(st) == D.public_state(st2)


def test_out_size_is_never_exceeded():
    rng = np.random.default_rng(3)
    for _ in range(200):
        x, fl, sync = _random_case(rng)
        st, p = None, 0
        for c in _random_cuts(rng, len(x)):
            f, _, st = D.deframe_bits(x[p:p + c], fl, sync, st)
            assert len(f) <= D.out_size(c, fl), (c, fl, len(f))
            p += c
    assert D.out_size(0, 7) == 0 and D.out_size(1, 7) == 1 and D.out_size(7, 7) == 1 and D.out_size(8, 7) == 2
    assert D.frame_bytes(1) == 1 and D.frame_bytes(8) == 1 and D.frame_bytes(9) == 2


def test_one_sync_gives_six_frames_then_silence():
    sync = np.array([1, 0, 1, 1, 0, 0, 1, 0] * 4, np.uint8)
    x = np.concatenate([np.zeros(50, np.uint8), sync, np.zeros(64 * 8, np.uint8), sync, np.zeros(200, np.uint8)])
    f, starts, st = D.deframe_bits(x, 64, sync)
    # (the work buffer lags the input by sync_len: the frame starts where the sync word's last byte has just arrived)
    assert starts[:6] == [82 + 64 * k for k in range(6)] and len(f) == 6 + 3 and starts[6] == 82 + 64 * 8 + 32


def test_recorded_run_of_the_reference_deframer():
    """tests/golden/deframer_ref_io.npz: an input, a 32-bit sync word and the frames (256 bits) that the reference's own
    dsp::Deframer wrote for it in blocks of 100 bytes, recorded once from a program outside this repository."""
    g = np.load(os.path.join(HERE, "golden", "deframer_ref_io.npz"))
    x, sync, frames, fl, block = g["x"], g["sync"], g["frames"], int(g["frame_len"]), int(g["block"])
    assert len(sync) == 32 and fl == 256 and len(x) >= 3000 and block >= len(sync) and len(frames) >= 10
    cuts = [block] * (len(x) // block) + ([len(x) % block] if len(x) % block else [])
    for fn in (D.deframe_bits, D.deframe_ref):
        f, _, _, _ = D.run_cuts(fn, x, fl, sync, cuts)
        assert f.shape == frames.shape and f.tobytes() == frames.tobytes(), fn.__name__


def test_threshold_ref_edge_values():
    x = np.array([np.nan, -0.0, 0.0, -1e-45, 1e-45, np.inf, -np.inf, 1.0, -1.0], np.float32)
    assert D.threshold_ref(x).tolist() == [0, 0, 0, 0, 1, 1, 0, 1, 0]


# ---- parameter errors (checked before a device is looked for) ----

def test_create_parameter_errors():
    L = capi.load()
    h = C.c_void_p()
    sync = (C.c_uint8 * 300)(*([1] * 300))
    p = C.cast(sync, C.c_void_p)
    for kind, nchan, maxb, fl, sp, sl in ((2, 1, 16, 8, p, 4), (-1, 1, 16, 8, p, 4), (0, 1, 16, 0, p, 4), (0, 1, 16, (1 << 20) + 1, p, 4),
                                          (0, 1, 16, 8, None, 4), (0, 1, 16, 8, p, 0), (0, 1, 16, 8, p, 257), (0, 0, 16, 8, p, 4),
                                          (0, 65536, 16, 8, p, 4), (0, 1, -1, 8, p, 4)):
        assert L.qdsp_hip_deframer_create(C.byref(h), 0, kind, nchan, maxb, fl, sp, sl) == EINVAL, (kind, nchan, maxb, fl, sl)
        assert not h.value
    assert L.qdsp_hip_deframer_create(None, 0, 0, 1, 16, 8, p, 4) == EINVAL
    for nchan, maxb in ((0, 16), (65536, 16), (1, -1)):
        assert L.qdsp_hip_threshold_create(C.byref(h), 0, nchan, maxb) == EINVAL
    assert L.qdsp_hip_threshold_create(None, 0, 1, 16) == EINVAL
    # not a handle of that kind
    junk = C.create_string_buffer(64)
    assert L.qdsp_hip_deframer_out_size(junk, 10) == EINVAL and L.qdsp_hip_deframer_frame_bytes(junk) == EINVAL
    assert L.qdsp_hip_deframer_reset(junk) == EINVAL and L.qdsp_hip_deframer_set_state(junk, 0, -1, 5, 0) == EINVAL
    assert L.qdsp_hip_threshold_process_dev(junk, None, 0, None, None) == EINVAL
    assert L.qdsp_hip_deframer_tile() > 0 and L.qdsp_hip_deframer_pack_span() > 0 and L.qdsp_hip_threshold_span() > 0


def test_mirror_headers_compile_with_the_reference_usage(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text("""
#include <dsp/deframing.h>
#include <dsp/processing.h>
int main() {
    dsp::stream<float> a; dsp::stream<uint8_t> b;
    uint8_t sync[4] = {1, 0, 1, 1};
    dsp::Threshold t(&a);
    t.setLevel(1.0f); float l = t.getLevel(); t.setInput(&a);
    dsp::Deframer d(&t.out, 64, sync, 4);
    dsp::Deframer e; e.init(&b, 9, sync, 4);
    return d.out.writeBuf == nullptr || l != 1.0f;
}
""")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_build_makes_frame_check():
    subprocess.check_call(["make", "-C", HOST, "build/frame_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "frame_check")
    assert os.access(exe, os.X_OK)
    und = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    assert "qdsp_hip_deframer_process_ex" in und and "qdsp_hip_threshold_create" in und
    # none of the older harnesses has come to need the new entry points (they link against the tests' older fake library)
    for other in ("graph_check", "demod_check", "clock_check", "psk_check"):
        p = os.path.join(HOST, "build", other)
        if os.path.exists(p):
            u = subprocess.check_output(["nm", "-D", "--undefined-only", p], text=True)
            assert "qdsp_hip_deframer" not in u and "qdsp_hip_threshold" not in u, other


# ---- the harness on the fake library, plain and under the sanitizers ----

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_frame_check_on_the_fake_library(tmp_path, sanitize):
    """frame_check and the real stream_op.cpp as one program of its own, on the fake HIP runtime, the tests' fake library (unchanged) and
    fake_deframe.cpp, whose operators are the reference's plain loops: the frames are those of the definition, whatever the block
    size and the link."""
    hip_inc = "/opt/rocm/include"
    if not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("needs the HIP headers")
    out = os.path.join(FAKE, "build", "address_deframe" if sanitize else "plain_deframe")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "frame_check")
    flags = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined"] if sanitize else []
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-Wall", "-pthread",
                        "-D__HIP_PLATFORM_AMD__", "-DFAKE_HIP", f"-I{hip_inc}", f"-I{HOST}", f"-I{os.path.join(ROOT, 'include')}", "-o", exe,
                        os.path.join(HOST, "examples", "frame_check.cpp"), os.path.join(ROOT, "qdsp_amd", "csrc", "stream_op.cpp"),
                        os.path.join(FAKE, "fake_hip_runtime.cpp"), os.path.join(FAKE, "fake_qdsp_hip.cpp"), os.path.join(FAKE, "fake_deframe.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(5)
    sync = rng.integers(0, 2, 32).astype(np.uint8)
    sync.tofile(tmp_path / "sync.u8")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1 exitcode=68")
    for fl in (256, 9):
        x = D.stream_with_frames(rng, 6000, fl, sync, gap=(0, 200), p_sync=0.7)
        x.tofile(tmp_path / "x.u8")
        soft = np.where(x > 0, 1.0, -1.0).astype(np.float32) * rng.uniform(0.1, 2.0, len(x)).astype(np.float32)
        soft.tofile(tmp_path / "x.f32")
        want, _, _ = D.deframe_bits(x, fl, sync)
        assert len(want) >= 5
        for kind, link, ext in (("b", "host", "u8"), ("f", "dev", "f32"), ("f", "host", "f32")):
            for block in (4096, 33, 5):
                y = tmp_path / f"y_{kind}_{link}.bin"
                p = subprocess.run([exe, kind, link, f"x.{ext}", str(y), str(block), str(fl), "sync.u8"], cwd=tmp_path, env=env,
                                   capture_output=True, text=True, timeout=300)
                bad = [ln for ln in p.stderr.splitlines() if any(k in ln for k in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:"))]
                assert p.returncode == 0 and not bad and "graph ok" in p.stdout, p.stderr[-3000:]
                got = np.fromfile(y, dtype=np.uint8)
                assert got.tobytes() == want.tobytes(), (fl, kind, link, block)
