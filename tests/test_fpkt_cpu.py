"""FalconPacketSync without a GPU: the definition the GPU tests compare against (tests/_fpkt_ref.py: run() transcribed, with the two
departures) against a recording of the reference's own block; the closed form the kernels use against the transcription from every
start state and across every cut into two calls; the two output bounds, reached; the library's surface, argument errors and the
handle table's sub-kind; and the C++ mirror's harness on a fake library, plain and under the sanitizers.
"""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _fpkt_ref as R
from qdsp_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "qdsp_amd", "host")
FAKE = os.path.join(HERE, "fake_hip")
CSRC = os.path.join(ROOT, "qdsp_amd", "csrc")
EINVAL = -10001

ENTRY = ["create", "out_size", "out_packets", "frame_stride", "process", "process_ex", "process_dev", "process_batch_dev", "offs_dev",
         "get_offsets", "get_counts", "get_state", "set_state", "reset", "destroy"]


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "fpkt_ref_io.npz"))
    return {k: g[k] for k in g.files}


# ---- the recording of the reference's block ----

def test_transcription_reproduces_the_recording(golden):
    frames = golden["frames"]
    assert frames.shape == (300, R.RS_FRAME) and not R.in_departure_domain(frames), "the reference stays inside its buffers on this input"
    got = R.PacketSync().process(frames)
    lens, at = golden["packet_len"], golden["packet_frame"]
    assert len(got) == len(lens) >= 500
    assert [f for f, _ in got] == at.tolist() and [len(p) for _, p in got] == lens.tolist()
    assert b"".join(p for _, p in got) == golden["packet_bytes"].tobytes()


def test_the_recording_covers_the_stated_patterns(golden):
    frames, lens = golden["frames"], golden["packet_len"]
    hdr = [R.parse_header(f) for f in frames]
    ctr = [c for c, _ in hdr]
    assert sum(1 for _, p in hdr if p == R.CONT) >= 10, "continuation frames"
    assert (lens > R.DATA).sum() >= 10 and lens.max() > 2 * R.DATA, "packets longer than one and two frames"
    assert sum(1 for a, b in zip(ctr, ctr[1:]) if b != a + 1) >= 3, "counter breaks"
    assert any(a == (1 << 19) - 1 and b == 0 for a, b in zip(ctr, ctr[1:])), "the wrap at 2^19"
    tails = [R.walk(f)[3] for f in frames]
    assert any(0 < t < 4 for t in tails) and any(t >= 4 for t in tails) and any(t == -1 for t in tails)
    assert (frames[:, R.FRAME:] != 0).any(), "bytes behind byte 1194 that the block must not read"


# ---- the closed form against the transcription ----

def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


START_STATES = ["nothing", "one_byte", "two_bytes", "three_bytes", "full"]


def _start(kind, rng):
    n = {"nothing": 0, "one_byte": 1, "two_bytes": 2, "three_bytes": 3, "full": R.CAP}[kind]
    return rng.integers(0, 256, n).astype(np.uint8).tobytes()


@pytest.mark.parametrize("start", START_STATES)
def test_closed_form_equals_the_transcription(start):
    emitted_pending = 0
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        fr = R.random_stream(rng, 60, big=0.06, breaks=0.04, zero=0.03, bad_ptr=0.02, wrap=seed % 2 == 0)
        pend = _start(start, rng)
        ctr0, _ = R.parse_header(fr[0])
        for last in ((ctr0 - 1) & 0xFFFFFFFF, ctr0):          # the carried packet lives / is dropped at frame 0
            a, b = R.serial_row(fr, last, pend), R.closed_form(fr, last, pend)
            assert _same(a, b), (seed, last)
            if pend and last != ctr0 and R.parse_header(fr[0])[1] <= R.DATA and len(pend) + R.parse_header(fr[0])[1] <= R.CAP:
                assert R.split(a[0], a[1])[0][:len(pend)] == pend
                emitted_pending += 1
    assert start == "nothing" or emitted_pending >= 1


def test_closed_form_across_every_cut_into_two_calls():
    for seed in range(3):
        rng = np.random.default_rng(200 + seed)
        fr = R.random_stream(rng, 40, mean=500, big=0.15, breaks=0.04, zero=0.03, bad_ptr=0.02)
        whole = R.serial_row(fr)
        assert len(whole[1]) > 20 and any(len(p) > R.DATA for p in R.split(whole[0], whole[1]))
        for cut in range(len(fr) + 1):
            a = R.closed_form(fr[:cut])
            b = R.closed_form(fr[cut:], a[2][0], a[2][2])
            assert a[2][1] == (len(a[2][2]) if a[2][2] else -1)
            assert a[0] + b[0] == whole[0] and b[2] == whole[2], (seed, cut)
            assert R.split(a[0], a[1]) + R.split(b[0], b[1]) == R.split(whole[0], whole[1]), (seed, cut)


def test_empty_call_keeps_the_state():
    pend = bytes(range(1, 200))
    out, offs, st = R.closed_form(np.zeros((0, R.FRAME), np.uint8), 77, pend)
    assert out == b"" and offs.tolist() == [0] and st == (77, len(pend), pend) == R.serial_row(np.zeros((0, R.FRAME), np.uint8), 77, pend)[2]


# ---- the bounds, reached ----

def three_byte_frame(ctr, stride=R.FRAME):
    """A frame of 397 packets of three bytes (a length field of 1)."""
    data = np.tile(np.array([0x00, 0x01, 0x5A], np.uint8), R.DATA // 3)
    data[2::3] = np.arange(R.DATA // 3) & 0xFF
    return R.make_frame(ctr, 0, data.tobytes(), stride)


def test_the_packet_bound_holds_and_how_close_a_frame_comes():
    """A frame filled with three-byte packets behind a pending one.  out_packets(1) = 398 counts the pending packet and 1191 // 3 =
    397 walked ones; the walk itself stops one short of that: a header needs four bytes left, so the three bytes at 1188 are no
    packet but a residue (and a last packet that ends with the frame has at least four bytes).  396 walked packets and the pending
    one, 397, is the most a frame emits: the bound holds with one to spare per frame."""
    fr = three_byte_frame(5)[None]
    for f in (R.serial_row, R.closed_form):
        out, offs, st = f(fr, 4, b"\x0f\xff\x01")
        assert len(offs) - 1 == 397 == R.out_packets(1) - 1 and st[1] == 3 and st[2] == bytes(fr[0, -3:])
        assert np.diff(offs).tolist() == [3] * 397
    # every frame after it completes the residue of the one before: 397 per frame again, and a packet that ends with the frame
    two = np.stack([three_byte_frame(5), three_byte_frame(6)])
    two[1, R.HEADER + 1185:R.FRAME] = [0x00, 0x04, 1, 2, 3, 4]
    out, offs, st = R.closed_form(two, 4, b"\x01")
    assert len(offs) - 1 == 2 * 397 <= R.out_packets(2) and st[1] == -1 and _same((out, offs, st), R.serial_row(two, 4, b"\x01"))


def test_the_byte_bound_is_reached():
    """A full carry completed by a frame whose whole data area is walked: 16392 + 1191 = out_size(1); every further such frame adds
    1191."""
    pend = bytes(np.random.default_rng(3).integers(0, 256, R.CAP).astype(np.uint8))
    rng = np.random.default_rng(4)
    fr = np.stack([R.make_frame(9 + k, 0, R.make_packet(R.DATA, rng)) for k in range(3)])
    for n in (1, 3):
        for f in (R.serial_row, R.closed_form):
            out, offs, st = f(fr[:n], 8, pend)
            assert len(out) == R.out_size(n) == R.CAP + R.DATA * n and out[:R.CAP] == pend and offs[1] == R.CAP
    # one byte more would pass the cap: the carry is dropped instead
    fr1 = R.make_frame(9, 1, bytes(R.DATA))[None]
    assert _same(R.serial_row(fr1, 8, pend), R.closed_form(fr1, 8, pend)) and R.closed_form(fr1, 8, pend)[0] == b""


# ---- the library's surface ----

def test_symbols_declared_and_exported():
    want = {f"qdsp_hip_fpkt_{n}" for n in ENTRY}
    assert want <= set(capi.declared_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    have = set(re.findall(r"\bT (qdsp_hip_fpkt_\w+)", out))
    assert have == want, (sorted(want - have), sorted(have - want))
    assert not [s for s in want if re.fullmatch(r"qdsp_hip_(?:falcon_)?rs_\w+", s)], "the prefix is no other unit's"
    L = capi.load()
    assert all(getattr(L, s).argtypes is not None for s in want), "declared in capi.py"
    with open(capi.HEADER_PATH) as f:
        text = f.read()
    assert re.search(r"#define QDSP_HIP_FPKT_FRAME_BYTES 1195\b", text) and re.search(r"#define QDSP_HIP_FPKT_MAX_PACKET 16392\b", text)


def test_create_parameter_errors():
    L = capi.load()
    h = C.c_void_p()
    for nchan, maxb, fs in ((0, 16, 1275), (65536, 16, 1275), (1, -1, 1275), (1, 16, 1194), (1, 16, 4097), (1, 16, 0), (1, (1 << 20) + 1, 1275)):
        assert L.qdsp_hip_fpkt_create(C.byref(h), 0, nchan, maxb, fs) == EINVAL and not h.value
    assert L.qdsp_hip_fpkt_create(None, 0, 1, 16, 1275) == EINVAL
    junk = C.create_string_buffer(64)
    st, ctr, i64 = (C.c_int * 2)(), C.c_uint32(), C.c_int64()
    p1, p2 = C.c_void_p(), C.c_void_p()
    f = lambda n: getattr(L, "qdsp_hip_fpkt_" + n)        # noqa: E731
    assert f("out_size")(junk, 1) == EINVAL and f("out_packets")(junk, 1) == EINVAL and f("frame_stride")(junk) == EINVAL
    assert f("process_dev")(junk, None, 0, None, None) == EINVAL and f("process_ex")(junk, None, 0, 0, None, 0) == EINVAL
    assert f("process")(junk, None, 0, None) == EINVAL
    assert f("process_batch_dev")(junk, None, 0, 0, None, None, 0, None, 0, None, None) == EINVAL
    assert f("get_counts")(junk, st) == EINVAL and f("get_offsets")(junk, 0, st, 1) == EINVAL
    assert f("offs_dev")(junk, C.byref(p1), C.byref(i64), C.byref(p2)) == EINVAL
    assert f("get_state")(junk, 0, C.byref(ctr), st, None) == EINVAL and f("set_state")(junk, 0, 0, -1, None) == EINVAL
    assert f("reset")(junk) == EINVAL and f("destroy")(junk) is None
    # a handle of neither unit is refused by both
    assert L.qdsp_hip_rs_out_size(junk, 1) == EINVAL


def test_module_surface():
    import qdsp_amd
    from qdsp_amd import falcon, fec, noaa, ops

    assert qdsp_amd.falcon is falcon and falcon.__all__ == ["FalconPacketSync"]
    cls = falcon.FalconPacketSync
    assert issubclass(cls, ops._RowOp) and issubclass(cls, ops._Counts)
    for m in ("process", "process_batch", "process_ex", "out_size", "out_packets", "counts", "offsets", "get_state", "set_state", "reset",
              "time_dev", "packets", "last_kernel"):
        assert callable(getattr(cls, m)), m
    assert not hasattr(ops, "FalconPacketSync") and not hasattr(fec, "FalconPacketSync") and not hasattr(noaa, "FalconPacketSync")
    assert (cls.FRAME, cls.DATA, cls.MAX_PACKET, cls.PER_FRAME) == (R.FRAME, R.DATA, R.CAP, R.PER_FRAME)
    for fs in (1194, 0, 4097):
        with pytest.raises(ValueError):
            cls(frame_stride=fs)
    with open(os.path.join(ROOT, "qdsp_amd", "__init__.py")) as f:
        assert re.search(r"^\s+falcon\.py\s", f.read(), re.M)
    # the static helper splits a row
    out = np.arange(10, dtype=np.uint8)
    assert cls.packets(out, np.array([0, 3, 4, 9, 99], np.int32), 3) == [bytes([0, 1, 2]), bytes([3]), bytes([4, 5, 6, 7, 8])]
    assert cls.packets(out, np.array([0], np.int32), 0) == []


# ---- the handle kinds ----

def test_the_enum_is_untouched_and_the_subkind_in_place():
    hdr = open(os.path.join(CSRC, "stream_op.h")).read()
    body = re.search(r"enum class OpKind : int \{(.*?)\n\};", hdr, re.S).group(1)
    names = [m for m in re.findall(r"\b([A-Z]\w*)\b(?=\s*(?:=\s*\d+\s*)?,)", re.sub(r"//[^\n]*", "", body))]
    assert len(names) == 17 and names[-4:] == ["Rs", "Hrpt", "Tip", "Hirs"] and "constexpr OpKind kLastOpKind = OpKind::Hirs;" in hdr
    assert "void stream_op_register(StreamOp* d, OpKind kind, int sub = 0);" in hdr
    assert "StreamOp* stream_op_lookup(void* h, OpKind kind, int sub = 0);" in hdr
    fh = open(os.path.join(CSRC, "fpkt.hip.h")).read()
    assert "static constexpr OpKind kKind = OpKind::Rs;" in fh and "static constexpr int kSub = 1;" in fh
    # every other unit stays at sub 0: no other handle names a kSub
    for name in os.listdir(CSRC):
        if name.endswith((".h", ".hip", ".cpp")) and name not in ("fpkt.hip.h", "stream_op.h"):
            assert "kSub" not in open(os.path.join(CSRC, name)).read(), name


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_subkind_selftest_under_the_sanitizers():
    hip_inc = "/opt/rocm/include"
    if not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("needs the HIP headers")
    out = os.path.join(FAKE, "build", "address_subkind")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "stream_op_subkind_selftest")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-Wall", "-pthread",
                        "-D__HIP_PLATFORM_AMD__", "-DFAKE_HIP", f"-I{hip_inc}", "-o", exe, os.path.join(FAKE, "stream_op_subkind_selftest.cpp"),
                        os.path.join(CSRC, "stream_op.cpp"), os.path.join(FAKE, "fake_hip_runtime.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1 exitcode=68")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "subkind ok" in p.stdout and "runtime error:" not in p.stderr, (p.stdout, p.stderr[-3000:])


# ---- the C++ mirror ----

def test_mirror_header_compiles_with_the_reference_usage(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text("""
#include <dsp/falcon_fec.h>
#include <dsp/falcon_packet.h>
int main() {
    dsp::stream<uint8_t> in;
    dsp::FalconRS falconRS(&in);
    dsp::FalconPacketSync pkt(&falconRS.out);
    dsp::FalconPacketSync p2; p2.init(&falconRS.out);
    pkt.start(); pkt.stop();
    return pkt.out.writeBuf == nullptr;
}
""")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_build_makes_packet_check():
    subprocess.check_call(["make", "-C", HOST, "build/packet_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "packet_check")
    assert os.access(exe, os.X_OK)
    und = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    for s in ("qdsp_hip_fpkt_process_ex", "qdsp_hip_fpkt_create", "qdsp_hip_fpkt_get_offsets"):
        assert s in und, s
    with open(os.path.join(HOST, "Makefile")) as f:
        assert "build/packet_check" in f.read().split("all:")[1].splitlines()[0]


def packet_check_input():
    """Frames of 1275 bytes with long packets, breaks, a bad pointer and a zero length, and the definition's packets."""
    rng = np.random.default_rng(60)
    fr = R.random_stream(rng, 48, stride=R.RS_FRAME, mean=400, big=0.1, breaks=0.05, zero=0.04, bad_ptr=0.03, fill=True)
    want = [p for _, p in R.PacketSync().process(fr)]
    assert len(want) > 50 and any(len(p) > R.DATA for p in want)
    return fr, want


def read_packets(path):
    raw, o, got = open(path, "rb").read(), 0, []
    while o < len(raw):
        (n,) = struct.unpack_from("<I", raw, o)
        got.append(raw[o + 4:o + 4 + n])
        o += 4 + n
    return got


def run_packet_check(exe, tmp_path, frames, want, env=None, pers=(1, 5, 48)):
    frames.tofile(tmp_path / "x.u8")
    for link in ("host", "dev"):
        for per in pers:
            out = tmp_path / f"out_{link}_{per}.bin"
            p = subprocess.run([exe, link, "x.u8", str(out), str(per)], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
            bad = [ln for ln in p.stderr.splitlines() if any(k in ln for k in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:"))]
            assert p.returncode == 0 and not bad and "graph ok" in p.stdout, (p.stdout, p.stderr[-3000:])
            assert read_packets(out) == want, (link, per)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_packet_check_on_the_fake_library(tmp_path, sanitize):
    """packet_check and the real stream_op.cpp as one program of its own, on the fake HIP runtime, the tests' fake library
    (unchanged) and fake_fpkt.cpp, whose operator is the serial loop: the packets are the definition's, whatever the block size
    and the link."""
    hip_inc = "/opt/rocm/include"
    if not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("needs the HIP headers")
    out = os.path.join(FAKE, "build", "address_fpkt" if sanitize else "plain_fpkt")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "packet_check")
    flags = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined"] if sanitize else []
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-Wall", "-pthread",
                        "-D__HIP_PLATFORM_AMD__", "-DFAKE_HIP", f"-I{hip_inc}", f"-I{HOST}", f"-I{os.path.join(ROOT, 'include')}", "-o", exe,
                        os.path.join(HOST, "examples", "packet_check.cpp"), os.path.join(CSRC, "stream_op.cpp"),
                        os.path.join(FAKE, "fake_hip_runtime.cpp"), os.path.join(FAKE, "fake_qdsp_hip.cpp"), os.path.join(FAKE, "fake_fpkt.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    frames, want = packet_check_input()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1 exitcode=68")
    run_packet_check(exe, tmp_path, frames, want, env)
