"""The NOAA HRPT tail without a GPU: the definition the GPU tests compare against (tests/_noaa_ref.py: readBits and the three run()
loops transcribed) against big-integer extraction, its own inverses and walking-one frames; the closed form of HIRSDemux's line
breaks that the kernels use against the serial loop from every start state; the library's surface and argument errors; and the
C++ mirror's harness on a fake library, plain and under the sanitizers.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _noaa_ref as R
from qdsp_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "qdsp_amd", "host")
FAKE = os.path.join(HERE, "fake_hip")
EINVAL = -10001

COMMON = ["create", "out_size", "process", "process_ex", "process_dev", "process_batch_dev", "get_counts", "destroy"]
ENTRY = {"hrpt": COMMON + ["tip_dev", "aip_dev", "get_tip", "get_aip", "get_frame_slots"],
         "tip": COMMON,
         "hirs": COMMON + ["packet_stride", "get_state", "set_state", "reset"]}


def test_symbols_declared_and_exported():
    want = {f"qdsp_hip_{u}_{n}" for u, names in ENTRY.items() for n in names}
    assert want <= set(capi.declared_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    have = set(re.findall(r"\bT (qdsp_hip_(?:hrpt|tip|hirs)_\w+)", out))
    assert have == want, (sorted(want - have), sorted(have - want))
    L = capi.load()
    assert all(getattr(L, s).argtypes is not None for s in want), "declared in capi.py"
    with open(capi.HEADER_PATH) as f:
        text = f.read()
    for name, val in (("RECORD_BYTES", 74), ("HIRS_OFFSET", 0), ("SEM_OFFSET", 36), ("DCS_OFFSET", 38), ("SBUV_OFFSET", 70)):
        assert re.search(rf"#define QDSP_HIP_TIP_{name} {val}\b", text), name


def test_the_handle_kinds():
    """Every enumerator of OpKind (not one per line: several may share a line): seventeen, counted as the compiler counts them, all
    different, none 0; the three new ones are the last, kLastOpKind is the last of them, and the handles name them."""
    csrc = os.path.join(ROOT, "qdsp_amd", "csrc")
    hdr = open(os.path.join(csrc, "stream_op.h")).read()
    body = re.search(r"enum class OpKind : int \{(.*?)\n\};", hdr, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    values, nxt = {}, 0
    for item in (s.strip() for s in body.split(",")):
        if not item:
            continue
        m = re.fullmatch(r"(\w+)(?:\s*=\s*(\d+))?", item)
        assert m, item
        nxt = int(m.group(2)) if m.group(2) else nxt
        values[m.group(1)] = nxt
        nxt += 1
    assert len(values) == len(set(values.values())) == 17 and 0 not in values.values()
    assert list(values)[-4:] == ["Rs", "Hrpt", "Tip", "Hirs"] and values["Hirs"] == 17
    assert "constexpr OpKind kLastOpKind = OpKind::Hirs;" in hdr
    nh = open(os.path.join(csrc, "noaa.hip.h")).read()
    for kind in ("Hrpt", "Tip", "Hirs"):
        assert f"static constexpr OpKind kKind = OpKind::{kind};" in nh, kind


def test_noaa_surface_and_ops_and_fec_untouched():
    import qdsp_amd
    from qdsp_amd import fec, noaa, ops

    assert qdsp_amd.noaa is noaa
    assert set(noaa.__all__) == {"HrptDemux", "TipDemux", "HirsDemux"}
    for name in noaa.__all__:
        cls = getattr(noaa, name)
        assert issubclass(cls, ops._RowOp) and issubclass(cls, ops._Counts)
        for m in ("process", "process_batch", "process_ex", "out_size", "counts", "last_kernel", "time_dev", "reset"):
            assert callable(getattr(cls, m)), (name, m)
        assert not hasattr(ops, name) and not hasattr(fec, name)
    assert set(fec.__all__) == {"RsDecoder", "FalconRs", "ccsds_dual_basis", "ccsds_randomizer"}
    T = noaa.TipDemux
    assert (T.HIRS, T.SEM, T.DCS, T.SBUV, T.RECORD) == R.SECTIONS == (0, 36, 38, 70, 74)
    rec = np.arange(3 * 74, dtype=np.uint8).reshape(3, 74)
    parts = T.split(rec)
    assert [p.shape[1] for p in parts] == [36, 2, 32, 4] and all(np.shares_memory(p, rec) for p in parts)
    assert np.array_equal(np.concatenate(parts, axis=1), rec)
    for m in ("get_state", "set_state"):
        assert callable(getattr(noaa.HirsDemux, m))


# ---- readBits ----

def test_read_bits_equals_big_integer_extraction():
    """Every (offset, length) the three blocks use: all 11090 words of a frame and its minor field; the element and the twenty
    radiances of a packet."""
    rng = np.random.default_rng(1)
    frame = rng.integers(0, 256, R.FRAME_BYTES).astype(np.uint8)
    big = int.from_bytes(frame.tobytes(), "big")
    nb = 8 * R.FRAME_BYTES
    for off, ln in [(61, 2)] + [(10 * w, 10) for w in range(R.WORDS)]:
        assert R.read_bits(off, ln, frame) == (big >> (nb - off - ln)) & ((1 << ln) - 1), (off, ln)
    for _ in range(20):
        pk = rng.integers(0, 256, R.PACKET_BYTES).astype(np.uint8)
        for off, ln in [(R.ELEMENT_BIT, R.ELEMENT_LEN)] + [(o, 13) for o in R.RAD_BITS]:
            assert R.read_bits(off, ln, pk) == R.big_int_bits(off, ln, pk), (off, ln)
    # the single-byte branch, and fields that end on a byte boundary
    b = np.array([0b10110100, 0b01101001, 0xFF], np.uint8)
    assert R.read_bits(1, 3, b) == 0b011 and R.read_bits(0, 8, b) == 0xB4 and R.read_bits(4, 12, b) == 0x469 and R.read_bits(7, 2, b) == 0


def test_the_tables():
    assert len(R.RECORD_SRC) == 74 and len(set(R.RECORD_SRC)) == 74 and min(R.RECORD_SRC) == 16 and max(R.RECORD_SRC) == 95
    # the reference's twenty offsets: 26 + 13 k but for its 119 (k = 7 would be 117), kept as it has it
    assert len(R.RAD_BITS) == 20 and sorted(R.RAD_BITS) == [26 + 13 * k + (2 if k == 7 else 0) for k in range(20)]
    assert max(R.RAD_BITS) + 13 <= 8 * R.PACKET_BYTES


# ---- the inverses ----

def _random_frame(rng, minor):
    tip = rng.integers(0, 256, (5, R.MINOR_BYTES)).astype(np.uint8)
    av = rng.integers(0, 1024, (R.PLANES, R.PIXELS)).astype(np.uint16)
    return R.make_frame(minor, tip, av, fill=rng.integers(0, 256, R.FRAME_BYTES)), tip, av


@pytest.mark.parametrize("minor", range(4))
def test_demux_of_make_frame(minor):
    rng = np.random.default_rng(10 + minor)
    frame, tip, av = _random_frame(rng, minor)
    m, t, a, v = R.hrpt_run(frame)
    assert m == minor and np.array_equal(v, av)
    assert (t is not None) == (minor == 1) and (a is not None) == (minor == 3)
    if minor == 1:
        assert np.array_equal(t, tip)
    if minor == 3:
        assert np.array_equal(a, tip)
    assert [R.read_word(w, frame) for w in range(6)] == R.STD_SYNC_WORDS


def test_demux_of_make_packet():
    rng = np.random.default_rng(20)
    assert all(R.hirs_signed_to_unsigned(R.hirs_unsigned_to_signed(u)) == u for u in range(0x2000))
    assert sorted(R.hirs_signed_to_unsigned(n) for n in range(0x2000)) == list(range(0x2000))
    h = R.Hirs()
    lines = []
    for e in (3, 55):
        rad = R.random_radiances(rng)
        pk = R.make_packet(e, rad, fill=rng.integers(0, 256, R.PACKET_BYTES))
        assert R.read_bits(R.ELEMENT_BIT, R.ELEMENT_LEN, pk) == e
        h.run(pk, lines)
        got = lines[-1][:, e] if e == 55 else h.buf[:, e]
        assert np.array_equal(got, rad)
    assert len(lines) == 1 and (lines[0][:, 4:55] == 0xFFF).all()


def test_tip_run_is_the_four_lists():
    mf = np.arange(104, dtype=np.uint8)
    rec = R.tip_run(mf)
    assert rec[:36].tolist() == R.HIRS_SRC and rec[36:38].tolist() == R.SEM_SRC and rec[38:70].tolist() == R.DCS_SRC and rec[70:].tolist() == R.SBUV_SRC


def test_fast_forms_equal_the_transcription():
    rng = np.random.default_rng(30)
    frames = rng.integers(0, 256, (4, R.FRAME_BYTES)).astype(np.uint8)
    frames[:, 7] = (frames[:, 7] & 0xF9) | (np.array([1, 3, 0, 1]) << 1)
    slow, fast = R.hrpt_demux(frames), R.hrpt_demux_fast(frames)
    assert all(np.array_equal(s, f) for s, f in zip(slow, fast)) and len(slow[1]) == 10 and len(slow[2]) == 5
    pk = rng.integers(0, 256, 300 * 74).astype(np.uint8)
    for stride in (36, 74):
        a, b = R.Hirs().process(pk, stride), R.HirsFast().process(pk, stride)
        assert a.shape[1] >= 3 and np.array_equal(a, b)


# ---- walking-one frames ----

WALK = [60, 61, 62, 63, 1029, 1030, 1031, 6229, 6230, 6231, 7499, 7500, 7501, 109899, 109900]


@pytest.mark.parametrize("base_minor", [0, 1, 3])
@pytest.mark.parametrize("bit", WALK)
def test_walking_one(bit, base_minor):
    """One set bit (on a frame that is zero but for a `minor` of 0, 1 or 3) lights exactly the output bit its position says, or
    none."""
    frame = np.zeros(R.FRAME_BYTES, np.uint8)
    R._put_bits(frame, 61, 2, base_minor)
    frame[bit // 8] |= 0x80 >> (bit % 8)
    minor = base_minor | (2 if bit == 61 else 0) | (1 if bit == 62 else 0)
    want_av = np.zeros((R.PLANES, R.PIXELS), np.uint16)
    if 7500 <= bit < 109900:
        w, k = divmod(bit, 10)
        p, c = divmod(w - 750, 5)
        want_av[c, p] = 1 << (9 - k)
    want_tb = np.zeros(5 * R.MINOR_BYTES, np.uint8)
    if 1030 <= bit < 6230 and bit % 10 < 8:
        want_tb[bit // 10 - 103] = 0x80 >> (bit % 10)
    m, t, a, v = R.hrpt_run(frame)
    assert m == minor and np.array_equal(v, want_av)
    assert (t is not None) == (minor == 1) and (a is not None) == (minor == 3)
    for got in (t, a):
        if got is not None:
            assert np.array_equal(got.ravel(), want_tb)
    lit = int(want_av.astype(bool).sum()) + int(want_tb.astype(bool).sum())
    assert lit == (1 if bit in (1030, 1031, 7500, 7501, 109899) else 0)


# ---- the closed form of HIRSDemux against the serial loop ----

def _element_sets():
    rng = np.random.default_rng(40)
    sets = {"random": [rng.integers(0, 64, 300).tolist() for _ in range(3)],
            "edge_values": [rng.choice([54, 55, 56, 0, 1, 63], 200).tolist() for _ in range(3)]}
    mono = []
    for _ in range(3):
        seq, e = [], int(rng.integers(0, 56))
        while len(seq) < 300:
            seq.append(e)
            r = rng.random()
            if r < 0.1:
                pass                                              # a repeated element
            elif r < 0.15:
                seq.append(int(rng.integers(56, 64)))             # a non-image element in the line
            else:
                e += int(rng.integers(1, 4))
            if e > 55:
                e = int(rng.integers(0, 3))                       # the wrap, with or without an element 55 before it
        mono.append(seq)
    sets["monotone_with_wrap"] = mono
    return sets


@pytest.mark.parametrize("kind", ["random", "monotone_with_wrap", "edge_values"])
def test_parallel_hirs_form_equals_the_serial_loop(kind):
    seqs = _element_sets()[kind]
    # the inputs do exercise the cases: asserted on the definition's output, so that nothing passes on an empty result
    lines = dup = hi = 0
    for s in seqs:
        per, n, _ = R.hirs_elements_serial(s)
        lines += n
        dup += sum(1 for i in range(len(s) - 1) if s[i] == s[i + 1] and per[i] >= 0 and per[i] == per[i + 1])
        nid = False
        for e in s:
            hi += 1 if (e > 55 and nid) else 0
            nid = e < 55
    assert lines >= 3 and dup >= 1 and hi >= 1, (lines, dup, hi)
    for s in seqs:
        for last in range(64):
            for nid in (False, True):
                for cut in (len(s), 1, 0):
                    a = R.hirs_elements_serial(s[:cut], last, nid)
                    b = R.hirs_elements_parallel(s[:cut], last, nid)
                    assert a == b, (kind, last, nid, cut)
                assert R.hirs_map_serial(s, last, nid) == R.hirs_map_parallel(s, last, nid), (kind, last, nid)


def test_both_flushes_on_the_first_packet():
    per, n, st = R.hirs_elements_serial([55], 60, True)
    assert (per, n, st) == ([1], 2, (55, False)) == R.hirs_elements_parallel([55], 60, True)


# ---- create and argument errors (checked before a device is looked for) ----

def test_create_parameter_errors():
    L = capi.load()
    h = C.c_void_p()
    for fn in (L.qdsp_hip_hrpt_create, L.qdsp_hip_tip_create):
        for nchan, maxb in ((0, 16), (65536, 16), (1, -1)):
            assert fn(C.byref(h), 0, nchan, maxb) == EINVAL and not h.value
        assert fn(None, 0, 1, 16) == EINVAL
    assert L.qdsp_hip_hrpt_create(C.byref(h), 0, 1, (1 << 20) + 1) == EINVAL
    for nchan, maxb, ps in ((0, 16, 36), (1, -1, 36), (1, 16, 35), (1, 16, 4097), (1, 16, 0), (1, (1 << 22) + 1, 36)):
        assert L.qdsp_hip_hirs_create(C.byref(h), 0, nchan, maxb, ps) == EINVAL and not h.value
    assert L.qdsp_hip_hirs_create(None, 0, 1, 16, 36) == EINVAL
    junk = C.create_string_buffer(64)
    st = (C.c_int * 2)()
    for u in ("hrpt", "tip", "hirs"):
        f = lambda n: getattr(L, f"qdsp_hip_{u}_{n}")
        assert f("out_size")(junk, 1) == EINVAL and f("process_dev")(junk, None, 0, None, None) == EINVAL
        assert f("get_counts")(junk, st) == EINVAL and f("process_ex")(junk, None, 0, 0, None, 0) == EINVAL
        assert f("destroy")(junk) is None
    assert L.qdsp_hip_hrpt_process_batch_dev(junk, None, 0, 0, None, None, 0, 0, None, 0, None, None, 0, None, None) == EINVAL
    assert L.qdsp_hip_tip_process_batch_dev(junk, None, 0, 0, None, None, 0, None, None) == EINVAL
    assert L.qdsp_hip_hirs_process_batch_dev(junk, None, 0, 0, None, None, 0, 0, None, None) == EINVAL
    assert L.qdsp_hip_hirs_reset(junk) == EINVAL and L.qdsp_hip_hirs_set_state(junk, 0, 0, 0) == EINVAL
    assert L.qdsp_hip_hirs_get_state(junk, 0, st, st) == EINVAL and L.qdsp_hip_hirs_packet_stride(junk) == EINVAL
    assert L.qdsp_hip_hrpt_get_tip(junk, 0, None, 0) == EINVAL and L.qdsp_hip_hrpt_get_frame_slots(junk, 0, None, 0) == EINVAL


def test_noaa_argument_checks():
    from qdsp_amd import noaa

    for ps in (35, 0, 4097):
        with pytest.raises(ValueError):
            noaa.HirsDemux(packet_stride=ps)
    with pytest.raises(ValueError):
        noaa._Noaa._whole(None, 13862, 13863)
    assert noaa._Noaa._whole(None, 2 * 13863, 13863) == 2


# ---- the C++ mirror ----

def test_mirror_headers_compile_with_the_reference_usage(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text("""
#include <dsp/noaa/hrpt.h>
#include <dsp/noaa/tip.h>
int main() {
    dsp::stream<uint8_t> packedIn;
    dsp::noaa::HRPTDemux demux(&packedIn);
    dsp::noaa::TIPDemux tipDemux(&demux.TIPOut);
    dsp::noaa::HIRSDemux hirsDemux(&tipDemux.HIRSOut);
    dsp::noaa::HRPTDemux d2; d2.init(&packedIn); d2.setInput(&packedIn);
    dsp::noaa::TIPDemux t2; t2.init(&demux.AIPOut); t2.setInput(&demux.TIPOut);
    dsp::noaa::HIRSDemux h2; h2.init(&tipDemux.HIRSOut); h2.setInput(&tipDemux.HIRSOut);
    dsp::stream<uint16_t>* av[5] = {&demux.AVHRRChan1Out, &demux.AVHRRChan2Out, &demux.AVHRRChan3Out, &demux.AVHRRChan4Out, &demux.AVHRRChan5Out};
    dsp::stream<uint8_t>* tp[3] = {&tipDemux.SEMOut, &tipDemux.DCSOut, &tipDemux.SBUVOut};
    demux.start(); tipDemux.start(); hirsDemux.start();
    hirsDemux.stop(); tipDemux.stop(); demux.stop();
    return av[4]->writeBuf == nullptr || tp[2]->writeBuf == nullptr || hirsDemux.radChannels[19].writeBuf == nullptr;
}
""")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_build_makes_noaa_check():
    subprocess.check_call(["make", "-C", HOST, "build/noaa_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "noaa_check")
    assert os.access(exe, os.X_OK)
    und = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    for s in ("qdsp_hip_hrpt_process_ex", "qdsp_hip_tip_process_ex", "qdsp_hip_hirs_process_ex", "qdsp_hip_hirs_create"):
        assert s in und, s
    with open(os.path.join(HOST, "Makefile")) as f:
        assert "build/noaa_check" in f.read().split("all:")[1].splitlines()[0]


def noaa_check_input(nframes=9, min_lines=3):
    """Frames with all four `minor` values whose TIP minor frames carry HIRS packets that finish lines, and what the definition
    chain makes of them: {sink name: array}."""
    rng = np.random.default_rng(50)
    minors = [1, 1, 3, 0, 1, 2, 1, 3, 1, 1, 0, 3][:nframes]
    elements = ([48, 49, 50, 52, 53, 54, 55, 0, 1, 2, 2, 3, 60, 5, 6, 4, 7, 54, 55, 55, 63, 0, 10, 20, 30] * 3)[:5 * minors.count(1)]
    frames, k = [], 0
    for m in minors:
        tb = rng.integers(0, 256, (5, R.MINOR_BYTES)).astype(np.uint8)
        if m == 1:
            for i in range(5):
                tb[i, R.HIRS_SRC] = R.make_packet(elements[k], R.random_radiances(rng), fill=rng.integers(0, 256, R.PACKET_BYTES))
                k += 1
        frames.append(R.make_frame(m, tb, rng.integers(0, 1024, (R.PLANES, R.PIXELS)), fill=rng.integers(0, 256, R.FRAME_BYTES)))
    frames = np.stack(frames)
    av, tip, aip, got_minors = R.hrpt_demux_fast(frames)
    assert got_minors.tolist() == minors and len(tip) and len(aip) and (got_minors % 2 == 0).any()
    rec = R.tip_demux(tip)
    lines = R.HirsFast().process(np.ascontiguousarray(rec[:, :36]))
    assert lines.shape[1] >= min_lines
    want = {f"avhrr{c + 1}": av[c] for c in range(R.PLANES)}
    want.update(aip=aip, sem=rec[:, 36:38], dcs=rec[:, 38:70], sbuv=rec[:, 70:74])
    want.update({f"hirs{i + 1:02d}": lines[i] for i in range(R.CHANNELS)})
    return frames, want


def run_noaa_check(exe, tmp_path, frames, want, env=None, pers=(1, 4, 9)):
    frames.tofile(tmp_path / "x.u8")
    for link in ("host", "dev"):
        for per in pers:
            out = tmp_path / f"out_{link}_{per}"
            os.makedirs(out, exist_ok=True)
            p = subprocess.run([exe, link, "x.u8", str(out), str(per)], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
            bad = [ln for ln in p.stderr.splitlines() if any(k in ln for k in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:"))]
            assert p.returncode == 0 and not bad and "graph ok" in p.stdout, (p.stdout, p.stderr[-3000:])
            assert len(re.findall(r"fnv1a [0-9a-f]{16}", p.stdout)) == 29
            for name, arr in want.items():
                got = np.fromfile(out / f"{name}.bin", dtype=arr.dtype)
                assert got.tobytes() == np.ascontiguousarray(arr).tobytes(), (link, per, name)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_noaa_check_on_the_fake_library(tmp_path, sanitize):
    """noaa_check and the real stream_op.cpp as one program of its own, on the fake HIP runtime, the tests' fake library (unchanged)
    and fake_noaa.cpp, whose three operators are plain bit-by-bit loops: all 29 outputs are the definition chain's, whatever the
    block size and the link."""
    hip_inc = "/opt/rocm/include"
    if not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("needs the HIP headers")
    out = os.path.join(FAKE, "build", "address_noaa" if sanitize else "plain_noaa")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "noaa_check")
    flags = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined"] if sanitize else []
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-Wall", "-pthread",
                        "-D__HIP_PLATFORM_AMD__", "-DFAKE_HIP", f"-I{hip_inc}", f"-I{HOST}", f"-I{os.path.join(ROOT, 'include')}", "-o", exe,
                        os.path.join(HOST, "examples", "noaa_check.cpp"), os.path.join(ROOT, "qdsp_amd", "csrc", "stream_op.cpp"),
                        os.path.join(FAKE, "fake_hip_runtime.cpp"), os.path.join(FAKE, "fake_qdsp_hip.cpp"), os.path.join(FAKE, "fake_noaa.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    frames, want = noaa_check_input()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1 exitcode=68")
    run_noaa_check(exe, tmp_path, frames, want, env)
