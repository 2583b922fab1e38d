"""The Reed-Solomon decoder and FalconRS without a GPU: the numpy definition the GPU tests compare against (tests/_rs_ref.py)
against two recordings of libcorrect's own answers (three codes with multiples of four roots; eight with 2 .. 31 roots off that grid,
first roots 0 and 255 and other gaps), the two CCSDS tables from their closed forms, the frame layout, the library's
surface and parameter errors, fec.py's argument checks, and the C++ mirror's harness on a fake library, plain and under the
sanitizers.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _rs_ref as R
from qdsp_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "qdsp_amd", "host")
FAKE = os.path.join(HERE, "fake_hip")
EINVAL = -10001
CONFIGS = ((0x187, 120, 11, 16), (0x187, 112, 11, 32), (0x11d, 1, 1, 4))

RS_ENTRY = ["create", "set_maps", "out_size", "frame_in_bytes", "frame_out_bytes", "process", "process_ex", "process_dev", "process_batch_dev",
            "get_counts", "destroy"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "rs_ref_io.npz"))


def test_symbols_declared_and_exported():
    want = {"qdsp_hip_rs_" + n for n in RS_ENTRY} | {"qdsp_hip_falcon_rs_create"}
    assert want <= set(capi.declared_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    have = set(re.findall(r"\bT (qdsp_hip_(?:falcon_)?rs_\w+)", out))
    assert have == want, (sorted(want - have), sorted(have - want))
    L = capi.load()
    assert all(getattr(L, s).argtypes is not None for s in want), "declared in capi.py"


def test_fec_surface_and_ops_untouched():
    from qdsp_amd import fec, ops

    assert set(fec.__all__) == {"RsDecoder", "FalconRs", "ccsds_dual_basis", "ccsds_randomizer"}
    assert issubclass(fec.RsDecoder, ops._RowOp) and issubclass(fec.RsDecoder, ops._Counts) and issubclass(fec.FalconRs, fec.RsDecoder)
    for name in ("process", "process_batch", "process_ex", "out_size", "counts", "set_maps", "last_kernel", "time_dev", "reset"):
        assert callable(getattr(fec.RsDecoder, name)), name
    assert not hasattr(ops, "RsDecoder") and not hasattr(ops, "FalconRs")


# ---- the definition against libcorrect's recorded answers ----

@pytest.mark.parametrize("ci", range(3))
def test_definition_equals_the_recording_word_for_word(golden, ci):
    """tests/golden/rs_ref_io.npz: received words and what libcorrect's correct_reed_solomon_decode returned for them (return code,
    message, the order its locator search left), recorded once by a program outside this repository that links libcorrect's own
    reed-solomon sources."""
    p = golden[f"params_{ci}"]
    assert tuple(int(v) for v in p) == CONFIGS[ci]
    code = R.Code(*p)
    words, rc, order, msg = golden[f"words_{ci}"], golden[f"rc_{ci}"], golden[f"order_{ci}"], golden[f"msg_{ci}"]
    assert words.shape[1] == 255 and msg.shape == (len(words), code.k) and set(np.unique(rc).tolist()) <= {-1, code.k}
    m, ok, o = R.decode(code, words)
    assert np.array_equal(ok, rc >= 0), np.nonzero(ok != (rc >= 0))
    assert np.array_equal(o, order), np.nonzero(o != order)
    assert np.array_equal(m[ok], msg[ok])


@pytest.mark.parametrize("ci", range(3))
def test_the_recording_covers_the_stated_patterns(golden, ci):
    code = R.Code(*golden[f"params_{ci}"])
    t = code.num_roots // 2
    words, sent, kind, rc, order, msg = (golden[f"{n}_{ci}"] for n in ("words", "sent", "kind", "rc", "order", "msg"))
    good = rc >= 0
    for e in range(t + 1):                                         # 0 .. t errors at random places: corrected, order = errors
        sel = kind == e
        assert sel.sum() >= 3 and good[sel].all() and (order[sel] == e).all() and np.array_equal(msg[sel], sent[sel])
    edge = kind == 100                                             # errors in byte 0 and in byte 254 (coefficient 0)
    nerr = (words[edge] != code.encode(sent[edge])).sum(axis=1)
    assert edge.sum() >= 3 and good[edge].all() and np.array_equal(msg[edge], sent[edge]) and np.array_equal(order[edge], nerr)
    cw = code.encode(sent[edge])
    assert (words[edge][:, 0] != cw[:, 0]).any() and (words[edge][:, 254] != cw[:, 254]).any()
    par = kind == 101                                              # errors in the parity bytes only
    assert par.sum() >= 3 and good[par].all() and np.array_equal(words[par][:, :code.k], sent[par]) and (order[par] > 0).all()
    over = (kind > 200) & (kind < 400)                             # t + 1 .. t + 3 errors
    assert (~good[over]).sum() >= 8
    mis = good & (kind < 400) & (msg != sent).any(axis=1)          # ... that libcorrect takes to another codeword
    assert mis.sum() >= 8 and (kind[mis] > 200).all()
    assert (kind == 400).sum() == 2 and len(words) <= 120


@pytest.fixture(scope="module")
def codes():
    return np.load(os.path.join(HERE, "golden", "rs_ref_codes.npz"))


@pytest.mark.parametrize("ci", range(len(R.ODD_CODES)))
def test_definition_equals_the_recording_of_the_odd_codes(codes, ci):
    """tests/golden/rs_ref_codes.npz: libcorrect's answers for R.ODD_CODES -- num_roots 2, 3, 5, 6, 7, 10, 30 and 31, first roots 0
    and 255, gaps 2, 7 and 254 -- recorded by tests/golden/make_rs_codes.py through oracle/_ref/librs_ref.so (make -C oracle rs_ref)."""
    p = codes[f"params_{ci}"]
    assert tuple(int(v) for v in p) == R.ODD_CODES[ci]
    code = R.Code(*p)
    words, rc, order, msg = codes[f"words_{ci}"], codes[f"rc_{ci}"], codes[f"order_{ci}"], codes[f"msg_{ci}"]
    assert words.shape[1] == 255 and msg.shape == (len(words), code.k) and set(np.unique(rc).tolist()) <= {-1, code.k}
    m, ok, o = R.decode(code, words)
    assert np.array_equal(ok, rc >= 0), np.nonzero(ok != (rc >= 0))
    assert np.array_equal(o, order), np.nonzero(o != order)
    assert np.array_equal(m[ok], msg[ok])


@pytest.mark.parametrize("ci", range(len(R.ODD_CODES)))
def test_the_odd_codes_recording_covers_the_stated_places(codes, ci):
    code = R.Code(*codes[f"params_{ci}"])
    nr, t, k = code.num_roots, code.num_roots // 2, code.k
    words, sent, kind, rc, order, msg = (codes[f"{n}_{ci}"] for n in ("words", "sent", "kind", "rc", "order", "msg"))
    assert len(words) <= 64 and np.array_equal(code.encode(sent)[:, :k], sent)
    diff = words != code.encode(sent)                               # the definition's encoder is libcorrect's: where the errors are
    nerr, good = diff.sum(axis=1), rc >= 0
    within = kind < R.KIND_OVER
    assert (nerr[within] <= t).all() and good[within].all() and np.array_equal(msg[within], sent[within])
    assert np.array_equal(order[within], nerr[within])
    for e in range(t + 1):                                         # 0 .. t errors at random places
        assert ((kind == e) & (nerr == e)).sum() >= 2, e
    ends = kind == R.KIND_ENDS
    assert diff[ends][:, 0].any() and diff[ends][:, 254].any() and (t < 2 or (diff[ends][:, 0] & diff[ends][:, 254]).any())
    par = kind == R.KIND_PARITY
    assert par.sum() >= 2 and not diff[par][:, :k].any() and nerr[par].min() >= 1 and nerr[par].max() == t
    l63 = kind == R.KIND_LANE63                                     # coefficients 252 .. 254 are bytes 2, 1, 0
    assert l63.sum() >= 2 and (nerr[l63] == t).all() and (diff[l63][:, :3].sum(axis=1) == min(t, 3)).all()
    inv = np.zeros(255, np.int64)                                  # coefficient -> the locator's root for an error there
    inv[code.loc[1:]] = np.arange(1, 256)
    for b, kd in R.KIND_STRADDLE.items():
        sel = np.flatnonzero(kind == kd)
        assert len(sel) >= 2
        roots = [np.sort(inv[254 - np.flatnonzero(diff[i])]) for i in sel]
        assert all(len(r) == t and r.max() - r.min() == t - 1 for r in roots), roots       # t neighbours ...
        assert any(b - 1 in r for r in roots) and any(b in r for r in roots)               # ... of the cut,
        assert t < 2 or all(b - 1 in r and b in r for r in roots)                          # on both sides of it
    over = kind > R.KIND_OVER
    assert set(np.unique(kind[over] - R.KIND_OVER).tolist()) <= {1, 2, 3} and np.array_equal(nerr[over], t + kind[over] - R.KIND_OVER)
    mis = good & over & (msg != sent).any(axis=1)
    assert (~good[over]).sum() >= 4 and (nr >= 10 or mis.sum() >= 4), ((~good[over]).sum(), mis.sum())    # (rare from 10 roots on)
    assert not (good & over & ~mis).any()                          # (no word beyond t comes back as sent)
    # a miscorrection is another codeword, `order` places away: at most t, or with an odd number of roots, where the locator search
    # takes one step more and may grow once more, (num_roots + 1) / 2
    dist = (code.encode(msg[mis]) != words[mis]).sum(axis=1)
    assert (dist <= (nr + 1) // 2).all() and np.array_equal(order[mis], dist)


def test_miscorrected_words_come_out_as_the_other_codeword(golden):
    for ci in range(3):
        code = R.Code(*golden[f"params_{ci}"])
        words, sent, kind, rc, msg = (golden[f"{n}_{ci}"] for n in ("words", "sent", "kind", "rc", "msg"))
        mis = (rc >= 0) & (kind < 400) & (msg != sent).any(axis=1)
        cw = code.encode(msg[mis])
        d_other, d_sent = (cw != words[mis]).sum(axis=1), (code.encode(sent[mis]) != words[mis]).sum(axis=1)
        assert (d_other <= code.num_roots // 2).all() and (d_sent > code.num_roots // 2).all()
        m, ok, _ = R.decode(code, words[mis])
        assert ok.all() and np.array_equal(m, msg[mis])


def test_definition_rate():
    """A few thousand codewords per second, so that the GPU tests stay at seconds."""
    import time

    code = R.Code(*CONFIGS[0])
    rng = np.random.default_rng(0)
    w = code.encode(rng.integers(0, 256, (2000, code.k)))
    for i in range(len(w)):
        w[i, rng.choice(255, i % 11, replace=False)] ^= 0x5a
    t0 = time.perf_counter()
    m, ok, order = R.decode(code, w)
    dt = time.perf_counter() - t0
    assert np.array_equal(order[ok], (np.arange(2000) % 11)[ok]) and ok[np.arange(2000) % 11 <= 8].all()
    assert len(w) / dt > 2000, dt


# ---- the two CCSDS tables ----

def test_closed_form_tables():
    from qdsp_amd import fec

    to_db, from_db = R.ccsds_dual_basis()
    rnd = R.ccsds_randomizer()
    assert rnd.shape == (255,) and rnd[:8].tolist() == [0xFF, 0x48, 0x0E, 0xC0, 0x9A, 0x0D, 0x70, 0xBC]
    assert to_db[0] == 0 and to_db[1] == 0x7b and to_db[2] == 0xaf and from_db[1] == 0xcc
    assert sorted(to_db.tolist()) == list(range(256)) and np.array_equal(from_db[to_db], np.arange(256))
    a, b = np.meshgrid(np.arange(256), np.arange(256))
    assert np.array_equal(to_db[a ^ b], to_db[a] ^ to_db[b]), "GF(2)-linear"
    # the sequence has the period of its degree-8 recurrence
    bits = np.unpackbits(rnd)
    assert bits.sum() == 1024 and not any(np.array_equal(bits[:2040 - s], bits[s:]) for s in (1, 3, 5, 15, 17, 51, 85))
    t2, f2 = fec.ccsds_dual_basis()
    assert np.array_equal(t2, to_db) and np.array_equal(f2, from_db) and np.array_equal(fec.ccsds_randomizer(), rnd)


# ---- the frame layout ----

@pytest.mark.parametrize("full_out", [0, 1])
def test_frame_layout(full_out):
    rng = np.random.default_rng(4)
    code = R.Code(*CONFIGS[0])
    in_map = rng.permutation(256).astype(np.uint8)
    out_map = rng.permutation(256).astype(np.uint8)
    xor = rng.integers(0, 256, 7).astype(np.uint8)
    lay = R.Layout(code, 3, 2, full_out, in_map, out_map, xor)
    assert lay.frame_in == 2 + 765 and lay.frame_out == (765 if full_out else 3 * code.k)
    msgs = rng.integers(0, 256, (4, 3, code.k)).astype(np.uint8)
    frames = lay.encode(msgs)
    frames[:, :2] = 0xEE                                           # the skipped bytes are not looked at
    assert np.array_equal(in_map[frames[0, 2 + 5 * 3 + 1]], msgs[0, 1, 5])      # cw[c][p] = in_map[d[p I + c]]
    frames[1, 2 + 3 * 10 + 2] ^= 1                                 # one error in codeword 2 of frame 1
    frames[3, 2 + np.arange(12) * 3] ^= 0x80                      # twelve in codeword 0 of frame 3
    out, good, errs = lay.decode(frames)
    assert good.tolist() == [True, True, True, False] and errs.tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 0], [-1, 0, 0]]
    i = np.arange(lay.frame_out)
    for f in range(3):
        body = np.where(i // 3 < code.k, msgs[f, i % 3, np.minimum(i // 3, code.k - 1)], 0).astype(np.uint8)
        assert np.array_equal(out[f], out_map[body] ^ xor[i % 7])
    if full_out:
        assert np.array_equal(out[0, 3 * code.k:], out_map[0] ^ xor[np.arange(3 * code.k, 765) % 7])


def test_recorded_frames_of_the_reference_sequence(golden):
    """Ten Falcon frames through the reference block's own sequence -- fromDB de-interleave, five libcorrect decodes, toDB
    re-interleave, randVals -- recorded with the words above."""
    lay = R.falcon_layout()
    frames, fgood, fout = golden["frames"], golden["frame_good"], golden["frame_out"]
    assert frames.shape == (10, 1279) and fout.shape == (10, 1275) and 3 <= fgood.sum() <= 7
    out, good, errs = lay.decode(frames)
    assert np.array_equal(good, fgood) and np.array_equal(out[good], fout[fgood])
    assert (errs[good] >= 0).all() and (errs[~good] < 0).any(axis=1).all() and errs.max() == 8
    # the last 80 bytes of a good frame: toDB[0] ^ randVals
    assert np.array_equal(out[good][:, 1195:], np.broadcast_to(R.ccsds_randomizer()[np.arange(1195, 1275) % 255], (int(good.sum()), 80)))


# ---- parameter errors (checked before a device is looked for) ----

def test_create_parameter_errors():
    L = capi.load()
    h = C.c_void_p()
    m = (C.c_uint8 * 256)(*range(256))
    p = C.cast(m, C.c_void_p)
    ok = dict(nchan=1, maxb=16, poly=0x187, first=120, gap=11, roots=16, depth=5, skip=4, full=1, xor=p, xlen=255)
    bad = [dict(poly=0x11b), dict(poly=0x87), dict(poly=0x387), dict(poly=0x186), dict(first=-1), dict(first=256), dict(gap=0), dict(gap=3),
           dict(gap=85), dict(gap=255), dict(roots=1), dict(roots=33), dict(depth=0), dict(depth=9), dict(skip=-1), dict(skip=65),
           dict(full=2), dict(xlen=0), dict(xlen=1276), dict(nchan=0), dict(nchan=65536), dict(maxb=-1)]
    for b in bad:
        a = dict(ok, **b)
        rc = L.qdsp_hip_rs_create(C.byref(h), 0, a["nchan"], a["maxb"], a["poly"], a["first"], a["gap"], a["roots"], a["depth"], a["skip"],
                                  a["full"], p, p, a["xor"], a["xlen"])
        assert rc == EINVAL and not h.value, b
    assert L.qdsp_hip_rs_create(None, 0, 1, 16, 0x187, 120, 11, 16, 5, 4, 1, None, None, None, 0) == EINVAL
    assert L.qdsp_hip_falcon_rs_create(None, 0, 1, 16) == EINVAL and L.qdsp_hip_falcon_rs_create(C.byref(h), 0, 0, 16) == EINVAL
    junk = C.create_string_buffer(64)
    assert L.qdsp_hip_rs_out_size(junk, 1) == EINVAL and L.qdsp_hip_rs_frame_in_bytes(junk) == EINVAL
    assert L.qdsp_hip_rs_frame_out_bytes(junk) == EINVAL and L.qdsp_hip_rs_set_maps(junk, None, None, None, 0) == EINVAL
    assert L.qdsp_hip_rs_process_dev(junk, None, 0, None, None) == EINVAL and L.qdsp_hip_rs_get_counts(junk, None) == EINVAL
    assert L.qdsp_hip_rs_process_batch_dev(junk, None, 0, 0, None, None, 0, None, None, None) == EINVAL


def test_fec_argument_checks():
    from qdsp_amd import fec

    ident = np.arange(256, dtype=np.uint8)
    for kw in (dict(prim_poly=0x87), dict(prim_poly=0x200), dict(first_root=256), dict(first_root=-1), dict(root_gap=0), dict(root_gap=5),
               dict(root_gap=51), dict(num_roots=1), dict(num_roots=33), dict(depth=0), dict(depth=9), dict(skip=-1), dict(skip=65),
               dict(in_map=ident[:255]), dict(out_map=ident.astype(np.int32)), dict(in_map=ident.reshape(16, 16)),
               dict(xor=np.zeros(0, np.uint8)), dict(xor=np.zeros(256, np.uint8)), dict(xor=np.zeros(4, np.float32))):
        a = dict(dict(prim_poly=0x187, first_root=120, root_gap=11, num_roots=16), **kw)
        with pytest.raises(ValueError):
            fec.RsDecoder(**a)
    with pytest.raises(ValueError):
        fec.RsDecoder._whole_frames(_Sized(255), 254)              # process: whole frames only
    assert fec.RsDecoder._whole_frames(_Sized(255), 510) == 2


class _Sized:
    def __init__(self, frame_in):
        self.frame_in = frame_in


# ---- the C++ mirror ----

def test_mirror_header_compiles_with_the_reference_usage(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text("""
#include <dsp/falcon_fec.h>
int main() {
    dsp::stream<uint8_t> a;
    dsp::FalconRS r(&a);
    dsp::FalconRS s; s.init(&a);
    return r.out.writeBuf == nullptr;
}
""")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", HOST,
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_build_makes_falcon_check():
    subprocess.check_call(["make", "-C", HOST, "build/falcon_check"], stdout=subprocess.DEVNULL, timeout=300)
    exe = os.path.join(HOST, "build", "falcon_check")
    assert os.access(exe, os.X_OK)
    und = subprocess.check_output(["nm", "-D", "--undefined-only", exe], text=True)
    assert "qdsp_hip_rs_process_ex" in und and "qdsp_hip_falcon_rs_create" in und
    for other in ("graph_check", "demod_check", "clock_check", "psk_check", "frame_check"):
        p = os.path.join(HOST, "build", other)
        if os.path.exists(p):
            assert "qdsp_hip_rs_" not in subprocess.check_output(["nm", "-D", "--undefined-only", p], text=True), other


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_falcon_check_on_the_fake_library(tmp_path, golden, sanitize):
    """falcon_check and the real stream_op.cpp as one program of its own, on the fake HIP runtime, the tests' fake library
    (unchanged) and fake_rs.cpp, whose decoder is a plain scalar loop: the good frames are those of the definition, whatever the
    block size and the link."""
    hip_inc = "/opt/rocm/include"
    if not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("needs the HIP headers")
    out = os.path.join(FAKE, "build", "address_rs" if sanitize else "plain_rs")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "falcon_check")
    flags = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined"] if sanitize else []
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-Wall", "-pthread",
                        "-D__HIP_PLATFORM_AMD__", "-DFAKE_HIP", f"-I{hip_inc}", f"-I{HOST}", f"-I{os.path.join(ROOT, 'include')}", "-o", exe,
                        os.path.join(HOST, "examples", "falcon_check.cpp"), os.path.join(ROOT, "qdsp_amd", "csrc", "stream_op.cpp"),
                        os.path.join(FAKE, "fake_hip_runtime.cpp"), os.path.join(FAKE, "fake_qdsp_hip.cpp"), os.path.join(FAKE, "fake_rs.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lay = R.falcon_layout()
    rng = np.random.default_rng(6)
    frames = lay.encode(rng.integers(0, 256, (12, 5, lay.code.k)).astype(np.uint8))
    for f in range(12):
        for c in range(5):
            ne = [0, 1, 8, 3, 9, 0, 12, 5, 8, 2, 0, 7][(f + 3 * c) % 12] if f % 4 else (f + c) % 9
            frames[f, 4 + rng.choice(255, ne, replace=False) * 5 + c] ^= rng.integers(1, 256, ne).astype(np.uint8)
    frames = np.concatenate([golden["frames"], frames])
    want, good, _ = lay.decode(frames)
    assert 5 <= good.sum() < len(frames)
    frames.tofile(tmp_path / "x.u8")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1 exitcode=68")
    for link in ("host", "dev"):
        for per in (1, 3, 22):
            y = tmp_path / f"y_{link}.bin"
            p = subprocess.run([exe, link, "x.u8", str(y), str(per)], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
            bad = [ln for ln in p.stderr.splitlines() if any(k in ln for k in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:"))]
            assert p.returncode == 0 and not bad and "graph ok" in p.stdout, (p.stdout, p.stderr[-3000:])
            got = np.fromfile(y, dtype=np.uint8)
            assert got.tobytes() == want[good].tobytes(), (link, per)
