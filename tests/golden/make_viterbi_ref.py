#!/usr/bin/env python3
"""Records tests/golden/viterbi_ref_io.npz: what libcorrect's own correct_convolutional_decode / _decode_soft answer, every frame
on a freshly created correct_convolutional, and a few of its encodings.

Needs oracle/_ref/libconv_ref.so, libcorrect's convolutional sources as they are:

    gcc -O2 -fPIC -shared -I<reference>/src/libcorrect <reference>/src/libcorrect/convolutional/*.c -o oracle/_ref/libconv_ref.so

Only seeds, parameters and answers are stored: the inputs come from tests/_viterbi_ref.py's make_input(seed), so a second run
writes the same file byte for byte.  Cases (rows of `cases`: rate, order, poly0, poly1, poly2, soft, kind, sets, seed, returned):
the eight published codes and ODD_CODE, hard and soft, coded frames with moderate noise, pure noise and (soft) bytes of 0 and 255
only, at edge_sets(rate, order); rate 3 order 7 at 1200 and 1203 sets (a renormalisation and a traceback on one step); 8168 sets
for (2, 7) and (2, 9).  `out` / `out_off`: the decoded bytes back to back, `returned` each.  `enc_*`: messages and encodings.

Run:  python tests/golden/make_viterbi_ref.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _viterbi_ref as V  # noqa: E402
from make_rs_codes import write_npz  # noqa: E402


def load():
    L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libconv_ref.so"))
    L.correct_convolutional_create.restype = C.c_void_p
    L.correct_convolutional_create.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p]
    L.correct_convolutional_destroy.argtypes = [C.c_void_p]
    L.correct_convolutional_encode_len.restype = C.c_size_t
    L.correct_convolutional_encode_len.argtypes = [C.c_void_p, C.c_size_t]
    L.correct_convolutional_encode.restype = C.c_size_t
    L.correct_convolutional_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    for f in (L.correct_convolutional_decode, L.correct_convolutional_decode_soft):
        f.restype = C.c_ssize_t
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return L


SENTINEL = 0xA5


def lib_decode(L, rate, order, poly, x, sets, soft):
    """On a fresh object.  Returns (returned length, the bytes written)."""
    p = (C.c_uint16 * rate)(*poly)
    conv = L.correct_convolutional_create(rate, order, p)
    assert conv
    msg = np.full(sets // 8 + 64, SENTINEL, np.uint8)
    x = np.ascontiguousarray(np.concatenate([x, np.zeros(8, np.uint8)]))              # (the bit reader may look one byte ahead)
    rc = (L.correct_convolutional_decode_soft if soft else L.correct_convolutional_decode)(conv, x.ctypes.data, sets * rate, msg.ctypes.data)
    L.correct_convolutional_destroy(conv)
    assert rc >= 0 and (msg[rc:] == SENTINEL).all(), "bytes behind the returned length were written"
    return int(rc), msg[:rc].copy()


def lib_encode(L, rate, order, poly, msg):
    p = (C.c_uint16 * rate)(*poly)
    conv = L.correct_convolutional_create(rate, order, p)
    nbits = L.correct_convolutional_encode_len(conv, msg.size)
    out = np.zeros((nbits + 7) // 8, np.uint8)
    assert L.correct_convolutional_encode(conv, msg.ctypes.data, msg.size, out.ctypes.data) == nbits
    L.correct_convolutional_destroy(conv)
    return out


def case_list():
    codes = [(r, o, p) for (r, o), p in sorted(V.CODES.items())] + [V.ODD_CODE]
    cases, seed = [], 5000
    for rate, order, poly in codes:
        lengths = V.edge_sets(rate, order)
        if (rate, order) == (3, 7) and poly == V.CODES[(3, 7)]:
            lengths = lengths + [1200, 1203]
        if rate == 2 and order in (7, 9) and poly == V.CODES[(2, order)]:
            lengths = lengths + [8168]
        for soft in (0, 1):
            for sets in lengths:
                kinds = [V.KIND_CODED, V.KIND_NOISE] + ([V.KIND_SATURATED] if soft else [])
                if sets == 8168:
                    kinds = [V.KIND_CODED] if soft else [V.KIND_NOISE]
                for kind in kinds:
                    seed += 1
                    cases.append((rate, order, poly[0], poly[1], poly[2] if rate == 3 else 0, soft, kind, sets, seed))
    return cases


def main():
    L = load()
    rows, outs = [], []
    for rate, order, p0, p1, p2, soft, kind, sets, seed in case_list():
        poly = (p0, p1, p2)[:rate]
        x = V.make_input(rate, order, poly, sets, bool(soft), kind, seed)
        rc, y = lib_decode(L, rate, order, poly, x, sets, bool(soft))
        rows.append((rate, order, p0, p1, p2, soft, kind, sets, seed, rc))
        outs.append(y)
    off = np.concatenate([[0], np.cumsum([len(y) for y in outs])]).astype(np.int64)
    enc_msg, enc_out, enc_off = [], [], [0]
    rng = np.random.default_rng(77)
    codes = [(r, o, p) for (r, o), p in sorted(V.CODES.items())] + [V.ODD_CODE]
    for rate, order, poly in codes:
        m = rng.integers(0, 256, 6).astype(np.uint8)
        e = lib_encode(L, rate, order, poly, m)
        enc_msg.append(m)
        enc_out.append(e)
        enc_off.append(enc_off[-1] + e.size)
    arrays = {"cases": np.asarray(rows, np.int32), "out": np.concatenate(outs), "out_off": off,
              "enc_codes": np.asarray([(r, o, p[0], p[1], p[2] if r == 3 else 0) for r, o, p in codes], np.int32),
              "enc_msg": np.stack(enc_msg), "enc_out": np.concatenate(enc_out), "enc_off": np.asarray(enc_off, np.int64)}
    path = os.path.join(HERE, "viterbi_ref_io.npz")
    write_npz(path, arrays)
    print(f"{len(rows)} frames, {int(off[-1])} decoded bytes -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
