#!/usr/bin/env python3
"""Records tests/golden/rs_ref_codes.npz: what libcorrect's own correct_reed_solomon_decode answers for the codes of
tests/_rs_ref.py's ODD_CODES, with the keys of rs_ref_io.npz (params_i, words_i, sent_i, kind_i, rc_i, order_i, msg_i).

Needs oracle/_ref/librs_ref.so (make -C oracle rs_ref REFERENCE=<the reference's tree>): libcorrect's Reed-Solomon sources and
oracle/rs_ref_shim.c.  Encoding and decoding are libcorrect's; this script only chooses messages and error places, from fixed
seeds, so that a second run writes the same file byte for byte.  Per code at most 64 words (kind_i, tests/_rs_ref.py):

    e = 0 .. t        e errors at random places (t = num_roots // 2)
    KIND_ENDS         errors in byte 0 and in byte 254 (the highest and the lowest coefficient)
    KIND_PARITY       errors in the parity bytes only
    KIND_LANE63       t errors, as many as fit in coefficients 252 .. 254 (bytes 2, 1, 0): the three of the kernel's last lane
    KIND_STRADDLE[b]  t errors whose locator roots are the elements b - 1, b, b - 2, b + 1, ... (and b, b - 1, b + 1, ...) for
                      b = 64, 128, 192: on both sides of the cuts between the kernel's four root-search passes; the places come
                      from Code.loc, the definition's table of libcorrect's root-to-place search
    KIND_OVER + e     t + e errors, e = 1 .. 3: of 4000 candidates the first ones libcorrect fails on and the first ones it takes
                      to another codeword, half the remaining words each where both occur, else what comes

Run:  python tests/golden/make_rs_codes.py
"""
import ctypes as C
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import _rs_ref as R  # noqa: E402

MAX_WORDS, CANDIDATES = 64, 4000


def load():
    L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "librs_ref.so"))
    L.correct_reed_solomon_create.restype = C.c_void_p
    L.correct_reed_solomon_create.argtypes = [C.c_uint16, C.c_uint8, C.c_uint8, C.c_size_t]
    L.correct_reed_solomon_destroy.argtypes = [C.c_void_p]
    for f in (L.correct_reed_solomon_encode, L.correct_reed_solomon_decode):
        f.restype = C.c_ssize_t
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.rs_ref_locator_order.restype = C.c_uint
    L.rs_ref_locator_order.argtypes = [C.c_void_p]
    L.rs_ref_clear_locator_order.argtypes = [C.c_void_p]
    return L


class Lib:
    def __init__(self, L, params):
        self.L, self.k = L, 255 - params[3]
        self.rs = L.correct_reed_solomon_create(*params)
        assert self.rs

    def encode(self, msg):
        out = np.zeros(255, np.uint8)
        assert self.L.correct_reed_solomon_encode(self.rs, msg.ctypes.data, self.k, out.ctypes.data) == 255
        return out

    def decode(self, word):
        msg = np.zeros(self.k, np.uint8)
        self.L.rs_ref_clear_locator_order(self.rs)
        rc = self.L.correct_reed_solomon_decode(self.rs, word.ctypes.data, 255, msg.ctypes.data)
        if rc < 0:
            msg[:] = 0
        return int(rc), int(self.L.rs_ref_locator_order(self.rs)), msg

    def close(self):
        self.L.correct_reed_solomon_destroy(self.rs)


def around(b, first, t):
    """t elements alternating around the cut b: b - 1, b, b - 2, b + 1, ... (first = 0) or b, b - 1, b + 1, b - 2, ... (first = 1)."""
    lo, hi = [b - 1 - i for i in range(t)], [b + i for i in range(t)]
    seq = [v for pair in (zip(lo, hi) if first == 0 else zip(hi, lo)) for v in pair]
    return np.asarray(seq[:t], np.int64)


def record(L, params, rng):
    lib, code = Lib(L, params), R.Code(*params)
    k, t = code.k, params[3] // 2
    rows = []

    def word(kind, places, lib=lib):
        sent = rng.integers(0, 256, k).astype(np.uint8)
        w = lib.encode(sent)
        places = np.asarray(places, np.int64)
        assert len(set(places.tolist())) == len(places) and (len(places) == 0 or (0 <= places.min() and places.max() <= 254))
        w[places] ^= rng.integers(1, 256, len(places)).astype(np.uint8)
        return kind, sent, w

    def rand(n, lo=0, hi=255, without=()):
        pool = np.setdiff1d(np.arange(lo, hi), np.asarray(without, np.int64))
        return rng.choice(pool, n, replace=False)

    for e in range(t + 1):
        for _ in range(3 if t <= 3 else 2):
            rows.append(word(e, rand(e)))
    rows.append(word(R.KIND_ENDS, [0, 254][:t]))                              # (t = 1: one word for either end)
    rows.append(word(R.KIND_ENDS, [254, 0][:t] + rand(int(rng.integers(0, max(t - 2, 0) + 1)), 1, 254).tolist()))
    rows.append(word(R.KIND_PARITY, rand(1, k, 255)))
    rows.append(word(R.KIND_PARITY, rand(t, k, 255)))
    for _ in range(2):
        m = min(t, 3)
        rows.append(word(R.KIND_LANE63, rand(m, 0, 3).tolist() + rand(t - m, 3, 255).tolist()))
    for b, kind in R.KIND_STRADDLE.items():
        for first in (0, 1):
            rows.append(word(kind, 254 - code.loc[around(b, first, t)]))      # coefficient i is byte 254 - i
    room = min(20, MAX_WORDS - len(rows))
    cand = []
    for i in range(CANDIDATES):
        e = 1 + i % 3
        kind, sent, w = word(R.KIND_OVER + e, rand(t + e))
        rc, _, msg = lib.decode(w)
        cand.append((kind, sent, w, "fail" if rc < 0 else ("mis" if not np.array_equal(msg, sent) else "back")))
    have = {"fail": 0, "mis": 0, "back": 0}
    pick = []
    for i, c in enumerate(cand):                                             # half each, in the order they came
        if c[3] != "back" and have[c[3]] < room // 2:
            have[c[3]] += 1
            pick.append(i)
    for i, c in enumerate(cand):                                             # and what comes, where one kind is too rare
        if len(pick) < room and i not in pick:
            pick.append(i)
    rows += [cand[i][:3] for i in sorted(pick)]
    assert len(rows) <= MAX_WORDS
    kind = np.asarray([r[0] for r in rows], np.int32)
    sent, words = np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])
    ans = [lib.decode(w) for w in words]
    lib.close()
    return {"params": np.asarray(params, np.int32), "words": words, "sent": sent, "kind": kind, "rc": np.asarray([a[0] for a in ans], np.int32),
            "order": np.asarray([a[1] for a in ans], np.int32), "msg": np.stack([a[2] for a in ans])}


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates, so that the same arrays give the same file."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    L = load()
    out = {}
    for ci, params in enumerate(R.ODD_CODES):
        rec = record(L, params, np.random.default_rng(1000 + ci))
        good = rec["rc"] >= 0
        mis = good & (rec["msg"] != rec["sent"]).any(axis=1)
        print(f"{params}: {len(good)} words, {int((~good).sum())} failed, {int(mis.sum())} taken to another codeword")
        for name, a in rec.items():
            out[f"{name}_{ci}"] = a
    write_npz(os.path.join(HERE, "rs_ref_codes.npz"), out)


if __name__ == "__main__":
    main()
