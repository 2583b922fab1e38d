"""The numpy definition of the Reed-Solomon decoder and of the frame layout (include/qdsp_hip.h: Reed-Solomon decoder and
FalconRS), vectorised over codewords: the locator search and the root search run over a batch with masks.  It follows libcorrect's
correct_reed_solomon_decode step by step, also where that is not the textbook's: the order its locator search tracks, the
coefficients it leaves stale, its log 1 = 255, its search for the position of a root.  tests/golden/rs_ref_io.npz holds what
libcorrect itself answered (tests/test_rs_cpu.py compares word for word).
"""
import numpy as np

N = 255

# The codes of tests/golden/rs_ref_codes.npz (tests/golden/make_rs_codes.py records libcorrect's answers for them): num_roots off
# the kernel's grid of four syndromes per dword, the smallest and the largest it takes, first roots 0 and 255, gaps 2, 7 and 254.
ODD_CODES = ((0x11d, 1, 1, 2), (0x11d, 0, 1, 3), (0x187, 255, 2, 5), (0x12b, 7, 254, 6), (0x11d, 1, 1, 7), (0x187, 112, 11, 10),
             (0x11d, 0, 1, 30), (0x12d, 3, 7, 31))
# kind_i of that file: 0 .. t = that many errors at random places, and
KIND_ENDS, KIND_PARITY, KIND_LANE63 = 100, 101, 102    # errors in byte 0 and byte 254; in the parity only; in coefficients 252 .. 254
KIND_STRADDLE = {64: 103, 128: 104, 192: 105}          # t errors whose locator roots lie around that element of the root search
KIND_OVER = 200                                        # 200 + e: t + e errors, e = 1 .. 3


class Code:
    """RS(255, 255 - num_roots) over GF(2^8) / poly, generator roots alpha^(root_gap (first_root + i)), i < num_roots."""

    def __init__(self, poly, first_root, root_gap, num_roots):
        self.poly, self.first_root, self.root_gap, self.num_roots = int(poly), int(first_root), int(root_gap), int(num_roots)
        self.k = N - self.num_roots
        exp = np.zeros(512, np.uint8)
        log = np.zeros(256, np.uint8)
        e = 1
        exp[0] = 1
        for i in range(1, 512):
            e <<= 1
            if e > 255:
                e ^= self.poly
            exp[i] = e
            if i < 256:
                log[e] = i                      # log[1] ends as 255; log[0] stays 0
        assert len(set(exp[:255].tolist())) == 255 and 0 not in exp[:255], "not a primitive polynomial"
        self.exp, self.log = exp, log
        self.iexp, self.ilog = exp.astype(np.int64), log.astype(np.int64)
        # the logarithm of (generator root i)^k
        i = np.arange(self.num_roots)[:, None]
        k = np.arange(N)[None, :]
        self.syn_pow = (self.root_gap * (self.first_root + i) * k) % 255
        x = np.arange(256)
        # x^j for j <= num_roots, 0^j = 0 (the value at 0 is handled apart)
        self.xpow = np.zeros((self.num_roots + 1, 256), np.uint8)
        for j in range(self.num_roots + 1):
            self.xpow[j, 1:] = exp[(self.ilog[1:] * j) % 255]
        # the position of root x, found as libcorrect finds it: the first j in 0 .. 255 with pow(j, root_gap) == 1 / x, then log[j]
        powj = exp[(self.ilog[x] * self.root_gap) % 255]            # pow(0, gap) = exp[0] = 1
        self.loc = np.zeros(256, np.int64)
        for r in range(1, 256):
            inv = exp[255 + 255 - self.ilog[r]]                    # field_div(1, r) with log 1 = 255
            j = int(np.argmax(powj == inv))
            assert powj[j] == inv
            self.loc[r] = self.ilog[j]
        self.rpow = exp[(self.ilog[x] * (self.first_root - 1)) % 255]   # pow(x, first_root - 1); Python's % is never negative
        # the generator polynomial, highest coefficient first (for encode)
        g = np.array([1], np.uint8)
        for r in range(self.num_roots):
            root = exp[(self.root_gap * (self.first_root + r)) % 255]
            g = np.concatenate([g, [0]]).astype(np.uint8) ^ np.concatenate([[0], self.mul(g, root)]).astype(np.uint8)
        self.gen = g

    def mul(self, a, b):
        a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
        return np.where((a != 0) & (b != 0), self.exp[self.ilog[a] + self.ilog[b]], 0).astype(np.uint8)

    def div(self, a, b):
        a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
        return np.where((a != 0) & (b != 0), self.exp[255 + self.ilog[a] - self.ilog[b]], 0).astype(np.uint8)   # x / 0 = 0

    def encode(self, msg):
        """(n, k) message bytes -> (n, 255) systematic codewords (byte 0 is the highest coefficient)."""
        msg = np.atleast_2d(np.asarray(msg, np.uint8))
        reg = np.zeros((msg.shape[0], self.num_roots), np.uint8)
        for i in range(self.k):
            fb = msg[:, i] ^ reg[:, 0]
            reg = np.concatenate([reg[:, 1:], np.zeros((msg.shape[0], 1), np.uint8)], axis=1) ^ self.mul(fb[:, None], self.gen[None, 1:])
        return np.concatenate([msg, reg], axis=1)


def decode(code, words):
    """(n, 255) received words -> (msg (n, k) uint8, ok (n,) bool, order (n,) int32).  msg of a failed word is the received one's."""
    words = np.atleast_2d(np.asarray(words, np.uint8))
    n, nr = words.shape[0], code.num_roots
    assert words.shape[1] == N
    coeff = words[:, ::-1].copy()                                  # coeff[i] = encoded[254 - i]
    lc = code.ilog[coeff]
    syn = np.zeros((n, nr), np.uint8)
    for i in range(nr):
        syn[:, i] = np.bitwise_xor.reduce(np.where(coeff != 0, code.exp[lc + code.syn_pow[i][None, :]], 0).astype(np.uint8), axis=1)
    dirty = syn.any(axis=1)
    # ---- the locator (reed_solomon_find_error_locator), every word at once ----
    W = 2 * nr + 4
    col = np.arange(W)[None, :]
    C = np.zeros((n, W), np.uint8)
    C[:, 0] = 1
    B = C.copy()
    L = np.zeros(n, np.int64)
    order, lorder = L.copy(), L.copy()
    delay = np.ones(n, np.int64)
    last_d = np.ones(n, np.uint8)
    for i in range(nr):
        d = syn[:, i].copy()
        for j in range(1, i + 1):
            d ^= np.where(j <= L, code.mul(C[:, j], syn[:, i - j]), 0).astype(np.uint8)
        hit = d != 0
        grow = hit & (2 * L <= i)
        keep = hit & ~grow
        src = col - delay[:, None]
        live = (src >= 0) & (src <= lorder[:, None])
        bsrc = np.take_along_axis(B, np.clip(src, 0, W - 1), axis=1)
        term = np.where(live, code.div(code.mul(bsrc, d[:, None]), last_d[:, None]), 0).astype(np.uint8)
        top = lorder + delay
        assert int(top[hit].max(initial=0)) < W
        # the register grows: the last locator is shifted and scaled in place (zeros below the delay, its old values above
        # last order + delay), then the two are exchanged over coefficients 0 .. last order + delay only
        shifted = np.where(col < delay[:, None], 0, np.where(live, term, B)).astype(np.uint8)
        inside = col <= top[:, None]
        g = grow[:, None]
        newC = np.where(g & inside, C ^ shifted, C)
        newB = np.where(g, np.where(inside, C, shifted), B)
        # it does not grow: only the locator changes, and its order is a maximum
        newC = np.where(keep[:, None], C ^ term, newC)
        C, B = newC.astype(np.uint8), newB.astype(np.uint8)
        order, lorder = np.where(grow, top, np.where(keep, np.maximum(order, top), order)), np.where(grow, order, lorder)
        L = np.where(grow, i + 1 - L, L)
        last_d = np.where(grow, d, last_d).astype(np.uint8)
        delay = np.where(grow, 1, delay + 1)
    order = np.where(dirty, order, 0)
    # ---- the roots of the locator's coefficients 0 .. order among all 256 elements ----
    val = np.zeros((n, 256), np.uint8)
    for j in range(min(int(order.max(initial=0)), nr) + 1):
        val ^= np.where((j <= order)[:, None], code.mul(C[:, j, None], code.xpow[j][None, :]), 0).astype(np.uint8)
    val[:, 0] = C[:, 0]                                            # at 0 a polynomial is its constant term
    root = (val == 0) & dirty[:, None]
    ok = ~dirty | (root.sum(axis=1) == order)
    # ---- the values (reed_solomon_find_error_values) ----
    om = np.zeros((n, nr), np.uint8)
    for m in range(nr):
        for i in range(m + 1):
            om[:, m] ^= np.where(i <= order, code.mul(C[:, i], syn[:, m - i]), 0).astype(np.uint8)
    num = np.zeros((n, 256), np.uint8)
    den = np.zeros((n, 256), np.uint8)
    for k in range(nr):
        num ^= code.mul(om[:, k, None], code.xpow[k][None, :])
    for k in range(1, nr + 1, 2):                                  # the formal derivative keeps the odd coefficients
        den ^= np.where((k <= order)[:, None], code.mul(C[:, k, None], code.xpow[k - 1][None, :]), 0).astype(np.uint8)
    ev = code.mul(code.rpow[None, :], code.div(num, den))
    wi, xi = np.nonzero(root & ok[:, None])
    np.bitwise_xor.at(coeff, (wi, code.loc[xi]), ev[wi, xi])
    fixed = np.where(ok[:, None], coeff[:, ::-1], words)
    return fixed[:, :code.k].copy(), ok, order.astype(np.int32)


# ---- the two CCSDS tables, from their closed forms ----

def ccsds_randomizer():
    s = [1] * 8
    for n in range(255 * 8 - 8):
        s.append(s[n] ^ s[n + 3] ^ s[n + 5] ^ s[n + 7])
    return np.packbits(np.array(s, np.uint8))                      # MSB first, 255 bytes


def ccsds_dual_basis():
    """(to_db, from_db): bit (7 - j) of to_db[x] is Tr(alpha^(117 j mod 255) x) over 0x187."""
    c = Code(0x187, 120, 11, 16)
    x = np.arange(256).astype(np.uint8)
    to_db = np.zeros(256, np.uint8)
    for j in range(8):
        y = c.mul(c.exp[(117 * j) % 255], x)
        tr = np.zeros(256, np.uint8)
        for _ in range(8):
            tr ^= y
            y = c.mul(y, y)
        assert set(tr.tolist()) <= {0, 1}
        to_db |= (tr << (7 - j)).astype(np.uint8)
    from_db = np.zeros(256, np.uint8)
    from_db[to_db] = x
    return to_db, from_db


# ---- frames ----

class Layout:
    def __init__(self, code, depth, skip=0, full_out=0, in_map=None, out_map=None, xor=None):
        self.code, self.depth, self.skip, self.full_out = code, int(depth), int(skip), int(full_out)
        ident = np.arange(256).astype(np.uint8)
        self.in_map = ident if in_map is None else np.asarray(in_map, np.uint8)
        self.out_map = ident if out_map is None else np.asarray(out_map, np.uint8)
        self.xor = np.zeros(1, np.uint8) if xor is None else np.asarray(xor, np.uint8)
        self.frame_in = self.skip + N * self.depth
        self.frame_out = (N if full_out else code.k) * self.depth

    def decode(self, frames):
        """(F, frame_in) -> (out (F, frame_out), good (F,) bool, errs (F, depth) int32: -1 failed, else the symbols corrected)."""
        frames = np.asarray(frames, np.uint8).reshape(-1, self.frame_in)
        F, I, k = frames.shape[0], self.depth, self.code.k
        d = self.in_map[frames[:, self.skip:]].reshape(F, N, I)   # d[p I + c] -> [p][c]
        cw = d.transpose(0, 2, 1).reshape(F * I, N)
        msg, ok, order = decode(self.code, cw)
        full = np.zeros((F, I, N), np.uint8)
        full[:, :, :k] = msg.reshape(F, I, k)
        i = np.arange(self.frame_out)
        out = self.out_map[full[:, i % I, i // I]] ^ self.xor[i % len(self.xor)][None, :]
        ok = ok.reshape(F, I)
        return out, ok.all(axis=1), np.where(ok, order.reshape(F, I), -1).astype(np.int32)

    def encode(self, msgs):
        """(F, depth, k) message bytes in the decoder's (mapped) domain -> (F, frame_in) frames with a zero prefix: what decodes to
        them."""
        msgs = np.asarray(msgs, np.uint8)
        F, I = msgs.shape[0], self.depth
        cw = self.code.encode(msgs.reshape(F * I, self.code.k)).reshape(F, I, N)
        return self.interleave(cw)

    def interleave(self, cw):
        """(F, depth, 255) codewords in the decoder's domain -> frames (the input map has to be a permutation)."""
        inv = np.zeros(256, np.uint8)
        inv[self.in_map] = np.arange(256).astype(np.uint8)
        F = cw.shape[0]
        body = inv[cw.transpose(0, 2, 1).reshape(F, N * self.depth)]
        return np.concatenate([np.zeros((F, self.skip), np.uint8), body], axis=1)


def falcon_layout():
    to_db, from_db = ccsds_dual_basis()
    return Layout(Code(0x187, 120, 11, 16), 5, 4, 1, from_db, to_db, ccsds_randomizer())


def pack_rows(out, good, counts):
    """Per row the good frames of its first counts[r] frames, back to back: a list of (g, frame_out) arrays."""
    return [out[r, :counts[r]][good[r, :counts[r]]] for r in range(out.shape[0])]
