"""The numpy definition of the Viterbi decoder (include/qdsp_hip.h: Viterbi decoder): libcorrect's convolutional codec
(src/libcorrect/convolutional) followed step by step -- fill_table, the encoder, and the decoder with its two error buffers, its
history ring with the entries the tail leaves stale, its renormalisation counter and its bit writer -- vectorised over the states
and over a batch of frames, stepping in time.  Every frame is decoded as by a freshly created correct_convolutional.
tests/golden/viterbi_ref_io.npz holds what libcorrect itself answered (tests/test_viterbi_cpu.py compares byte for byte).
"""
import numpy as np

# libcorrect's published codes (correct.h), by (rate, order)
CODES = {(2, 6): (0o73, 0o61), (2, 7): (0o161, 0o127), (2, 8): (0o225, 0o373), (2, 9): (0o767, 0o545),
         (3, 6): (0o53, 0o75, 0o47), (3, 7): (0o137, 0o153, 0o121), (3, 8): (0o333, 0o257, 0o351), (3, 9): (0o417, 0o627, 0o675)}
ODD_CODE = (2, 7, (0o155, 0o117))     # polynomials that are not the published ones

# what a processed step did (history_buffer_process_skip's four cases)
NEITHER, RENORM, BOTH, TRACEBACK = 0, 1, 2, 3
# input kinds of the recording
KIND_CODED, KIND_NOISE, KIND_SATURATED = 0, 1, 2


def _parity(v):
    v = np.asarray(v, np.int64).copy()
    p = np.zeros_like(v)
    while v.any():
        p ^= v & 1
        v >>= 1
    return p


def fill_table(rate, order, poly):
    """table[r] over the order-bit register r: polynomial i gives bit i."""
    r = np.arange(1 << order, dtype=np.int64)
    out = np.zeros(1 << order, np.int64)
    for i in range(rate):
        out |= _parity(r & int(poly[i])) << i
    return out


def renorm_interval(rate):
    return 65535 // (255 * rate)


def encode_bits(rate, order, poly, msg):
    """correct_convolutional_encode: the rate * (8 len + order + 1) code bits of `msg`, in the order they are written."""
    table = fill_table(rate, order, poly)
    bits = np.unpackbits(np.asarray(msg, np.uint8))
    mask, sr, out = (1 << order) - 1, 0, []
    for b in list(bits) + [0] * (order + 1):
        sr = ((sr << 1) | int(b)) & mask
        o = int(table[sr])
        out += [(o >> i) & 1 for i in range(rate)]
    return np.asarray(out, np.uint8)


def encode(rate, order, poly, msg):
    """... packed MSB first, the last byte zero-filled, as the library returns them."""
    return np.packbits(encode_bits(rate, order, poly, msg))


def frame_in_bytes(rate, sets, soft):
    return sets * rate if soft else (sets * rate + 7) // 8


def frame_out_bytes(order, sets):
    return (sets - order + 1) // 8


def schedule(rate, order, sets):
    """What every processed step n = 1 .. sets - order + 1 of a fresh decoder does: (cases, tail_tracebacks) -- cases[n - 1] one of
    NEITHER / RENORM / BOTH / TRACEBACK; tail_tracebacks the tail steps k = 1 .. order - 1 on which a traceback falls."""
    cap, mtb, interval = 20 * order, 5 * order, renorm_interval(rate)
    steps = sets - order + 1
    cases, tails, ln, ctr = [], [], 0, 0
    for n in range(1, steps + 1):
        ln += 1
        ctr += 1
        ren, tb = ctr == interval, ln == cap
        if ren:
            ctr = 0
        if tb:
            ln = mtb
            k = n - (steps - (order - 1))
            if k >= 1:
                tails.append(k)
        cases.append(BOTH if ren and tb else RENORM if ren else TRACEBACK if tb else NEITHER)
    return cases, tails


def decode(rate, order, poly, x, sets, soft):
    """x: (B, frame_in_bytes) uint8.  Returns ((B, frame_out_bytes) uint8, cases, tail_tracebacks); frame_out_bytes is what the
    library's call returns."""
    x = np.atleast_2d(np.asarray(x, np.uint8))
    B = x.shape[0]
    assert sets >= order - 1 and x.shape[1] == frame_in_bytes(rate, sets, soft)
    table = fill_table(rate, order, poly)
    ns, highbit = 1 << (order - 1), 1 << (order - 1)
    cap, mtb, interval = 20 * order, 5 * order, renorm_interval(rate)
    lab = (np.arange(1 << rate)[:, None] >> np.arange(rate)[None, :]) & 1             # (2^rate, rate)
    if soft:
        y = x.reshape(B, sets, rate).astype(np.int64)
    else:
        y = np.unpackbits(x, axis=1)[:, :sets * rate].reshape(B, sets, rate).astype(np.int64)

    def distances(t):
        """(B, 2^rate): metric_soft_distance_linear / metric_distance of every label against set t"""
        if soft:
            return np.abs(y[:, t, None, :] - 255 * lab[None, :, :]).sum(axis=2)
        return (y[:, t, None, :] ^ lab[None, :, :]).sum(axis=2)

    err = [np.zeros((B, 1 << order), np.int64), np.zeros((B, 1 << order), np.int64)]   # error_buffer: numstates entries each
    eb = {"index": 0, "rd": 0, "wr": 1}

    def swap():
        """error_buffer_swap as it is written: the read side becomes errors[index] BEFORE index moves on, so the first swap after
        a reset changes nothing -- what warm-up step 0 wrote is overwritten by step 1, which reads zeros."""
        eb["rd"] = eb["index"]
        eb["index"] = (eb["index"] + 1) % 2
        eb["wr"] = eb["index"]

    hist = np.zeros((B, cap, ns), np.uint8)
    st = {"index": 0, "len": 0, "ctr": 0}
    emitted, cases, tails = [], [], []
    rows = np.arange(B)

    def search(w, every):
        states = np.arange(0, ns, every)
        v = w[:, states]
        assert (v.min(axis=1) < 65535).all(), "every searched metric is USHRT_MAX: the C code's answer is not defined"
        return states[np.argmin(v, axis=1)]                                            # the first at the minimum

    def traceback(best, min_len):
        best = best.copy()
        index, fetched = st["index"], []
        for j in range(st["len"]):
            index = cap - 1 if index == 0 else index - 1
            h = hist[rows, index, best].astype(np.int64)
            best = (best | np.where(h != 0, highbit, 0)) >> 1
            if j >= min_len:
                fetched.append((h != 0).astype(np.uint8))
        if fetched:
            emitted.append(np.stack(fetched[::-1], axis=1))                           # bit_writer_write_bitlist_reversed
        st["len"] -= len(fetched)

    def process_skip(w, skip):
        st["index"] = (st["index"] + 1) % cap
        st["ctr"] += 1
        st["len"] += 1
        if st["ctr"] == interval:
            st["ctr"] = 0
            best = search(w, skip)
            w -= w[rows, best][:, None]
            w &= 0xffff
            if st["len"] == cap:
                cases.append(BOTH)
                traceback(best, mtb)
                return True
            cases.append(RENORM)
        elif st["len"] == cap:
            cases.append(TRACEBACK)
            traceback(search(w, skip), mtb)
            return True
        else:
            cases.append(NEITHER)
        return False

    for i in range(min(order - 1, sets)):                                              # warm-up
        d = distances(i)
        j = np.arange(1 << (i + 1))
        err[eb["wr"]][:, j] = (d[:, table[j]] + err[eb["rd"]][:, j >> 1]) & 0xffff
        swap()
    j = np.arange(ns)
    for i in range(order - 1, sets - order + 1):                                       # inner
        d = distances(i)
        lo = (d[:, table[j]] + err[eb["rd"]][:, j >> 1]) & 0xffff
        hi = (d[:, table[j | highbit]] + err[eb["rd"]][:, (j >> 1) | (highbit >> 1)]) & 0xffff
        take_lo = lo <= hi
        err[eb["wr"]][:, j] = np.where(take_lo, lo, hi)
        hist[:, st["index"], :] = ~take_lo
        process_skip(err[eb["wr"]], 1)
        swap()
    for i in range(sets - order + 1, sets):                                            # tail
        d = distances(i)
        skip = 1 << (order - (sets - i))
        low = np.arange(0, highbit, skip)
        lo = (d[:, table[low]] + err[eb["rd"]][:, low >> 1]) & 0xffff
        hi = (d[:, table[low | highbit]] + err[eb["rd"]][:, (highbit >> 1) + (low >> 1)]) & 0xffff
        take_lo = lo < hi
        err[eb["wr"]][:, low] = np.where(take_lo, lo, hi)
        hist[:, st["index"], low] = ~take_lo                                           # (the other entries of the slice stay as they were)
        if process_skip(err[eb["wr"]], skip):
            tails.append(i - (sets - order + 1) + 1)
        swap()
    traceback(np.zeros(B, np.int64), 0)                                                # history_buffer_flush
    bits = np.concatenate(emitted, axis=1) if emitted else np.zeros((B, 0), np.uint8)
    nb = bits.shape[1] // 8                                                            # the partial byte is never stored
    out = np.packbits(bits[:, :8 * nb], axis=1) if nb else np.zeros((B, 0), np.uint8)
    return out, cases, tails


# ---- the inputs of the recording and of the tests, from a seed ----
def make_input(rate, order, poly, sets, soft, kind, seed):
    """One frame of frame_in_bytes.  KIND_CODED: the encoding of a random message, cut (or zero-extended) to `sets` sets, with
    moderate noise (soft: Gaussian, sigma 60 around 0 / 255, clipped; hard: 3 % of the bits flipped); KIND_NOISE: uniform bytes;
    KIND_SATURATED (soft): bytes of 0 and 255 only."""
    rng = np.random.default_rng(int(seed))
    nbits = sets * rate
    if kind == KIND_CODED:
        msg = rng.integers(0, 256, max((sets - order - 1 + 7) // 8, 1)).astype(np.uint8)
        b = encode_bits(rate, order, poly, msg)
        b = np.concatenate([b, np.zeros(max(nbits - b.size, 0), np.uint8)])[:nbits]
        if soft:
            v = 255.0 * b + rng.normal(0.0, 60.0, nbits)
            return np.clip(np.rint(v), 0, 255).astype(np.uint8)
        return np.packbits(b ^ (rng.random(nbits) < 0.03).astype(np.uint8))
    if kind == KIND_SATURATED:
        assert soft
        return (255 * rng.integers(0, 2, nbits)).astype(np.uint8)
    assert kind == KIND_NOISE
    return rng.integers(0, 256, frame_in_bytes(rate, sets, soft)).astype(np.uint8)


def edge_sets(rate, order):
    """The frame lengths at which the bookkeeping takes another path (cap = 20 order slices, 15 order bits per traceback)."""
    cap, g, o = 20 * order, 15 * order, order
    s = [o + 7, o + 8, o + 21, cap - 3,                       # no traceback at all
         cap + o - 2, cap + o - 1, cap + o,                    # the step before the first traceback, it (on the last tail step), the step after
         cap + g + o - 2, cap + g + o - 1, cap + g + o,        # the second traceback
         cap + 2 * o - 3, cap + 2 * (o - 1) - o // 2,          # a traceback on the first and on a middle tail step
         cap + g + 37]                                         # an output length off every boundary
    return sorted(set(s))
