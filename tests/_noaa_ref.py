"""The definition of the NOAA HRPT tail: readBits (src/dsp/utils/bitstream.h:4-42) and the run() loops of HRPTDemux
(src/dsp/noaa/hrpt.h:36-78), TIPDemux (src/dsp/noaa/tip.h:31-124) and HIRSDemux (src/dsp/noaa/tip.h:168-229), transcribed call by
call and bit by bit, serial, in plain Python over numpy byte arrays; and the inverses the tests build their inputs with.  The
reference's own blocks are not built here (DESIGN.md "Oracle": VOLK is absent), so this transcription carries the definition, as
_mmcr_ref.py and _deframer_ref.py do."""
import numpy as np

FRAME_BITS, FRAME_BYTES, WORDS = 110900, 13863, 11090
MINOR_BYTES, RECORD_BYTES, PACKET_BYTES = 104, 74, 36
PIXELS, PLANES, CHANNELS, LINE = 2048, 5, 20, 56

# src/dsp/noaa/tip.h:36-71, 75-76, 80-111, 115-118
HIRS_SRC = [16, 17, 22, 23, 26, 27, 30, 31, 34, 35, 38, 39, 42, 43, 54, 55, 58, 59, 62, 63, 66, 67, 70, 71, 74, 75, 78, 79, 82, 83, 84, 85, 88, 89,
            92, 93]
SEM_SRC = [20, 21]
DCS_SRC = [18, 19, 24, 25, 28, 29, 32, 33, 40, 41, 44, 45, 52, 53, 56, 57, 60, 61, 64, 65, 68, 69, 72, 73, 76, 77, 86, 87, 90, 91, 94, 95]
SBUV_SRC = [36, 37, 80, 81]
RECORD_SRC = HIRS_SRC + SEM_SRC + DCS_SRC + SBUV_SRC
SECTIONS = (0, 36, 38, 70, 74)
# src/dsp/noaa/tip.h:192-211
RAD_BITS = [26, 52, 65, 91, 221, 208, 143, 156, 273, 182, 119, 247, 78, 195, 234, 260, 39, 104, 130, 169]
ELEMENT_BIT, ELEMENT_LEN = 19, 6
STD_SYNC_WORDS = [0x284, 0x16F, 0x35C, 0x19D, 0x20F, 0x095]


def read_bits(offset: int, length: int, buffer) -> int:
    """bitstream.h:4-42, statement by statement."""
    output = 0
    last_bit = offset + (length - 1)
    first_word = offset // 8
    last_word = last_bit // 8
    first_offset = offset - first_word * 8
    last_offset = last_bit - last_word * 8
    word_count = (last_word - first_word) + 1
    if word_count == 1:
        return (int(buffer[first_word]) & (0xFF >> first_offset)) >> (7 - last_offset)
    bits_read = length
    for i in range(word_count):
        if i == 0:
            bits_read -= 8 - first_offset
            output |= (int(buffer[first_word]) & (0xFF >> first_offset)) << bits_read
            continue
        if i == word_count - 1:
            output |= int(buffer[last_word]) >> (7 - last_offset)
            break
        bits_read -= 8
        output |= int(buffer[first_word + i]) << bits_read
    return output


def big_int_bits(offset: int, length: int, buffer) -> int:
    """The same field out of the buffer as one big-endian integer."""
    v = int.from_bytes(bytes(bytearray(buffer)), "big")
    return (v >> (8 * len(buffer) - offset - length)) & ((1 << length) - 1)


def read_word(offset: int, buffer) -> int:
    """hrpt.h:7-9"""
    return read_bits(offset * 10, 10, buffer) & 0xFFFF


def hrpt_run(frame):
    """One run() of HRPTDemux on one frame: (minor, tip or None, aip or None, avhrr (5, 2048)); tip / aip are (5, 104)."""
    minor = read_bits(61, 2, frame)
    tip = aip = None
    if minor == 1:
        tip = np.zeros((5, MINOR_BYTES), np.uint8)
        for i in range(5):
            for j in range(MINOR_BYTES):
                tip[i, j] = (read_word(103 + i * 104 + j, frame) >> 2) & 0xFF
    elif minor == 3:
        aip = np.zeros((5, MINOR_BYTES), np.uint8)
        for i in range(5):
            for j in range(MINOR_BYTES):
                aip[i, j] = (read_word(103 + i * 104 + j, frame) >> 2) & 0xFF
    avhrr = np.zeros((PLANES, PIXELS), np.uint16)
    for i in range(PIXELS):
        for c in range(PLANES):
            avhrr[c, i] = read_word(750 + i * 5 + c, frame)
    return minor, tip, aip, avhrr


def hrpt_demux(frames):
    """frames (n, 13863) -> (avhrr (5, n, 2048), tip (k, 104), aip (m, 104), minors (n,))."""
    frames = np.asarray(frames, np.uint8).reshape(-1, FRAME_BYTES)
    av = np.zeros((PLANES, len(frames), PIXELS), np.uint16)
    tips, aips, minors = [], [], []
    for f, fr in enumerate(frames):
        m, t, a, v = hrpt_run(fr)
        minors.append(m)
        av[:, f] = v
        if t is not None:
            tips.append(t)
        if a is not None:
            aips.append(a)
    cat = lambda l: np.concatenate(l) if l else np.zeros((0, MINOR_BYTES), np.uint8)
    return av, cat(tips), cat(aips), np.array(minors, np.int64)


def tip_run(minor_frame):
    """One run() of TIPDemux: the four outputs in the record's order, (74,)."""
    return np.array([minor_frame[s] for s in RECORD_SRC], np.uint8)


def tip_demux(minor_frames):
    mf = np.asarray(minor_frames, np.uint8).reshape(-1, MINOR_BYTES)
    return np.stack([tip_run(m) for m in mf]) if len(mf) else np.zeros((0, RECORD_BYTES), np.uint8)


def hirs_signed_to_unsigned(n: int) -> int:
    """tip.h:136-138"""
    return (0x1000 + (n & 0xFFF)) if (n & 0x1000) else (0xFFF - (n & 0xFFF))


class Hirs:
    """HIRSDemux's state and run(): the write buffers (20, 56), lastElement, newImageData."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.buf = np.full((CHANNELS, LINE), 0xFFF, np.uint16)
        self.last_element = 0
        self.new_image_data = False

    def _swap(self, lines):
        lines.append(self.buf.copy())
        self.buf[:] = 0xFFF

    def run(self, packet, lines):
        element = read_bits(ELEMENT_BIT, ELEMENT_LEN, packet)
        if (element < self.last_element or element > 55) and self.new_image_data:
            self.new_image_data = False
            self._swap(lines)
        self.last_element = element
        if element <= 55:
            self.new_image_data = True
            for ch in range(CHANNELS):
                self.buf[ch, element] = hirs_signed_to_unsigned(read_bits(RAD_BITS[ch], 13, packet))
        if element == 55:
            self.new_image_data = False
            self._swap(lines)

    def process(self, packets, stride: int = PACKET_BYTES):
        """packets: bytes, `stride` apart -> (20, lines, 56)."""
        b = np.asarray(packets, np.uint8).ravel()
        lines = []
        for i in range(len(b) // stride):
            self.run(b[i * stride:i * stride + PACKET_BYTES], lines)
        return np.stack(lines, axis=1) if lines else np.zeros((CHANNELS, 0, LINE), np.uint16)


def hirs_elements_serial(elements, last_element=0, new_image_data=False):
    """The serial loop on elements alone: per packet (line, or -1 where it writes nothing), lines emitted, the new state."""
    out, lines = [], 0
    for e in elements:
        if (e < last_element or e > 55) and new_image_data:
            new_image_data = False
            lines += 1
        last_element = e
        if e <= 55:
            new_image_data = True
            out.append(lines)
        else:
            out.append(-1)
        if e == 55:
            new_image_data = False
            lines += 1
    return out, lines, (last_element, new_image_data)


def hirs_elements_parallel(elements, last_element=0, new_image_data=False):
    """The closed form the kernels use: fb, fa, an exclusive prefix sum; the same three results."""
    e = np.asarray(elements, np.int64)
    n = len(e)
    if n == 0:
        return [], 0, (last_element, bool(new_image_data))
    prev = np.concatenate([[last_element], e[:-1]])
    nid = np.concatenate([[bool(new_image_data)], e[:-1] < 55])
    fb = ((e < prev) | (e > 55)) & nid
    fa = e == 55
    c = fb.astype(np.int64) + fa
    line = np.cumsum(c) - c + fb
    return [int(l) if x <= 55 else -1 for l, x in zip(line, e)], int(c.sum()), (int(e[-1]), bool(e[-1] < 55))


def hirs_map_parallel(elements, last_element=0, new_image_data=False):
    """{(line, slot): packet} with the closed form's drop rule: packet i is dropped when packet i + 1 repeats its element and
    e[i] != 55."""
    line, _, _ = hirs_elements_parallel(elements, last_element, new_image_data)
    m = {}
    for i, (l, e) in enumerate(zip(line, elements)):
        if l < 0:
            continue
        if i + 1 < len(elements) and e != 55 and elements[i + 1] == e:
            continue
        assert (l, e) not in m, "one writer per (line, slot)"
        m[(l, e)] = i
    return m


def hirs_map_serial(elements, last_element=0, new_image_data=False):
    """{(line, slot): packet}: the last writer, from the serial loop."""
    line, _, _ = hirs_elements_serial(elements, last_element, new_image_data)
    m = {}
    for i, (l, e) in enumerate(zip(line, elements)):
        if l >= 0:
            m[(l, e)] = i
    return m


# ---- the inverses ----

def _put_bits(buf, offset: int, length: int, value: int):
    for k in range(length):
        bit = (value >> (length - 1 - k)) & 1
        byte, sh = (offset + k) // 8, 7 - (offset + k) % 8
        buf[byte] = (int(buf[byte]) & ~(1 << sh)) | (bit << sh)


def make_frame(minor: int, tip_bytes, avhrr, fill=None, sync_words=STD_SYNC_WORDS):
    """A frame whose demultiplexing gives back `minor`, `tip_bytes` (5, 104: the TIP or AIP bytes; the two low bits of their words
    come from `fill`) and `avhrr` (5, 2048) values below 1024.  `fill`: 13863 bytes under everything else (None: zeros)."""
    buf = np.zeros(FRAME_BYTES, np.uint8) if fill is None else np.array(fill, np.uint8).copy()
    buf[-1] &= 0xF0                                               # 110900 bits: the last four of the last byte are not the frame's
    for w, v in enumerate(sync_words):
        _put_bits(buf, 10 * w, 10, v)
    _put_bits(buf, 61, 2, minor)
    tb = np.asarray(tip_bytes, np.uint8).reshape(5 * MINOR_BYTES)
    for j in range(5 * MINOR_BYTES):
        _put_bits(buf, 10 * (103 + j), 8, int(tb[j]))
    av = np.asarray(avhrr).reshape(PLANES, PIXELS)
    for p in range(PIXELS):
        for c in range(PLANES):
            _put_bits(buf, 10 * (750 + 5 * p + c), 10, int(av[c, p]))
    return buf


def hirs_unsigned_to_signed(u: int) -> int:
    """The 13-bit field n with hirs_signed_to_unsigned(n) == u, u in 0 .. 0x1FFF."""
    return (0x1000 | (u - 0x1000)) if u >= 0x1000 else (0xFFF - u)


def random_radiances(rng):
    """Twenty output values (0 .. 0x1FFF) that one packet can hold: the reference's fields at bits 119 (channel 10) and 130
    (channel 18) share bits 130 and 131, so the two lowest bits of the first are the two highest of the second."""
    n = rng.integers(0, 0x2000, CHANNELS)
    n[10] = (n[10] & ~3) | (n[18] >> 11)
    return np.array([hirs_signed_to_unsigned(int(v)) for v in n], np.int64)


def make_packet(element: int, radiances, fill=None):
    """A 36-byte packet with the given element (0 .. 63) and the 20 output values (0 .. 0x1FFF) of its radiance channels (values
    one packet can hold: random_radiances)."""
    buf = np.zeros(PACKET_BYTES, np.uint8) if fill is None else np.array(fill, np.uint8).copy()
    _put_bits(buf, ELEMENT_BIT, ELEMENT_LEN, element)
    for ch in range(CHANNELS):
        _put_bits(buf, RAD_BITS[ch], 13, hirs_unsigned_to_signed(int(radiances[ch])))
    assert all(hirs_signed_to_unsigned(read_bits(RAD_BITS[ch], 13, buf)) == int(radiances[ch]) for ch in range(CHANNELS)), "fields 119 and 130 overlap"
    return buf


def sync_bits(sync_words=STD_SYNC_WORDS):
    """The 60-bit sync word, one bit per byte, as the Deframer takes it."""
    return np.array([(w >> (9 - k)) & 1 for w in sync_words for k in range(10)], np.uint8)


# ---- fast forms for the GPU tests' larger inputs (equal to the transcription: tests/test_noaa_cpu.py) ----

def frame_words(frames):
    """(n, 11090) uint16: every 10-bit word of every frame."""
    fr = np.asarray(frames, np.uint8).reshape(-1, FRAME_BYTES)
    bits = np.unpackbits(fr, axis=1)[:, :FRAME_BITS].reshape(len(fr), WORDS, 10).astype(np.uint16)
    return (bits << np.arange(9, -1, -1, dtype=np.uint16)).sum(axis=2).astype(np.uint16)


def hrpt_demux_fast(frames):
    fr = np.asarray(frames, np.uint8).reshape(-1, FRAME_BYTES)
    w = frame_words(fr)
    av = np.ascontiguousarray(w[:, 750:750 + PLANES * PIXELS].reshape(len(fr), PIXELS, PLANES).transpose(2, 0, 1))
    minors = (fr[:, 7].astype(np.int64) >> 1) & 3
    tb = ((w[:, 103:103 + 5 * MINOR_BYTES] >> 2) & 0xFF).astype(np.uint8)
    return av, tb[minors == 1].reshape(-1, MINOR_BYTES), tb[minors == 3].reshape(-1, MINOR_BYTES), minors


def hirs_fields_fast(packets, stride: int = PACKET_BYTES):
    """(elements (n,), values (n, 20)) of packets `stride` bytes apart."""
    b = np.asarray(packets, np.uint8).ravel()
    n = len(b) // stride
    if n == 0:
        return np.zeros(0, np.int64), np.zeros((0, CHANNELS), np.uint16)
    pk = np.stack([b[i * stride:i * stride + PACKET_BYTES] for i in range(n)])
    bits = np.unpackbits(pk, axis=1).astype(np.int64)
    field = lambda o, l: (bits[:, o:o + l] << np.arange(l - 1, -1, -1)).sum(axis=1)
    e = field(ELEMENT_BIT, ELEMENT_LEN)
    raw = np.stack([field(o, 13) for o in RAD_BITS], axis=1)
    vals = np.where(raw & 0x1000, 0x1000 + (raw & 0xFFF), 0xFFF - (raw & 0xFFF)).astype(np.uint16)
    return e, vals


class HirsFast:
    """Hirs on the fast field extraction: the serial loop over precomputed elements and values."""

    def __init__(self):
        self.reset()

    reset = Hirs.reset

    def set_state(self, last_element, new_image_data):
        self.last_element, self.new_image_data = int(last_element), bool(new_image_data)

    def process(self, packets, stride: int = PACKET_BYTES):
        e, vals = hirs_fields_fast(packets, stride)
        lines = []
        for i in range(len(e)):
            el = int(e[i])
            if (el < self.last_element or el > 55) and self.new_image_data:
                self.new_image_data = False
                Hirs._swap(self, lines)
            self.last_element = el
            if el <= 55:
                self.new_image_data = True
                self.buf[:, el] = vals[i]
            if el == 55:
                self.new_image_data = False
                Hirs._swap(self, lines)
        return np.stack(lines, axis=1) if lines else np.zeros((CHANNELS, 0, LINE), np.uint16)
