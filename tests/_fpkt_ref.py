"""FalconPacketSync without a GPU: the definition the GPU tests compare against.

`PacketSync.run` is dsp::FalconPacketSync::run() (src/dsp/falcon_packet.h:28-107) statement by statement, with the two departures
include/qdsp_hip.h names (overflow of the 16392-byte packet, a first-header pointer of 1192 .. 2046), each marked.  `closed_form`
is the same block as the kernels compute it: a summary per frame that depends on the frame alone, a look-back over at most 14
frames for the pending length, two exclusive prefix sums, and a gather.  The builders are the definition's inverses.
"""
import numpy as np

HEADER, DATA, FRAME = 4, 1191, 1195
CAP = 0x4008
CONT = 2047
PER_FRAME = 1 + DATA // 3
RS_FRAME = 1275


def out_size(n):
    return CAP + DATA * n


def out_packets(n):
    return PER_FRAME * n


def make_header(ctr, pkt):
    """The four bytes in front of the data area: the inverse of parse_header for ctr < 2^19 and pkt < 2^11 (the two top bits of
    b0 are free; they are set from `ctr` bits 19 and 20 so that a test can light them)."""
    return bytes([(ctr >> 13) & 0xFF, (ctr >> 5) & 0xFF, ((ctr & 0x1F) << 3) | ((pkt >> 8) & 7), pkt & 0xFF])


def parse_header(buf):
    b0, b1, b2, b3 = (int(v) for v in buf[:4])
    return (b2 >> 3) | (b1 << 5) | ((b0 & 0b111111) << 13), b3 | ((b2 & 0b111) << 8)


def make_frame(ctr, pkt, data, stride=FRAME, fill=0):
    """One frame of `stride` bytes: header, `data` (1191 bytes, shorter is padded with zeros), `fill` behind byte 1194."""
    f = np.full(stride, fill, np.uint8)
    f[:HEADER] = np.frombuffer(make_header(ctr, pkt), np.uint8)
    d = np.frombuffer(bytes(data), np.uint8)
    assert d.size <= DATA
    f[HEADER:HEADER + DATA] = 0
    f[HEADER:HEADER + d.size] = d
    return f


def make_packet(length, rng=None, value=None, ramp=None):
    """A packet of `length` bytes (3 .. 4097) whose length field says so; the top four bits of byte 0 are free.  The payload is
    random (`rng`), a ramp that begins at `ramp`, or `value` throughout."""
    assert 3 <= length <= 4097
    if ramp is not None:
        p = ((int(ramp) + np.arange(length)) & 0xFF).astype(np.uint8)
    elif rng is not None:
        p = rng.integers(0, 256, length).astype(np.uint8)
    else:
        p = np.full(length, 0xA5 if value is None else value, np.uint8)
    p[0] = (p[0] & 0xF0) | ((length - 2) >> 8)
    p[1] = (length - 2) & 0xFF
    return p.tobytes()


def build_stream(packets, ctr0=1, stride=FRAME, fill=0):
    """Frames that carry `packets` back to back, counters ctr0, ctr0 + 1, ...: a frame's pointer is the first header that begins in
    it; 1191 where none does and a packet ends with the frame; 2047 where none does and none ends.  The last frame is padded with
    zeros, which the walk reads as a zero length (or keeps as a residue of fewer than four bytes)."""
    body = b"".join(packets)
    starts, o = [], 0
    for p in packets:
        starts.append(o)
        o += len(p)
    starts.append(o)                                         # the padding
    nfr = max(1, -(-len(body) // DATA))
    body = body + bytes(nfr * DATA - len(body))
    frames = []
    for j in range(nfr):
        lo, hi = j * DATA, (j + 1) * DATA
        first = [s for s in starts if lo <= s < hi]
        if first:
            pkt = first[0] - lo
        else:
            pkt = DATA if hi in starts else CONT
        frames.append(make_frame((ctr0 + j) & 0x7FFFF, pkt, body[lo:hi], stride, fill))
    return np.stack(frames)


class PacketSync:
    """The reference block.  `run` takes one frame (at least 1195 bytes) and returns the packets it emitted, in order."""

    def __init__(self, last_counter=0, pending=b""):
        self.lastCounter = int(last_counter) & 0xFFFFFFFF
        self.packet = bytearray(CAP)
        self.packetRead = -1
        if pending:
            assert len(pending) <= CAP
            self.packetRead = len(pending)
            self.packet[:len(pending)] = pending

    def state(self):
        return self.lastCounter, self.packetRead, bytes(self.packet[:max(self.packetRead, 0)])

    def run(self, buf):
        out = []
        # Parse frame header
        packet = int(buf[3]) | ((int(buf[2]) & 0b111) << 8)
        counter = (int(buf[2]) >> 3) | (int(buf[1]) << 5) | ((int(buf[0]) & 0b111111) << 13)
        # Pointer to the data area of the frame
        data = bytes(buf[4:4 + DATA])
        dataLen = DATA
        # If a frame was missed, cancel reading the current packet
        if (self.lastCounter + 1) & 0xFFFFFFFF != counter:
            self.packetRead = -1
        self.lastCounter = counter
        # If frame is just a continuation of a single packet, save it
        if packet == 2047 and self.packetRead >= 0:
            if self.packetRead + dataLen > CAP:               # departure: overflow
                self.packetRead = -1
                return out
            self.packet[self.packetRead:self.packetRead + dataLen] = data
            self.packetRead += dataLen
            return out
        elif packet == 2047:
            return out
        if packet > dataLen:                                  # departure: bad pointer
            self.packetRead = -1
            return out
        # Finish reading the last package and send it
        if self.packetRead >= 0:
            if self.packetRead + packet > CAP:                # departure: overflow
                self.packetRead = -1
            else:
                self.packet[self.packetRead:self.packetRead + packet] = data[:packet]
                out.append(bytes(self.packet[:self.packetRead + packet]))
                self.packetRead = -1
        # Iterate through every packet of the frame
        i = packet
        while i < dataLen:
            # First, check if we can read the header. If not, save and wait for next frame
            if dataLen - i < 4:
                self.packetRead = dataLen - i
                self.packet[:self.packetRead] = data[i:]
                break
            # Extract packet length
            length = ((((data[i] & 0b1111) << 8) | data[i + 1]) + 2) & 0xFFFF
            # Check if it's not an invalid zero length packet
            if length <= 2:
                self.packetRead = -1
                break
            # If the packet doesn't fit the frame, save and go to next frame
            if dataLen - i < length:
                self.packetRead = dataLen - i
                self.packet[:self.packetRead] = data[i:]
                break
            # Here, the package fits fully, read it and jump to the next
            out.append(data[i:i + length])
            i += length
        return out

    def process(self, frames):
        """[(frame index, packet)] of the frames (n, >= 1195)."""
        got = []
        for f, fr in enumerate(frames):
            got += [(f, p) for p in self.run(fr)]
        return got


def in_departure_domain(frames, last_counter=0, pending=b""):
    """Whether the stream takes one of the two departures anywhere (then the reference itself is out of bounds)."""
    s = PacketSync(last_counter, pending)
    for fr in frames:
        _, pkt = parse_header(fr)
        if 1192 <= pkt <= 2046:
            return True
        ctr, _ = parse_header(fr)
        alive = s.packetRead >= 0 and (s.lastCounter + 1) & 0xFFFFFFFF == ctr
        if alive and s.packetRead + (DATA if pkt == CONT else pkt) > CAP:
            return True
        s.run(fr)
    return False


def pending_runs(frames, last_counter=0, pending=b""):
    """[(g, f, length)] of every pending packet the stream emits: begun by frame g's residue (-1: the carried one), emitted by
    frame f."""
    s, origin, runs = PacketSync(last_counter, pending), -1, []
    for f, fr in enumerate(frames):
        ctr, pkt = parse_header(fr)
        alive = s.packetRead >= 0 and (s.lastCounter + 1) & 0xFFFFFFFF == ctr
        emits = alive and pkt <= DATA and s.packetRead + pkt <= CAP
        before = s.packetRead
        out = s.run(fr)
        if emits:
            assert len(out[0]) == before + pkt
            runs.append((origin, f, len(out[0])))
        if pkt != CONT:
            origin = f
    return runs


# ---- the closed form, as the kernels compute it ----

def walk(frame):
    """What a frame determines by itself: (ctr, pkt, e, T, starts): the end of its walked packets, its tail (-1, or the residue
    length 1191 - e) and where its packets begin in the data area.  Continuation frames and bad pointers: e = 0, T = -1, none."""
    ctr, pkt = parse_header(frame)
    data = frame[HEADER:HEADER + DATA]
    e, tail, starts = 0, -1, []
    if pkt <= DATA:
        i = pkt
        while i < DATA:
            left = DATA - i
            if left < 4:
                tail = left
                break
            ln = (((int(data[i]) & 15) << 8) | int(data[i + 1])) + 2
            if ln <= 2:
                break
            if left < ln:
                tail = left
                break
            starts.append(i)
            i += ln
        e = i
    return ctr, pkt, e, tail, starts


def closed_form(frames, last_counter=0, pending=b""):
    """(out bytes, offs (count + 1), state) of one row and call, by summaries, look-back, prefix sums and gather."""
    n = len(frames)
    sums = [walk(fr) for fr in frames]
    last0, read0 = int(last_counter) & 0xFFFFFFFF, (len(pending) if pending else -1)

    def ctr_of(j):
        return last0 if j < 0 else sums[j][0]

    def incoming(f):
        k = 0
        if f < n and (ctr_of(f - 1) + 1) & 0xFFFFFFFF != ctr_of(f):
            return -1, 0
        base, j = -1, f - 1
        while True:
            if j < 0:
                base = read0
                break
            ctr, pkt, e, tail, _ = sums[j]
            if pkt != CONT:
                base = tail if pkt <= DATA else -1
                break
            if (ctr_of(j - 1) + 1) & 0xFFFFFFFF != ctr:
                break
            k += 1
            if k > 13:
                break
            j -= 1
        if base < 0:
            return -1, k
        v = base + DATA * k
        return (v, k) if v <= CAP else (-1, k)

    def gather(f, inl, k, head):
        g = f - 1 - k
        first = inl - DATA * k
        parts = [bytes(frames[g][FRAME - first:FRAME]) if g >= 0 else bytes(pending[:first])]
        parts += [bytes(frames[j][HEADER:FRAME]) for j in range(g + 1, f)]
        if head:
            parts.append(bytes(frames[f][HEADER:HEADER + head]))
        return b"".join(parts)

    npk, nby, ins = np.zeros(n, np.int64), np.zeros(n, np.int64), [(-1, 0)] * n
    for f, (ctr, pkt, e, tail, starts) in enumerate(sums):
        if pkt <= DATA:
            inl, k = incoming(f)
            if inl >= 0 and inl + pkt > CAP:
                inl = -1
            ins[f] = (inl, k)
            npk[f] = len(starts) + (1 if inl >= 0 else 0)
            nby[f] = e - pkt + (inl + pkt if inl >= 0 else 0)
    pk0 = np.concatenate([[0], np.cumsum(npk)])
    by0 = np.concatenate([[0], np.cumsum(nby)])
    out = bytearray(int(by0[n]))
    offs = np.zeros(int(pk0[n]) + 1, np.int32)
    offs[-1] = by0[n]
    for f, (ctr, pkt, e, tail, starts) in enumerate(sums):
        if pkt > DATA:
            continue
        o, q = int(by0[f]), int(pk0[f])
        inl, k = ins[f]
        if inl >= 0:
            p = gather(f, inl, k, pkt)
            assert len(p) == inl + pkt
            out[o:o + len(p)] = p
            offs[q] = o
            o, q = o + len(p), q + 1
        out[o:o + e - pkt] = bytes(frames[f][HEADER + pkt:HEADER + e])
        for r, s in enumerate(starts):
            offs[q + r] = o + s - pkt
    inl, k = incoming(n)
    carry = gather(n, inl, k, 0) if inl >= 0 else b""
    return bytes(out), offs, (ctr_of(n - 1), inl, carry)


def serial_row(frames, last_counter=0, pending=b""):
    """The same triple by the transcription."""
    s = PacketSync(last_counter, pending)
    pk = [p for _, p in s.process(frames)]
    offs = np.zeros(len(pk) + 1, np.int32)
    offs[1:] = np.cumsum([len(p) for p in pk])
    return b"".join(pk), offs, s.state()


def split(out, offs):
    return [bytes(out[int(offs[k]):int(offs[k + 1])]) for k in range(len(offs) - 1)]


# ---- streams ----

def random_stream(rng, nframes, stride=FRAME, mean=300, big=0.02, breaks=0.03, zero=0.02, bad_ptr=0.0, ctr0=None, wrap=False, fill=None, ramps=False):
    """A seeded stream of `nframes` frames: packets of about `mean` bytes, a share `big` of 1200 .. 4097 bytes (continuation frames),
    counter breaks, zero lengths that end a frame's walk early, and -- only where asked -- bad pointers.  `ramps`: payloads that
    compress (the golden file's)."""
    packets, total = [], 0
    while total < nframes * DATA:
        if rng.random() < big:
            ln = int(rng.integers(1200, 4098))
        else:
            ln = int(min(4097, max(3, rng.geometric(1.0 / mean) + 2)))
        packets.append(make_packet(ln, rng, ramp=int(rng.integers(0, 256)) if ramps else None))
        total += ln
    if ctr0 is None:
        ctr0 = (1 << 19) - nframes // 2 if wrap else int(rng.integers(1, 1 << 18))
    fr = build_stream(packets, ctr0, stride, 0)[:nframes].copy()
    if fill is not None and stride > FRAME:
        fr[:, FRAME:] = rng.integers(0, 256, (nframes, stride - FRAME))
    for f in range(nframes):
        r = rng.random()
        ctr, pkt = parse_header(fr[f])
        if r < breaks:
            ctr = (ctr + int(rng.integers(2, 50))) & 0x7FFFF                 # a missed frame
            fr[f, :HEADER] = np.frombuffer(make_header(ctr, pkt), np.uint8)
        elif r < breaks + zero:
            if pkt <= DATA - 8:
                fr[f, HEADER + pkt] &= 0xF0                                   # a zero length at the first header
                fr[f, HEADER + pkt + 1] = 0
        elif r < breaks + zero + bad_ptr:
            fr[f, :HEADER] = np.frombuffer(make_header(ctr, int(rng.integers(1192, 2047))), np.uint8)
    return fr
