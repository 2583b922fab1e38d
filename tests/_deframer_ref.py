"""The definition the Deframer tests compare against: dsp::Deframer (src/dsp/deframing.h) in numpy.

`deframe_bits` is the literal per-bit transcription of the reference's run() loop over its work buffer -- the row's last sync_len
bytes (zeros at the start) followed by the call's bytes.  `deframe_ref` is the event form include/qdsp_hip.h states (whole frames
while reading, the next match while searching); tests/test_deframer_cpu.py asserts the two equal.  Both take and return a state, so a
stream may be cut into calls anywhere, and both report the position (in bytes since the reset) at which every frame started.
`threshold_ref` is dsp::Threshold.
"""
import numpy as np


def threshold_ref(x):
    return (np.asarray(x, dtype=np.float32) > np.float32(0.0)).astype(np.uint8)


def frame_bytes(frame_len: int) -> int:
    return (frame_len + 7) // 8


def out_size(count: int, frame_len: int) -> int:
    return 0 if count <= 0 else (count + frame_len - 1) // frame_len


def new_state(frame_len: int, sync_len: int) -> dict:
    return {"bits_read": -1, "bad": 5, "after": False, "tail": np.zeros(sync_len, dtype=np.uint8),
            "cur": np.zeros(frame_bytes(frame_len), dtype=np.uint8), "pos": 0, "start": -1}


def _copy(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def public_state(st):
    """(bits_read, bad, after) as get_state reports them: `after` only means something between two frames."""
    return st["bits_read"], st["bad"], bool(st["after"]) and st["bits_read"] < 0


def deframe_bits(x, frame_len: int, sync, st=None):
    """One call of the reference's loop, bit by bit.  Returns (frames [nf, frame_bytes] uint8, starts, state)."""
    sync = np.asarray(sync, dtype=np.uint8)
    L, fb = len(sync), frame_bytes(frame_len)
    st = new_state(frame_len, L) if st is None else _copy(st)
    x = np.asarray(x, dtype=np.uint8)
    n = len(x)
    buf = np.concatenate([st["tail"], x])
    sw = sync.tobytes()
    raw = buf.tobytes()
    frames, starts = [], []
    bits_read, bad, after, cur = st["bits_read"], st["bad"], st["after"], st["cur"]
    i = 0
    while i < n:
        if bits_read >= 0:
            if bits_read % 8 == 0:
                cur[bits_read // 8] = 0
            cur[bits_read // 8] |= (int(buf[i]) << (7 - bits_read % 8)) & 0xFF
            i += 1
            bits_read += 1
            if bits_read >= frame_len:
                frames.append(cur[:fb].copy())
                starts.append(st["start"])
                bits_read = -1
                after = True
            continue
        elif raw[i:i + L] == sw:
            bits_read = 0
            bad = 0
            st["start"] = st["pos"] + i
            continue
        elif after:
            after = False
            if bad < 5:
                bad += 1
                bits_read = 0
                st["start"] = st["pos"] + i
                continue
        else:
            i += 1
        after = False
    st.update(bits_read=bits_read, bad=bad, after=after, tail=buf[n:n + L].copy(), pos=st["pos"] + n)
    return (np.stack(frames) if frames else np.zeros((0, fb), dtype=np.uint8)), starts, st


def match_map(buf, n: int, sync):
    """match(i) for the n positions of a call over its work buffer (len n + sync_len)."""
    L = len(sync)
    if n == 0:
        return np.zeros(0, dtype=bool)
    win = np.lib.stride_tricks.sliding_window_view(buf, L)[:n]
    return (win == sync[None, :]).all(axis=1)


def deframe_ref(x, frame_len: int, sync, st=None):
    """One call in the event form.  Returns (frames, starts, state) as deframe_bits does."""
    sync = np.asarray(sync, dtype=np.uint8)
    L, fb = len(sync), frame_bytes(frame_len)
    st = new_state(frame_len, L) if st is None else _copy(st)
    x = np.asarray(x, dtype=np.uint8)
    n = len(x)
    buf = np.concatenate([st["tail"], x])
    match = match_map(buf, n, sync)
    hits = np.flatnonzero(match)
    frames, starts = [], []
    bits_read, bad, after, cur = st["bits_read"], st["bad"], bool(st["after"]) and st["bits_read"] < 0, st["cur"]
    i = 0
    while i < n:
        if bits_read >= 0:
            step = min(frame_len - bits_read, n - i)
            k = np.arange(bits_read, bits_read + step)
            if bits_read == 0:
                cur[:] = 0
            np.bitwise_or.at(cur, k // 8, ((buf[i:i + step].astype(np.int64) << (7 - k % 8)) & 0xFF).astype(np.uint8))
            i += step
            bits_read += step
            if bits_read == frame_len:
                frames.append(cur[:fb].copy())
                starts.append(st["start"])
                bits_read = -1
                after = True
            continue
        if after:
            after = False
            if match[i]:
                bad, bits_read = 0, 0
                st["start"] = st["pos"] + i
            elif bad < 5:
                bad, bits_read = bad + 1, 0
                st["start"] = st["pos"] + i
            continue
        j = np.searchsorted(hits, i)
        if j == len(hits):
            i = n
            break
        i = int(hits[j])
        bad, bits_read = 0, 0
        st["start"] = st["pos"] + i
    st.update(bits_read=bits_read, bad=bad, after=after, tail=buf[n:n + L].copy(), pos=st["pos"] + n)
    return (np.stack(frames) if frames else np.zeros((0, fb), dtype=np.uint8)), starts, st


def run_cuts(fn, x, frame_len, sync, cuts, st=None):
    """`fn` over x cut into calls of the given sizes (their sum is len(x)).  Returns (frames, per-call counts, starts, state)."""
    assert sum(cuts) == len(x)
    st = new_state(frame_len, len(sync)) if st is None else st
    frames, counts, starts, p = [], [], [], 0
    for c in cuts:
        f, s, st = fn(x[p:p + c], frame_len, sync, st)
        frames.append(f)
        counts.append(len(f))
        starts += s
        p += c
    return np.concatenate(frames) if frames else np.zeros((0, frame_bytes(frame_len)), np.uint8), counts, starts, st


def stream_with_frames(rng, n: int, frame_len: int, sync, gap=(0, 40), p_sync=0.8, values=(0, 1)):
    """n bytes: runs of frames that begin with the sync word (or, with probability 1 - p_sync, with noise: a bad frame), random
    payloads, and random gaps of noise."""
    sync = np.asarray(sync, dtype=np.uint8)
    out = [np.zeros(0, dtype=np.uint8)]
    total = 0
    while total < n:
        g = int(rng.integers(gap[0], gap[1] + 1))
        parts = [rng.choice(values, size=g).astype(np.uint8)]
        for _ in range(int(rng.integers(1, 5))):
            body = rng.choice(values, size=max(frame_len, len(sync))).astype(np.uint8)
            if rng.random() < p_sync:
                body[:len(sync)] = sync
            parts.append(body[:max(frame_len, 1)] if frame_len >= len(sync) else body)
        for p in parts:
            out.append(p)
            total += len(p)
    return np.concatenate(out)[:n]
