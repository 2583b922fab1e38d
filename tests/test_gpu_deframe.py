"""Threshold and Deframer on the GPU against their numpy definition (tests/_deframer_ref.py), bit for bit: frames, per-call counts
and the state read back, with sentinel bytes around every output row and behind each row's last frame; shapes around the kernels'
boundaries, call cuts, the state machine's corners, input bytes other than 0 / 1, batches with per-row counts, float rows, the
MSK chain feeding the deframer on one stream, Threshold alone, the link codes, and the C++ mirror's frame_check on the real library.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _deframer_ref as D
from qdsp_amd import capi, ops

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
SENT = 0xA5
HOSTL, DEVL, PIPE, DEFER = 0, 1, 2, 3


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits_of(kind, x):
    return D.threshold_ref(x) if kind else np.asarray(x, np.uint8)


def soft(rng, bits):
    """Float soft symbols whose threshold is `bits` (bytes other than 0 count as 1)."""
    mag = rng.uniform(0.05, 3.0, len(bits)).astype(np.float32)
    return np.where(np.asarray(bits) > 0, mag, -mag).astype(np.float32)


def call(torch, d, rows, count, states, fl, sync, in_counts=None, in_pad=5, out_pad=7, lead=0, olead=0):
    """One process_batch call over `rows` (nchan arrays of at least `count` elements) laid out with strides larger than the call,
    checked against deframe_ref: every byte of the output buffer is either a frame byte of the definition or the sentinel, and the
    per-row counts are the definition's.  `states` (a list, None at the start) moves on.  Returns the frames per row."""
    nchan, fb = d.nchan, d.frame_bytes
    dt = np.float32 if d.kind else np.uint8
    stride = count + in_pad
    host = np.zeros(lead + nchan * stride + 16, dt)
    for r in range(nchan):
        host[lead + r * stride: lead + r * stride + count] = rows[r][:count]
    xb = dev(torch, host)
    x = xb.as_strided((nchan, max(count, 1)), (stride, 1), lead)
    nb = d.out_size(count) * fb
    assert nb == D.out_size(count, fl) * D.frame_bytes(fl)
    ostride = nb + out_pad
    ob = torch.full((olead + nchan * ostride + 16,), SENT, dtype=torch.uint8, device="cuda")
    out = ob.as_strided((nchan, max(nb, 1)), (ostride, 1), olead)
    cnt = torch.full((nchan,), -7, dtype=torch.int32, device="cuda")
    ic = None if in_counts is None else dev(torch, np.asarray(in_counts, np.int32))
    d.process_batch(x, out, count=count, in_counts=ic, counts=cnt)
    got, c = ob.cpu().numpy(), cnt.cpu().numpy()
    want = np.full_like(got, SENT)
    frames = []
    for r in range(nchan):
        n = count if in_counts is None else min(max(int(in_counts[r]), 0), count)
        f, _, states[r] = D.deframe_ref(bits_of(d.kind, rows[r][:n]), fl, sync, states[r])
        assert len(f) <= D.out_size(count, fl)
        want[olead + r * ostride: olead + r * ostride + f.size] = f.ravel()
        frames.append(f)
    assert c.tolist() == [len(f) for f in frames], (c.tolist(), [len(f) for f in frames])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (count, bad[:8], got[bad[:8]], want[bad[:8]])
    return frames


def check_states(d, states):
    for r, st in enumerate(states):
        assert d.get_state(r) == D.public_state(st), (r, d.get_state(r), D.public_state(st))


def make_sync(rng, L):
    s = rng.integers(0, 2, L).astype(np.uint8)
    s[0] = 1                       # (never the all-zero word: that one matches through the zero prefix and has a test of its own)
    return s


# ---- 1. shapes ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(L, fl) for L in (1, 8, 32, 60, 256) for fl in (1, 7, 8, 9, 64, 1000)] + [(32, 16)]


@pytest.mark.parametrize("sync_len,frame_len", SHAPES)
def test_shapes_around_the_kernel_boundaries(torch, sync_len, frame_len):
    """Calls of 63, 64, 65 bytes, then next to the match tile and next to the pack workgroup's span, one after the other on one
    handle of three rows (9618 bytes per row)."""
    tile, span = ops.Deframer.tile(), ops.Deframer.pack_span()
    assert (tile, span) == (1024, 2048)
    counts = [63, 64, 65, tile - 1, tile, tile + 1, span - 1, span, span + 1]
    n = sum(counts)
    rng = np.random.default_rng(100 * sync_len + frame_len)
    sync = make_sync(rng, sync_len)
    rows = [D.stream_with_frames(rng, n, frame_len, sync, gap=(0, 2 * sync_len + 30), p_sync=0.7) for _ in range(3)]
    d = ops.Deframer(frame_len, sync, 0, nchan=3, max_block=span + 1)
    assert d.frame_bytes == D.frame_bytes(frame_len) and d.out_size(0) == 0
    states, p, total = [None] * 3, 0, 0
    for c in counts:
        total += sum(len(f) for f in call(torch, d, [r[p:p + c] for r in rows], c, states, frame_len, sync))
        p += c
    check_states(d, states)
    assert total >= 3 * (n // max(frame_len, sync_len)) // 4        # the rows do hold frames
    assert d.last_kernel()["name"] == "deframe_match_kernel"


@pytest.mark.parametrize("nchan", [1, 17, 64, 65])
def test_channel_counts(torch, nchan):
    rng = np.random.default_rng(nchan)
    sync = make_sync(rng, 8)
    rows = [D.stream_with_frames(rng, 300, 24, sync, gap=(0, 40), p_sync=0.7) for _ in range(nchan)]
    d = ops.Deframer(24, sync, 0, nchan=nchan, max_block=300)
    states = [None] * nchan
    for a, b in ((0, 130), (130, 131), (131, 300)):
        call(torch, d, [r[a:b] for r in rows], b - a, states, 24, sync)
    check_states(d, states)


# ---- 2. call cuts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sync_len,frame_len", [(32, 64), (8, 9), (5, 3)])
def test_call_cuts_do_not_matter(torch, sync_len, frame_len):
    """One call, one-byte calls, random cuts that include 0, and cuts inside a sync word, at the first and last bit of a frame and
    in mid-byte of a frame: frames, per-call counts and the final state are the definition's every time, and the frames and the
    final state are the same across the cuts."""
    n = 1200
    rng = np.random.default_rng(7 + sync_len)
    sync = make_sync(rng, sync_len)
    x = D.stream_with_frames(rng, n, frame_len, sync, gap=(0, 50), p_sync=0.7)
    whole, _, starts, st_whole = D.run_cuts(D.deframe_ref, x, frame_len, sync, [n])
    assert len(whole) >= 10
    marks = set()
    for s in starts[:6] + starts[-3:]:
        marks |= {s - sync_len // 2 - 1, s - 1, s, s + 1, s + frame_len - 1, s + frame_len, s + min(4, frame_len - 1), s + 8 + 3}
    marks = sorted(m for m in marks if 0 < m < n)
    crafted = [b - a for a, b in zip([0] + marks, marks + [n])]
    random_cuts = [0]
    while sum(random_cuts) < n:
        random_cuts.append(min(int(rng.integers(0, 60)), n - sum(random_cuts)))
        if len(random_cuts) % 7 == 0:
            random_cuts.append(0)
    assert random_cuts.count(0) >= 3 and sum(random_cuts) == n
    for cuts in ([n], [1] * n, random_cuts, crafted):
        d = ops.Deframer(frame_len, sync, 0, nchan=1, max_block=n)
        states, p, frames = [None], 0, []
        for c in cuts:
            frames.append(call(torch, d, [x[p:p + c]], c, states, frame_len, sync, in_pad=3, out_pad=2)[0])
            p += c
        assert np.concatenate(frames).tobytes() == whole.tobytes()
        check_states(d, states)
        assert d.get_state(0) == D.public_state(st_whole)


# ---- 3. the state machine -----------------------------------------------------------------------------------------------------------
def test_one_sync_then_five_saves_then_silence_then_resume(torch):
    sync = np.array([1, 0, 1, 1, 0, 0, 1, 0] * 4, np.uint8)
    x = np.concatenate([np.zeros(50, np.uint8), sync, np.zeros(64 * 8, np.uint8), sync, np.zeros(200, np.uint8)])
    d = ops.Deframer(64, sync, 0, nchan=1, max_block=len(x))
    states = [None]
    a = 50 + 32 + 64 * 8
    f1 = call(torch, d, [x[:a]], a, states, 64, sync)[0]
    assert len(f1) == 1 + 5 and d.get_state(0) == (-1, 5, False)
    assert f1[0].tobytes() == np.packbits(np.concatenate([sync, np.zeros(32, np.uint8)])).tobytes() and not f1[1:].any()
    f2 = call(torch, d, [x[a:]], len(x) - a, states, 64, sync)[0]
    assert len(f2) == 3 and d.get_state(0) == (8, 3, False)        # the second sync, two saves, and a third one in progress
    check_states(d, states)


def test_a_sync_right_after_a_frame_resets_bad(torch):
    rng = np.random.default_rng(11)
    sync, fl = np.array([1, 1, 1, 0, 0, 1, 0, 1], np.uint8), 24
    pay = lambda: np.concatenate([np.zeros(8, np.uint8), rng.integers(0, 2, 8).astype(np.uint8)])   # noqa: E731  (no sync inside)
    good = lambda: np.concatenate([sync, pay()])                                                     # noqa: E731
    lost = lambda: np.concatenate([np.zeros(8, np.uint8), pay()])                                    # noqa: E731
    x = np.concatenate([np.zeros(10, np.uint8), good(), lost(), lost(), good(), good(), np.zeros(30, np.uint8)])
    d = ops.Deframer(fl, sync, 0, nchan=1, max_block=len(x))
    states, p, seen = [None], 0, []
    for c in (18 + 3 * fl - 2, 4, fl, len(x) - (18 + 3 * fl - 2) - 4 - fl):
        call(torch, d, [x[p:p + c]], c, states, fl, sync)
        p += c
        seen.append(d.get_state(0))
    assert [s[1] for s in seen[:3]] == [2, 0, 0] and seen[0][0] == fl - 2 and seen[1][0] == 2, seen
    check_states(d, states)


def test_overlapping_matches_and_the_zero_prefix(torch):
    ones = np.ones(8, np.uint8)
    x = np.concatenate([np.zeros(5, np.uint8), np.ones(60, np.uint8), np.zeros(40, np.uint8), np.ones(31, np.uint8), np.zeros(9, np.uint8)])
    for cuts in ([len(x)], [7, 6, 1, 50, len(x) - 64]):
        d = ops.Deframer(12, ones, 0, nchan=1, max_block=len(x))
        states, p, n = [None], 0, 0
        for c in cuts:
            n += len(call(torch, d, [x[p:p + c]], c, states, 12, ones)[0])
            p += c
        assert n >= 8
        check_states(d, states)
    # an all-zero sync word matches at position 0 through the zeroed prefix, whatever the first bytes are
    zeros = np.zeros(16, np.uint8)
    y = np.concatenate([np.ones(40, np.uint8), np.zeros(40, np.uint8), np.ones(20, np.uint8)])
    _, starts, _ = D.deframe_ref(y, 20, zeros)
    assert starts[0] == 0
    d = ops.Deframer(20, zeros, 0, nchan=1, max_block=len(y))
    states = [None]
    f = call(torch, d, [y], len(y), states, 20, zeros)[0]
    assert f[0].tobytes() == np.packbits(np.concatenate([np.zeros(16, np.uint8), y[:4]])).tobytes()
    check_states(d, states)


def test_reset_and_state_round_trip(torch):
    rng = np.random.default_rng(13)
    sync = make_sync(rng, 8)
    x = D.stream_with_frames(rng, 700, 40, sync, gap=(0, 30), p_sync=0.8)
    whole, _, starts, _ = D.run_cuts(D.deframe_ref, x, 40, sync, [700])
    d = ops.Deframer(40, sync, 0, nchan=2, max_block=700)
    states = [None, None]
    cut = starts[3] + 13                                   # mid-frame, mid-byte
    a = call(torch, d, [x[:cut], x[:cut]], cut, states, 40, sync)
    st = d.get_state(0)
    assert st == (13, states[0]["bad"], False) and d.get_state(1) == st
    d.set_state(*st, chan=0)                               # the same values: nothing changes, the frame in progress is kept
    d.set_state(-1, 5, False, chan=1)                      # row 1 drops its frame and searches
    states[1] = dict(states[1], bits_read=-1, bad=5, after=False)
    b = call(torch, d, [x[cut:], x[cut:]], 700 - cut, states, 40, sync)
    assert np.concatenate([a[0], b[0]]).tobytes() == whole.tobytes()
    assert np.concatenate([a[1], b[1]]).tobytes() != whole.tobytes()
    check_states(d, states)
    d.reset()
    assert d.get_state(0) == (-1, 5, False) and d.counts().tolist() == [0, 0]
    states = [None, None]
    again = call(torch, d, [x, x], 700, states, 40, sync)
    assert again[0].tobytes() == whole.tobytes() and again[1].tobytes() == whole.tobytes()
    # set_state's domain
    L_ = capi.load()
    for br, bad, aft in ((40, 0, 0), (-2, 0, 0), (0, 6, 0), (0, -1, 0), (-1, 5, 2), (3, 0, 1)):
        assert L_.qdsp_hip_deframer_set_state(d._h, 0, br, bad, aft) == EINVAL, (br, bad, aft)
    assert L_.qdsp_hip_deframer_set_state(d._h, 2, -1, 5, 0) == EINVAL
    assert d.get_state(0) == D.public_state(states[0])


# ---- 4. bytes other than 0 / 1 ------------------------------------------------------------------------------------------------------
def test_other_byte_values_follow_shift_and_truncate(torch):
    rng = np.random.default_rng(17)
    sync = np.array([1, 0, 3, 1, 1, 0], np.uint8)          # matches only with the exact byte 3 in place
    vals = (0, 1, 2, 3, 128, 255)
    x = D.stream_with_frames(rng, 2000, 20, sync, gap=(0, 20), p_sync=0.7, values=vals)
    near = sync.copy()
    near[2] = 1
    x[100:106] = near                                      # the 0 / 1 look-alike of the sync word
    assert all((x == v).any() for v in vals)
    whole, _, starts, _ = D.run_cuts(D.deframe_bits, x, 20, sync, [2000])
    assert len(whole) > 20 and np.isin(whole, [0, 1]).mean() < 0.5
    d = ops.Deframer(20, sync, 0, nchan=1, max_block=2000)
    states, p = [None], 0
    for c in (333, 667, 1000):
        call(torch, d, [x[p:p + c]], c, states, 20, sync)
        p += c
    check_states(d, states)
    d.set_sync(near)                                       # a new word of the same length, from the next call
    d.reset()
    states = [None]
    call(torch, d, [x], 2000, states, 20, near)
    assert capi.load().qdsp_hip_deframer_set_sync(d._h, near.ctypes.data, 5) == EINVAL


# ---- 5. batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_per_row_counts_strides_and_alignment(torch, kind):
    """17 rows whose input counts all differ (0 and `count` among them, one negative, one above `count`), input stride count + 1
    elements -- so the rows start at every byte offset modulo 16 -- and two calls.  Rows 3 and 11 carry the same input and counts."""
    nchan, count, fl = 17, 600, 24
    rng = np.random.default_rng(19 + kind)
    sync = make_sync(rng, 8)
    rows = [D.stream_with_frames(rng, 2 * count, fl, sync, gap=(0, 40), p_sync=0.7) for _ in range(nchan)]
    rows[11] = rows[3].copy()
    if kind:
        rows = [soft(rng, r) for r in rows]
        rows[11] = rows[3].copy()
    ic1 = [0, count, 37, 599, 1, 64, 65, 63, 300, 511, 512, 513, 7, 8, 9, -5, count + 9]
    ic1[11] = ic1[3]
    assert len(set(ic1)) == nchan - 1
    ic2 = list(reversed(ic1))
    ic2[3] = ic2[11] = 77
    d = ops.Deframer(fl, sync, kind, nchan=nchan, max_block=count)
    states = [None] * nchan
    pos = [0] * nchan
    every = []
    for ic, lead, olead in ((ic1, 0, 0), (ic2, 3, 5)):
        f = call(torch, d, [rows[r][pos[r]:pos[r] + count] for r in range(nchan)], count, states, fl, sync, in_counts=ic, in_pad=1, out_pad=3,
                 lead=lead, olead=olead)
        every.append(f)
        pos = [p + min(max(c, 0), count) for p, c in zip(pos, ic)]
    check_states(d, states)
    for f in every:
        assert f[3].tobytes() == f[11].tobytes()
    assert sum(len(f) for fs in every for f in fs) > 100
    # a row alone gives what it gave in the batch
    for r in (2, 8):
        e = ops.Deframer(fl, sync, kind, nchan=1, max_block=count)
        st = [None]
        p = 0
        for k, ic in enumerate((ic1, ic2)):
            n = min(max(ic[r], 0), count)
            f = call(torch, e, [rows[r][p:p + n]], n, st, fl, sync)[0]
            assert f.tobytes() == every[k][r].tobytes()
            p += n


def test_argument_errors(torch):
    sync = np.array([1, 0, 1, 1], np.uint8)
    d = ops.Deframer(16, sync, 0, nchan=2, max_block=64)
    L_ = capi.load()
    x = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    y = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    f = L_.qdsp_hip_deframer_process_batch_dev
    need = d.out_size(100) * d.frame_bytes
    assert need == 14
    assert f(d._h, x.data_ptr(), 100, 100, None, y.data_ptr(), need, None, None) == 0
    assert f(d._h, x.data_ptr(), 100, 99, None, y.data_ptr(), need, None, None) == EINVAL           # short input stride
    assert f(d._h, x.data_ptr(), 100, 100, None, y.data_ptr(), need - 1, None, None) == EINVAL      # short output stride
    assert f(d._h, x.data_ptr(), 100, 100, None, x.data_ptr(), need, None, None) == EINVAL          # equal
    assert f(d._h, x.data_ptr(), 100, 100, None, x.data_ptr() + 150, need, None, None) == EINVAL    # overlapping
    assert f(d._h, x.data_ptr(), -1, 100, None, y.data_ptr(), need, None, None) == EINVAL
    assert f(d._h, None, 100, 100, None, y.data_ptr(), need, None, None) == EINVAL
    assert f(d._h, x.data_ptr(), (1 << 30) + 1, (1 << 30) + 1, None, y.data_ptr(), 1 << 30, None, None) == EINVAL
    torch.cuda.synchronize()
    st = d.get_state(0)
    assert f(d._h, x.data_ptr(), 0, 0, None, y.data_ptr(), 0, None, None) == 0 and d.get_state(0) == st and d.counts().tolist() == [0, 0]
    one = ops.Deframer(16, sync, 0, nchan=1, max_block=64)
    h = np.zeros(200, np.uint8)
    o = np.zeros(200, np.uint8)
    assert L_.qdsp_hip_deframer_process(one._h, h.ctypes.data, 65, o.ctypes.data) == ESIZE
    assert L_.qdsp_hip_deframer_process(d._h, h.ctypes.data, 10, o.ctypes.data) == EINVAL           # two channels: no host entry point
    fl = ops.Deframer(16, sync, 1, nchan=1, max_block=64)
    xf = torch.zeros(64, dtype=torch.float32, device="cuda")
    assert f(fl._h, xf.data_ptr() + 2, 10, 10, None, y.data_ptr(), 2, None, None) == EINVAL          # float rows: 4-byte aligned


def test_handles_are_known_by_kind_and_only_while_alive(torch):
    """Like every per-row kind, the two are looked up by address in the library's handle table.  A handle of the other kind, of
    another unit's kind, a destroyed one and plain memory are all QDSP_HIP_EINVAL, and the shared entry points (last_kernel) take
    the live ones.  (tests/test_gpu_handles.py asks the same of all fourteen kinds.)"""
    L_ = capi.load()
    sync = np.array([1, 0, 1, 1], np.uint8)
    d, t, fm = ops.Deframer(16, sync, 0, nchan=1, max_block=64), ops.Threshold(nchan=1, max_block=64), ops.AmDemod(nchan=1, max_block=64)
    junk = C.create_string_buffer(256)
    for h in (t._h, fm._h, junk):
        assert L_.qdsp_hip_deframer_out_size(h, 10) == EINVAL and L_.qdsp_hip_deframer_reset(h) == EINVAL
    for h in (d._h, fm._h, junk):
        assert L_.qdsp_hip_threshold_process_dev(h, None, 0, None, None) == EINVAL
    assert L_.qdsp_hip_demod_reset(d._h) == EINVAL and L_.qdsp_hip_demod_reset(t._h) == EINVAL
    assert L_.qdsp_hip_deframer_out_size(d._h, 10) == 1 and L_.qdsp_hip_threshold_process_dev(t._h, None, 0, None, None) == 0
    assert d.last_kernel()["name"] == "" and t.last_kernel()["name"] == ""
    old = C.c_void_p(d._h.value)
    d.close()
    assert L_.qdsp_hip_deframer_out_size(old, 10) == EINVAL       # (a look-up by address: the freed handle is not read)


# ---- 5b. the walk's own boundaries: 64 match words (4096 positions) per search step, 2048 words (131072 positions) per chunk --------
WALK_STEP, WALK_CHUNK = 4096, 131072        # (qdsp_amd/csrc/deframe.hip.h: 64 lanes x 64 bits; kDfWalkWords x 64)


def quiet_row(rng, n, sync, words):
    """n random bits in which the sync word occurs exactly where `words` puts it: x[q - len(sync) : q] = sync makes match(q) true.
    Every other occurrence is broken by flipping a bit (and the row is searched again until none is left)."""
    L = len(sync)
    x = rng.integers(0, 2, n).astype(np.uint8)
    for q in words:
        x[q - L:q] = sync
    keep = np.zeros(n, bool)
    for q in words:
        keep[q - L:q] = True
    while True:
        hits = np.flatnonzero(D.match_map(np.concatenate([np.zeros(L, np.uint8), x]), n, sync))
        extra = [q for q in hits if q not in words]
        if not extra:
            assert sorted(hits) == sorted(words)
            return x
        for q in extra:
            free = [p for p in range(q - L, q) if not keep[p]]
            x[free[len(free) // 2]] ^= 1


def test_search_steps_past_4096_positions(torch):
    """One call of 17000 bytes per row.  Row 0: the first word only at position 5000, so the search from 0 takes a step that finds
    nothing; after 1 + 5 frames the search starts again at 5384 (word 84, bit 8) and the next word lies three steps on, placed so
    that a frame ends exactly at 16384 = 4 x 4096.  Row 1: the same 37 positions later, so nothing is aligned.  Row 2: no word."""
    rng = np.random.default_rng(51)
    sync, fl, n = make_sync(rng, 32), 64, 17000
    q1, q2 = 5000, 4 * WALK_STEP - 2 * fl
    stop = q1 + 6 * fl
    assert q1 > WALK_STEP and q2 - stop > 2 * WALK_STEP and (stop >> 6) % 64 != 0 and stop % 64 != 0
    rows = [quiet_row(rng, n, sync, [q1, q2]), quiet_row(rng, n, sync, [q1 + 37, q2 + 37]), quiet_row(rng, n, sync, [])]
    for r, off in ((0, 0), (1, 37)):
        _, starts, _ = D.deframe_ref(rows[r], fl, sync)
        assert starts[:7] == [q1 + off + k * fl for k in range(6)] + [q2 + off] and (r or q2 + 2 * fl == 4 * WALK_STEP)
        assert len(starts) == 6 + 6                         # the second word, five saves, and a search to the end of the call
    d = ops.Deframer(fl, sync, 0, nchan=3, max_block=n)
    states = [None] * 3
    f = call(torch, d, rows, n, states, fl, sync)
    assert [len(v) for v in f] == [12, 12, 0]
    check_states(d, states)
    assert d.get_state(0) == (-1, 5, False) and d.get_state(2) == (-1, 5, False)
    # ... and the same rows cut at the step boundaries and next to them
    e = ops.Deframer(fl, sync, 0, nchan=3, max_block=n)
    st2, p, parts = [None] * 3, 0, [[], [], []]
    for c in (WALK_STEP - 1, 2, WALK_STEP - 1, 2 * WALK_STEP, n - 4 * WALK_STEP):
        for r, v in enumerate(call(torch, e, [x[p:p + c] for x in rows], c, st2, fl, sync)):
            parts[r].append(v)
        p += c
    for r in range(3):
        assert np.concatenate(parts[r]).tobytes() == f[r].tobytes()


def test_walk_across_its_chunk_of_match_words(torch):
    """One call just past 131072 positions, four rows, every one with an early word (frames, five saves, then a search of 31 steps
    whose last one is clipped at the chunk's end).  At the chunk boundary C: row 0 has a frame that spans it; row 1 a frame that
    ends exactly on it with the next word right behind, so the bit tested after the frame is the first of the next chunk; row 2
    the same without that word (a saved frame starts at C); row 3 searches across it and finds its word 500 positions on."""
    rng = np.random.default_rng(53)
    sync, fl, C_ = make_sync(rng, 32), 64, WALK_CHUNK
    n = C_ + 4000
    early = 1000
    words = [[early, C_ - 30], [early, C_ - fl, C_], [early, C_ - fl], [early, C_ + 500]]
    rows = [quiet_row(rng, n, sync, w) for w in words]
    want_starts = [[C_ - 30, C_ - 30 + fl], [C_ - fl, C_, C_ + fl], [C_ - fl, C_, C_ + fl], [C_ + 500, C_ + 500 + fl]]
    for r in range(4):
        _, starts, st = D.deframe_ref(rows[r], fl, sync)
        assert starts[:6] == [early + k * fl for k in range(6)] and starts[6:6 + len(want_starts[r])] == want_starts[r], (r, starts[:10])
        assert len(starts) == (13 if r == 1 else 12) and st["bits_read"] == -1 and st["bad"] == 5   # each row ends searching, in the second chunk
    d = ops.Deframer(fl, sync, 0, nchan=4, max_block=n)
    states = [None] * 4
    f = call(torch, d, rows, n, states, fl, sync)
    assert [len(v) for v in f] == [12, 13, 12, 12]
    check_states(d, states)
    # a second call on the same handle: the state carried out of the second chunk is good, and a float row takes the same walk
    call(torch, d, [x[:3000] for x in rows], 3000, states, fl, sync)
    check_states(d, states)
    e = ops.Deframer(fl, sync, 1, nchan=1, max_block=n)
    stf = [None]
    g = call(torch, e, [soft(rng, rows[1])], n, stf, fl, sync)
    assert g[0].tobytes() == f[1].tobytes()


# ---- 6. float rows ------------------------------------------------------------------------------------------------------------------
SPECIAL = np.array([np.nan, -np.nan, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, np.inf, -np.inf, 1.0, -1.0], np.float32)


def test_float_rows_equal_threshold_then_bytes(torch):
    rng = np.random.default_rng(23)
    sync, fl, n, nchan = make_sync(rng, 8), 24, 1500, 3
    rows = []
    for _ in range(nchan):
        x = soft(rng, D.stream_with_frames(rng, n, fl, sync, gap=(0, 40), p_sync=0.7))
        zero = np.flatnonzero(x < 0)
        one = np.flatnonzero(x > 0)
        x[rng.choice(zero, 60)] = rng.choice(SPECIAL[[0, 1, 2, 3, 5, 7, 9]], 60)       # values that give 0
        x[rng.choice(one, 60)] = rng.choice(SPECIAL[[4, 6, 8]], 60)                    # values that give 1
        rows.append(x)
    assert D.threshold_ref(SPECIAL).tolist() == [0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    d1 = ops.Deframer(fl, sync, np.float32, nchan=nchan, max_block=n)
    st1 = [None] * nchan
    f1 = []
    for a, b in ((0, 700), (700, n)):
        f1.append(call(torch, d1, [r[a:b] for r in rows], b - a, st1, fl, sync, in_pad=3))
    # Threshold, then the byte kind, all on the device
    thr = ops.Threshold(nchan=nchan, max_block=n)
    d0 = ops.Deframer(fl, sync, np.uint8, nchan=nchan, max_block=n)
    for k, (a, b) in enumerate(((0, 700), (700, n))):
        xt = dev(torch, np.stack([r[a:b] for r in rows]))
        by = thr.process_batch(xt)
        assert by.dtype == torch.uint8 and np.array_equal(by.cpu().numpy(), np.stack([D.threshold_ref(r[a:b]) for r in rows]))
        out, cnt = d0.process_batch(by)
        o, c = out.cpu().numpy(), cnt.cpu().numpy()
        for r in range(nchan):
            assert c[r] == len(f1[k][r]) and o[r, :c[r] * d0.frame_bytes].tobytes() == f1[k][r].tobytes()
    for r in range(nchan):
        assert d0.get_state(r) == d1.get_state(r)


def test_msk_chain_feeds_the_deframer_on_one_stream(torch):
    """MskDemod.process_batch -> Deframer.process_batch(in_counts = the chain's counts) with no host step in between equals the
    chain read back and deframed row by row through the host entry point, and the definition."""
    rng = np.random.default_rng(29)
    nchan, n, sps, fl = 4, 4000, 4, 16
    sync = np.array([1, 0], np.uint8)
    rows = []
    for _ in range(nchan):
        b = rng.integers(0, 2, n // sps + 1) * 2.0 - 1.0
        ph = np.cumsum(np.repeat(b, sps)[:n] * (np.pi / 2 / sps))
        rows.append((np.exp(1j * ph) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64))
    x = np.stack(rows)
    mk = lambda: ops.MskDemod(48000.0, 3000.0, 12000.0, nchan=nchan, max_block=n)   # noqa: E731
    chain, d = mk(), ops.Deframer(fl, sync, np.float32, nchan=nchan, max_block=n)
    chain2 = mk()
    hosts = [ops.Deframer(fl, sync, np.float32, nchan=1, max_block=n) for _ in range(nchan)]
    states = [None] * nchan
    total = 0
    for a, b in ((0, 1700), (1700, n)):
        xt = dev(torch, x[:, a:b])
        sym, cnt = chain.process_batch(xt)
        out, fc = d.process_batch(sym, in_counts=cnt)                  # same stream, nothing read back in between
        o, c = out.cpu().numpy(), fc.cpu().numpy()
        sym2, cnt2 = chain2.process_batch(xt)
        s2, c2 = sym2.cpu().numpy(), cnt2.cpu().numpy()
        for r in range(nchan):
            want = hosts[r].process(s2[r, :c2[r]])
            ref, _, states[r] = D.deframe_ref(D.threshold_ref(s2[r, :c2[r]]), fl, sync, states[r])
            assert want.tobytes() == ref.tobytes() and c[r] == len(ref)
            assert o[r, :c[r] * d.frame_bytes].tobytes() == ref.tobytes()
            total += len(ref)
    assert total > 100
    check_states(d, states)


# ---- 7. Threshold alone -------------------------------------------------------------------------------------------------------------
def test_threshold_every_small_count_and_offset(torch):
    """Every count from 0 to 70 and counts around one workgroup's span, at every output offset modulo 16, with the input 16-byte
    aligned and not; sentinels around every output."""
    span = ops.Threshold.span()
    assert span == 4096
    counts = list(range(0, 71)) + [span - 1, span, span + 1, span + 15, span + 16, span + 17, 2 * span + 5]
    rng = np.random.default_rng(31)
    nmax = max(counts)
    x = rng.standard_normal(nmax + 8).astype(np.float32)
    x[rng.integers(0, nmax, 400)] = rng.choice(SPECIAL, 400)
    x[:12] = SPECIAL
    xt = dev(torch, x)
    t = ops.Threshold(nchan=1, max_block=nmax)
    width = (nmax + 48 + 15) // 16 * 16                   # every row of the output buffer starts on a 16-byte boundary
    for xoff in (0, 1):
        want_bits = D.threshold_ref(x[xoff:])
        for off in range(16):
            ob = torch.full((len(counts), width), SENT, dtype=torch.uint8, device="cuda")
            assert ob.data_ptr() % 16 == 0 and width % 16 == 0
            for k, n in enumerate(counts):
                t.process(xt[xoff:xoff + n], ob[k, off:off + max(n, 1)])
            got = ob.cpu().numpy()
            want = np.full_like(got, SENT)
            for k, n in enumerate(counts):
                want[k, off:off + n] = want_bits[:n]
            assert np.array_equal(got, want), (xoff, off, np.argwhere(got != want)[:5])
    assert t.last_kernel()["name"] == "threshold_kernel"
    # the host entry point
    assert np.array_equal(t.process(x[:1000]), D.threshold_ref(x[:1000])) and len(t.process(x[:0])) == 0


def test_threshold_batch_counts_and_errors(torch):
    rng = np.random.default_rng(37)
    nchan, count = 5, 200
    x = rng.standard_normal((nchan, count + 3)).astype(np.float32)
    xt = dev(torch, x)
    t = ops.Threshold(nchan=nchan, max_block=count)
    ic = [0, count, 17, -3, count + 50]
    ob = torch.full((nchan, count + 9), SENT, dtype=torch.uint8, device="cuda")
    t.process_batch(xt, ob[:, 1:], count=count, in_counts=dev(torch, np.asarray(ic, np.int32)))
    got = ob.cpu().numpy()
    want = np.full_like(got, SENT)
    for r, c in enumerate(ic):
        n = min(max(c, 0), count)
        want[r, 1:1 + n] = D.threshold_ref(x[r, :n])
    assert np.array_equal(got, want)
    L_ = capi.load()
    f = L_.qdsp_hip_threshold_process_batch_dev
    y = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    assert f(t._h, xt.data_ptr(), count, count - 1, None, y.data_ptr(), count, None) == EINVAL
    assert f(t._h, xt.data_ptr(), count, count + 3, None, y.data_ptr(), count - 1, None) == EINVAL
    assert f(t._h, xt.data_ptr(), count, count + 3, None, xt.data_ptr(), count, None) == EINVAL
    assert f(t._h, xt.data_ptr() + 1, count, count + 3, None, y.data_ptr(), count, None) == EINVAL
    assert f(t._h, xt.data_ptr(), 0, 0, None, y.data_ptr(), 0, None) == 0
    one = ops.Threshold(nchan=1, max_block=16)
    h, o = np.zeros(32, np.float32), np.zeros(32, np.uint8)
    assert L_.qdsp_hip_threshold_process(one._h, h.ctypes.data, 17, o.ctypes.data) == ESIZE


# ---- 8. link codes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_deframer_process_ex_links(torch, kind):
    rng = np.random.default_rng(41 + kind)
    sync, fl, n = make_sync(rng, 8), 24, 900
    bits = D.stream_with_frames(rng, n, fl, sync, gap=(0, 40), p_sync=0.7)
    x = soft(rng, bits) if kind else bits
    xt = dev(torch, x)
    cuts = [0, 300, 301, 640, n]
    whole, counts, _, st = D.run_cuts(D.deframe_ref, bits_of(kind, x), fl, sync, [b - a for a, b in zip(cuts, cuts[1:])])
    for il in (HOSTL, DEVL, PIPE):
        for ol in (HOSTL, DEVL):
            d = ops.Deframer(fl, sync, kind, nchan=1, max_block=n)
            parts, got_counts = [], []
            for a, b in zip(cuts, cuts[1:]):
                cap = max(d.out_size(b - a) * d.frame_bytes, 1)
                yh = np.full(cap + 4, SENT, np.uint8)
                yd = torch.full((cap + 4,), SENT, dtype=torch.uint8, device="cuda")
                src = x[a:b].ctypes.data if il == HOSTL else xt[a:b].data_ptr()
                torch.cuda.synchronize()
                nf = d.process_ex(src, il, b - a, yh.ctypes.data if ol == HOSTL else yd.data_ptr(), ol)
                y = yh if ol == HOSTL else yd.cpu().numpy()
                assert (y[cap:] == SENT).all()
                parts.append(y[:nf * d.frame_bytes].copy())
                got_counts.append(nf)
            assert np.concatenate(parts).tobytes() == whole.tobytes() and got_counts == counts, (il, ol)
            assert d.get_state(0) == D.public_state(st)
    d = ops.Deframer(fl, sync, kind, nchan=1, max_block=n)
    y = np.zeros(n, np.uint8)
    L_ = capi.load()
    for ol in (PIPE, DEFER, 4, -1):
        assert L_.qdsp_hip_deframer_process_ex(d._h, x.ctypes.data, HOSTL, 10, y.ctypes.data, ol) == EINVAL, ol
    for il in (DEFER, 4, -1):
        assert L_.qdsp_hip_deframer_process_ex(d._h, x.ctypes.data, il, 10, y.ctypes.data, HOSTL) == EINVAL, il
    assert d.get_state(0) == (-1, 5, False)
    # the one-row entry points on tensors and arrays
    assert d.process(x).tobytes() == whole.tobytes()
    d.reset()
    assert d.process(xt).cpu().numpy().tobytes() == whole.tobytes()


def test_threshold_process_ex_links(torch):
    rng = np.random.default_rng(43)
    n = 777
    x = rng.standard_normal(n).astype(np.float32)
    xt = dev(torch, x)
    want = D.threshold_ref(x)
    L_ = capi.load()
    ev = C.c_void_p()
    capi.check(L_.qdsp_hip_event_create(0, C.byref(ev)))
    t = ops.Threshold(nchan=1, max_block=n)
    t.set_done_event(ev.value)                             # (only a deferred host output records it)
    for il in (HOSTL, DEVL, PIPE):
        for ol in (HOSTL, DEVL, PIPE, DEFER):
            yh = np.full(n + 4, SENT, np.uint8)
            yd = torch.full((n + 4,), SENT, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            host_out = ol in (HOSTL, DEFER)
            src = x.ctypes.data if il == HOSTL else xt.data_ptr()
            assert t.process_ex(src, il, n, yh.ctypes.data if host_out else yd.data_ptr(), ol) == 0
            capi.check(L_.qdsp_hip_device_sync(0))
            y = yh if host_out else yd.cpu().numpy()
            assert np.array_equal(y[:n], want) and (y[n:] == SENT).all(), (il, ol)
    fresh = ops.Threshold(nchan=1, max_block=n)
    y = np.zeros(n, np.uint8)
    assert L_.qdsp_hip_threshold_process_ex(fresh._h, x.ctypes.data, HOSTL, 10, y.ctypes.data, DEFER) == EINVAL      # no event set
    for il, ol in ((HOSTL, 4), (HOSTL, -1), (DEFER, HOSTL), (-1, HOSTL)):
        assert L_.qdsp_hip_threshold_process_ex(fresh._h, x.ctypes.data, il, 10, y.ctypes.data, ol) == EINVAL, (il, ol)
    L_.qdsp_hip_event_destroy(ev)


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "frame_check")


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST, "build/frame_check"], stdout=subprocess.DEVNULL, timeout=300)
    return BIN


@pytest.fixture(scope="module")
def mirror_streams():
    """The streams of tests/test_deframer_cpu.py's run of the harness on the fake library: a random 32-bit sync word, then per frame
    length 6000 bits and their soft symbols, and what the bit-by-bit definition cuts from them (computed once)."""
    rng = np.random.default_rng(5)
    sync = rng.integers(0, 2, 32).astype(np.uint8)
    out = {"sync": sync}
    for fl in (256, 9):
        x = D.stream_with_frames(rng, 6000, fl, sync, gap=(0, 200), p_sync=0.7)
        soft_x = np.where(x > 0, 1.0, -1.0).astype(np.float32) * rng.uniform(0.1, 2.0, len(x)).astype(np.float32)
        want, _, _ = D.deframe_bits(x, fl, sync)
        assert len(want) >= 5
        out[fl] = (x, soft_x, want)
    return out


@pytest.mark.parametrize("block", [4096, 33, 5])
@pytest.mark.parametrize("fl", [256, 9])
@pytest.mark.parametrize("kind,link", [("b", "host"), ("f", "dev"), ("f", "host")])
def test_frame_check_files_are_the_operators(torch, harness, mirror_streams, tmp_path, kind, link, fl, block):
    """source -> [Threshold ->] Deframer -> sink of the C++ mirror on the real library, the Threshold's output handed over in device
    memory or through the host buffers: the file is what one Deframer handle gives over the same blocks, and the definition's."""
    sync = mirror_streams["sync"]
    x, soft_x, want = mirror_streams[fl]
    src = soft_x if kind == "f" else x
    sync.tofile(tmp_path / "sync.u8")
    src.tofile(tmp_path / "x.bin")
    p = subprocess.run([harness, kind, link, "x.bin", "y.bin", str(block), str(fl), "sync.u8"], cwd=tmp_path, check=True, timeout=180,
                       capture_output=True, text=True)
    assert "graph ok" in p.stdout and f"{link} link" in p.stdout, p.stdout
    got = np.fromfile(tmp_path / "y.bin", dtype=np.uint8)
    op = ops.Deframer(fl, sync, 1 if kind == "f" else 0, max_block=block)
    mine = [op.process(src[a:a + block]) for a in range(0, len(src), block)]
    mine = np.concatenate(mine)
    assert len(want) >= 5 and mine.shape == want.shape
    assert got.tobytes() == mine.tobytes(), "the mirror's file is not the operator's frames"
    assert got.tobytes() == want.tobytes(), "the mirror's file is not the definition's frames"
