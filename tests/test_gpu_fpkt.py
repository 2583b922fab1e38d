"""FalconPacketSync on the GPU against the definition (tests/_fpkt_ref.py: run() transcribed), bit for bit, with sentinels around the
output bytes, the offset table and the counts: the frame cases of the definition one by one, pending runs across the waves and
passes of the scan, row alignments and strides (head, body and tail of the 16-byte copies), per-row device counts, calls cut at
every frame, state through empty calls and empty rows, the handle plumbing, the chain behind Deframer and FalconRs on one
non-blocking stream, and the C++ mirror's harness on the real library.  The conditions the inputs have to meet are asserted on the
CPU when the module is imported."""
import ctypes as C
import os

import numpy as np
import pytest

import _async as A
import _deframer_ref as D
import _fpkt_ref as R
import _rs_ref as RS
from qdsp_amd import capi, falcon, fec, ops
from test_fpkt_cpu import HOST as HOST_DIR
from test_fpkt_cpu import packet_check_input, run_packet_check, three_byte_frame

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
HOST, DEVICE, PIPELINED, DEFERRED = 0, 1, 2, 3
LINKS = [(i, o) for i in (HOST, DEVICE, PIPELINED) for o in (HOST, DEVICE, PIPELINED, DEFERRED)]
S8, S32 = 0x5A, -0x5A5A5A5B


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def batch(torch, op, rows, states, nframes=None, counts=None, in_off=0, in_pad=0, out_off=0, out_pad=0, own_offs=False, junk_seed=1):
    """One process_batch call.  rows[r]: the (n_r, frame_stride) frames of row r; states[r] = (lastCounter, pending bytes) before
    the call, replaced by the state after it.  `counts`: the int32 in_counts to pass (None: none; then every row has `nframes`
    frames); rows are filled up to `nframes` frames with random bytes that a kernel which reads past a count would walk.
    Everything the call may write is compared with the definition, everything else with the sentinels.  Returns the packets per
    row."""
    nchan, fs = len(rows), op.frame_stride
    n = max(len(r) for r in rows) if nframes is None else nframes
    rng = np.random.default_rng(junk_seed)
    istride = n * fs + in_pad
    xh = rng.integers(0, 256, in_off + nchan * istride + 32).astype(np.uint8)
    have = []
    for r, fr in enumerate(rows):
        c = len(fr) if counts is None else min(max(int(counts[r]), 0), n)
        assert c <= len(fr) and (counts is not None or c == n)
        have.append(c)
        xh[in_off + r * istride:in_off + r * istride + c * fs] = np.asarray(fr[:c], np.uint8).ravel()
    x = dev(torch, xh).as_strided((nchan, n * fs), (istride, 1), in_off)
    nb, npk = R.out_size(n), R.out_packets(n)
    assert op.out_size(n) == nb and op.out_packets(n) == npk
    ostride, fstride = nb + out_pad, npk + 1 + 3
    ob = torch.full((out_off + nchan * ostride + 32,), S8, dtype=torch.uint8, device="cuda")
    out = ob.as_strided((nchan, nb), (ostride, 1), out_off)
    fb = torch.full((2 + nchan * fstride,), S32, dtype=torch.int32, device="cuda")
    offs = False if own_offs else fb.as_strided((nchan, npk + 1), (fstride, 1), 2)
    cb = torch.full((nchan + 4,), S32, dtype=torch.int32, device="cuda")
    ic = None if counts is None else dev(torch, np.asarray(counts, np.int32))
    _, _, cnt = op.process_batch(x, out, offs, nframes=n, in_counts=ic, counts=cb[2:2 + nchan])
    torch.cuda.synchronize()
    want_o = np.full(ob.numel(), S8, np.uint8)
    want_f = np.full(fb.numel(), S32, np.int32)
    want_c = np.full(cb.numel(), S32, np.int32)
    packets, totals = [], np.zeros((2, nchan), np.int32)
    for r in range(nchan):
        o, f, st = R.serial_row(rows[r][:have[r]], states[r][0], states[r][1])
        assert len(o) <= nb and len(f) - 1 <= npk
        want_o[out_off + r * ostride:out_off + r * ostride + len(o)] = np.frombuffer(o, np.uint8)
        want_f[2 + r * fstride:2 + r * fstride + len(f)] = f
        want_c[2 + r] = len(f) - 1
        totals[:, r] = len(f) - 1, len(o)
        states[r] = (st[0], st[2])
        packets.append(R.split(o, f))
    got_o, got_c = ob.cpu().numpy(), cb.cpu().numpy()
    assert np.array_equal(got_c, want_c), (got_c.tolist(), want_c.tolist())
    if own_offs:
        assert (fb.cpu().numpy() == S32).all()
        for r in range(nchan):
            f = op.offsets(r)
            assert np.array_equal(f, want_f[2 + r * fstride:2 + r * fstride + len(f)]) and len(f) == totals[0, r] + 1, r
    else:
        got_f = fb.cpu().numpy()
        bad = np.flatnonzero(got_f != want_f)
        assert bad.size == 0, ("offsets", bad[:8].tolist(), got_f[bad[:8]].tolist(), want_f[bad[:8]].tolist())
    bad = np.flatnonzero(got_o != want_o)
    assert bad.size == 0, ("bytes", bad[:8].tolist(), len(bad))
    assert np.array_equal(op.counts(), totals)
    for r in range(nchan):
        ctr, rd, pend = op.get_state(r)
        assert (ctr, pend) == states[r] and rd == (len(pend) if pend else -1), (r, ctr, rd, states[r][0], len(states[r][1]))
    return packets


# ---- the frame cases ----

def _frames(*parts):
    return np.concatenate([np.atleast_2d(p) for p in parts])


def _renumber(frames, ctr0):
    """The frames with counters ctr0, ctr0 + 1, ... (pointers kept)."""
    out = frames.copy()
    for j, f in enumerate(out):
        f[:R.HEADER] = np.frombuffer(R.make_header((ctr0 + j) & 0x7FFFF, R.parse_header(f)[1]), np.uint8)
    return out


def _cont(rng):
    return R.make_frame(0, R.CONT, rng.integers(0, 256, R.DATA).astype(np.uint8).tobytes())


def _case(name):
    """(frames (n <= 20, 1195), lastCounter, pending bytes, a check of the case's own condition on the definition's output)."""
    rng = np.random.default_rng(sum(name.encode()))
    P = lambda n: R.make_packet(n, rng)                       # noqa: E731
    tail = [P(300), P(200), P(700)]
    if name == "ends_with_the_frame":
        fr = R.build_stream([P(500), P(691)] + tail, 10)
        return fr, 9, b"", lambda runs, pk: R.walk(fr[0])[2:4] == (R.DATA, -1) and R.parse_header(fr[1])[1] == 0
    if name.startswith("residue_"):
        k = int(name[-1])
        fr = R.build_stream([P(600), P(591 - k), P(100)] + tail, 10)
        return fr, 9, b"", lambda runs, pk: R.walk(fr[0])[3] == k and runs[0] == (0, 1, 100)
    if name == "zero_length":
        fr = R.build_stream([P(400), P(300), P(2000)] + tail, 10)
        fr[0, R.HEADER + 400] &= 0xF0
        fr[0, R.HEADER + 401] = 0
        return fr, 9, b"", lambda runs, pk: R.walk(fr[0])[2:4] == (400, -1) and len(pk[0]) == 400 and (0, 1, 0) not in [(g, f, 0) for g, f, _ in runs]
    if name == "pointer_0_with_a_packet_pending":
        a, b = R.build_stream([P(1000), P(300)], 10), R.build_stream([P(200)] + tail, 11)
        fr = _frames(a[0], b)
        return fr, 9, b"", lambda runs, pk: runs[0] == (0, 1, 191) and R.parse_header(fr[1])[1] == 0
    if name == "pointer_1191":
        fr = R.build_stream([P(800), P(391 + R.DATA)] + tail, 10)
        return fr, 9, b"", lambda runs, pk: R.parse_header(fr[1])[1] == R.DATA and runs[0] == (0, 1, 391 + R.DATA)
    if name in ("pointer_1192", "pointer_2046"):
        a, b = R.build_stream([P(1000), P(300)], 10), R.build_stream(tail + [P(900)], 12)
        bad = R.make_frame(11, int(name[-4:]), rng.integers(0, 256, R.DATA).astype(np.uint8).tobytes())
        fr = _frames(a[0], bad, b)
        return fr, 9, b"", lambda runs, pk: not [1 for g, f, _ in runs if f <= 2] and len(R.PacketSync(11).run(fr[1])) == 0 and len(pk) > 3
    if name == "packet_of_4097_over_four_frames":
        fr = R.build_stream([P(300), P(4097), P(200)] + tail, 10)
        return fr, 9, b"", lambda runs, pk: runs[0] == (0, 3, 4097) and [R.parse_header(f)[1] for f in fr[1:3]] == [R.CONT] * 2
    if name in ("13_continuation_frames", "14_continuation_frames", "completion_to_the_cap", "completion_past_the_cap"):
        ncont = 14 if name.startswith("14") else 13
        a, head = R.build_stream([P(1000), P(300)], 10), 100
        if name.startswith("completion"):
            head = R.CAP - 191 - 13 * R.DATA + (1 if "past" in name else 0)          # 718 reaches 16392 exactly, 719 passes it
        last = R.build_stream([P(R.DATA + head)] + tail, 0)[1:]                        # its first frame's pointer is `head`
        assert R.parse_header(last[0])[1] == head
        fr = _renumber(_frames(a[0], *[_cont(rng) for _ in range(ncont)], last), 10)
        emitted = name in ("13_continuation_frames", "completion_to_the_cap")
        want = 191 + 13 * R.DATA + (100 if name.startswith("13") else R.CAP - 191 - 13 * R.DATA)
        return fr, 9, b"", lambda runs, pk: (runs[:1] == [(0, ncont + 1, want)]) if emitted else (not runs or runs[0][1] > ncont + 1)
    if name == "counter_break_inside_a_pending_run":
        fr = R.build_stream([P(300), P(4097), P(200)] + tail, 10)
        fr[2, :R.HEADER] = np.frombuffer(R.make_header(40, R.CONT), np.uint8)
        fr[3:] = _renumber(fr[3:], 41)
        return fr, 9, b"", lambda runs, pk: not [1 for g, f, _ in runs if f == 3] and len(pk) >= 4
    if name == "wrap_at_2_19":
        fr = R.build_stream([P(900), P(800), P(700), P(2500), P(600), P(900)], (1 << 19) - 2)
        ctr = [R.parse_header(f)[0] for f in fr]
        return fr, (1 << 19) - 3, b"", lambda runs, pk: ctr[:3] == [(1 << 19) - 2, (1 << 19) - 1, 0] and [f for _, f, _ in runs][:1] == [1] and 2 not in [f for _, f, _ in runs]
    if name == "filled_with_three_byte_packets":
        fr = np.stack([three_byte_frame(10 + k) for k in range(3)])
        return fr, 9, b"\x0f\xff\x01", lambda runs, pk: len(pk) == 3 * 397 and runs[0][0] == -1
    raise KeyError(name)


CASES = ["ends_with_the_frame", "residue_1", "residue_2", "residue_3", "zero_length", "pointer_0_with_a_packet_pending", "pointer_1191",
         "pointer_1192", "pointer_2046", "packet_of_4097_over_four_frames", "13_continuation_frames", "14_continuation_frames",
         "completion_to_the_cap", "completion_past_the_cap", "counter_break_inside_a_pending_run", "wrap_at_2_19",
         "filled_with_three_byte_packets"]
for _name in CASES:
    _fr, _last, _pend, _ok = _case(_name)
    assert len(_fr) <= 20 and _fr.shape[1] == R.FRAME, _name
    _o, _f, _ = R.serial_row(_fr, _last, _pend)
    assert _ok(R.pending_runs(_fr, _last, _pend), R.split(_o, _f)), _name


@pytest.mark.parametrize("name", CASES)
def test_frame_cases(torch, name):
    fr, last, pend, _ = _case(name)
    op = falcon.FalconPacketSync(frame_stride=R.FRAME, nchan=1, max_block=len(fr))
    if pend or last:
        op.set_state(last, pend)
    states = [(last, pend)]
    batch(torch, op, [fr], states, out_off=3)
    # and frame by frame: every frame's result goes through the carried state
    op.reset()
    op.set_state(last, pend)
    states, got = [(last, pend)], []
    for f in fr:
        got += batch(torch, op, [f[None]], states, own_offs=True)[0]
    o, ofs, _ = R.serial_row(fr, last, pend)
    assert got == R.split(o, ofs)
    op.close()


# ---- pending runs across the scan's waves and passes ----

LONG_N = [63, 64, 65, 255, 256, 257, 515]
BOUNDS = (64, 256, 512)


def _long_rows(nchan=3, n=max(LONG_N)):
    """Rows of n frames with a packet pending across frames 64, 256 and 512 -- begun one, two or three frames in front of them,
    by row, and completed by them -- and packets of a few hundred bytes elsewhere."""
    rows = []
    for r in range(nchan):
        rng = np.random.default_rng(900 + r)
        packets, total = [], 0
        for b in BOUNDS + (n + 8,):
            start = (b - 1 - r) * R.DATA + 200 + 100 * r           # in frame b - 1 - r
            while total < start - 700:
                ln = int(min(600, max(3, rng.geometric(1.0 / 250) + 2)))
                packets.append(R.make_packet(ln, rng))
                total += ln
            packets.append(R.make_packet(start - total, rng))
            big = (b * R.DATA + 400) - start                     # ends 400 bytes into frame b
            packets.append(R.make_packet(big, rng))
            total = start + big
        fr = R.build_stream(packets, 100 + 1000 * r)[:n].copy()
        rows.append(fr)
    return rows


LONG_ROWS = _long_rows()
for _n in LONG_N:
    for _b in BOUNDS:
        if _n > _b:
            for _r, _fr in enumerate(LONG_ROWS):
                assert any(g == _b - 1 - _r and f == _b for g, f, _ in R.pending_runs(_fr[:_n], 99 + 1000 * _r)), (_n, _b, _r)
assert all(any(g < 512 <= f for g, f, _ in R.pending_runs(fr, 99 + 1000 * r)) for r, fr in enumerate(LONG_ROWS)), "the carry taken twice"


@pytest.mark.parametrize("n", LONG_N)
def test_scan_cuts(torch, n):
    op = falcon.FalconPacketSync(frame_stride=R.FRAME, nchan=3, max_block=n)
    states = []
    for r in range(3):
        op.set_state(99 + 1000 * r, None, r)
        states.append((99 + 1000 * r, b""))
    packets = batch(torch, op, [fr[:n] for fr in LONG_ROWS], states, in_off=1, in_pad=5, out_off=1, out_pad=3)
    assert all(len(p) > n for p in packets)
    assert op.last_kernel()["name"] == "fpkt_pack_kernel"
    op.close()


# ---- layout ----

def _layout_rows(fs, nchan=3, n=12):
    rows = []
    for r in range(nchan):
        rng = np.random.default_rng(50 + 7 * r + fs)
        rows.append(R.random_stream(rng, n, stride=fs, mean=150, big=0.08, breaks=0.05, zero=0.05, bad_ptr=0.03, ctr0=5000 * (r + 1), fill=True))
    return rows


for _fs in (1195, 1275, 1300):
    for _r, _fr in enumerate(_layout_rows(_fs)):
        assert len(R.pending_runs(_fr, 5000 * (_r + 1) - 1)) >= 2, (_fs, _r)


@pytest.mark.parametrize("fs", [1195, 1275, 1300])
@pytest.mark.parametrize("in_off", [0, 1, 3, 15])
def test_row_offsets_strides_and_frame_strides(torch, in_off, fs):
    """Rows that begin 0, 1, 3 and 15 bytes into an allocation with padded strides; output rows at even and odd bytes, so that the
    head, body and tail of the 16-byte copies are all taken; the caller's offset table and the library's."""
    rows = _layout_rows(fs)
    op = falcon.FalconPacketSync(frame_stride=fs, nchan=3, max_block=12)
    assert op.frame_stride == fs == int(op._fn("frame_stride")(op._h))
    states = []
    for r in range(3):
        pend = bytes(range(1, 1 + r))                          # nothing, one and two bytes pending
        op.set_state(5000 * (r + 1) - 1, pend, r)
        states.append((5000 * (r + 1) - 1, pend))
    for k, (out_off, out_pad, own) in enumerate([(0, 0, False), (1, 1, True), (7, 6, False), (16, 16, False)]):
        batch(torch, op, [fr[3 * k:3 * k + 3] for fr in rows], states, in_off=in_off, in_pad=(0, 1, 3, 29)[k], out_off=out_off, out_pad=out_pad,
              own_offs=own)
    op.close()


def test_device_counts_of_zero_negative_and_above_nframes(torch):
    n, rows = 9, _layout_rows(1275, nchan=5, n=9)
    op = falcon.FalconPacketSync(nchan=5, max_block=n)
    states = []
    for r in range(5):
        op.set_state(5000 * (r + 1) - 1, b"\x07" * (r + 1), r)
        states.append((5000 * (r + 1) - 1, b"\x07" * (r + 1)))
    batch(torch, op, rows, states, counts=[0, -3, n + 5, n - 1, 4], nframes=n, in_off=3, out_off=5)
    # the rows without frames kept their state and their pending bytes; now they get their frames
    assert states[0] == (4999, b"\x07") and states[1] == (9999, b"\x07\x07")
    batch(torch, op, [rows[0], rows[1], rows[2][:0], rows[3][n - 1:], rows[4][4:]], states, counts=[n, n, 0, 1, n - 4], nframes=n)
    op.close()


# ---- state ----

def test_cut_into_two_calls_at_every_boundary(torch):
    """Row c of 25 takes frames [0, c) in the first call and [c, 24) in the second: every row's packets are the whole stream's."""
    rng = np.random.default_rng(77)
    fr = R.random_stream(rng, 24, mean=400, big=0.2, breaks=0.04, zero=0.04, bad_ptr=0.03, ctr0=700)
    whole, wf, wst = R.serial_row(fr, 699)
    runs = R.pending_runs(fr, 699)
    assert len(runs) >= 6 and any(f - g >= 2 for g, f, _ in runs), "pending packets, some through continuation frames"
    nchan = len(fr) + 1
    op = falcon.FalconPacketSync(frame_stride=R.FRAME, nchan=nchan, max_block=24)
    op.set_state(699, None)
    states = [(699, b"")] * nchan
    first = batch(torch, op, [fr] * nchan, states, counts=list(range(nchan)), nframes=24, out_off=1)
    second = batch(torch, op, [fr[c:] for c in range(nchan)], states, counts=[24 - c for c in range(nchan)], nframes=24, in_off=1)
    for c in range(nchan):
        assert first[c] + second[c] == R.split(whole, wf), c
        assert states[c] == (wst[0], wst[2])
    op.close()


def test_empty_calls_and_empty_rows_keep_state_and_pending_bytes(torch):
    rng = np.random.default_rng(78)
    pend = [rng.integers(0, 256, k).astype(np.uint8).tobytes() for k in (1, 3, 5000, R.CAP)]
    op = falcon.FalconPacketSync(nchan=4, max_block=4)
    for r in range(4):
        op.set_state(40 + r, pend[r], r)
    assert [op.get_state(r) for r in range(4)] == [(40 + r, len(pend[r]), pend[r]) for r in range(4)]        # the round trip
    x = torch.zeros((4, 1275), dtype=torch.uint8, device="cuda")
    _, _, cnt = op.process_batch(x, nframes=0)
    assert cnt.cpu().tolist() == [0] * 4 and op.counts().tolist() == [[0] * 4] * 2
    assert [op.get_state(r) for r in range(4)] == [(40 + r, len(pend[r]), pend[r]) for r in range(4)]
    states = [(40 + r, pend[r]) for r in range(4)]
    zero = [np.zeros((0, 1275), np.uint8)] * 4
    for k in range(3):                                         # both slots of the double buffer, and back
        batch(torch, op, zero, states, counts=[0, -1, 0, 0], nframes=2, own_offs=k == 1)
    assert states == [(40 + r, pend[r]) for r in range(4)]
    # the carried bytes come out when the rows get a frame: a completion of 0, 1 and 2 bytes, and the full one dropped by one byte
    rows = [R.make_frame(41 + r, (0, 1, 2, 1)[r], R.make_packet(200, rng) * 4)[None] for r in range(4)]
    rows = [np.pad(f, ((0, 0), (0, 80))) for f in rows]
    got = batch(torch, op, rows, states, out_off=1)
    assert [len(g[0]) for g in got[:3]] == [1, 4, 5002] and all(len(p) != R.CAP + 1 for p in got[3])
    op.reset()
    assert [op.get_state(r) for r in range(4)] == [(0, -1, b"")] * 4
    op.close()


def test_set_state_on_one_row_of_many(torch):
    rng = np.random.default_rng(79)
    rows = [R.random_stream(rng, 6, stride=1275, mean=300, big=0.0, breaks=0.0, zero=0.0, ctr0=100 * (r + 1)) for r in range(3)]
    op = falcon.FalconPacketSync(nchan=3, max_block=6)
    states = [(0, b"")] * 3
    batch(torch, op, [fr[:3] for fr in rows], states)
    pend = rng.integers(0, 256, 777).astype(np.uint8).tobytes()
    op.set_state(202, pend, 1)                                 # row 1 only: its next frame completes these bytes
    states[1] = (202, pend)
    got = batch(torch, op, [fr[3:] for fr in rows], states)
    assert got[1][0][:777] == pend
    with pytest.raises(capi.QdspHipError):
        op.set_state(0, b"", 3)
    with pytest.raises(ValueError):
        op.set_state(0, bytes(R.CAP + 1))
    op.close()


# ---- plumbing ----

def test_every_link_pair_of_process_ex(torch):
    L = capi.load()
    rng = np.random.default_rng(80)
    fr = R.random_stream(rng, 8, stride=1275, mean=300, big=0.2, ctr0=300)
    halves = [fr[:4], fr[4:]]
    ev = C.c_void_p()
    capi.check(L.qdsp_hip_event_create(0, C.byref(ev)))
    xd = [dev(torch, h) for h in halves]
    nb = R.out_size(4)
    for il, ol in LINKS:
        op = falcon.FalconPacketSync(max_block=4)
        op.set_state(299, None)
        st = (299, b"")
        if ol == DEFERRED:
            assert L.qdsp_hip_set_done_event(op._h, ev) == 0
        for b in range(2):
            yh = np.full(nb, S8, np.uint8)
            yd = dev(torch, yh)
            torch.cuda.synchronize()
            src = halves[b].ctypes.data if il == HOST else xd[b].data_ptr()
            dst = yh.ctypes.data if ol == HOST else yd.data_ptr()
            rc = op._fn("process_ex")(op._h, src, il, 4, dst, ol)
            if ol in (PIPELINED, DEFERRED):
                assert rc == EINVAL                       # the packet count is returned: the call has to have run
                break
            if ol == DEVICE:
                torch.cuda.synchronize()
                yh = yd.cpu().numpy()
            o, f, s2 = R.serial_row(halves[b], st[0], st[1])
            st = (s2[0], s2[2])
            assert rc == len(f) - 1 > 0, (il, ol, b, rc)
            assert np.array_equal(op.offsets(0, rc), f) and yh[:len(o)].tobytes() == o, (il, ol, b)
        op.close()
    capi.check(L.qdsp_hip_event_destroy(ev))


def test_entry_forms_and_argument_errors(torch):
    L = capi.load()
    rng = np.random.default_rng(81)
    fr = R.random_stream(rng, 6, stride=1275, mean=300, big=0.2, ctr0=300)
    want = [p for _, p in R.PacketSync(0).process(fr)]
    op = falcon.FalconPacketSync(max_block=6)
    assert op.process(fr) == want                                                    # the host entry point
    op.reset()
    body, offs = op.process(dev(torch, fr.ravel()), with_offs=True)                  # process_dev
    assert R.split(body, offs) == want
    assert op.process(fr[:0]) == []
    with pytest.raises(ValueError):
        op.process(fr.ravel()[:1274])
    # over max_block with a side on the host
    big = np.zeros(7 * 1275, np.uint8)
    out = np.zeros(R.out_size(7), np.uint8)
    assert op._fn("process")(op._h, big.ctypes.data, 7, out.ctypes.data) == ESIZE
    # the overlap, the short strides, too many frames
    x = torch.zeros(2 * R.out_size(6), dtype=torch.uint8, device="cuda")
    f = op._fn("process_batch_dev")
    o32 = torch.zeros(R.out_packets(6) + 1, dtype=torch.int32, device="cuda")
    args = lambda **kw: [kw.get(k, v) for k, v in (("h", op._h), ("x", x.data_ptr()), ("n", 6), ("istride", 6 * 1275), ("ic", None),       # noqa: E731
                                                    ("y", x.data_ptr() + 6 * 1275), ("ostride", R.out_size(6)), ("offs", o32.data_ptr()),
                                                    ("fstride", R.out_packets(6) + 1), ("cnt", None), ("s", None))]
    assert f(*args()) == 0
    assert f(*args(y=x.data_ptr() + 6 * 1275 - 81)) == EINVAL                        # the last frame's bytes 1194 and the output
    assert f(*args(y=x.data_ptr() + 5 * 1275 + 1195)) == 0                           # ... but not the bytes behind 1194
    assert f(*args(istride=5 * 1275 + 1194)) == EINVAL and f(*args(istride=5 * 1275 + 1195)) == 0
    assert f(*args(ostride=R.out_size(6) - 1)) == EINVAL and f(*args(fstride=R.out_packets(6))) == EINVAL
    assert f(*args(n=(1 << 20) + 1)) == EINVAL and f(*args(n=-1)) == EINVAL
    assert f(*args(x=None)) == EINVAL and f(*args(y=None)) == EINVAL
    torch.cuda.synchronize()
    op.close()


def test_handles_of_the_two_falcon_units_refuse_each_other(torch):
    L = capi.load()
    pk, rs = falcon.FalconPacketSync(max_block=2), fec.FalconRs(max_block=2)
    st, ctr = (C.c_int * 2)(), C.c_uint32()
    # an Rs handle given to fpkt
    assert L.qdsp_hip_fpkt_out_size(rs._h, 1) == EINVAL and L.qdsp_hip_fpkt_process_dev(rs._h, None, 0, None, None) == EINVAL
    assert L.qdsp_hip_fpkt_get_counts(rs._h, st) == EINVAL and L.qdsp_hip_fpkt_get_state(rs._h, 0, C.byref(ctr), st, None) == EINVAL
    assert L.qdsp_hip_fpkt_process_batch_dev(rs._h, None, 0, 0, None, None, 0, None, 0, None, None) == EINVAL and L.qdsp_hip_fpkt_reset(rs._h) == EINVAL
    # an fpkt handle given to rs
    assert L.qdsp_hip_rs_out_size(pk._h, 1) == EINVAL and L.qdsp_hip_rs_process_dev(pk._h, None, 0, None, None) == EINVAL
    assert L.qdsp_hip_rs_get_counts(pk._h, st) == EINVAL and L.qdsp_hip_rs_frame_in_bytes(pk._h) == EINVAL
    assert L.qdsp_hip_rs_process_batch_dev(pk._h, None, 0, 0, None, None, 0, None, None, None) == EINVAL
    assert L.qdsp_hip_rs_set_maps(pk._h, None, None, None, 0) == EINVAL
    # each takes its own, and the shared helpers take both
    assert L.qdsp_hip_fpkt_out_size(pk._h, 1) == R.out_size(1) and L.qdsp_hip_rs_out_size(rs._h, 1) == 1
    assert pk.last_kernel()["name"] == "" and rs.last_kernel()["name"] == ""
    # the wrong destroy leaves the handle alive; the right one, twice
    L.qdsp_hip_rs_destroy(pk._h)
    L.qdsp_hip_fpkt_destroy(rs._h)
    assert L.qdsp_hip_fpkt_out_size(pk._h, 1) == R.out_size(1) and L.qdsp_hip_rs_out_size(rs._h, 1) == 1
    h = C.c_void_p(pk._h.value)
    pk.close()
    assert L.qdsp_hip_fpkt_out_size(h, 1) == EINVAL and L.qdsp_hip_fpkt_destroy(h) is None
    rs.close()


def test_work_still_queued_on_a_non_blocking_stream(torch):
    """Calls, getters, set_state and reset with earlier calls still queued: the same bits as with a synchronise after every step."""
    rng = np.random.default_rng(82)
    rows = np.stack([R.random_stream(rng, 12, stride=1275, mean=300, big=0.15, ctr0=100 * (r + 1)) for r in range(2)])
    pend = rng.integers(0, 256, 300).astype(np.uint8).tobytes()

    def scenario():
        x = dev(torch, rows.reshape(2, -1))
        op = falcon.FalconPacketSync(nchan=2, max_block=4)
        op.process_batch(x[:, :2 * 1275].contiguous(), offs=False)      # the library's table is made here: making it drains the queue
        op.reset()
        call = lambda k: A.Call(f"call{k}", lambda: op.process_batch(x[:, 2 * k * 1275:2 * (k + 1) * 1275].contiguous(),      # noqa: E731
                                                                      offs=False if k == 3 else None), op, {"fpkt_pack_kernel"})
        # (every host action has a call queued in front of it)
        return [call(0), A.H(op, "get_state", 0), call(1), A.H(op, "counts"), call(2), A.H(op, "set_state", 205, pend, 1),
                call(3), A.H(op, "offsets", 0), call(4), A.H(op, "reset"), call(5), A.H(op, "close")]

    null, serial, asy = A.run_modes("fpkt", scenario)
    # the definition's results of the six calls (call 3 leaves its offsets in the library's table: row 0's are read back)
    st, want = [(0, b""), (0, b"")], {}
    for k in range(6):
        if k == 3:
            st[1] = (205, pend)
        if k == 5:
            st = [(0, b""), (0, b"")]
        for r in range(2):
            wo, wf, ws = R.serial_row(rows[r, 2 * k:2 * k + 2], st[r][0], st[r][1])
            st[r] = (ws[0], ws[2])
            want[k, r] = wo, wf
    assert sum(len(wf) - 1 for _, wf in want.values()) > 20 and want[3, 1][0][:300] == pend
    for res, what in ((null, "null"), (serial, "serial"), (asy, "async")):
        for (la, va), (lb, vb) in zip(null.outputs, res.outputs):
            assert la == lb and len(va) == len(vb)
            if la.startswith("call"):
                # bytes and offsets behind the counts are never written: what the counts cover is compared
                k = int(la[4:])
                o, c = vb[0], vb[-1]
                for r in range(2):
                    wo, wf = want[k, r]
                    assert int(c[r]) == len(wf) - 1 and o[r, :len(wo)].tobytes() == wo, (what, la, r)
                    if len(vb) == 3:
                        assert np.array_equal(vb[1][r, :len(wf)], wf), (what, la, r)
            else:
                assert all(A.same_bits(x, y) for x, y in zip(va, vb)), (what, la)
        assert np.array_equal(dict(res.outputs)["FalconPacketSync.offsets(0,)"][0], want[3, 0][1]), what
    assert asy.kernels == serial.kernels == null.kernels


# ---- the chain ----

def test_chain_behind_the_deframer_and_the_decoder_on_one_stream(torch):
    """Deframer -> FalconRs -> FalconPacketSync over 3 rows of 12 frames on one non-blocking stream, every stage reading the
    previous one's device counts, no host synchronisation in between.  The frames are built by the definitions' inverses; some are
    corrupted past correction, so that the decoder drops them and the packet sync sees the counter break."""
    rng = np.random.default_rng(83)
    lay = RS.falcon_layout()
    sync = np.unpackbits(np.array([0x1A, 0xCF, 0xFC, 0x1D], np.uint8))
    fl, nchan, nfr = 1279 * 8, 3, 12
    i = np.arange(R.FRAME)
    rows, want, dropped = [], [], 0
    for r in range(nchan):
        pk = R.random_stream(rng, nfr, mean=350, big=0.15, breaks=0.0, zero=0.0, ctr0=2000 * (r + 1))
        msgs = lay.in_map[pk ^ lay.xor[i % 255][None, :]].reshape(nfr, 239, 5).transpose(0, 2, 1)      # out_map^-1 = in_map: the dual basis
        enc = lay.encode(msgs)
        for f in ((3, 8) if r != 1 else (0, 5, 6)):
            enc[f, 4 + 5 * rng.choice(255, 12, replace=False)] ^= rng.integers(1, 256, 12).astype(np.uint8)   # 12 errors in codeword 0
        enc[:, :4] = [0x1A, 0xCF, 0xFC, 0x1D]
        out, good, _ = lay.decode(enc)
        assert np.array_equal(out[good][:, :R.FRAME], pk[good]) and 0 < (~good).sum() < nfr
        dropped += int((~good).sum())
        bits = np.concatenate([rng.integers(0, 2, int(rng.integers(0, 200))).astype(np.uint8)] + [np.unpackbits(f) for f in enc])
        rows.append(bits)
        want.append((int(good.sum()), R.serial_row(out[good])))
    assert dropped >= 6
    n = max(len(b) for b in rows) + 64
    x = np.zeros((nchan, n), np.uint8)
    for r in range(nchan):
        x[r, :len(rows[r])] = rows[r]
        fdef, _, _ = D.deframe_ref(x[r], fl, sync, None)
        assert len(fdef) == nfr
    df = ops.Deframer(fl, sync, 0, nchan=nchan, max_block=n)
    cap = df.out_size(n)
    rs = fec.FalconRs(nchan=nchan, max_block=cap)
    ps = falcon.FalconPacketSync(nchan=nchan, max_block=cap)
    xd = dev(torch, x)
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        frames, counts = df.process_batch(xd)
        dec, good = rs.process_batch(frames, nframes=cap, in_counts=counts)
        out, offs, npk = ps.process_batch(dec, nframes=cap, in_counts=good)
    s.synchronize()
    out, offs, npk, good = out.cpu().numpy(), offs.cpu().numpy(), npk.cpu().numpy(), good.cpu().numpy()
    for r in range(nchan):
        ng, (wo, wf, ws) = want[r]
        assert int(good[r]) == ng and int(npk[r]) == len(wf) - 1 > 5, r
        assert np.array_equal(offs[r, :len(wf)], wf) and out[r, :len(wo)].tobytes() == wo, r
        ctr, rd, pend = ps.get_state(r)
        assert (ctr, rd if rd >= 0 else -1, pend) == (ws[0], ws[1], ws[2])
    for o in (df, rs, ps):
        o.close()


# ---- the mirror's harness ----

def test_packet_check_files_are_the_operator(tmp_path, torch):
    """packet_check on the real library, host- and device-linked: its packets are the definition's and the operator's."""
    exe = os.path.join(HOST_DIR, "build", "packet_check")
    assert os.access(exe, os.X_OK), "build() makes it"
    frames, want = packet_check_input()
    op = falcon.FalconPacketSync(max_block=len(frames))
    assert op.process(frames) == want
    op.close()
    run_packet_check(exe, tmp_path, frames, want, pers=(1, 5))
