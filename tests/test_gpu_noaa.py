"""HrptDemux, TipDemux and HirsDemux on the GPU against the definition (tests/_noaa_ref.py), bit for bit, with sentinels around
every output: row alignments and strides (both store forms of every kernel), per-row device counts, null outputs, calls cut at
every position, state, the handle plumbing, the three operators behind a Deframer on one non-blocking stream, and the C++
mirror's harness on the real library; the HRPT slot ranks past one wave and one pass of the scan, the HIRS state and line in
progress through zero-count rows, count == 0 calls, set_state on one row of many and scans of several passes.  The conditions
those inputs have to meet are asserted on the CPU when the module is imported (the *_plan functions and
assert_minors_reach_every_rank_term)."""
import ctypes as C
import os

import numpy as np
import pytest

import _async as A
import _noaa_ref as R
from qdsp_amd import capi, fec, noaa, ops
from test_noaa_cpu import HOST as HOST_DIR
from test_noaa_cpu import noaa_check_input, run_noaa_check

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
HOST, DEVICE, PIPELINED, DEFERRED = 0, 1, 2, 3
LINKS = [(i, o) for i in (HOST, DEVICE, PIPELINED) for o in (HOST, DEVICE, PIPELINED, DEFERRED)]
S16, S8 = 0xA5C3, 0x5A          # sentinels (0xA5C3 > 0x1FFF and > 1023: no output value)
MINORS = [1, 3, 0, 1, 2, 3, 1]


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def strided(buf, shape, strides, offset):
    """A writable view of the 1-D numpy array `buf`: strides and offset in elements."""
    return np.lib.stride_tricks.as_strided(buf[offset:], shape, [s * buf.itemsize for s in strides])


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_rows(torch, rows, stride, offset, pad=0x77):
    """The 2-D uint8 tensor whose row r is rows[r], `stride` bytes apart, beginning `offset` bytes into an allocation."""
    nchan, width = len(rows), max(len(r) for r in rows)
    host = np.full(offset + nchan * stride + width + 16, pad, np.uint8)
    for r, row in enumerate(rows):
        host[offset + r * stride:offset + r * stride + len(row)] = row
    return dev(torch, host).as_strided((nchan, width), (stride, 1), offset)


# ---- HrptDemux ----

_FRAMES = {}


def hrpt_rows(nchan, n):
    """(frames (nchan, n, 13863) of random bytes with all four `minor` values mixed in every row, the definition's results per
    row); computed once per shape."""
    if (nchan, n) not in _FRAMES:
        rng = np.random.default_rng(100 * nchan + n)
        fr = rng.integers(0, 256, (nchan, n, R.FRAME_BYTES)).astype(np.uint8)
        for r in range(nchan):
            m = np.array([MINORS[(f + r) % len(MINORS)] for f in range(n)], np.uint8)
            fr[r, :, 7] = (fr[r, :, 7] & 0xF9) | (m << 1)
        _FRAMES[nchan, n] = fr, [R.hrpt_demux_fast(fr[r]) for r in range(nchan)]
    return _FRAMES[nchan, n]


SCAN_WAVE, SCAN_PASS = 64, 256    # hrpt_scan_kernel: lanes of a wave (one ballot), frames of a pass (kHrptScanNT)
LONG_N = [63, 64, 65, 255, 256, 257, 515]      # next to a wave, next to a pass, the pass-to-pass carry taken twice
P_TIP, P_AIP = [0.45, 0.15, 0.3, 0.35, 0.2], [0.15, 0.45, 0.3, 0.1, 0.35]     # per row (mod 5): unequal, so the waves' totals differ


def hrpt_long_minors(nchan, n, seed=7):
    """(nchan, n) `minor` values drawn at random, every row with its own probabilities; the first two frames of every wave of the
    first pass and of every later pass are a TIP and an AIP frame (which one first alternates with the row), so that every such
    span holds both even where it is cut short behind its first frame."""
    rng = np.random.default_rng(seed)
    m = np.empty((nchan, n), np.uint8)
    for r in range(nchan):
        pt, pa = P_TIP[r % 5], P_AIP[r % 5]
        m[r] = rng.choice(4, n, p=[(1 - pt - pa) * 0.5, pt, (1 - pt - pa) * 0.5, pa])
        for s in scan_spans(n):
            m[r, s[0]:s[0] + 2] = ([1, 3] if r % 2 == 0 else [3, 1])[:s[1] - s[0]]
    return m


def scan_spans(n):
    """[first, end) of every wave of hrpt_scan_kernel's first pass and of every later pass, for a row of n frames."""
    first = [(s, min(s + SCAN_WAVE, n)) for s in range(0, min(n, SCAN_PASS), SCAN_WAVE)]
    return first + [(s, min(s + SCAN_PASS, n)) for s in range(SCAN_PASS, n, SCAN_PASS)]


def assert_minors_reach_every_rank_term(m, n):
    """The inputs' own conditions, on the CPU: in the first n frames every wave of the first pass and every pass holds a TIP and an
    AIP frame in every row (a span of one frame: a TIP frame in one row and an AIP frame in another), and the waves' totals differ
    -- equal totals could hide a wave offset taken from the wrong wave."""
    m = m[:, :n]
    for a, b in scan_spans(n):
        if b - a >= 2:
            assert all((m[r, a:b] == v).any() for r in range(len(m)) for v in (1, 3)), (n, a, b)
        else:
            assert {1, 3} <= set(m[:, a].tolist()), (n, a)
    if n > SCAN_WAVE:
        for r in range(len(m)):
            for v in (1, 3):
                totals = [int((m[r, a:b] == v).sum()) for a, b in scan_spans(min(n, SCAN_PASS))]
                assert len(set(totals)) >= 2, (n, r, v, totals)


LONG_MINORS = hrpt_long_minors(2, max(LONG_N))             # the sizes of LONG_N are its prefixes
COUNTS_MINORS = hrpt_long_minors(5, 257, seed=8)
for _n in LONG_N:
    assert_minors_reach_every_rank_term(LONG_MINORS, _n)
for _n in (257, 65):                                       # the per-row device counts of test_hrpt_device_counts_past_one_pass
    assert_minors_reach_every_rank_term(COUNTS_MINORS, _n)


def hrpt_long_rows(minors, n):
    """(frames (nchan, n, 13863) of random bytes with minors[:, :n] in the `minor` field, the definition's results per row);
    computed once per (minors, n)."""
    key = (id(minors), n)
    if key not in _FRAMES:
        nchan = len(minors)
        fr = np.random.default_rng(1000 + n).integers(0, 256, (nchan, n, R.FRAME_BYTES), dtype=np.uint8)
        fr[:, :, 7] = (fr[:, :, 7] & 0xF9) | (minors[:, :n] << 1)
        ref = [R.hrpt_demux_fast(fr[r]) for r in range(nchan)]
        assert all(np.array_equal(ref[r][3], minors[r, :n]) for r in range(nchan))
        _FRAMES[key] = fr, ref
    return _FRAMES[key]


def check_hrpt(torch, nchan, n, in_off, aligned, counts=None, skip=(), data=None):
    """One process_batch call on rows that begin `in_off` bytes into an allocation; `aligned`: strides and bases that allow the
    16-byte (AVHRR) and 4-byte (TIP / AIP) stores, else odd ones.  Everything the call may write is compared with the definition,
    everything else with the sentinels.  `data`: (frames, the definition's results) in place of hrpt_rows(nchan, n)."""
    fr, ref = hrpt_rows(nchan, n) if data is None else data
    m = max(n, 1)
    x = dev_rows(torch, [fr[r].ravel() for r in range(nchan)], n * R.FRAME_BYTES + (0 if aligned else 5), in_off)
    ps = m * 2048 + (8 if aligned else 3)
    rs = 5 * ps + (16 if aligned else 1)
    a_off = 8 if aligned else 1
    av_host = np.full(a_off + nchan * rs + 8, S16, np.uint16)
    ts = m * 520 + (8 if aligned else 7)
    t_off = 4 if aligned else 1
    tip_host, aip_host = np.full(t_off + nchan * ts + 8, S8, np.uint8), np.full(t_off + nchan * ts + 8, S8, np.uint8)
    av_d, tip_d, aip_d = dev(torch, av_host), dev(torch, tip_host), dev(torch, aip_host)
    ic = None if counts is None else dev(torch, np.asarray(counts, np.int32))
    eff = [n if counts is None else min(max(int(c), 0), n) for c in (counts if counts is not None else [0] * nchan)]
    op = noaa.HrptDemux(nchan=nchan, max_block=m)
    got = op.process_batch(x, nframes=n, in_counts=ic,
                           avhrr=False if "avhrr" in skip else av_d.as_strided((nchan, 5, m, 2048), (rs, ps, 2048, 1), a_off),
                           tip=False if "tip" in skip else tip_d.as_strided((nchan, m * 520), (ts, 1), t_off),
                           aip=False if "aip" in skip else aip_d.as_strided((nchan, m * 520), (ts, 1), t_off),
                           tip_counts=False if "tip_counts" in skip else None, aip_counts=False if "aip_counts" in skip else None)
    torch.cuda.synchronize()
    want_av, want_tip, want_aip = av_host.copy(), tip_host.copy(), aip_host.copy()
    wt, wa = [], []
    for r in range(nchan):
        c = eff[r]
        av, tip, aip, _ = R.hrpt_demux_fast(fr[r, :c]) if c != n else ref[r]
        strided(want_av, (nchan, 5, m, 2048), (rs, ps, 2048, 1), a_off)[r, :, :c] = av
        want_tip[t_off + r * ts:t_off + r * ts + tip.size] = tip.ravel()
        want_aip[t_off + r * ts:t_off + r * ts + aip.size] = aip.ravel()
        wt.append(len(tip))
        wa.append(len(aip))
    for name, d, want, base in (("avhrr", av_d, want_av, av_host), ("tip", tip_d, want_tip, tip_host), ("aip", aip_d, want_aip, aip_host)):
        got_h, want_h = d.cpu().numpy(), base if name in skip else want
        assert np.array_equal(got_h, want_h), (name, nchan, n, in_off, aligned, counts, skip, "first at", np.flatnonzero(got_h != want_h)[:4].tolist())
    if "tip_counts" not in skip:
        assert got[2].cpu().numpy().tolist() == wt
    if "aip_counts" not in skip:
        assert got[4].cpu().numpy().tolist() == wa
    assert op.counts().tolist() == [eff, wt, wa]
    if n and "avhrr" not in skip:
        assert op.last_kernel()["name"] == "hrpt_avhrr_kernel"
    op.close()
    return wt, wa


@pytest.mark.parametrize("nchan", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 7])
def test_hrpt_rows_at_every_byte_offset(torch, n, nchan):
    """Rows that begin at each byte offset 0 .. 15 of an allocation (13863 is odd: every frame of a row has another alignment);
    even offsets with strides that allow the wide stores, odd ones with odd strides."""
    for off in range(16):
        wt, wa = check_hrpt(torch, nchan, n, off, off % 2 == 0)
    if n == 7:
        _, ref = hrpt_rows(nchan, n)
        assert all(t > 0 and a > 0 for t, a in zip(wt, wa)) and all((ref[r][3] % 2 == 0).any() for r in range(nchan))


@pytest.mark.parametrize("aligned", [True, False])
def test_hrpt_device_counts_and_null_outputs(torch, aligned):
    check_hrpt(torch, 3, 3, 3, aligned, counts=[3, 0, 2])
    check_hrpt(torch, 3, 3, 8, aligned, counts=[9, -1, 1])
    for skip in (("avhrr",), ("tip", "tip_counts"), ("aip",), ("tip", "aip"), ("avhrr", "tip", "aip", "tip_counts", "aip_counts"), ("aip_counts",)):
        check_hrpt(torch, 3, 3, 5, aligned, skip=skip)


def test_hrpt_single_output_forms_and_cuts(torch):
    fr, ref = hrpt_rows(1, 7)
    av, tip, aip, _ = ref[0]
    op = noaa.HrptDemux(max_block=3)                  # (the device forms take more than max_block: the library's rows grow)
    a, t, p = op.process(dev(torch, fr[0].ravel()))
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), av) and np.array_equal(t, tip) and np.array_equal(p, aip)
    # the same frames cut into calls: stateless, so the pieces are the whole
    for cuts in ([3, 4], [1, 1, 5], [0, 7]):
        pos, parts = 0, []
        for c in cuts:
            a, t, p = op.process(dev(torch, fr[0, pos:pos + c].ravel()))
            parts.append((a.cpu().numpy().copy(), t.copy(), p.copy()))
            pos += c
        assert np.array_equal(np.concatenate([q[0] for q in parts], axis=1), av)
        assert np.array_equal(np.concatenate([q[1] for q in parts]), tip) and np.array_equal(np.concatenate([q[2] for q in parts]), aip)
    a, t, p = op.process(fr[0, :3].ravel())           # the host entry point
    av3, tip3, aip3, _ = R.hrpt_demux_fast(fr[0, :3])
    assert np.array_equal(a, av3) and np.array_equal(t, tip3) and np.array_equal(p, aip3) and len(tip3) == 5 == len(aip3)
    L = capi.load()
    assert L.qdsp_hip_hrpt_process(op._h, fr[0].ctypes.data, 4, a.ctypes.data) == ESIZE
    ptr, stride, cnt = op.own_dev("tip")
    assert ptr and cnt and stride >= 3 * 520
    assert op.out_size(5) == 5
    op.close()


@pytest.mark.parametrize("n", LONG_N)
def test_hrpt_scan_past_one_wave_and_one_pass(torch, n):
    """hrpt_scan_kernel's three rank terms -- the ballot below the lane, the totals of the waves below (through LDS) and the
    totals carried from pass to pass -- on two rows of random `minor` sequences (assert_minors_reach_every_rank_term): a wrong
    term puts two frames into one TIP / AIP slot and leaves another slot's sentinels, with the counts still right.  Both store
    forms; the AVHRR lines too, but for the longest size."""
    data = hrpt_long_rows(LONG_MINORS, n)
    for aligned in (True, False):
        wt, wa = check_hrpt(torch, 2, n, 8 if aligned else 3, aligned, skip=("avhrr",) if n > 257 else (), data=data)
        assert wt == [5 * int((LONG_MINORS[r, :n] == 1).sum()) for r in range(2)] and min(wt) > 0 and min(wa) > 0


@pytest.mark.parametrize("aligned", [True, False])
def test_hrpt_device_counts_past_one_pass(torch, aligned):
    """One call of 257 frames over five rows whose device counts are 257, 0, 65, 300 and -1: the scan's loop ends per row, the
    gather's grid is the call's."""
    check_hrpt(torch, 5, 257, 5 if aligned else 8, aligned, counts=[257, 0, 65, 300, -1], data=hrpt_long_rows(COUNTS_MINORS, 257))


def test_hrpt_frame_slots_past_one_pass(torch):
    """qdsp_hip_hrpt_get_frame_slots after a single-row call of 257 frames: TIP frame k -> k, AIP frame k -> k | 1 << 30, any
    other -1, from the definition's `minor` values; the frame count is returned, min(count, cap) entries are written."""
    n = 257
    fr, ref = hrpt_long_rows(LONG_MINORS, n)
    av, tip, aip, minors = ref[0]
    want = np.full(n, -1, np.int32)
    want[minors == 1] = np.arange((minors == 1).sum())
    want[minors == 3] = np.arange((minors == 3).sum()) | (1 << 30)
    assert (want[SCAN_PASS:] >= 0).any() and (want[SCAN_WAVE:SCAN_PASS] >= 0).any() and sorted(set(want.tolist()))[0] == -1
    op = noaa.HrptDemux(max_block=n)
    a, t, p = op.process(dev(torch, fr[0].ravel()))
    assert np.array_equal(a.cpu().numpy(), av) and np.array_equal(t, tip) and np.array_equal(p, aip)
    L = capi.load()
    for cap in (100, n, 300):
        slots = np.full(cap + 3, -7, np.int32)
        assert L.qdsp_hip_hrpt_get_frame_slots(op._h, 0, slots.ctypes.data, cap) == n
        m = min(n, cap)
        assert np.array_equal(slots[:m], want[:m]) and (slots[m:] == -7).all(), cap
    assert L.qdsp_hip_hrpt_get_frame_slots(op._h, 0, None, 0) == n and L.qdsp_hip_hrpt_get_frame_slots(op._h, 1, slots.ctypes.data, 1) == EINVAL
    op.close()


# ---- TipDemux ----

@pytest.mark.parametrize("nchan", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 5, 63, 64, 65])
def test_tip_rows(torch, n, nchan):
    rng = np.random.default_rng(200 + n)
    mf = rng.integers(0, 256, (nchan, n, 104)).astype(np.uint8)
    want_rec = [R.tip_demux(mf[r]) for r in range(nchan)]
    m = max(n, 1)
    op = noaa.TipDemux(nchan=nchan, max_block=m)
    for off in range(16):
        for counts in (None, [max(n - 1 - r, -1) for r in range(nchan)]):
            x = dev_rows(torch, [mf[r].ravel() for r in range(nchan)], n * 104 + (0 if off % 2 == 0 else 3), off)
            o_off, os_ = (off * 5) % 16, m * 74 + (6 if off % 2 == 0 else 9)
            host = np.full(o_off + nchan * os_ + 16, S8, np.uint8)
            out_d = dev(torch, host)
            ic = None if counts is None else dev(torch, np.asarray(counts, np.int32))
            y, cnt = op.process_batch(x, out_d.as_strided((nchan, m * 74), (os_, 1), o_off), count=n, in_counts=ic)
            torch.cuda.synchronize()
            eff = [n if counts is None else min(max(c, 0), n) for c in (counts or [0] * nchan)]
            want = host.copy()
            for r in range(nchan):
                want[o_off + r * os_:o_off + r * os_ + eff[r] * 74] = want_rec[r][:eff[r]].ravel()
            assert np.array_equal(out_d.cpu().numpy(), want), (n, nchan, off, counts)
            assert cnt.cpu().numpy().tolist() == eff and op.counts().tolist() == eff
    if n:
        assert op.last_kernel()["name"] == "tip_kernel"
        one = noaa.TipDemux(max_block=m)
        assert np.array_equal(one.process(mf[0].ravel()), want_rec[0])                              # host
        assert np.array_equal(one.process(dev(torch, mf[0].ravel())).cpu().numpy(), want_rec[0])     # one device row
        h, s, d, b = noaa.TipDemux.split(one.process(mf[0].ravel()))
        assert np.array_equal(h, mf[0][:, R.HIRS_SRC]) and np.array_equal(b, mf[0][:, R.SBUV_SRC])
        one.close()
    op.close()


# ---- HirsDemux ----

def hirs_packets(rng, n, kind="lines"):
    """n packets of random bytes (n, 36) whose elements walk up the line with repeats, non-image elements and wraps ("lines"), or
    are random ("random")."""
    pk = rng.integers(0, 256, (n, 36)).astype(np.uint8)
    e = int(rng.integers(40, 56))
    for i in range(n):
        if kind == "random":
            el = int(rng.integers(0, 64))
        else:
            r = rng.random()
            el = e
            if r < 0.08:
                el = int(rng.integers(56, 64))
            elif r < 0.16:
                pass
            else:
                e += int(rng.integers(1, 4))
                if e > 55:
                    e = int(rng.integers(0, 3)) if rng.random() < 0.5 else 55
                el = e
                if e == 55:
                    e = int(rng.integers(0, 2))
        R._put_bits(pk[i], R.ELEMENT_BIT, R.ELEMENT_LEN, el)
    return pk


def spread(pk, stride, rng):
    """The packets `stride` bytes apart, random bytes between them."""
    out = rng.integers(0, 256, (len(pk), stride)).astype(np.uint8)
    out[:, :36] = pk
    return out.ravel()


def check_hirs(torch, op, rows, n, stride, off, aligned, refs, counts=None, lines_out=None, states=False):
    """One process_batch call of `n` packets per row on `op`; refs: one HirsFast per row, carried along like the handle's state.
    `lines_out`: a list that takes the definition's lines of every row; `states`: get_state of every row is compared too."""
    nchan = len(rows)
    x = dev_rows(torch, rows, max(len(r) for r in rows) + (0 if aligned else 3), off)
    ps = (n + 1) * 56 + (8 if aligned else 5)
    rs = 20 * ps + (8 if aligned else 3)
    o_off = 8 if aligned else 3
    host = np.full(o_off + nchan * rs + 8, S16, np.uint16)
    out_d = dev(torch, host)
    ic = None if counts is None else dev(torch, np.asarray(counts, np.int32))
    y, cnt = op.process_batch(x, out_d.as_strided((nchan, 20, n + 1, 56), (rs, ps, 56, 1), o_off), count=n, in_counts=ic)
    torch.cuda.synchronize()
    want, wc = host.copy(), []
    for r in range(nchan):
        c = n if counts is None else min(max(int(counts[r]), 0), n)
        lines = refs[r].process(rows[r][:c * stride], stride)
        strided(want, (nchan, 20, n + 1, 56), (rs, ps, 56, 1), o_off)[r, :, :lines.shape[1]] = lines
        wc.append(lines.shape[1])
        if lines_out is not None:
            lines_out.append(lines)
    got = out_d.cpu().numpy()
    assert np.array_equal(got, want), (nchan, n, stride, off, aligned, counts, np.flatnonzero(got != want)[:4].tolist())
    assert cnt.cpu().numpy().tolist() == wc and op.counts().tolist() == wc
    if states:
        got_st = [op.get_state(r) for r in range(nchan)]
        assert got_st == [(ref.last_element, ref.new_image_data) for ref in refs], (n, counts, got_st)
    return wc


@pytest.mark.parametrize("stride", [36, 74])
@pytest.mark.parametrize("nchan", [1, 17])
def test_hirs_rows(torch, nchan, stride):
    """Every count in turn on one handle, so that the state and the line in progress carry from call to call; rows with different
    sequences; offsets and strides for both store forms; then per-row device counts."""
    rng = np.random.default_rng(300 + nchan + stride)
    op = noaa.HirsDemux(packet_stride=stride, nchan=nchan, max_block=300)
    refs = [R.HirsFast() for _ in range(nchan)]
    total = 0
    for k, n in enumerate([0, 1, 2, 55, 56, 57, 113, 300, 57]):
        rows = [spread(hirs_packets(rng, n, "random" if (r + k) % 4 == 3 else "lines"), stride, rng) for r in range(nchan)]
        counts = None if k < 8 else [(n - 5 * r) if r % 3 else (0 if r else n + 9) for r in range(nchan)]
        total += sum(check_hirs(torch, op, rows, n, stride, (5 * k + 1) % 16, k % 2 == 0, refs, counts))
        for r in (0, nchan - 1):
            assert op.get_state(r) == (refs[r].last_element, refs[r].new_image_data)
    assert total >= 3 * nchan and op.last_kernel()["name"] == "hirs_pack_kernel"
    op.close()


CARRY_ROWS, CARRY_STRIDE = 17, 74


class Climb:
    """Per row, packets whose elements go up by one from where the row's last ones ended (55 ends the line, 0 follows it)."""

    def __init__(self, nchan, seed, stride=CARRY_STRIDE):
        self.rng, self.pos, self.stride = np.random.default_rng(seed), [(3 * r) % 40 for r in range(nchan)], stride

    def packets(self, r, n, eff=None, kind="climb"):
        """n packets of row r of which the first `eff` are the row's: the others carry element 55, which would end a line if a
        kernel read past the row's count."""
        eff = n if eff is None else eff
        pk = hirs_packets(self.rng, n, "random") if kind == "random" else self.rng.integers(0, 256, (n, 36)).astype(np.uint8)
        for i in range(n):
            if i >= eff:
                R._put_bits(pk[i], R.ELEMENT_BIT, R.ELEMENT_LEN, 55)
            elif kind == "climb":
                R._put_bits(pk[i], R.ELEMENT_BIT, R.ELEMENT_LEN, self.pos[r])
                self.pos[r] = 0 if self.pos[r] == 55 else self.pos[r] + 1
        return spread(pk, self.stride, self.rng)


def hirs_carry_plan():
    """The calls of test_hirs_lines_carried_through_every_kind_of_call -- (count, per-row device counts, the rows' bytes) -- and, from
    the definition alone, the proof that they hold what the test is for.  Rows 0, 3, .. 15 ("idle") have a line in progress after
    call 0, get count 0 in calls 1 and 2 (one flip of the state and partial-line buffers each way) while the other rows get
    packets; call 2 has negative counts and counts above the call's; call 3 has count == 0 for all (no flip); call 4 ends every
    row's line."""
    nchan, eff = CARRY_ROWS, lambda c, n: min(max(c, 0), n)
    spec = [(12, [12 - r % 5 for r in range(nchan)]),
            (9, [0 if r % 3 == 0 else 9 - r % 4 for r in range(nchan)]),
            (7, [0 if r % 3 == 0 else (-1 - r if r % 3 == 1 else 7 + r) for r in range(nchan)]),
            (0, [3] * nchan),
            (75, [75 - r for r in range(nchan)]),
            (30, [(35, -3, 0, 17)[r % 4] for r in range(nchan)]),
            (5, [5] * nchan)]
    gen, calls = Climb(nchan, 330), []
    for k, (n, counts) in enumerate(spec):
        kind = lambda r: "random" if k == 5 and r % 2 else "climb"      # noqa: E731
        calls.append((n, counts, [gen.packets(r, n, eff(counts[r], n), kind(r)) for r in range(nchan)]))
    # the definition's run
    refs, idle = [R.HirsFast() for _ in range(nchan)], list(range(0, nchan, 3))
    snap, spans = {}, 0
    for k, (n, counts, rows) in enumerate(calls):
        if k == 3:
            before = [(ref.buf.copy(), ref.new_image_data) for ref in refs]
        lines = [refs[r].process(rows[r][:eff(counts[r], n) * CARRY_STRIDE], CARRY_STRIDE) for r in range(nchan)]
        if k == 0:
            for r in idle:
                snap[r] = refs[r].buf.copy()
                assert refs[r].new_image_data and 0 < (snap[r] != 0xFFF).any(axis=0).sum() < 55, r
        if k in (1, 2):
            assert all(eff(counts[r], n) == 0 and np.array_equal(refs[r].buf, snap[r]) for r in idle)
            assert sum(eff(counts[r], n) > 0 for r in range(nchan)) >= 5
        if k == 2:
            assert min(counts) < 0 and max(counts) > n
        if k == 4:
            shared = 0
            for r in range(nchan):
                buf, nid = before[r]
                w = buf != 0xFFF
                assert lines[r].shape[1] >= 1 and np.array_equal(lines[r][:, 0][w], buf[w]), r
                shared += bool(nid and w.any())
            assert shared >= 12                      # rows whose line is shared by the calls before and after call 3
            for r in idle:
                w = snap[r] != 0xFFF
                spans += bool(np.array_equal(lines[r][:, 0][w], snap[r][w]) and (lines[r][:, 0][~w] != 0xFFF).any())
    assert spans >= 3 and len(calls) >= 6
    return calls


HIRS_CARRY = hirs_carry_plan()


def test_hirs_lines_carried_through_every_kind_of_call(torch):
    """17 rows, every call with per-row device counts (hirs_carry_plan): a line in progress survives two calls in which its row has
    no packet while others have (hirs_scan_kernel's n == 0 branch and hirs_pack_kernel's line == total == 0 path, once per
    buffer) and a call with count == 0; after every call the whole output allocation, the counts and every row's state are the
    definition's."""
    op = noaa.HirsDemux(packet_stride=CARRY_STRIDE, nchan=CARRY_ROWS, max_block=80)
    refs = [R.HirsFast() for _ in range(CARRY_ROWS)]
    emitted = 0
    for k, (n, counts, rows) in enumerate(HIRS_CARRY):
        emitted += sum(check_hirs(torch, op, rows, n, CARRY_STRIDE, (5 * k + 1) % 16, k % 2 == 0, refs, counts, states=True))
    assert emitted >= CARRY_ROWS
    op.close()


def hirs_long_plan():
    """(count, the two rows' bytes) of test_hirs_scan_past_one_pass; in every row a line ends (element 55) in every span of 256
    packets that is at least 100 long, so that every pass hands a running total on and takes one."""
    rng, calls = np.random.default_rng(340), []
    for n, kinds in [(511, ("lines", "lines")), (512, ("lines", "random")), (513, ("lines", "lines")), (777, ("random", "lines"))]:
        rows = [spread(hirs_packets(rng, n, kind), 36, rng) for kind in kinds]
        for row in rows:
            e = R.hirs_fields_fast(row)[0]
            assert all((e[s:s + 256] == 55).any() for s in range(0, n - 100, 256)), (n, kinds)
        calls.append((n, rows))
    return calls


HIRS_LONG = hirs_long_plan()


def test_hirs_scan_past_one_pass(torch):
    """Calls of 511, 512, 513 and 777 packets on one handle of two rows: hirs_scan_kernel's running line number is carried over one,
    two and three passes of 256 packets, with lines ending in every pass."""
    op = noaa.HirsDemux(nchan=2, max_block=777)
    refs = [R.HirsFast(), R.HirsFast()]
    for k, (n, rows) in enumerate(HIRS_LONG):
        wc = check_hirs(torch, op, rows, n, 36, (3 * k + 2) % 16, k % 2 == 1, refs, states=True)
        assert min(wc) >= 3
    op.close()


def test_hirs_set_state_on_one_row_of_many(torch):
    """set_state(.., chan=5) with lines in progress on all 17 rows: row 5 follows the definition's set_state, the others go on with
    their lines; set_state for all rows; reset clears every row's line in progress."""
    nchan = CARRY_ROWS
    gen = Climb(nchan, 350)
    op = noaa.HirsDemux(packet_stride=CARRY_STRIDE, nchan=nchan, max_block=16)
    refs = [R.HirsFast() for _ in range(nchan)]

    def call(k, n):
        lines = []
        check_hirs(torch, op, [gen.packets(r, n) for r in range(nchan)], n, CARRY_STRIDE, 3 * k + 1, k % 2 == 0, refs, states=True, lines_out=lines)
        return lines

    assert all(ln.shape[1] == 0 for ln in call(0, 10)) and all(ref.new_image_data and (ref.buf != 0xFFF).any() for ref in refs)
    carried = [ref.buf.copy() for ref in refs]
    op.set_state(60, True, chan=5)
    refs[5].set_state(60, True)
    lines = call(1, 6)
    assert [ln.shape[1] for ln in lines] == [int(r == 5) for r in range(nchan)]       # row 5 alone flushes: its element fell below 60
    assert np.array_equal(lines[5][:, 0], carried[5])
    assert all(((ref.buf == c) | (c == 0xFFF)).all() for r, (ref, c) in enumerate(zip(refs, carried)) if r != 5)   # the others' lines go on
    op.set_state(7, False, chan=-1)
    for ref in refs:
        ref.set_state(7, False)
    call(2, 8)
    assert any(ref.new_image_data and (ref.buf != 0xFFF).any() for ref in refs)
    op.reset()
    for ref in refs:
        ref.reset()
    assert all(op.get_state(r) == (0, False) for r in range(nchan))
    gen.pos = [55] * nchan
    lines = call(3, 1)
    assert all(ln.shape[1] == 1 and (ln[:, 0, :55] == 0xFFF).all() and (ln[:, 0, 55] != 0xFFF).any() for ln in lines)
    op.close()


def test_hirs_cut_at_every_position(torch):
    rng = np.random.default_rng(310)
    pk = hirs_packets(rng, 120)
    whole = R.HirsFast().process(pk.ravel())
    assert whole.shape[1] >= 3
    op = noaa.HirsDemux(max_block=120)
    one = op.process(dev(torch, pk.ravel()))
    assert np.array_equal(one.cpu().numpy(), whole)
    for cut in range(1, 120):
        op.reset()
        a = op.process(dev(torch, pk[:cut].ravel())).cpu().numpy()
        b = op.process(dev(torch, pk[cut:].ravel())).cpu().numpy()
        assert np.array_equal(np.concatenate([a, b], axis=1), whole), cut
    op.reset()
    assert np.array_equal(op.process(pk.ravel()), whole)                                             # the host entry point
    assert op.get_state() == (int(R.read_bits(19, 6, pk[-1])), bool(R.read_bits(19, 6, pk[-1]) < 55))
    op.close()


def test_hirs_state_reset_and_the_out_size_bound(torch):
    rng = np.random.default_rng(320)
    op = noaa.HirsDemux(max_block=8)
    assert op.get_state() == (0, False) and op.out_size(1) == 2 and op.out_size(0) == 1
    # an element in the line in progress, then the inconsistent state no stream produces: both flushes fall on one packet
    first = hirs_packets(rng, 1)
    R._put_bits(first[0], 19, 6, 7)
    ref = R.HirsFast()
    assert op.process(first.ravel()).shape[1] == 0 and ref.process(first.ravel()).shape[1] == 0
    op.set_state(60, True)
    ref.set_state(60, True)
    assert op.get_state() == (60, True)
    pk = hirs_packets(rng, 1)
    R._put_bits(pk[0], 19, 6, 55)
    got, want = op.process(pk.ravel()), ref.process(pk.ravel())
    assert want.shape[1] == 2 == op.out_size(1) and np.array_equal(got, want)
    assert (want[:, 0, 7] != 0xFFF).any() and (want[:, 0, :7] == 0xFFF).all()        # the carried line went out first
    assert op.get_state() == (55, False)
    # reset: the state after create, the line in progress cleared
    mid = hirs_packets(rng, 3)
    for i, e in enumerate((3, 4, 5)):
        R._put_bits(mid[i], 19, 6, e)
    op.process(mid.ravel())
    op.reset()
    assert op.get_state() == (0, False)
    end = hirs_packets(rng, 1)
    R._put_bits(end[0], 19, 6, 55)
    got = op.process(end.ravel())
    assert np.array_equal(got, R.HirsFast().process(end.ravel())) and (got[:, 0, :55] == 0xFFF).all()
    L = capi.load()
    for bad in ((64, 0), (-1, 0), (3, 2)):
        assert L.qdsp_hip_hirs_set_state(op._h, 0, *bad) == EINVAL
    assert L.qdsp_hip_hirs_set_state(op._h, 1, 0, 0) == EINVAL
    op.close()


# ---- handles ----

def _ex_cases(rng):
    """(make, input bytes per call (two calls), items, output dtype, output elements, reference (rc, output) per call)."""
    fr, ref = hrpt_rows(1, 2)
    mf = rng.integers(0, 256, (2, 5, 104)).astype(np.uint8)
    pk = hirs_packets(rng, 112)
    hr = R.HirsFast()
    hirs_want = []
    for half in (pk[:56], pk[56:]):
        lines = hr.process(half.ravel())
        full = np.full((20, 57, 56), 0, np.uint16)
        full[:, :lines.shape[1]] = lines
        hirs_want.append((lines.shape[1], full))
    return {
        "hrpt": (lambda: noaa.HrptDemux(max_block=2), [fr[0].ravel(), fr[0, ::-1].ravel()], 2, np.uint16, 2 * 10240,
                 [(0, ref[0][0]), (0, ref[0][0][:, ::-1])]),
        "tip": (lambda: noaa.TipDemux(max_block=5), [mf[0].ravel(), mf[1].ravel()], 5, np.uint8, 5 * 74,
                [(0, R.tip_demux(mf[0])), (0, R.tip_demux(mf[1]))]),
        "hirs": (lambda: noaa.HirsDemux(max_block=56), [pk[:56].ravel(), pk[56:].ravel()], 56, np.uint16, 20 * 57 * 56, hirs_want),
    }


@pytest.mark.parametrize("unit", ["hrpt", "tip", "hirs"])
def test_every_link_pair_of_process_ex(torch, unit):
    L = capi.load()
    make, xs, n, dt, nout, want = _ex_cases(np.random.default_rng(400))[unit]
    ev = C.c_void_p()
    capi.check(L.qdsp_hip_event_create(0, C.byref(ev)))
    xd = [dev(torch, x) for x in xs]
    for il, ol in LINKS:
        op = make()
        if ol == DEFERRED:
            assert L.qdsp_hip_set_done_event(op._h, ev) == 0
        for b in range(2):
            yh = np.zeros(nout, dt)
            yd = dev(torch, yh)
            torch.cuda.synchronize()
            src = xs[b].ctypes.data if il == HOST else xd[b].data_ptr()
            dst = yh.ctypes.data if ol in (HOST, DEFERRED) else yd.data_ptr()
            rc = op._fn("process_ex")(op._h, src, il, n, dst, ol)
            if unit == "hirs" and ol in (PIPELINED, DEFERRED):
                assert rc == EINVAL                   # the line count is returned: the call has to have run
                break
            if ol == DEFERRED:
                assert L.qdsp_hip_event_wait(ev) == 0
            if ol in (DEVICE, PIPELINED):
                torch.cuda.synchronize()
                yh = yd.cpu().numpy()
            wrc, wy = want[b]
            assert rc == wrc, (unit, il, ol, b, rc)
            got = yh.reshape(wy.shape)
            if unit == "hirs":
                got = got[:, :wrc]
                wy = wy[:, :wrc]
            assert np.array_equal(got, wy), (unit, il, ol, b)
        op.close()
    capi.check(L.qdsp_hip_event_destroy(ev))


def test_handles_are_refused_by_other_kinds_and_after_destroy(torch):
    L = capi.load()
    new = {"hrpt": noaa.HrptDemux(max_block=2), "tip": noaa.TipDemux(max_block=2), "hirs": noaa.HirsDemux(max_block=2)}
    old = {"deframer": ops.Deframer(64, np.ones(8, np.uint8), max_block=64), "rs": fec.FalconRs(max_block=2), "threshold": ops.Threshold(max_block=64)}
    probe = lambda prefix, h: int(getattr(L, f"{prefix}_process_dev")(h, None, 0, None, None))
    for name, op in new.items():
        for other in list(new.values()) + list(old.values()):
            rc = probe(other._prefix, op._h)
            assert (rc >= 0) if other is op else (rc == EINVAL), (name, other._prefix, rc)
        for o in old.values():
            assert probe(op._prefix, o._h) == EINVAL
        assert op.last_kernel()["name"] == ""         # the shared helpers take it
    st = (C.c_int * 2)()
    assert L.qdsp_hip_hirs_get_state(new["tip"]._h, 0, st, st) == EINVAL and L.qdsp_hip_hrpt_get_tip(new["hirs"]._h, 0, None, 0) == EINVAL
    for name, op in new.items():
        h = C.c_void_p(op._h.value)
        op.close()
        assert probe(op._prefix, h) == EINVAL and int(getattr(L, f"{op._prefix}_out_size")(h, 1)) == EINVAL
        assert getattr(L, f"{op._prefix}_destroy")(h) is None       # a second destroy: nothing happens
    for o in old.values():
        o.close()


# ---- the chain ----

def test_chain_behind_the_deframer_on_one_stream(torch):
    """Deframer(110900, the 60-bit sync) -> HrptDemux -> TipDemux -> HirsDemux(stride 74) over 2 rows of 3 and 2 frames, every stage
    reading the previous one's device counts; with no synchronisation in between the same bits come out as with one after each
    step, and they are the definition chain's."""
    frames, want = noaa_check_input(5, min_lines=1)
    rows = [frames[:3], frames[3:5]]
    refs = []
    for fr in rows:
        av, tip, aip, _ = R.hrpt_demux_fast(fr)
        rec = R.tip_demux(tip)
        refs.append((av, tip, aip, rec, R.HirsFast().process(rec.ravel(), 74)))
    assert sum(len(r[1]) for r in refs) and sum(len(r[2]) for r in refs) and sum(r[4].shape[1] for r in refs) >= 1
    # (the Deframer works one sync length behind its input; a row's bits end before an unsynchronised frame of zeros could fill)
    width = 41 + 3 * R.FRAME_BITS + 100
    bits = np.zeros((2, width), np.uint8)
    for r, fr in enumerate(rows):
        b = np.unpackbits(fr, axis=1)[:, :R.FRAME_BITS].ravel()
        bits[r, 41 - 4 * r:41 - 4 * r + b.size] = b
    nbits = np.array([width, 37 + 2 * R.FRAME_BITS + 80], np.int32)

    def scenario():
        x, xn = dev(torch, bits), dev(torch, nbits)
        df = ops.Deframer(R.FRAME_BITS, R.sync_bits(), nchan=2, max_block=width)
        hr, tp, hi = noaa.HrptDemux(nchan=2, max_block=4), noaa.TipDemux(nchan=2, max_block=20), noaa.HirsDemux(74, nchan=2, max_block=20)
        cap = df.out_size(width)
        s = {}

        def deframe():
            s["frames"], s["nf"] = df.process_batch(x, in_counts=xn)
            return s["frames"], s["nf"]

        def hrpt():
            s["hr"] = hr.process_batch(s["frames"], nframes=cap, in_counts=s["nf"])
            return s["hr"]

        def tip():
            s["rec"], s["nr"] = tp.process_batch(s["hr"][1], count=5 * cap, in_counts=s["hr"][2])
            return s["rec"], s["nr"]

        def hirs():
            return hi.process_batch(s["rec"], count=5 * cap, in_counts=s["nr"])

        return [A.Call("deframe", deframe, df), A.Call("hrpt", hrpt, hr, {"hrpt_avhrr_kernel"}), A.Call("tip", tip, tp, {"tip_kernel"}),
                A.Call("hirs", hirs, hi, {"hirs_pack_kernel"})]

    null, serial, asy = A.run_modes("noaa_chain", scenario)
    # slots behind a row's count are never written: what the counts cover is compared, in all three runs
    out, out_s, out_n = dict(asy.outputs), dict(serial.outputs), dict(null.outputs)
    for r, (av, tip, aip, rec, lines) in enumerate(refs):
        for o in (out, out_s, out_n):
            nf = int(o["deframe"][1][r])
            assert nf == len(rows[r]) and np.array_equal(o["deframe"][0][r, :nf * R.FRAME_BYTES].reshape(nf, -1), rows[r])
            a, t, tc, p, pc = o["hrpt"]
            assert np.array_equal(a[r][:, :nf], av) and int(tc[r]) == len(tip) and int(pc[r]) == len(aip)
            assert np.array_equal(t[r, :tip.size], tip.ravel()) and np.array_equal(p[r, :aip.size], aip.ravel())
            assert int(o["tip"][1][r]) == len(rec) and np.array_equal(o["tip"][0][r, :rec.size], rec.ravel())
            ln, lc = o["hirs"]
            assert int(lc[r]) == lines.shape[1] and np.array_equal(ln[r][:, :lines.shape[1]], lines)
    assert asy.kernels == serial.kernels


# ---- the mirror's harness ----

def test_noaa_check_files_are_the_operators(tmp_path):
    """noaa_check on the real library, host- and device-linked: its 29 files are the definition chain's."""
    exe = os.path.join(HOST_DIR, "build", "noaa_check")
    assert os.access(exe, os.X_OK), "build() makes it"
    frames, want = noaa_check_input()
    run_noaa_check(exe, tmp_path, frames, want, pers=(1, 4))
