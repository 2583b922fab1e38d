"""The Viterbi decoder on the GPU against the numpy definition (tests/_viterbi_ref.py, which tests/test_viterbi_cpu.py ties to the
recording of libcorrect's own answers), bit for bit, over whole sentinel-filled output buffers: the bytes between frames' rows, behind
a row's last frame and of frames behind a row's count are checked too.
"""
import ctypes as C

import numpy as np
import pytest

import _async as A
import _deframer_ref as D
import _viterbi_ref as V
from qdsp_amd import capi, fec, ops, viterbi

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
SENT = 0xA5
HOSTL, DEVL = 0, 1
ALL = [(r, o, s) for (r, o) in sorted(V.CODES) for s in (False, True)]


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def frames_of(rate, order, poly, sets, soft, n, seed):
    """n frames: coded with noise, pure noise and (soft) saturated, in turn"""
    kinds = [V.KIND_CODED, V.KIND_NOISE] + ([V.KIND_SATURATED] if soft else [])
    return np.stack([V.make_input(rate, order, poly, sets, soft, kinds[i % len(kinds)], seed + i) for i in range(n)])


def run(torch, dec, x, counts=None, lead=(1, 3), pad=(5, 7)):
    """x: (nchan, n, frame_in) through process_batch with rows `pad` bytes longer than their frames and both buffers `lead` bytes
    off their allocation.  Returns (the whole output allocation, lead, row stride)."""
    nchan, n, fin = x.shape
    fo = dec.frame_out_bytes
    assert fin == dec.frame_in_bytes
    istride, ostride = n * fin + pad[0], n * fo + pad[1]
    ib = torch.zeros(lead[0] + nchan * istride + 8, dtype=torch.uint8, device="cuda")
    xin = ib[lead[0]:lead[0] + nchan * istride].view(nchan, istride)
    xin[:, :n * fin] = dev(torch, x.reshape(nchan, n * fin))
    ob = torch.full((lead[1] + nchan * ostride + 8,), SENT, dtype=torch.uint8, device="cuda")
    out = ob[lead[1]:lead[1] + nchan * ostride].view(nchan, ostride)
    ct = None if counts is None else dev(torch, np.asarray(counts, np.int32))
    dec.process_batch(xin, n, ct, out=out)
    torch.cuda.synchronize()
    return ob.cpu().numpy(), lead[1], ostride


def expected(want, counts, total, lead, ostride):
    """want: (nchan, n, frame_out); the whole allocation as it must look"""
    nchan, n, fo = want.shape
    e = np.full(total, SENT, np.uint8)
    for r in range(nchan):
        c = n if counts is None else min(max(int(counts[r]), 0), n)
        e[lead + r * ostride:lead + r * ostride + c * fo] = want[r, :c].reshape(-1)
    return e


def check(torch, dec, x, want, counts=None, lead=(1, 3), pad=(5, 7), what=""):
    got, ld, ostride = run(torch, dec, x, counts, lead, pad)
    e = expected(want, counts, got.size, ld, ostride)
    bad = np.flatnonzero(got != e)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:6].tolist()} (row stride {ostride}, lead {ld})"


def make(rate, order, poly, sets, soft, nchan=1, max_block=64):
    return viterbi.ViterbiDecoder(rate, order, poly, sets, soft=soft, nchan=nchan, max_block=max_block)


@pytest.mark.parametrize("rate,order,soft", ALL)
def test_every_code_at_every_bookkeeping_edge(torch, rate, order, soft):
    """No traceback; the first traceback, the step before and after; the second; a traceback on the first, a middle and the last
    tail step; a renormalisation without a traceback; an output length off every boundary -- coded, noise and saturated frames,
    six a call (a workgroup and a half), both buffers at odd addresses."""
    poly = V.CODES[(rate, order)]
    for k, sets in enumerate(V.edge_sets(rate, order)):
        x = frames_of(rate, order, poly, sets, soft, 6, 100 * sets + order)
        want, _, _ = V.decode(rate, order, poly, x, sets, soft)
        assert want.shape == (6, V.frame_out_bytes(order, sets))
        d = make(rate, order, poly, sets, soft)
        assert (d.frame_in_bytes, d.frame_out_bytes) == (V.frame_in_bytes(rate, sets, soft), V.frame_out_bytes(order, sets))
        check(torch, d, x[None], want[None], lead=(1 + k % 4, 3 - k % 4), what=f"sets {sets}")
        lk = d.last_kernel()
        assert lk["name"] == "viterbi_decode_kernel" and lk["block"] == 256 and lk["grid"] == 2
        d.close()


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("sets", [1200, 1203])
def test_renormalisation_and_traceback_on_one_step(torch, sets, soft):
    """rate 3, order 7: processed step 1190 = 140 + 10 * 105 = 14 * 85"""
    poly = V.CODES[(3, 7)]
    cases, _ = V.schedule(3, 7, sets)
    assert cases[1189] == V.BOTH and V.RENORM in cases and V.TRACEBACK in cases
    x = frames_of(3, 7, poly, sets, soft, 3, 7 * sets)
    want, got_cases, _ = V.decode(3, 7, poly, x, sets, soft)
    assert got_cases == cases
    d = make(3, 7, poly, sets, soft)
    check(torch, d, x[None], want[None])


@pytest.mark.parametrize("rate,order,soft", [(2, 7, True), (2, 7, False), (2, 9, True), (3, 9, True)])
def test_one_long_frame(torch, rate, order, soft):
    poly = V.CODES[(rate, order)]
    x = frames_of(rate, order, poly, 8168, soft, 1 if order == 9 else 3, 8168 + order)
    want, _, _ = V.decode(rate, order, poly, x, 8168, soft)
    d = make(rate, order, poly, 8168, soft)
    check(torch, d, x[None], want[None], lead=(3, 1))


@pytest.mark.parametrize("soft", [False, True])
def test_polynomials_that_are_not_the_published_ones(torch, soft):
    rate, order, poly = V.ODD_CODE
    for sets in (146, 251, 289):
        x = frames_of(rate, order, poly, sets, soft, 5, sets)
        want, _, _ = V.decode(rate, order, poly, x, sets, soft)
        check(torch, make(rate, order, poly, sets, soft), x[None], want[None], what=f"sets {sets}")


class Pool:
    """17 rows x 67 frames of Viterbi27 at 150 sets (one traceback in the tail), soft, and the definition's answer, computed once."""
    SETS, ROWS, FRAMES = 150, 17, 67

    def __init__(self):
        poly = V.CODES[(2, 7)]
        x = frames_of(2, 7, poly, self.SETS, True, self.ROWS * self.FRAMES, 4242)
        want, _, tails = V.decode(2, 7, poly, x, self.SETS, True)
        assert tails
        self.x = x.reshape(self.ROWS, self.FRAMES, -1)
        self.want = want.reshape(self.ROWS, self.FRAMES, -1)


@pytest.fixture(scope="module")
def pool():
    return Pool()


@pytest.mark.parametrize("nchan", [1, 2, 17])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 67])
def test_layouts(torch, pool, nchan, n):
    """A workgroup partly filled, several workgroups; rows with strides beyond their frames, every buffer at an odd address."""
    d = viterbi.Viterbi27(pool.SETS, nchan=nchan)
    for lead, pad in (((1, 3), (5, 7)), ((2, 1), (0, 0)), ((3, 2), (13, 2))):
        check(torch, d, pool.x[:nchan, :n], pool.want[:nchan, :n], lead=lead, pad=pad, what=f"lead {lead} pad {pad}")
    assert d.last_kernel()["grid"] == (nchan * n + 3) // 4


def test_rows_shorter_than_the_call(torch, pool):
    """d_in_counts of [n, 0, 1, n + 5, -1]: frames behind a row's count leave their output untouched"""
    n = 6
    d = viterbi.Viterbi27(pool.SETS, nchan=5)
    check(torch, d, pool.x[:5, :n], pool.want[:5, :n], counts=[n, 0, 1, n + 5, -1])


def test_no_frames_moves_nothing(torch, pool):
    d = viterbi.Viterbi27(pool.SETS, nchan=2)
    x = dev(torch, pool.x[:2, :2].reshape(2, -1))
    out = torch.full((2, 64), SENT, dtype=torch.uint8, device="cuda")
    y = d.process_batch(x, 0, out=out)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (2, 0) and (out.cpu().numpy() == SENT).all()
    L = capi.load()
    assert L.qdsp_hip_viterbi_process_batch_dev(d._h, None, 0, 0, None, None, 0, None) == 0
    d1 = viterbi.Viterbi27(pool.SETS)
    assert d1.process(np.zeros(0, np.uint8)).shape == (0, d1.frame_out_bytes)


def test_a_grid_of_more_than_one_round(torch):
    """17 rows x 1000 frames of the shortest frame there is: more waves than the launch's 4096 workgroups hold"""
    rate, order, sets = 2, 6, 13
    poly = V.CODES[(rate, order)]
    rng = np.random.default_rng(9)
    x = rng.integers(0, 256, (17 * 1000, V.frame_in_bytes(rate, sets, False))).astype(np.uint8)
    want, _, _ = V.decode(rate, order, poly, x, sets, False)
    d = make(rate, order, poly, sets, False, nchan=17)
    check(torch, d, x.reshape(17, 1000, -1), want.reshape(17, 1000, -1))
    assert d.last_kernel()["grid"] == 4096 < 17 * 1000 // 4


def test_entry_forms_agree_with_the_batch_form(torch, pool):
    n = 5
    frames, want = pool.x[0, :n], pool.want[0, :n]
    d = viterbi.Viterbi27(pool.SETS, max_block=n)
    y = d.process(frames)
    assert y.shape == want.shape and y.tobytes() == want.tobytes()
    xd = dev(torch, frames.ravel())
    yd = d.process(xd)
    assert tuple(yd.shape) == want.shape and yd.cpu().numpy().tobytes() == want.tobytes()
    yb = d.process(xd.reshape(1, -1))
    assert yb.cpu().numpy().tobytes() == want.tobytes()
    hin, fo = np.ascontiguousarray(frames.ravel()), d.frame_out_bytes
    for in_link, out_link in ((HOSTL, HOSTL), (HOSTL, DEVL), (DEVL, HOSTL), (DEVL, DEVL)):
        hout = np.full(n * fo + 8, SENT, np.uint8)
        dout = torch.full((n * fo + 8,), SENT, dtype=torch.uint8, device="cuda")
        src = hin.ctypes.data if in_link == HOSTL else xd.data_ptr()
        dst = hout.ctypes.data if out_link == HOSTL else dout.data_ptr()
        torch.cuda.synchronize()
        assert d.process_ex(src, in_link, n, dst, out_link) == 0
        torch.cuda.synchronize()
        res = hout if out_link == HOSTL else dout.cpu().numpy()
        assert res[:want.size].tobytes() == want.tobytes() and (res[want.size:] == SENT).all(), (in_link, out_link)
    assert d.process_ex(hin.ctypes.data, HOSTL, 0, 0, HOSTL) == 0


def test_a_call_queued_behind_held_work(torch, pool):
    """On a non-blocking stream with work still queued in front: the null-stream bits"""
    d = viterbi.Viterbi27(pool.SETS, nchan=3)
    x = dev(torch, pool.x[:3, :9].reshape(3, -1))
    ref = d.process_batch(x).cpu().numpy().copy()
    assert ref.tobytes() == pool.want[:3, :9].tobytes()
    s = A.side_stream()
    out = torch.full((3, 9 * d.frame_out_bytes), SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    A.hold(s, 20.0)
    w = A.Window(s)
    with torch.cuda.stream(s):
        d.process_batch(x, out=out)
    assert w.is_open(), "the hold had ended before the call was queued"
    s.synchronize()
    assert out.cpu().numpy().tobytes() == ref.tobytes()


def test_deframer_feeds_the_decoder_on_one_stream(torch):
    """Deframer -> ViterbiDecoder(hard) through the deframer's device counts with no synchronisation in between, on a non-default
    stream: the two run apart, and the two definitions composed.  The whole deframed frame, sync word included, is the code block."""
    rng = np.random.default_rng(21)
    rate, order, sets = 2, 7, 300
    poly = V.CODES[(rate, order)]
    fl, nchan = sets * rate, 3
    sync = np.unpackbits(np.array([0x1A, 0xCF, 0xFC, 0x1D], np.uint8))
    rows = []
    for r in range(nchan):
        bits = [rng.integers(0, 2, int(rng.integers(0, 200))).astype(np.uint8)]
        for f in range(2 + r):
            b = rng.integers(0, 2, fl).astype(np.uint8)
            b[:32] = sync
            bits.append(b)
        rows.append(np.concatenate(bits))
    n = max(len(b) for b in rows) + 64
    x = np.zeros((nchan, n), np.uint8)
    want = []
    for r in range(nchan):
        x[r, :len(rows[r])] = rows[r]
        fdef, _, _ = D.deframe_ref(x[r], fl, sync, None)
        assert len(fdef) >= 2
        want.append(V.decode(rate, order, poly, fdef, sets, False)[0])
    df = ops.Deframer(fl, sync, 0, nchan=nchan, max_block=n)
    cap = df.out_size(n)
    vd = make(rate, order, poly, sets, False, nchan=nchan, max_block=cap)
    assert df.frame_bytes == vd.frame_in_bytes
    fo = vd.frame_out_bytes
    xd = dev(torch, x)
    s = torch.cuda.Stream()
    ob = torch.full((nchan, cap * fo + 9), SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        frames, counts = df.process_batch(xd)
        vd.process_batch(frames, cap, counts, out=ob)
    s.synchronize()
    got, gc = ob.cpu().numpy(), counts.cpu().numpy()
    assert gc.tolist() == [len(w) for w in want]
    for r in range(nchan):
        assert got[r, :want[r].size].tobytes() == want[r].tobytes() and (got[r, want[r].size:] == SENT).all(), r
    # ... and apart: the deframer's frames taken to the host, decoded by a call of their own
    df2 = ops.Deframer(fl, sync, 0, nchan=1, max_block=n)
    for r in range(nchan):
        f = df2.process(x[r])
        df2.reset()
        assert make(rate, order, poly, sets, False, max_block=cap).process(f).tobytes() == want[r].tobytes()


def test_refusals_and_error_codes(torch, pool):
    L = capi.load()
    d = viterbi.Viterbi27(pool.SETS, nchan=2, max_block=2)
    h, fi, fo = d._h, d.frame_in_bytes, d.frame_out_bytes
    x = torch.zeros(2 * 3 * fi + 64, dtype=torch.uint8, device="cuda")
    y = torch.zeros(2 * 3 * fo + 64, dtype=torch.uint8, device="cuda")
    xp, yp = x.data_ptr(), y.data_ptr()
    f = L.qdsp_hip_viterbi_process_batch_dev
    assert f(h, xp, 2, 2 * fi, None, yp, 2 * fo, None) == 0
    assert f(h, xp, 2, 2 * fi - 1, None, yp, 2 * fo, None) == EINVAL            # short strides
    assert f(h, xp, 2, 2 * fi, None, yp, 2 * fo - 1, None) == EINVAL
    assert f(h, xp, -1, 2 * fi, None, yp, 2 * fo, None) == EINVAL
    assert f(h, xp, (1 << 22) + 1, 1 << 40, None, yp, 1 << 40, None) == EINVAL
    assert f(h, None, 2, 2 * fi, None, yp, 2 * fo, None) == EINVAL
    assert f(h, xp, 2, 2 * fi, None, None, 2 * fo, None) == EINVAL
    assert f(h, xp, 2, 2 * fi, None, xp + 100, 2 * fo, None) == EINVAL          # overlap
    assert L.qdsp_hip_viterbi_process_ex(h, xp, DEVL, 1, yp, DEVL) == EINVAL    # nchan 2
    d1 = viterbi.Viterbi27(pool.SETS, max_block=2)
    hbuf, obuf = np.zeros(3 * fi, np.uint8), np.zeros(3 * fo, np.uint8)
    assert L.qdsp_hip_viterbi_process_ex(d1._h, hbuf.ctypes.data, HOSTL, 3, obuf.ctypes.data, HOSTL) == ESIZE
    assert L.qdsp_hip_viterbi_process_ex(d1._h, xp, DEVL, 3, yp, DEVL) == 0     # device sides: past max_block is served
    # junk, a live handle of another kind, a destroyed decoder
    junk = (C.c_char * 4096)()
    rs = fec.FalconRs(nchan=1, max_block=2)
    old = C.c_void_p(d1._h.value)
    d1.close()
    for bad in (C.c_void_p(C.addressof(junk)), rs._h, old, None):
        assert L.qdsp_hip_viterbi_frame_in_bytes(bad) == EINVAL
        assert L.qdsp_hip_viterbi_frame_out_bytes(bad) == EINVAL
        assert L.qdsp_hip_viterbi_process_dev(bad, xp, 1, yp, None) == EINVAL
        assert f(bad, xp, 1, fi, None, yp, fo, None) == EINVAL
        assert L.qdsp_hip_viterbi_process_ex(bad, xp, DEVL, 1, yp, DEVL) == EINVAL
        assert L.qdsp_hip_viterbi_process(bad, hbuf.ctypes.data, 1, obuf.ctypes.data) == EINVAL
        L.qdsp_hip_viterbi_destroy(bad)                                          # (nothing happens)
    assert L.qdsp_hip_rs_frame_in_bytes(rs._h) == 1279                           # the other unit's handle is alive and well
    assert L.qdsp_hip_rs_frame_in_bytes(h) == EINVAL and L.qdsp_hip_fpkt_frame_stride(h) == EINVAL   # ... and refuses a decoder
    assert L.qdsp_hip_viterbi_frame_in_bytes(h) == fi
    torch.cuda.synchronize()


def test_destroy_takes_the_address_out_of_the_set(torch):
    """A few hundred decoders created and destroyed: every address is refused afterwards, and a second destroy does nothing."""
    L = capi.load()
    ds = [viterbi.Viterbi27(64, max_block=1) for _ in range(40)]
    seen = []
    for rnd in range(8):
        hs = [C.c_void_p(d._h.value) for d in ds]
        assert len({h.value for h in hs}) == len(hs)
        assert all(L.qdsp_hip_viterbi_frame_out_bytes(h) == (64 - 6) // 8 for h in hs)
        for d in ds:
            d.close()
        assert all(L.qdsp_hip_viterbi_frame_out_bytes(h) == EINVAL for h in hs)
        for h in hs:
            L.qdsp_hip_viterbi_destroy(h)
        seen += [h.value for h in hs]
        ds = [viterbi.Viterbi27(64, max_block=1) for _ in range(40)]
    live = {d._h.value for d in ds}
    for d in ds:
        d.close()
    assert len(seen) == 320
    assert all(L.qdsp_hip_viterbi_frame_out_bytes(C.c_void_p(v)) == EINVAL for v in set(seen) | live)
