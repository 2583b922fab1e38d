"""The Reed-Solomon decoder and FalconRS on the GPU against the numpy definition (tests/_rs_ref.py) and the recordings of libcorrect's
own answers (tests/golden/rs_ref_io.npz, rs_ref_codes.npz), bit for bit: output bytes with sentinels around every row and behind each
row's last good frame, the per-row counts and the per-codeword error counts with sentinels behind a short row; and the C++ mirror's
falcon_check on the real library.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _deframer_ref as D
import _rs_ref as R
from qdsp_amd import capi, fec, ops

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "falcon_check")
EINVAL, ESIZE = -10001, -10003
SENT, ESENT = 0xA5, -99
HOSTL, DEVL, PIPE, DEFER = 0, 1, 2, 3
CCSDS16, CCSDS32, OTHER4 = (0x187, 120, 11, 16), (0x187, 112, 11, 32), (0x11d, 1, 1, 4)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "rs_ref_io.npz"))


@pytest.fixture(scope="module")
def codes():
    return np.load(os.path.join(HERE, "golden", "rs_ref_codes.npz"))


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gen_frames(rng, lay, F, p_bad=0.3):
    """F frames of random messages: a good one has 0 .. t errors in every codeword, a bad one t + 1 .. t + 4 in one to three."""
    I, t = lay.depth, lay.code.num_roots // 2
    frames = lay.encode(rng.integers(0, 256, (F, I, lay.code.k)).astype(np.uint8))
    frames[:, :lay.skip] = rng.integers(0, 256, (F, lay.skip))
    for f in range(F):
        ne = rng.integers(0, t + 1, I)
        ne[rng.integers(0, I)] = t                                 # (every frame has a codeword at the limit)
        if rng.random() < p_bad:
            for c in rng.choice(I, min(I, int(rng.integers(1, 4))), replace=False):
                ne[c] = t + 1 + int(rng.integers(0, 4))
        for c in range(I):
            pos = rng.choice(255, int(ne[c]), replace=False)
            frames[f, lay.skip + pos * I + c] ^= rng.integers(1, 256, len(pos)).astype(np.uint8)
    return frames


class Pool:
    """Frames and what the definition makes of them, computed once."""

    def __init__(self, lay, frames):
        self.lay, self.frames = lay, frames
        self.out, self.good, self.errs = lay.decode(frames)


@pytest.fixture(scope="module")
def falcon():
    lay = R.falcon_layout()
    p = Pool(lay, gen_frames(np.random.default_rng(11), lay, 480))
    assert 0.5 < p.good.mean() < 0.85 and p.errs.max() == 8
    return p


def call(torch, d, pool, idx, nframes, in_counts=None, in_pad=5, out_pad=7, lead=0, olead=0, with_errs=True):
    """One process_batch call: row r holds the pool's frames idx[r] (nframes of them), laid out with strides larger than the call and
    `lead` bytes in front.  Every byte of the output buffer is a byte of the definition's packed good frames or the sentinel; counts
    and per-codeword errs are the definition's, errs untouched behind a short row."""
    lay = pool.lay
    nchan, fi, fo, I = d.nchan, lay.frame_in, lay.frame_out, lay.depth
    assert (d.frame_in, d.frame_out) == (fi, fo)
    stride = nframes * fi + in_pad
    host = np.full(lead + nchan * stride + 16, 0x3C, np.uint8)
    for r in range(nchan):
        host[lead + r * stride: lead + r * stride + nframes * fi] = pool.frames[idx[r]].ravel()
    xb = dev(torch, host)
    x = xb.as_strided((nchan, max(nframes * fi, 1)), (stride, 1), lead)
    ostride = nframes * fo + out_pad
    ob = torch.full((olead + nchan * ostride + 16,), SENT, dtype=torch.uint8, device="cuda")
    out = ob.as_strided((nchan, max(nframes * fo, 1)), (ostride, 1), olead)
    cnt = torch.full((nchan,), -7, dtype=torch.int32, device="cuda")
    eb = torch.full((nchan, max(nframes * I, 1)), ESENT, dtype=torch.int32, device="cuda") if with_errs else None
    ic = None if in_counts is None else dev(torch, np.asarray(in_counts, np.int32))
    rows, cnt2 = d.process_batch(x, out, nframes=nframes, in_counts=ic, counts=cnt, errs=eb)
    assert cnt2 is cnt and tuple(rows.shape) == (nchan, nframes * fo)
    got, c = ob.cpu().numpy(), cnt.cpu().numpy()
    want = np.full_like(got, SENT)
    wc, we = [], np.full((nchan, max(nframes * I, 1)), ESENT, np.int32)
    for r in range(nchan):
        n = nframes if in_counts is None else min(max(int(in_counts[r]), 0), nframes)
        sel = np.asarray(idx[r][:n], np.int64)
        g = pool.out[sel][pool.good[sel]]
        want[olead + r * ostride: olead + r * ostride + g.size] = g.ravel()
        wc.append(len(g))
        we[r, :n * I] = pool.errs[sel].ravel()
    assert c.tolist() == wc, (c.tolist(), wc)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (nframes, bad[:8], got[bad[:8]], want[bad[:8]])
    if with_errs:
        e = eb.cpu().numpy()
        assert np.array_equal(e, we), np.argwhere(e != we)[:8]
    assert d.counts().tolist() == wc
    return wc


# ---- 1. every recorded word ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ci", range(3 + len(R.ODD_CODES)))
def test_every_recorded_word(torch, golden, codes, ci):
    """The words libcorrect answered for, as frames of depth 1: message bytes, verdict and the order its locator search left.
    0 .. 2: the three codes of rs_ref_io.npz; from 3 on: the codes of rs_ref_codes.npz (R.ODD_CODES)."""
    if ci >= 3:
        golden, ci = codes, ci - 3
    p = tuple(int(v) for v in golden[f"params_{ci}"])
    words, rc, order, msg = golden[f"words_{ci}"], golden[f"rc_{ci}"], golden[f"order_{ci}"], golden[f"msg_{ci}"]
    k = 255 - p[3]
    d = fec.RsDecoder(*p, depth=1, max_block=len(words))
    assert (d.frame_in, d.frame_out) == (255, k)
    ob = torch.full((len(words) * k + 32,), SENT, dtype=torch.uint8, device="cuda")
    eb = torch.full((1, len(words)), ESENT, dtype=torch.int32, device="cuda")
    rows, cnt = d.process_batch(dev(torch, words.reshape(1, -1)), ob[:len(words) * k].reshape(1, -1), errs=eb)
    good = rc >= 0
    assert int(cnt.cpu()[0]) == int(good.sum())
    got = ob.cpu().numpy()
    ng = int(good.sum()) * k
    assert got[:ng].tobytes() == msg[good].tobytes() and (got[ng:] == SENT).all()
    assert np.array_equal(eb.cpu().numpy()[0], np.where(good, order, -1))
    assert d.last_kernel()["name"] == "rs_decode_kernel" and d.last_kernel()["block"] == 64


# ---- 2. Falcon frames over shapes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nchan", [1, 3, 65])
@pytest.mark.parametrize("nframes", [0, 1, 2, 7])
def test_falcon_shapes(torch, falcon, nchan, nframes):
    """Per-row counts from a device array (some 0, some nframes, one beyond and one negative), strides with slack, sentinels before,
    between and behind every row's output; then the same rows without counts."""
    rng = np.random.default_rng(100 * nchan + nframes)
    d = fec.FalconRs(nchan=nchan, max_block=8)
    idx = [rng.choice(len(falcon.frames), nframes, replace=False) for _ in range(nchan)]
    counts = rng.integers(0, nframes + 1, nchan)
    counts[0] = nframes
    if nchan > 1:
        counts[1] = 0
        counts[2] = nframes + 3
        counts[-1] = -2 if nchan > 3 else nframes
    lead = (5 * nchan + 3 * nframes) % 16
    call(torch, d, falcon, idx, nframes, in_counts=counts, lead=lead, olead=(lead * 7 + 1) % 16)
    total = sum(call(torch, d, falcon, idx, nframes, lead=(lead + 9) % 16, in_pad=0, out_pad=0))
    assert nframes == 0 or nchan < 65 or 0 < total < nchan * nframes


@pytest.mark.parametrize("lead", range(16))
def test_input_rows_at_every_byte_offset(torch, falcon, lead):
    d = fec.FalconRs(nchan=2, max_block=3)
    idx = [np.arange(3) + 6 * lead, np.arange(3) + 6 * lead + 3]
    call(torch, d, falcon, idx, 3, lead=lead, olead=15 - lead, in_pad=lead % 3, out_pad=lead % 5)


# ---- 3. which codeword fails, which frames drop ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def picked(falcon):
    """Falcon frames with exactly one bad codeword at a chosen place, and clean ones."""
    lay = falcon.lay
    rng = np.random.default_rng(12)
    frames = lay.encode(rng.integers(0, 256, (12, 5, lay.code.k)).astype(np.uint8))
    for f, c in enumerate((0, 2, 4, 0, 1, 3)):                     # frames 0 .. 5: codeword c takes 12 errors
        frames[f, 4 + rng.choice(255, 12, replace=False) * 5 + c] ^= 0x41
    for f in range(12):                                            # and everywhere a correctable scatter
        c = f % 5
        if f >= 6 or c != (0, 2, 4, 0, 1, 3)[f]:
            frames[f, 4 + rng.choice(255, 1 + f % 8, replace=False) * 5 + c] ^= 0x17
    p = Pool(lay, frames)
    assert p.good.tolist() == [False] * 6 + [True] * 6
    assert [int(np.flatnonzero(e < 0)[0]) for e in p.errs[:6]] == [0, 2, 4, 0, 1, 3] and ((p.errs[:6] < 0).sum(axis=1) == 1).all()
    return p


def test_one_bad_codeword_first_middle_last(torch, picked):
    d = fec.FalconRs(nchan=3, max_block=4)
    call(torch, d, picked, [[6, 0, 7, 8], [1, 9, 10, 2], [2, 1, 0, 11]], 4)


def test_rows_with_first_last_alternate_and_all_frames_dropped(torch, picked):
    G, B = [6, 7, 8, 9, 10, 11, 6], [0, 1, 2, 3, 4, 5, 0]
    rows = [[B[0]] + G[1:], G[:6] + [B[1]], [B[i] if i % 2 == 0 else G[i] for i in range(7)], [G[i] if i % 2 == 0 else B[i] for i in range(7)], B,
            G]
    d = fec.FalconRs(nchan=6, max_block=7)
    assert call(torch, d, picked, rows, 7, lead=3, olead=5) == [6, 6, 3, 4, 0, 7]


# ---- 4. other codes and depths ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,depth,skip,full_out", [(CCSDS32, 1, 0, 0), (CCSDS32, 4, 3, 1), (CCSDS32, 5, 64, 0), (CCSDS32, 8, 1, 1),
                                                        (OTHER4, 3, 2, 0), (OTHER4, 8, 0, 1), (CCSDS16, 2, 7, 0)])
def test_depths_roots_and_polynomials(torch, params, depth, skip, full_out):
    rng = np.random.default_rng(depth * 100 + params[3])
    in_map, out_map = rng.permutation(256).astype(np.uint8), rng.permutation(256).astype(np.uint8)
    xor = rng.integers(0, 256, int(rng.integers(1, 255 * depth + 1))).astype(np.uint8)
    lay = R.Layout(R.Code(*params), depth, skip, full_out, in_map, out_map, xor)
    pool = Pool(lay, gen_frames(rng, lay, 18, p_bad=0.35))
    assert 0 < pool.good.sum() < 18 and pool.errs.max() == params[3] // 2
    d = fec.RsDecoder(*params, depth=depth, skip=skip, full_out=full_out, in_map=in_map, out_map=out_map, xor=xor, nchan=3, max_block=6)
    assert d.out_size(6) == 6
    call(torch, d, pool, [np.arange(6), np.arange(6, 12), np.arange(12, 18)], 6, in_counts=[6, 4, 5], lead=depth, olead=depth + 1)
    assert d.last_kernel()["block"] == 64 * depth
    # the identity maps and no XOR sequence
    lay0 = R.Layout(lay.code, depth, skip, full_out)
    p0 = Pool(lay0, in_map[pool.frames[:4]])
    d0 = fec.RsDecoder(*params, depth=depth, skip=skip, full_out=full_out, nchan=1, max_block=4)
    call(torch, d0, p0, [np.arange(4)], 4)


def test_scan_past_its_step_of_256_frames(torch):
    """600 frames per row (the slot scan takes 256 a step), about a third dropped, also through scratch grown past max_block."""
    rng = np.random.default_rng(13)
    lay = R.Layout(R.Code(*OTHER4), 1, 0, 0)
    pool = Pool(lay, gen_frames(rng, lay, 1200, p_bad=0.3))
    d = fec.RsDecoder(*OTHER4, nchan=2, max_block=16)
    wc = call(torch, d, pool, [np.arange(600), np.arange(600, 1200)], 600, in_counts=[600, 513])
    assert 150 < wc[0] < 600 and 150 < wc[1] < 513
    call(torch, d, pool, [np.arange(256), np.arange(300, 556)], 256)
    call(torch, d, pool, [np.arange(257), np.arange(300, 557)], 257, in_counts=[255, 257])


@pytest.mark.parametrize("params", R.ODD_CODES, ids=lambda p: "%x-%d-%d-%d" % p)
def test_codes_off_the_dword_grid(torch, params):
    """num_roots that are no multiple of the four syndromes of a dword, the smallest and the largest the kernel takes, first roots
    0 and 255 and gaps 2, 7 and 254 (tests/test_rs_cpu.py holds the definition to libcorrect's recorded answers for these codes).
    From five roots on: depths 1, 3 and 8 over pools of 24 frames, maps and an XOR sequence, per-row counts.  With 2 and 3 roots
    nearly every word beyond t is taken to another codeword, not refused: depth 1 and 1200 frames, nine in ten of them beyond t."""
    nr = params[3]
    rng = np.random.default_rng(7000 + nr)
    if nr < 5:
        lay = R.Layout(R.Code(*params), 1, 0, 0)
        pool = Pool(lay, gen_frames(rng, lay, 1200, p_bad=0.9))
        used = np.r_[0:600, 600:1113]
        assert (~pool.good[used]).sum() >= 4 and pool.good[used].sum() >= 500 and pool.errs.max() >= nr // 2
        d = fec.RsDecoder(*params, nchan=2, max_block=16)
        call(torch, d, pool, [np.arange(600), np.arange(600, 1200)], 600, in_counts=[600, 513])
        assert d.last_kernel()["block"] == 64
        return
    for depth, skip, full_out in ((1, 0, 0), (3, 5, 1), (8, 2, 0)):
        in_map, out_map = rng.permutation(256).astype(np.uint8), rng.permutation(256).astype(np.uint8)
        xor = rng.integers(0, 256, int(rng.integers(1, 255 * depth + 1))).astype(np.uint8)
        lay = R.Layout(R.Code(*params), depth, skip, full_out, in_map, out_map, xor)
        pool = Pool(lay, gen_frames(rng, lay, 24, p_bad=0.35))
        used = np.r_[0:8, 8:13, 16:23]
        assert pool.good[used].sum() >= 2 and (~pool.good[used]).sum() >= 2 and pool.errs.max() >= nr // 2
        d = fec.RsDecoder(*params, depth=depth, skip=skip, full_out=full_out, in_map=in_map, out_map=out_map, xor=xor, nchan=3, max_block=8)
        call(torch, d, pool, [np.arange(8), np.arange(8, 16), np.arange(16, 24)], 8, in_counts=[8, 5, 7], lead=depth, olead=depth + 2)
        assert d.last_kernel()["block"] == 64 * depth


def test_frames_of_all_zeros_and_all_ones(torch):
    lay = R.falcon_layout()
    frames = np.zeros((4, 1279), np.uint8)
    frames[1] = 0xFF
    frames[2, 4:] = 0xFF
    frames[3, 4::2] = 0xFF
    pool = Pool(lay, frames)
    assert pool.good[0] and (pool.errs[0] == 0).all()                # the zero word is a codeword: toDB[0] ^ randVals comes out
    d = fec.FalconRs(nchan=1, max_block=4)
    call(torch, d, pool, [np.arange(4)], 4)
    lay1 = R.Layout(R.Code(*CCSDS32), 1)
    p1 = Pool(lay1, np.stack([np.zeros(255, np.uint8), np.full(255, 0xFF, np.uint8)]))
    call(torch, fec.RsDecoder(*CCSDS32, max_block=2), p1, [np.arange(2)], 2)


# ---- 5. maps, chaining, entry forms, errors --------------------------------------------------------------------------------------------

def test_set_maps_acts_from_the_next_call(torch, falcon):
    rng = np.random.default_rng(14)
    d = fec.FalconRs(nchan=2, max_block=4)
    idx = [np.arange(4), np.arange(4, 8)]
    call(torch, d, falcon, idx, 4)
    lay = falcon.lay
    out_map, xor = rng.permutation(256).astype(np.uint8), rng.integers(0, 256, 100).astype(np.uint8)
    lay2 = R.Layout(lay.code, 5, 4, 1, lay.in_map, out_map, xor)
    p2 = Pool(lay2, falcon.frames[:8])
    d.set_maps(lay.in_map, out_map, xor)
    call(torch, d, p2, idx, 4)
    lay3 = R.Layout(lay.code, 5, 4, 1)
    p3 = Pool(lay3, lay.in_map[falcon.frames[:8]])                   # identity maps: the frames already in the decoder's domain
    d.set_maps()
    call(torch, d, p3, idx, 4)
    with pytest.raises(capi.QdspHipError):
        d.set_maps(xor=np.zeros(1276, np.uint8))


def test_deframer_feeds_the_decoder_on_one_stream(torch, falcon):
    """Deframer -> FalconRs through the deframer's device counts, no synchronisation in between, on a non-default stream: the
    good frames of the two definitions composed."""
    rng = np.random.default_rng(15)
    sync = np.unpackbits(np.array([0x1A, 0xCF, 0xFC, 0x1D], np.uint8))
    fl, nchan = 1279 * 8, 3
    rows, want = [], []
    for r in range(nchan):
        fr = falcon.frames[20 * r: 20 * r + 3 + r % 2].copy()
        fr[:, :4] = [0x1A, 0xCF, 0xFC, 0x1D]
        bits = [rng.integers(0, 2, int(rng.integers(0, 300))).astype(np.uint8)]
        for f in fr:
            bits.append(np.unpackbits(f))                          # back to back: the next sync word is where the deframer looks
        rows.append(np.concatenate(bits))
    n = max(len(b) for b in rows) + 64
    x = np.zeros((nchan, n), np.uint8)
    for r in range(nchan):
        x[r, :len(rows[r])] = rows[r]
        fdef, _, _ = D.deframe_ref(x[r], fl, sync, None)
        o, g, _ = falcon.lay.decode(fdef.reshape(-1, 1279)) if len(fdef) else (np.zeros((0, 1275), np.uint8), np.zeros(0, bool), None)
        want.append(o[g])
        assert len(fdef) >= 3
    df = ops.Deframer(fl, sync, 0, nchan=nchan, max_block=n)
    cap = df.out_size(n)
    rs = fec.FalconRs(nchan=nchan, max_block=cap)
    xd = dev(torch, x)
    s = torch.cuda.Stream()
    ob = torch.full((nchan, cap * 1275 + 9), SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        frames, counts = df.process_batch(xd)
        out, good = rs.process_batch(frames, ob, nframes=cap, in_counts=counts)
    s.synchronize()
    got, gc = ob.cpu().numpy(), good.cpu().numpy()
    assert gc.tolist() == [len(w) for w in want] and gc.sum() > 0
    for r in range(nchan):
        assert got[r, :want[r].size].tobytes() == want[r].tobytes() and (got[r, want[r].size:] == SENT).all(), r


def test_entry_forms_give_the_same_bytes(torch, falcon):
    """process (host), process_ex over the host / device link pairs, process_dev and process_batch."""
    idx = np.arange(40, 46)
    frames = falcon.frames[idx]
    want = falcon.out[idx][falcon.good[idx]]
    assert 0 < len(want) < 6
    d = fec.FalconRs(nchan=1, max_block=6)
    y = d.process(frames)
    assert y.shape == want.shape and y.tobytes() == want.tobytes()
    assert d.process(frames.ravel()[:0]).shape == (0, 1275)
    xd = dev(torch, frames.ravel())
    yd = d.process(xd)
    assert tuple(yd.shape) == want.shape and yd.cpu().numpy().tobytes() == want.tobytes()
    yb, cnt = d.process_batch(xd.reshape(1, -1))
    assert int(cnt.cpu()[0]) == len(want) and yb.cpu().numpy()[0, :want.size].tobytes() == want.tobytes()
    hin = np.ascontiguousarray(frames.ravel())
    for in_link, out_link in ((HOSTL, HOSTL), (HOSTL, DEVL), (DEVL, HOSTL), (DEVL, DEVL)):
        hout = np.full(6 * 1275, SENT, np.uint8)
        dout = torch.full((6 * 1275,), SENT, dtype=torch.uint8, device="cuda")
        src = hin.ctypes.data if in_link == HOSTL else xd.data_ptr()
        dst = hout.ctypes.data if out_link == HOSTL else dout.data_ptr()
        torch.cuda.synchronize()
        n = d.process_ex(src, in_link, 6, dst, out_link)
        torch.cuda.synchronize()
        res = hout if out_link == HOSTL else dout.cpu().numpy()
        assert n == len(want) and res[:want.size].tobytes() == want.tobytes(), (in_link, out_link)
        if out_link == DEVL:
            assert (res[want.size:] == SENT).all()
    assert d.process_ex(hin.ctypes.data, HOSTL, 0, 0, HOSTL) == 0


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST, "build/falcon_check"], stdout=subprocess.DEVNULL, timeout=300)
    return BIN


@pytest.fixture(scope="module")
def mirror_frames(golden):
    """The input of tests/test_rs_cpu.py's run of the harness on the fake library: the recording's ten frames, then twelve with a
    table of error counts per codeword; what the definition makes of them, computed once."""
    lay = R.falcon_layout()
    rng = np.random.default_rng(6)
    frames = lay.encode(rng.integers(0, 256, (12, 5, lay.code.k)).astype(np.uint8))
    for f in range(12):
        for c in range(5):
            ne = [0, 1, 8, 3, 9, 0, 12, 5, 8, 2, 0, 7][(f + 3 * c) % 12] if f % 4 else (f + c) % 9
            frames[f, 4 + rng.choice(255, ne, replace=False) * 5 + c] ^= rng.integers(1, 256, ne).astype(np.uint8)
    frames = np.concatenate([golden["frames"], frames])
    want, good, _ = lay.decode(frames)
    assert 5 <= good.sum() < len(frames)
    return frames, want[good]


@pytest.mark.parametrize("per", [1, 3, 22])
@pytest.mark.parametrize("link", ["dev", "host"])
def test_falcon_check_files_are_the_operator(torch, harness, mirror_frames, tmp_path, link, per):
    """source -> FalconRS -> sink of the C++ mirror on the real library, the blocks handed over in device memory or in the host
    buffers, `per` frames to a block: the file is FalconRs.process over the same blocks, and the definition's good frames."""
    frames, want = mirror_frames
    frames.tofile(tmp_path / "x.u8")
    p = subprocess.run([harness, link, "x.u8", "y.bin", str(per)], cwd=tmp_path, check=True, timeout=180, capture_output=True, text=True)
    assert "graph ok" in p.stdout and f"{link} link" in p.stdout, p.stdout
    in_dev = int(re.search(r"\((\d+) in device memory\)", p.stdout).group(1))
    assert (in_dev > 0) == (link == "dev"), p.stdout
    got = np.fromfile(tmp_path / "y.bin", dtype=np.uint8)
    d = fec.FalconRs(nchan=1, max_block=per)
    mine = np.concatenate([d.process(frames[a:a + per]) for a in range(0, len(frames), per)])
    assert got.tobytes() == mine.tobytes(), "the mirror's file is not the operator's frames"
    assert got.tobytes() == want.tobytes(), "the mirror's file is not the definition's good frames"


def test_error_codes(torch, falcon):
    L = capi.load()
    d = fec.FalconRs(nchan=2, max_block=2)
    h = d._h
    x = torch.zeros(2 * 3 * 1279 + 64, dtype=torch.uint8, device="cuda")
    y = torch.zeros(2 * 3 * 1275 + 64, dtype=torch.uint8, device="cuda")
    xp, yp = x.data_ptr(), y.data_ptr()
    f = L.qdsp_hip_rs_process_batch_dev
    assert f(h, xp, 2, 2 * 1279, None, yp, 2 * 1275, None, None, None) == 0
    assert f(h, xp, 2, 2 * 1279 - 1, None, yp, 2 * 1275, None, None, None) == EINVAL       # short strides
    assert f(h, xp, 2, 2 * 1279, None, yp, 2 * 1275 - 1, None, None, None) == EINVAL
    assert f(h, xp, -1, 2 * 1279, None, yp, 2 * 1275, None, None, None) == EINVAL
    assert f(h, xp, (1 << 22) + 1, 1 << 40, None, yp, 1 << 40, None, None, None) == EINVAL
    assert f(h, None, 2, 2 * 1279, None, yp, 2 * 1275, None, None, None) == EINVAL
    assert f(h, xp, 2, 2 * 1279, None, None, 2 * 1275, None, None, None) == EINVAL
    assert f(h, xp, 2, 2 * 1279, None, xp + 100, 2 * 1275, None, None, None) == EINVAL     # overlap
    assert f(h, xp, 2, 2 * 1279, None, xp, 2 * 1275, None, None, None) == EINVAL
    assert f(h, xp, 0, 0, None, yp, 0, None, None, None) == 0 and d.counts().tolist() == [0, 0]   # nframes 0 clears the counts
    assert f(h, None, 0, 0, None, None, 0, None, None, None) == 0
    assert L.qdsp_hip_rs_process_ex(h, xp, DEVL, 1, yp, DEVL) == EINVAL                   # nchan 2
    d1 = fec.FalconRs(nchan=1, max_block=2)
    hbuf = np.zeros(3 * 1279, np.uint8)
    obuf = np.zeros(3 * 1275, np.uint8)
    assert L.qdsp_hip_rs_process_ex(d1._h, hbuf.ctypes.data, HOSTL, 3, obuf.ctypes.data, HOSTL) == ESIZE
    assert L.qdsp_hip_rs_process_ex(d1._h, xp, DEVL, 3, obuf.ctypes.data, HOSTL) == ESIZE
    for link in (PIPE, DEFER):
        assert L.qdsp_hip_rs_process_ex(d1._h, xp, DEVL, 1, yp, link) == EINVAL
    assert L.qdsp_hip_rs_process_ex(d1._h, xp, DEVL, 3, yp, DEVL) >= 0                    # device sides: past max_block is served
    assert L.qdsp_hip_rs_process_ex(d1._h, xp, 7, 1, yp, DEVL) == EINVAL
    assert L.qdsp_hip_rs_process_ex(d1._h, None, DEVL, 1, yp, DEVL) == EINVAL
    d1.close()
    assert L.qdsp_hip_rs_frame_in_bytes(h) == 1279 and d1._h.value is None
    with pytest.raises(capi.QdspHipError):
        fec.RsDecoder(0x11b, 1, 1, 4)                                # x^8 + x^4 + x^3 + x + 1 is irreducible, not primitive
