"""ComplexAGC on the GPU (qdsp_hip_cagc_*, ops.ComplexAgc, dsp::ComplexAGC) against the exact recurrence of the reference's float
parameters (tests/test_cagc_cpu.py: cagc_exact, sequential in np.longdouble).  For every output component and for the gain:
    |y - x g_truth| <= 0.5 ulp32(x g_truth) + |x| 2^-40 M_i,    |g - g_truth| <= 2^-40 M_i,    M_i = max(1, g_0 .. g_i) of the truth.
A reassociated FP64 scan cannot repeat the float loop of the reference bit for bit, so the reference enters as
|y - y_ref| <= |y_ref - truth| + bound and, for rows of at least 4096 samples, max |y - truth| <= max |y_ref - truth|.  Rows out of
the scan's domain are the float loop's bit for bit (cagc_ref)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from qdsp_amd import capi, ops
from test_cagc_cpu import (LD, MAX_PARTS, PARAMS, ROW_TILES, SIZES, TILE, _same_bits, cagc_exact, cagc_ref, case_list, case_table,
                           check_against_truth, check_gain, column, in_domain, limit_to_domain, make_input)

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "demod_check")
ROW, SCAN = "cagc_row_kernel", "cagc_scan_kernel"
ROW_N, SCAN_N = 3 * TILE + 5, (ROW_TILES + 1) * TILE + 5          # a size of each form, ragged


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def form_of(n):
    return ROW if -(-n // TILE) <= ROW_TILES else SCAN


def rows(torch, x, pad=0):
    """Columns of the numpy array x as the rows of a device tensor, `pad` samples of zeros behind each."""
    t = torch.zeros((x.shape[1], x.shape[0] + pad), dtype=torch.complex64, device="cuda")
    t[:, :x.shape[0]] = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    return t


def gains(d):
    return np.asarray([d.get_gain(c) for c in range(d.nchan)])


# ---- 1. accuracy against the exact recurrence ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_accuracy_against_the_exact_recurrence(torch, n):
    x, par, ref, gref, exact = case_table(n)
    ncol = x.shape[1]
    d = ops.ComplexAgc(par[0], par[1], par[2], nchan=ncol)
    y = d.process_batch(rows(torch, x)).cpu().numpy().T
    assert d.last_kernel()["name"] == form_of(n)
    g = gains(d)
    for k, (p, kind) in enumerate(case_list()):
        label = f"n={n} {p} {kind}"
        ex = column(exact, k)
        ratio, e_gpu, e_ref = check_against_truth(y[:, k], x[:, k], ex, ref[:, k], label)
        check_gain(g[k], ex, label)
        if n >= 4096:
            assert e_gpu <= e_ref, label
    # the host entry point and the one-row device entry point run the same launch
    for k in (0, ncol - 1):
        one = ops.ComplexAgc(*par[:, k], max_block=n)
        assert _same_bits(one.process(x[:, k].copy()), y[:, k]) and one.last_kernel()["name"] == form_of(n)
        one.reset()
        assert _same_bits(one.process(torch.from_numpy(x[:, k].copy()).cuda()).cpu().numpy(), y[:, k])
        assert one.get_gain() == g[k]


# ---- 2. call cuts and state ------------------------------------------------------------------------------------------------------------
def cuts_of(n, sizes=(1, 7, 4096, 65_537)):
    c = [0]
    for s in sizes:
        c.append(min(n, c[-1] + s))
    return c + [n]


def test_call_cuts_and_state(torch):
    n = 400_001
    par = PARAMS["ref_defaults"]
    x = make_input("gauss", n, seed=3)
    assert in_domain(x, par[2])
    exact = cagc_exact(x, *par)
    xt = torch.from_numpy(x).cuda()
    cuts = cuts_of(n)
    for path in ("host", "device"):
        one = ops.ComplexAgc(*par, max_block=n)
        y1 = one.process(x) if path == "host" else one.process(xt).cpu().numpy()
        check_against_truth(y1, x, exact, None, f"{path} one call")
        check_gain(one.get_gain(), exact, f"{path} one call")
        d = ops.ComplexAgc(*par, max_block=n)
        g = LD(1)
        for a, b in zip(cuts, cuts[1:]):
            y = d.process(x[a:b]) if path == "host" else d.process(xt[a:b]).cpu().numpy()
            ex = cagc_exact(x[a:b], *par, gain=g) if b - a < 100_000 else None
            if ex is None:      # the long piece: the one-call truth from the cut on (the same recurrence from the same gain)
                assert g == exact[2][a]
                Mp = np.maximum.accumulate(np.maximum(exact[2][a:], 1))
                ex = (exact[0][a:], exact[1][a:], exact[2][a:], Mp, exact[4])
            check_against_truth(y, x[a:b], ex, None, f"{path} [{a}, {b})")
            check_gain(d.get_gain(), ex, f"{path} [{a}, {b})")
            g = ex[4]
    # set_gain + process == a fresh handle with that gain
    a_, b_ = ops.ComplexAgc(*par), ops.ComplexAgc(*par)
    a_.process(xt[:5000])
    a_.set_gain(0.375)
    b_.set_gain(0.375)
    assert a_.get_gain() == 0.375
    ya = a_.process(xt[5000:90_000]).cpu().numpy()
    assert _same_bits(ya, b_.process(xt[5000:90_000]).cpu().numpy()) and a_.get_gain() == b_.get_gain()
    check_against_truth(ya[:3000], x[5000:8000], cagc_exact(x[5000:8000], *par, gain=0.375), None, "from a set gain")
    # count 0 keeps the state, reset gives 1
    assert len(b_.process(np.zeros(0, np.complex64))) == 0 and b_.get_gain() == a_.get_gain()
    b_.reset()
    assert b_.get_gain() == 1.0
    assert _same_bits(b_.process(xt[:3000]).cpu().numpy(), ops.ComplexAgc(*par).process(xt[:3000]).cpu().numpy())
    # a set between calls acts from the next call
    p2 = PARAMS["tight_clamp"]
    s = ops.ComplexAgc(*par)
    y1 = s.process(xt[:3000]).cpu().numpy()
    ex1 = cagc_exact(x[:3000], *par)
    check_against_truth(y1, x[:3000], ex1, None, "before set")
    s.set(*p2)
    y2 = s.process(xt[3000:9000]).cpu().numpy()
    ex2 = cagc_exact(x[3000:9000], *p2, gain=ex1[4])
    check_against_truth(y2, x[3000:9000], ex2, None, "after set")
    check_gain(s.get_gain(), ex2, "after set")


# ---- 3. batch on the real producer ---------------------------------------------------------------------------------------------------
def test_batch_on_channelizer_output(torch):
    nchan, M = 64, 64
    taps = O.lowpass_taps_f64(256, 1.0 / 64.0)
    incs = [ops.phase_delta(1.0, -(c - 31.5) / 64.0) for c in range(nchan)]
    chn = ops.Channelizer(taps, 1, M, incs, max_block=0)
    sps = np.asarray([0.25 * (1 + c % 4) for c in range(nchan)], F32)
    mgs = np.asarray([(3.0, 50.0, 65535.0)[c % 3] for c in range(nchan)], F32)
    rts = np.asarray([1e-3 * (1 + c % 5) for c in range(nchan)], F32)
    for pad in (37, 0):                     # rows padded by an odd number of samples: the scalar path; unpadded: the vector path
        ag = ops.ComplexAgc(sps, mgs, rts, nchan=nchan)
        singles = [ops.ComplexAgc(sps[c], mgs[c], rts[c]) for c in (0, 17, 63)]
        g = np.ones(nchan, LD)
        for call, n in enumerate((64 * 4096, 64 * 40_000)):
            xin = ops.synth_iq(n, first_sample=call * 10**7, seed=5)
            no = chn.out_size(n)
            cbuf = torch.zeros((nchan, no + pad), dtype=torch.complex64, device="cuda")
            yc = chn.process(xin)
            cbuf[:, :no] = yc
            obuf = torch.zeros_like(cbuf)
            y = ag.process_batch(cbuf, obuf, count=no)
            assert ag.last_kernel()["name"] == form_of(no)
            assert (cbuf.stride(0) % 2 == 1) == bool(pad)
            xh, yh = cbuf[:, :no].cpu().numpy(), y.cpu().numpy()
            if pad:
                assert float(obuf[:, no:].abs().max()) == 0, "the padding is not written"
            for c in range(nchan):
                assert in_domain(xh[c], rts[c]), c
            ex = cagc_exact(xh.T, sps, mgs, rts, gain=g)
            check_against_truth(yh.T, xh.T, ex, None, f"pad {pad} call {call}")
            check_gain(gains(ag), ex, f"pad {pad} call {call}")
            g = ex[4]
            for s, c in zip(singles, (0, 17, 63)):      # same tiling, same order: the same bits
                assert _same_bits(s.process(cbuf[c, :no].contiguous()).cpu().numpy(), yh[c]), (pad, call, c)
                assert s.get_gain() == ag.get_gain(c)


# ---- 4. rows out of the scan's domain ---------------------------------------------------------------------------------------------------
KINDS = ("nan", "inf", "rate_x_above_1", "negative_gain", "negative_set_point")


@pytest.mark.parametrize("n", [ROW_N, SCAN_N])
@pytest.mark.parametrize("kind", KINDS)
def test_out_of_domain_rows_take_the_reference_loop(torch, n, kind):
    par = np.asarray(PARAMS["ref_defaults"], F32)
    x = np.stack([make_input("gauss", n, seed=20 + r) for r in range(4)], axis=1)
    g0 = np.asarray([1.0, 0.5, 2.0, 1.25])
    bad_value = {"nan": np.nan, "inf": complex(0, -np.inf), "rate_x_above_1": 5000.0}.get(kind)
    places = sorted({5, (n // TILE // 2) * TILE + 777, n - 3}) if bad_value is not None else [0]
    assert in_domain(x, par[2])
    clean = ops.ComplexAgc(*par, nchan=4)
    for c in range(4):
        clean.set_gain(g0[c], c)
    y_clean = clean.process_batch(rows(torch, x)).cpu().numpy().T
    ex = cagc_exact(x, *par, gain=g0)
    check_against_truth(y_clean, x, ex, None, f"n={n} clean")
    # the offending rows of all places, one reference loop over them as columns
    bad_rows = [(i + 1) % 4 for i in range(len(places))]
    xb_cols, pb, gb = [], [], []
    for place, r in zip(places, bad_rows):
        col = x[:, r].copy()
        p, g = par.copy(), g0[r]
        if bad_value is not None:
            col[place] = bad_value
        elif kind == "negative_gain":
            g = -0.75
        else:
            p[0] = -0.5
        xb_cols.append(col)
        pb.append(p)
        gb.append(g)
    pb = np.asarray(pb, F32).T
    want, g_want = cagc_ref(np.stack(xb_cols, axis=1), pb[0], pb[1], pb[2], gain=np.asarray(gb, F32))
    for i, (place, r) in enumerate(zip(places, bad_rows)):
        xb = x.copy()
        xb[:, r] = xb_cols[i]
        for in_place in (False, True):
            d = ops.ComplexAgc(*par, nchan=4)
            d.set(*pb[:, i], chan=r)
            for c in range(4):
                d.set_gain(gb[i] if c == r else g0[c], c)
            buf = rows(torch, xb, pad=3)
            y = d.process_batch(buf, buf if in_place else None, count=n).cpu().numpy().T
            label = f"n={n} {kind} at {place} row {r} in_place={in_place}"
            assert d.last_kernel()["name"] == form_of(n), label
            assert _same_bits(y[:, r], want[:, i]), label
            gr = d.get_gain(r)                  # the loop's float gain, widened
            assert _same_bits([gr], [g_want[i]]) and (np.isnan(gr) or float(F32(gr)) == gr), label
            others = [c for c in range(4) if c != r]
            assert _same_bits(y[:, others], y_clean[:, others]), label
            assert all(d.get_gain(c) == clean.get_gain(c) for c in others), label
            if in_place:
                assert float(buf[:, n:].abs().max()) == 0, label
    # after a NaN gain the next call stays NaN, as in the reference, until set_gain or reset
    if kind == "nan":
        assert np.isnan(d.get_gain(r))
        x2 = make_input("gauss", 3000, seed=40)
        x4 = np.stack([x2] * 4, axis=1)
        g_before = gains(d)
        y = d.process_batch(rows(torch, x4)).cpu().numpy().T
        assert np.all(np.isnan(y[:, r].view(F32))) and np.isnan(d.get_gain(r))
        o = others[0]
        check_against_truth(y[:, o], x2, cagc_exact(x2, *par, gain=LD(g_before[o])), None, "beside the NaN row")
        d.set_gain(1.0, r)
        y = d.process_batch(rows(torch, x4)).cpu().numpy().T
        check_against_truth(y[:, r], x2, cagc_exact(x2, *par), None, "after set_gain")
        d.set_gain(float("nan"), r)
        d.reset()
        assert np.all(gains(d) == 1.0)
        check_against_truth(d.process_batch(rows(torch, x4)).cpu().numpy().T[:, r], x2, cagc_exact(x2, *par), None, "after reset")


# ---- 5. in place, 6. determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [TILE * ROW_TILES - 4, TILE * ROW_TILES + 4])
@pytest.mark.parametrize("pad", [2, 3])                 # even row stride: vector path; odd: scalar
def test_in_place_equals_out_of_place(torch, n, pad):
    par = PARAMS["tight_clamp"]
    nchan = 4
    x = torch.randn((nchan, n + pad), dtype=torch.complex64, device="cuda") * 0.7
    a, b = ops.ComplexAgc(*par, nchan=nchan), ops.ComplexAgc(*par, nchan=nchan)
    want = a.process_batch(x, count=n)
    assert a.last_kernel()["name"] == form_of(n)
    buf = x.clone()
    got = b.process_batch(buf, buf, count=n)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(torch.view_as_real(got).view(torch.int32), torch.view_as_real(want).view(torch.int32))
    assert torch.equal(torch.view_as_real(buf[:, n:]), torch.view_as_real(x[:, n:]))
    assert np.array_equal(gains(a), gains(b))
    # the same buffer with another stride is not "in place"
    L = capi.load()
    assert L.qdsp_hip_cagc_process_batch_dev(b._h, buf.data_ptr(), 100, n + pad, buf.data_ptr(), n + pad + 2, None) == EINVAL


def test_same_call_twice_gives_the_same_bits(torch):
    nchan, n = 64, 100_003
    x = torch.randn((nchan, n), dtype=torch.complex64, device="cuda") * 0.7
    d = ops.ComplexAgc(*PARAMS["tight_clamp"], nchan=nchan)
    d.set_gain(0.125)
    y1 = d.process_batch(x).clone()
    g1 = gains(d)
    assert d.last_kernel()["name"] == SCAN
    d.set_gain(0.125)
    y2 = d.process_batch(x)
    assert torch.equal(torch.view_as_real(y1).view(torch.int32), torch.view_as_real(y2).view(torch.int32)) and np.array_equal(g1, gains(d))


# ---- 7. argument errors, harness helpers ---------------------------------------------------------------------------------------------
def test_argument_errors(torch):
    L = capi.load()
    h = C.c_void_p()
    for nchan, mb in ((0, 10), (70_000, 10), (1, -5)):
        assert L.qdsp_hip_cagc_create(C.byref(h), 0, nchan, mb) == EINVAL
    two = ops.ComplexAgc(nchan=2, max_block=100)
    one = ops.ComplexAgc(max_block=100)
    x = np.zeros(101, np.complex64)
    y = np.zeros(101, np.complex64)
    assert L.qdsp_hip_cagc_process(one._h, x.ctypes.data, 101, y.ctypes.data) == ESIZE
    assert L.qdsp_hip_cagc_process(one._h, x.ctypes.data, -1, y.ctypes.data) == EINVAL
    assert L.qdsp_hip_cagc_process(two._h, x.ctypes.data, 10, y.ctypes.data) == EINVAL            # host path: one channel
    assert L.qdsp_hip_cagc_process_ex(one._h, x.ctypes.data, 7, 10, y.ctypes.data, 0) == EINVAL
    assert L.qdsp_hip_cagc_process_ex(one._h, x.ctypes.data, 0, 10, y.ctypes.data, 3) == EINVAL    # deferred without an event
    nan = float("nan")
    for p in ((nan, 1.0, 1e-3), (1.0, nan, 1e-3), (1.0, 1.0, nan)):
        assert L.qdsp_hip_cagc_set(one._h, 0, *p) == EINVAL, p
    assert L.qdsp_hip_cagc_set(two._h, 2, 1.0, 1.0, 1e-3) == EINVAL
    assert L.qdsp_hip_cagc_set(two._h, -1, -1.0, float("inf"), 0.5) == 0        # odd, not NaN: the reference takes them too
    g = C.c_double()
    assert L.qdsp_hip_cagc_get_gain(two._h, 2, C.byref(g)) == EINVAL
    assert L.qdsp_hip_cagc_get_gain(two._h, 0, None) == EINVAL
    assert L.qdsp_hip_cagc_get_gain(two._h, 1, C.byref(g)) == 0 and g.value == 1.0
    assert L.qdsp_hip_cagc_set_gain(two._h, 5, 1.0) == EINVAL
    xt = torch.zeros(1000, dtype=torch.complex64, device="cuda")
    yt = torch.zeros(1000, dtype=torch.complex64, device="cuda")
    bd = L.qdsp_hip_cagc_process_batch_dev
    assert bd(two._h, xt.data_ptr(), 400, 399, yt.data_ptr(), 400, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 400, 400, yt.data_ptr(), 300, None) == EINVAL
    assert bd(two._h, xt.data_ptr() + 4, 10, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 10, 10, yt.data_ptr() + 4, 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), -1, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, None, 10, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr() + 8, 10, 11, yt.data_ptr() + 8, 11, None) == 0               # 8-byte aligned rows are enough
    # handle kinds do not mix
    fm = ops.FmDemod(250e3, 75e3)
    agc = ops.Agc(20.0, 48e3)
    de = ops.Deemp(48e3, 50e-6)
    for other in (fm, agc, de):
        assert L.qdsp_hip_cagc_process_dev(other._h, xt.data_ptr(), 10, yt.data_ptr(), None) == EINVAL
        assert L.qdsp_hip_cagc_reset(other._h) == EINVAL and L.qdsp_hip_cagc_set_gain(other._h, 0, 1.0) == EINVAL
    assert L.qdsp_hip_demod_process_dev(one._h, xt.data_ptr(), 10, yt.data_ptr(), None) == EINVAL
    assert L.qdsp_hip_agc_process_dev(one._h, xt.data_ptr(), 10, yt.data_ptr(), None) == EINVAL
    assert L.qdsp_hip_deemp_reset(one._h) == EINVAL
    torch.cuda.synchronize()


def test_done_event_and_time(torch):
    L = capi.load()
    ev = C.c_void_p()
    capi.check(L.qdsp_hip_event_create(0, C.byref(ev)))
    d = ops.ComplexAgc()
    x = torch.randn(1 << 20, dtype=torch.complex64, device="cuda") * 0.7
    assert L.qdsp_hip_set_done_event(d._h, ev) == 0
    assert d.time_dev(x, torch.empty_like(x), 3) > 0
    assert d.last_kernel()["name"] == SCAN and d.last_kernel()["grid"] == 512
    capi.check(L.qdsp_hip_event_destroy(ev))


# ---- 8. more than one tile per chunk -----------------------------------------------------------------------------------------------------
def test_more_than_one_tile_per_chunk(torch):
    n = (MAX_PARTS + 3) * TILE + 77                     # just past kAmMaxParts tiles: two tiles per chunk
    sp, mg, rt = PARAMS["fast_x4"]                      # rate 0.125 on samples of about 2: the loop forgets within a few hundred
    x = limit_to_domain(make_input("gauss", n, seed=8) * F32(4), rt)
    assert in_domain(x, rt)
    d = ops.ComplexAgc(sp, mg, rt)
    y = d.process(torch.from_numpy(x).cuda()).cpu().numpy()
    k = d.last_kernel()
    assert k["name"] == SCAN and -(-n // TILE) > MAX_PARTS and k["grid"] < -(-n // TILE)
    a = 1.0 - float(F32(rt)) * np.abs(x.astype(np.complex128))
    lg = np.log2(np.maximum(a, 1e-300))
    extra = LD(2.0) ** -60 * LD(mg)
    for w0 in (0, (MAX_PARTS // 2) * 2 * TILE - 3000, n - 6000):
        w1 = min(n, w0 + 6000)
        s = w0
        if w0:                          # the run-in: back from the window until the product of the a_i is below 2^-60
            back = np.cumsum(lg[w0 - 1::-1][:20_000])
            s = w0 - 1 - int(np.argmax(back < -60))
            assert np.sum(lg[s:w0]) < -60
        # started from any gain in [0, max] a run-in before the window, the truth is within 2^-60 max of the row's own there
        ex = cagc_exact(x[s:w1], sp, mg, rt, 1.0 if s == 0 else 2.0)
        win = tuple(t[w0 - s:] for t in ex[:4]) + (ex[4],)
        check_against_truth(y[w0:w1], x[w0:w1], win, None, f"window at {w0}", extra=extra if s else 0)
        if w1 == n:
            check_gain(d.get_gain(), win, "the carried gain", extra=extra)


# ---- 9. the block graph ------------------------------------------------------------------------------------------------------------------
N, BLOCK, DECIM = 240_000, 24_000, 10
VFO_ARGS = ["300000", "2400000", "240000", "200000"]    # offset, inSR, outSR, bandwidth: 2.4 Msps -> 240 ksps


@pytest.fixture(scope="module")
def graph(tmp_path_factory):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL, timeout=300)
    d = tmp_path_factory.mktemp("cagcgraph")
    O.synth_iq(0, N, seed=42).tofile(d / "x.cf32")
    subprocess.run([BIN, "vfo", str(d / "x.cf32"), str(d / "v.cf32"), str(BLOCK)] + VFO_ARGS, check=True, timeout=180,
                   capture_output=True, text=True)
    v = np.fromfile(d / "v.cf32", dtype=np.complex64)
    assert len(v) == N // DECIM
    return d, v


@pytest.mark.parametrize("link", ["dev", "host"])
def test_vfo_then_complex_agc_blocks(graph, link):
    d, v = graph
    par = (1.0, 65535.0, 0.02)
    assert in_domain(v, par[2])
    out = d / f"cagc_{link}.cf32"
    r = subprocess.run([BIN, "cagc", link, str(d / "x.cf32"), str(out), str(BLOCK)] + VFO_ARGS + [repr(p) for p in par],
                       check=True, timeout=180, capture_output=True, text=True)
    assert "graph ok" in r.stdout and f"{link if link == 'host' else 'device'} link" in r.stdout
    y = np.fromfile(out, dtype=np.complex64)
    assert len(y) == len(v)
    vb = BLOCK // DECIM
    ag = ops.ComplexAgc(*par, max_block=vb)
    g = LD(1)
    for a in range(0, len(v), vb):          # one run() per VFO output block
        assert _same_bits(y[a:a + vb], ag.process(v[a:a + vb])), a
        ex = cagc_exact(v[a:a + vb], *par, gain=g)
        check_against_truth(y[a:a + vb], v[a:a + vb], ex, None, f"{link} block at {a}")
        g = ex[4]
    check_gain(ag.get_gain(), ex, f"{link} last block")
