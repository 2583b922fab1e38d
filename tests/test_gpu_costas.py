"""CostasLoop on the GPU (qdsp_hip_costas_*, ops.CostasLoop, dsp::CostasLoop<ORDER>).

Accuracy: against costas_truth (tests/test_costas_cpu.py: the recurrence in np.longdouble with exact decisions), for every case of
case_table(): e_gpu = max |y - truth| over both components <= 4 e_ref, e_ref the same maximum for costas_ref, the reference's float
loop, computed here; the carried frequency and phase within 4 x that loop's own deviation.  (Two float loops that differ in the last
bit of the cosine stand up to 1.8 x apart; a loop whose cosine carries 2^-21 of error stands 4.3 to 4.6 x off.)
Bit-identity: outputs and state do not depend on how a stream is cut into calls, on the entry point, on the row's place in the batch,
on the row layout, or on in-place use."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from qdsp_amd import capi, ops
from test_costas_cpu import LD, ROWS, WRAP32, _same_bits, case_table, chunks_of, costas_gains, costas_truth, deviation

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "demod_check")
SENT = 0x4B1DF00D                      # a finite float (1.0350605e7) no output of these inputs has
LAYOUTS = ("aligned", "in_stride_odd", "base_offset", "out_stride_odd")
FIRST = {2: 0.0, 4: np.pi / 4, 8: np.pi / 8}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def signal(nchan, n, order, seed):
    """`nchan` rows of PSK symbols of the order with a carrier offset per row and noise: loops that lock, slip and wrap."""
    rng = np.random.default_rng(seed)
    sym = np.exp(1j * (FIRST[order] + 2 * np.pi * rng.integers(0, order, (nchan, n)) / order))
    off = 0.02 * (np.arange(nchan) % 7 - 3)[:, None]
    noise = 0.1 * (rng.standard_normal((nchan, n)) + 1j * rng.standard_normal((nchan, n)))
    return (sym * np.exp(1j * (off * np.arange(n) + 0.3)) + noise).astype(np.complex64)


def bws(nchan):
    return np.asarray([0.002 * (1 + r % 5) for r in range(nchan)], F32)


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def states(d):
    return np.asarray([d.get_state(c) for c in range(d.nchan)])


def same_state(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


class Single:
    """One one-row handle per order, reset before every use: what a row gives alone."""

    def __init__(self):
        self.h = {}

    def __call__(self, torch, order, bw, row, state=(0.0, 0.0)):
        d = self.h.setdefault(order, ops.CostasLoop(order, 0.004, max_block=0))
        d.set_bandwidth(float(bw))
        d.set_state(*state)
        y = d.process(dev(torch, row)).cpu().numpy()
        return y, d.get_state()


@pytest.fixture(scope="module")
def single():
    return Single()


# ---- 1. accuracy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4, 8])
def test_accuracy_against_the_truth(torch, order):
    t = case_table()
    cols = [k for k, o in enumerate(t["order"]) if o == order]
    d = ops.CostasLoop(order, t["bw"][cols], nchan=len(cols), max_block=0)
    assert all(_same_bits(d.gains(i), [t["alpha"][k], t["beta"][k]]) for i, k in enumerate(cols))
    y = d.process_batch(dev(torch, t["x"][:, cols].T)).cpu().numpy().T
    assert d.last_kernel()["name"] == "costas_kernel" and d.last_kernel()["grid"] == 1
    st = states(d)
    tr = t["truth"]
    for i, k in enumerate(cols):
        name = t["names"][k]
        e_gpu, e_ref = deviation(y[:, i], tr, k), t["e_ref"][k]
        df, dp = abs(LD(st[i, 0]) - tr["freq"][k]), abs(LD(st[i, 1]) - tr["phase"][k])
        rf, rp = abs(LD(t["fref"][k]) - tr["freq"][k]), abs(LD(t["pref"][k]) - tr["phase"][k])
        print(f"{name}: e_gpu {e_gpu:.3g} e_ref {e_ref:.3g} ratio {e_gpu / e_ref:.3f}; freq {float(df):.3g} (ref {float(rf):.3g}) "
              f"phase {float(dp):.3g} (ref {float(rp):.3g})")
        assert e_gpu <= 4 * e_ref, name
        assert df <= 4 * rf and dp <= 4 * rp, name


# ---- 2. call cuts and entry points ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,nchan", [(2, 1), (4, 1), (8, 1), (4, 64), (8, 17)])
def test_cuts_and_entry_points_give_the_same_bits(torch, order, nchan):
    sizes = [s for c in chunks_of(nchan) for s in (1, 7, c - 1, c + 1)]         # (1, 7, chunk - 1, chunk + 1, rest) for every round length
    n = sum(sizes) + 2 * chunks_of(nchan)[-1] + 11
    cuts = [0] + list(np.cumsum(sizes)) + [n]
    x = signal(nchan, n, order, seed=order + nchan)
    xt = dev(torch, x)
    one = ops.CostasLoop(order, bws(nchan), nchan=nchan, max_block=n)
    y0 = one.process_batch(xt).cpu().numpy()
    s0 = states(one)
    d = ops.CostasLoop(order, bws(nchan), nchan=nchan, max_block=n)
    parts = [d.process_batch(xt[:, a:b]).cpu().numpy() for a, b in zip(cuts, cuts[1:])]      # rows n apart, counts b - a
    assert _same_bits(np.concatenate(parts, axis=1), y0) and same_state(states(d), s0)
    if nchan == 1:
        for path in ("host", "device"):
            e = ops.CostasLoop(order, bws(1), max_block=n)
            parts = [e.process(x[0, a:b]) if path == "host" else e.process(xt[0, a:b]).cpu().numpy() for a, b in zip(cuts, cuts[1:])]
            assert _same_bits(np.concatenate(parts), y0[0]) and same_state(states(e), s0), path
            e.reset()
            whole = e.process(x[0]) if path == "host" else e.process(xt[0]).cpu().numpy()
            assert _same_bits(whole, y0[0]) and same_state(states(e), s0), path


# ---- 3. row counts and sample counts; a row of a batch against the same row alone ---------------------------------------------
@pytest.mark.parametrize("nchan", [1, 15, 16, 17, 63, 64, 65, 130])
def test_rows_of_a_batch_equal_the_rows_alone(torch, single, nchan):
    order = {1: 2, 15: 4, 16: 8, 17: 2, 63: 4, 64: 8, 65: 4, 130: 2}[nchan]
    last = nchan % ROWS or ROWS
    chunks = chunks_of(nchan)
    counts = sorted({1} | {c + k for c in chunks for k in (-1, 0, 1)} | {2 * c + 5 for c in chunks})
    bw = bws(nchan)
    x = signal(nchan, counts[-1], order, seed=100 + nchan)
    picks = sorted({0, min(nchan, ROWS) - 1, nchan - last, nchan - 1})
    for n in counts:
        d = ops.CostasLoop(order, bw, nchan=nchan, max_block=0)
        y = d.process_batch(dev(torch, x[:, :n])).cpu().numpy()
        assert d.last_kernel() == {"name": "costas_kernel", "grid": -(-nchan // ROWS), "block": 64, "lds_bytes": (64 * 64 + ROWS) * 8}
        for r in picks:
            want, st = single(torch, order, bw[r], x[r, :n])
            assert _same_bits(y[r], want) and same_state(d.get_state(r), st), (n, r)


# ---- 4. row layouts, sentinels, in place ------------------------------------------------------------------------------------------
def geometry(layout, width):
    """(in_stride, out_stride, in_offset, out_offset) in samples.  Each layout but the first breaks one condition of 16-byte row
    accesses (even strides, 16-byte bases) and stays 8-byte aligned."""
    w = (width + 1) // 2 * 2 + 2
    ins, outs, io, oo = w, w, 0, 0
    if layout == "in_stride_odd":
        ins += 1
    elif layout == "base_offset":
        io, oo = 1, 1
    elif layout == "out_stride_odd":
        outs += 1
    else:
        assert layout == "aligned"
    return ins, outs, io, oo


@pytest.mark.parametrize("nchan", [5, 17])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_row_layouts_and_in_place(torch, layout, nchan):
    order = 4
    n = 2 * chunks_of(nchan)[-1] + 5
    x = signal(nchan, n, order, seed=7)
    base = ops.CostasLoop(order, bws(nchan), nchan=nchan, max_block=0)
    want = base.process_batch(dev(torch, x)).cpu().numpy()
    ins, outs, io, oo = geometry(layout, n)
    L = capi.load()
    stream = torch.cuda.current_stream().cuda_stream
    xb = torch.zeros(io + nchan * ins + 8, dtype=torch.complex64, device="cuda")
    xb[io:io + nchan * ins].view(nchan, ins)[:, :n] = dev(torch, x)
    yb = torch.full(((oo + nchan * outs + 64) * 2,), SENT, dtype=torch.int32, device="cuda")
    assert xb.data_ptr() % 16 == 0 and yb.data_ptr() % 16 == 0
    d = ops.CostasLoop(order, bws(nchan), nchan=nchan, max_block=0)
    assert L.qdsp_hip_costas_process_batch_dev(d._h, xb.data_ptr() + 8 * io, n, ins, yb.data_ptr() + 8 * oo, outs, stream) == 0
    h = yb.cpu().numpy()
    lo, hi = 2 * oo, 2 * (oo + nchan * outs)
    body = h[lo:hi].reshape(nchan, outs, 2)
    assert np.all(h[:lo] == SENT) and np.all(h[hi:] == SENT) and np.all(body[:, n:] == SENT), "wrote outside the rows"
    assert _same_bits(body[:, :n].copy().view(F32).reshape(nchan, 2 * n), want.view(F32)) and same_state(states(d), states(base))
    # in place: the same rows as input and output; what lies between count and the stride stays
    if ins == outs:
        zb = torch.full(((io + nchan * ins + 8) * 2,), SENT, dtype=torch.int32, device="cuda")
        zc = torch.view_as_complex(zb.view(torch.float32).view(-1, 2))
        zc[io:io + nchan * ins].view(nchan, ins)[:, :n] = dev(torch, x)
        e = ops.CostasLoop(order, bws(nchan), nchan=nchan, max_block=0)
        p = zb.data_ptr() + 8 * io
        assert L.qdsp_hip_costas_process_batch_dev(e._h, p, n, ins, p, ins, stream) == 0
        h = zb.cpu().numpy()
        body = h[2 * io:2 * (io + nchan * ins)].reshape(nchan, ins, 2)
        assert np.all(h[:2 * io] == SENT) and np.all(h[2 * (io + nchan * ins):] == SENT) and np.all(body[:, n:] == SENT)
        assert _same_bits(body[:, :n].copy().view(F32).reshape(nchan, 2 * n), want.view(F32)) and same_state(states(e), states(base))
        assert L.qdsp_hip_costas_process_batch_dev(e._h, p, 10, ins, p, ins + 2, stream) == EINVAL


# ---- 5. state -----------------------------------------------------------------------------------------------------------------------
def test_state_reset_and_bandwidth(torch, single):
    order, n = 8, 700
    x = signal(2, 3 * n, order, seed=9)
    xt = dev(torch, x)
    a = ops.CostasLoop(order, 0.004, nchan=2, max_block=0)
    assert same_state(states(a), np.zeros((2, 2)))
    a.process_batch(xt[:, :n])
    a.set_state(0.0125, -1.5)
    a.set_state(-0.25, 6.0, chan=1)
    assert same_state(states(a), [(0.0125, -1.5), (-0.25, 6.0)])
    ya = a.process_batch(xt[:, n:2 * n]).cpu().numpy()
    for r, st in enumerate([(0.0125, -1.5), (-0.25, 6.0)]):
        want, s1 = single(torch, order, 0.004, x[r, n:2 * n], st)      # a fresh handle given that state
        assert _same_bits(ya[r], want) and same_state(a.get_state(r), s1)
    # the state follows the truth from there
    al, be = costas_gains(0.004)
    tr = costas_truth(x[0, n:2 * n], order, al, be, LD(0.0125), LD(-1.5))
    assert deviation(ya[0], tr) < 1e-6 and abs(a.get_state(0)[1] - float(tr["phase"][0])) < 1e-9
    # count 0 keeps the state; a bandwidth set between calls acts from the next call
    before = states(a)
    assert a.process_batch(xt[:, :0]).shape == (2, 0) and same_state(states(a), before)
    a.set_bandwidth(0.05, chan=1)
    yb = a.process_batch(xt[:, 2 * n:]).cpu().numpy()
    w0, _ = single(torch, order, 0.004, x[0, 2 * n:], tuple(before[0]))
    w1, _ = single(torch, order, 0.05, x[1, 2 * n:], tuple(before[1]))
    w1_old, _ = single(torch, order, 0.004, x[1, 2 * n:], tuple(before[1]))
    assert _same_bits(yb[0], w0) and _same_bits(yb[1], w1) and not _same_bits(w1, w1_old)
    a.reset()
    assert same_state(states(a), np.zeros((2, 2)))
    assert _same_bits(a.process_batch(xt[:, :n]).cpu().numpy()[0], single(torch, order, 0.004, x[0, :n])[0])


# ---- 6. non-finite samples ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4, 8])
def test_nan_and_inf_samples_stay_in_their_row(torch, order):
    nchan, n = 4, 1500                          # 1024 samples per round: the second round carries the flag
    x = signal(nchan, 2 * n, order, seed=21)
    clean = ops.CostasLoop(order, bws(nchan), nchan=nchan, max_block=0)
    y_clean = clean.process_batch(dev(torch, x[:, :n])).cpu().numpy()
    s_clean = states(clean)
    fresh = ops.CostasLoop(order, bws(nchan), nchan=nchan, max_block=0)
    y_fresh = fresh.process_batch(dev(torch, x[:, n:])).cpu().numpy()      # what a row gives from (0, 0)
    for r, i, bad in ((2, 700, np.nan), (0, 0, complex(1.0, np.nan)), (3, n - 1, complex(np.nan, np.nan)), (1, 1100, np.nan)):
        xb = x[:, :n].copy()
        xb[r, i] = bad
        d = ops.CostasLoop(order, bws(nchan), nchan=nchan, max_block=0)
        y = d.process_batch(dev(torch, xb)).cpu().numpy()
        others = [c for c in range(nchan) if c != r]
        assert _same_bits(y[others], y_clean[others]) and same_state(states(d)[others], s_clean[others]), (r, i)
        assert _same_bits(y[r, :i], y_clean[r, :i]) and np.all(np.isnan(y[r, i:].view(F32))), (r, i)
        assert np.all(np.isnan(d.get_state(r)))
        # the next call: the row starts from (0, 0) like a fresh handle, the others carry on
        y2 = d.process_batch(dev(torch, x[:, n:])).cpu().numpy()
        assert _same_bits(y2[r], y_fresh[r]) and not np.any(np.isnan(y2.view(F32))), (r, i)
        assert same_state(d.get_state(r), fresh.get_state(r))
    for r, i, bad in ((1, 300, np.inf), (2, 0, complex(0.0, -np.inf)), (0, 1200, complex(np.inf, np.inf))):
        xb = x[:, :n].copy()
        xb[r, i] = bad
        d = ops.CostasLoop(order, bws(nchan), nchan=nchan, max_block=0)
        y = d.process_batch(dev(torch, xb)).cpu().numpy()          # (returns)
        others = [c for c in range(nchan) if c != r]
        assert _same_bits(y[others], y_clean[others]) and same_state(states(d)[others], s_clean[others]), (r, i)
        assert _same_bits(y[r, :i], y_clean[r, :i])


# ---- 7. argument errors, harness helpers ----------------------------------------------------------------------------------------
def test_argument_errors(torch):
    L = capi.load()
    h = C.c_void_p()
    for order, nchan, mb in ((3, 1, 10), (0, 1, 10), (16, 1, 10), (4, 0, 10), (4, 70_000, 10), (4, 1, -5)):
        assert L.qdsp_hip_costas_create(C.byref(h), 0, order, nchan, mb) == EINVAL
    two = ops.CostasLoop(4, 0.004, nchan=2, max_block=100)
    one = ops.CostasLoop(2, 0.004, max_block=100)
    x = np.zeros(101, np.complex64)
    y = np.zeros(101, np.complex64)
    assert L.qdsp_hip_costas_process(one._h, x.ctypes.data, 101, y.ctypes.data) == ESIZE
    assert L.qdsp_hip_costas_process(one._h, x.ctypes.data, -1, y.ctypes.data) == EINVAL
    assert L.qdsp_hip_costas_process(two._h, x.ctypes.data, 10, y.ctypes.data) == EINVAL            # host path: one channel
    assert L.qdsp_hip_costas_process_ex(one._h, x.ctypes.data, 7, 10, y.ctypes.data, 0) == EINVAL
    assert L.qdsp_hip_costas_process_ex(one._h, x.ctypes.data, 0, 10, y.ctypes.data, 3) == EINVAL    # deferred without an event
    for bw in (-0.001, float("nan"), float("inf"), -float("inf"), 1e30):
        assert L.qdsp_hip_costas_set_bandwidth(one._h, 0, bw) == EINVAL, bw
    assert _same_bits(one.gains(), costas_gains(0.004))                                            # a refused bandwidth changes nothing
    assert L.qdsp_hip_costas_set_bandwidth(two._h, 2, 0.004) == EINVAL
    assert L.qdsp_hip_costas_set_bandwidth(two._h, -2, 0.004) == EINVAL
    assert L.qdsp_hip_costas_set_bandwidth(two._h, -1, 0.0) == 0 and two.gains(1) == (0.0, 0.0)
    f, p = C.c_double(), C.c_double()
    assert L.qdsp_hip_costas_get_state(two._h, 2, C.byref(f), C.byref(p)) == EINVAL
    assert L.qdsp_hip_costas_get_state(two._h, 0, None, C.byref(p)) == EINVAL
    assert L.qdsp_hip_costas_get_state(two._h, 1, C.byref(f), C.byref(p)) == 0 and (f.value, p.value) == (0.0, 0.0)
    assert L.qdsp_hip_costas_set_state(two._h, 5, 0.0, 0.0) == EINVAL
    assert L.qdsp_hip_costas_set_state(two._h, 0, 0.0, 6.3) == EINVAL and L.qdsp_hip_costas_set_state(two._h, 0, 0.0, -7.0) == EINVAL
    assert L.qdsp_hip_costas_set_state(two._h, 0, 0.5, float(WRAP32)) == 0
    xt = torch.zeros(1000, dtype=torch.complex64, device="cuda")
    yt = torch.zeros(1000, dtype=torch.complex64, device="cuda")
    bd = L.qdsp_hip_costas_process_batch_dev
    assert bd(two._h, xt.data_ptr(), 400, 399, yt.data_ptr(), 400, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 400, 400, yt.data_ptr(), 300, None) == EINVAL
    assert bd(two._h, xt.data_ptr() + 4, 10, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 10, 10, yt.data_ptr() + 4, 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), -1, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, None, 10, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr() + 8, 10, 11, yt.data_ptr() + 8, 11, None) == 0               # 8-byte aligned rows are enough
    # handle kinds do not mix
    fm = ops.FmDemod(250e3, 75e3)
    cagc = ops.ComplexAgc()
    for other in (fm, cagc):
        assert L.qdsp_hip_costas_process_dev(other._h, xt.data_ptr(), 10, yt.data_ptr(), None) == EINVAL
        assert L.qdsp_hip_costas_reset(other._h) == EINVAL and L.qdsp_hip_costas_set_state(other._h, 0, 0.0, 0.0) == EINVAL
    assert L.qdsp_hip_demod_process_dev(one._h, xt.data_ptr(), 10, yt.data_ptr(), None) == EINVAL
    assert L.qdsp_hip_cagc_process_dev(one._h, xt.data_ptr(), 10, yt.data_ptr(), None) == EINVAL
    torch.cuda.synchronize()


def test_done_event_and_time(torch):
    L = capi.load()
    ev = C.c_void_p()
    capi.check(L.qdsp_hip_event_create(0, C.byref(ev)))
    d = ops.CostasLoop(4, 0.004, nchan=2)
    x = dev(torch, signal(2, 2000, 4, seed=3))
    assert L.qdsp_hip_set_done_event(d._h, ev) == 0
    assert d.time_dev(x, torch.empty_like(x), 3) > 0
    assert d.last_kernel()["name"] == "costas_kernel" and d.last_kernel()["grid"] == 1
    capi.check(L.qdsp_hip_event_destroy(ev))


# ---- 8. the real producer ---------------------------------------------------------------------------------------------------------
def test_batch_on_channelizer_output(torch, single):
    nchan, M = 64, 64
    taps = O.lowpass_taps_f64(256, 1.0 / 64.0)
    incs = [ops.phase_delta(1.0, -(c - 31.5) / 64.0) for c in range(nchan)]
    chn = ops.Channelizer(taps, 1, M, incs, max_block=0)
    bw = bws(nchan)
    loop = ops.CostasLoop(4, bw, nchan=nchan, max_block=0)
    st = {c: (0.0, 0.0) for c in (0, 17, 63)}
    for call, n in enumerate((64 * 300, 64 * 1000)):
        yc = chn.process(ops.synth_iq(n, first_sample=call * 10**6, seed=5))
        no = chn.out_size(n)
        assert yc.shape == (nchan, no)
        y = loop.process_batch(yc)                      # straight from the channelizer, with its strides
        assert loop.last_kernel()["name"] == "costas_kernel" and loop.last_kernel()["grid"] == 4
        yh, xh = y.cpu().numpy(), yc.cpu().numpy()
        assert np.all(np.isfinite(yh.view(F32)))
        for c in st:
            want, st[c] = single(torch, 4, bw[c], xh[c], st[c])
            assert _same_bits(yh[c], want) and same_state(loop.get_state(c), st[c]), (call, c)


# ---- 9. the block graph ------------------------------------------------------------------------------------------------------------
NG, BLOCK, DECIM = 120_000, 24_000, 10
VFO_ARGS = ["300000", "2400000", "240000", "200000"]    # offset, inSR, outSR, bandwidth: 2.4 Msps -> 240 ksps


@pytest.fixture(scope="module")
def graph(tmp_path_factory):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL, timeout=300)
    d = tmp_path_factory.mktemp("costasgraph")
    O.synth_iq(0, NG, seed=42).tofile(d / "x.cf32")
    subprocess.run([BIN, "vfo", str(d / "x.cf32"), str(d / "v.cf32"), str(BLOCK)] + VFO_ARGS, check=True, timeout=180,
                   capture_output=True, text=True)
    v = np.fromfile(d / "v.cf32", dtype=np.complex64)
    assert len(v) == NG // DECIM
    return d, v


@pytest.mark.parametrize("link,order", [("dev", 4), ("host", 4), ("dev", 2), ("dev", 8)])
def test_vfo_then_costas_loop_blocks(graph, link, order):
    d, v = graph
    out = d / f"costas_{link}_{order}.cf32"
    r = subprocess.run([BIN, "costas", link, str(d / "x.cf32"), str(out), str(BLOCK)] + VFO_ARGS + [str(order), "0.01"],
                       check=True, timeout=180, capture_output=True, text=True)
    assert "graph ok" in r.stdout and f"{link if link == 'host' else 'device'} link" in r.stdout
    y = np.fromfile(out, dtype=np.complex64)
    assert len(y) == len(v)
    vb = BLOCK // DECIM
    loop = ops.CostasLoop(order, 0.01, max_block=vb)
    for a in range(0, len(v), vb):          # one run() per VFO output block
        assert _same_bits(y[a:a + vb], loop.process(v[a:a + vb])), a
    assert np.all(np.isfinite(y.view(F32))) and float(np.max(np.abs(y))) > 0
