"""RowFir and DelayImag on the GPU (qdsp_amd/csrc/rowfir.hip).  RowFir bit for bit against `ops.Fir(...).set_mode(DIRECT)` run row
by row, over the tap counts around every boundary of the kernel's tap loop, call sizes around its tile, row counts, padded rows
that are only sample-aligned and sentinels around every output row; against the FP64 reference under the filter families' yardstick
rule; call cuts, row independence, NaN locality, state and argument errors.  DelayImag bit for bit against delay_imag_ref."""
import ctypes as C

import numpy as np
import pytest

from _numerics import FLOOR, K, direct_fma32, fir_ref64, region_check
from _psk_ref import delay_imag_ref
from qdsp_amd import capi, ops

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
F32 = np.float32
NP = {0: np.float32, 1: np.complex64}
SENT = F32(-7.25e11)                     # a finite float no output of these inputs has


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def geom():
    """(TILE, the taps per unrolled group of the kernel's tap loop), as the library reports them."""
    tile, group = ops.RowFir.tile(), ops.RowFir.tap_group()
    assert tile >= 256 and tile % 8 == 0 and 1 <= group <= 64
    return tile, group


def tap_counts(group):
    """1 and 2; every value around each unroll boundary of the tap loop; 32 and 33; the cap."""
    return sorted({1, 2, group - 1, group, group + 1, 2 * group, 2 * group + 1, 32, 33, 4096})


def call_sizes(T, tile):
    return [0, 1, max(T - 2, 0), T - 1, T, tile - 1, tile, tile + 1, 2 * tile + 5]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_taps(nchan, T, seed=3):
    """Differing taps per row, none of them zero (so that a NaN under a tap always shows)."""
    rng = np.random.default_rng(seed + T)
    t = rng.standard_normal((nchan, T)) / np.sqrt(T)
    t = np.where(np.abs(t) < 1e-3, 1e-3, t)
    return t.astype(F32)


def make_rows(kind, nchan, n, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nchan, n))
    if kind:
        x = x + 1j * rng.standard_normal((nchan, n))
    return x.astype(NP[kind])


def fir_direct(torch, kind, taps_row, x_row, cuts=None):
    """The yardstick of the bit tests: the single-stream FIR in its direct form over one row, call by call."""
    f = ops.Fir(taps_row, complex_data=bool(kind))
    f.set_mode(ops.Fir.DIRECT)
    cuts = cuts or [0, len(x_row)]
    xt = torch.from_numpy(np.ascontiguousarray(x_row)).cuda()
    parts = [f.process(xt[a:b].contiguous()).cpu().numpy() for a, b in zip(cuts, cuts[1:]) if b > a]
    return (np.concatenate(parts) if parts else np.zeros(0, NP[kind])), f


def padded(torch, x, lead=1):
    """The rows of x in a tensor whose row stride is odd and whose rows start `lead` samples in: only sample-aligned."""
    nchan, n = x.shape
    stride = n + lead + 2
    stride += 1 - stride % 2
    buf = torch.zeros((nchan, stride), dtype=torch.from_numpy(x[:1, :1]).dtype, device="cuda")
    buf[:, lead:lead + n] = torch.from_numpy(x).cuda()
    view = buf[:, lead:lead + n]
    assert view.stride(0) % 2 == 1
    return view


def guarded_out(torch, kind, nchan, n):
    """(guard tensor, the output view inside it): 8 sentinel samples in front of and at least 8 behind every output row, odd stride."""
    width = n + 16 + (n % 2 == 0)
    assert width % 2 == 1
    g = torch.full((nchan, width), float(SENT), dtype=torch.float32 if kind == 0 else torch.complex64, device="cuda")
    return g, g[:, 8:8 + n]


def sentinels_intact(g, n):
    a = g.cpu().numpy()
    edge = np.concatenate([a[:, :8], a[:, 8 + n:]], axis=1)
    return bool(np.all(edge.real == SENT)) and (not np.iscomplexobj(edge) or bool(np.all(edge.imag == 0)))


def run_calls(torch, op, xv, sizes, kind):
    """`op` over the padded rows xv call by call into guarded outputs: the concatenated rows [nchan, sum(sizes)]."""
    nchan = xv.shape[0]
    parts, a = [], 0
    for s in sizes:
        g, out = guarded_out(torch, kind, nchan, s)
        y = op.process_batch(xv[:, a:a + s], out=out, count=s)
        assert y.shape == (nchan, s)
        parts.append(y.cpu().numpy().reshape(nchan, s))
        assert sentinels_intact(g, s), ("sentinels around every output row", s)
        a += s
    return np.concatenate(parts, axis=1)


# ---- 1. bit identity with the single-stream FIR in its direct form ------------------------------------------------------------------
def test_geometry_is_exported(geom):
    tile, group = geom
    assert (tile, group) == (capi.load().qdsp_hip_rowfir_tile(), capi.load().qdsp_hip_rowfir_tap_group())


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("slot", range(10))
def test_bits_are_the_direct_firs(torch, geom, kind, slot):
    """Three rows with differing taps, one handle over calls of 0, 1, T-2, T-1, T, TILE-1, TILE, TILE+1 and 2 TILE + 5 samples, rows and
    outputs padded to odd strides: every row equals ops.Fir in DIRECT mode over the same row in one call; so does one call of the
    concatenation."""
    tile, group = geom
    counts = tap_counts(group)
    assert len(counts) == 10
    T = counts[slot]
    sizes = call_sizes(T, tile)
    n, nchan = sum(sizes), 3
    taps, x = make_taps(nchan, T), make_rows(kind, nchan, n, seed=T)
    want = np.stack([fir_direct(torch, kind, taps[c], x[c])[0] for c in range(nchan)])
    xv = padded(torch, x)
    op = ops.RowFir(kind, taps, nchan=nchan, max_block=16)
    assert op.ntaps == T
    got = run_calls(torch, op, xv, sizes, kind)
    assert op.last_kernel()["name"] == "row_fir_kernel" and op.last_kernel()["block"] == 256
    assert same_bits(got, want), ("cut calls", T, np.argwhere(got != want)[:4])
    one = ops.RowFir(kind, taps, nchan=nchan, max_block=16)
    assert same_bits(run_calls(torch, one, xv, [n], kind), want), ("one call", T)
    for c in range(nchan):                       # the carried history is the row's last T - 1 inputs
        assert same_bits(op.get_history(c), x[c, n - (T - 1):] if T > 1 else x[c, :0]), c


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("nchan", [1, 65])
def test_row_counts_and_row_independence(torch, geom, kind, nchan):
    """1 and 65 rows with differing taps; a row in the batch equals the row alone."""
    tile, group = geom
    T = 2 * group + 1
    sizes = [T - 1, tile + 1, 5]
    n = sum(sizes)
    taps, x = make_taps(nchan, T, seed=9), make_rows(kind, nchan, n, seed=40 + nchan)
    got = run_calls(torch, ops.RowFir(kind, taps, nchan=nchan, max_block=16), padded(torch, x), sizes, kind)
    for c in sorted({0, nchan // 2, nchan - 1}):
        assert same_bits(got[c], fir_direct(torch, kind, taps[c], x[c])[0]), c
        alone = ops.RowFir(kind, taps[c], nchan=1, max_block=16)
        assert same_bits(run_calls(torch, alone, padded(torch, x[c:c + 1]), sizes, kind)[0], got[c]), ("the row alone", c)


# ---- 2. the FP64 reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("T", [33, 4096])
def test_against_the_fp64_reference(torch, geom, kind, T):
    tile, _ = geom
    sizes = [T - 1, tile + 1, 2 * tile + 5]
    n = sum(sizes)
    taps, x = make_taps(2, T, seed=5), make_rows(kind, 2, n, seed=T + 1)
    got = run_calls(torch, ops.RowFir(kind, taps, nchan=2, max_block=16), padded(torch, x), sizes, kind)
    pos, cuts = np.arange(n), np.cumsum([0] + sizes)
    regions = {f"call {k}": (pos >= a) & (pos < b) for k, (a, b) in enumerate(zip(cuts, cuts[1:]))}
    regions["stream"] = np.ones(n, bool)
    for c in range(2):
        ok, rep = region_check(got[c], direct_fma32(taps[c], x[c]), fir_ref64(taps[c], x[c]), regions, k=K, floor=FLOOR)
        worst = max(rep.values(), key=lambda v: v["ratio"])
        print(f"kind={kind} T={T} row {c}: worst rms ratio to the yardstick {worst['ratio']:.3f} (bound {K})")
        assert ok, {k: v for k, v in rep.items() if not v["ok"]}


# ---- 3. NaN locality ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("T", [13, 33])
def test_a_nan_reaches_its_own_window_only(torch, geom, kind, T):
    """A NaN at sample p of row r changes exactly outputs p .. p + T - 1 of row r: at a tile edge, at a call edge (through the
    history) and in the first call (nothing before it but the zero history)."""
    tile, _ = geom
    sizes = [tile + 3, 7, tile]
    n, nchan, r = sum(sizes), 3, 1
    taps, x = make_taps(nchan, T), make_rows(kind, nchan, n, seed=77)
    xv = padded(torch, x)
    clean = run_calls(torch, ops.RowFir(kind, taps, nchan=nchan, max_block=16), xv, sizes, kind)
    for p in (0, tile - 3, sizes[0] - 2, sizes[0] + sizes[1] - 1):
        bad = x.copy()
        bad[r, p] = complex(np.nan, x[r, p].imag) if kind else np.nan      # (complex rows: the real part only)
        got = run_calls(torch, ops.RowFir(kind, taps, nchan=nchan, max_block=16), padded(torch, bad), sizes, kind)
        changed = got.view(np.uint32).reshape(nchan, n, -1) != clean.view(np.uint32).reshape(nchan, n, -1)
        hit = np.zeros((nchan, n), bool)
        hit[r, p:p + T] = True
        assert np.array_equal(changed.any(axis=2), hit), (p, np.argwhere(changed.any(axis=2) != hit)[:4])
        if kind == 0:
            assert np.all(np.isnan(got[r, p:p + T]))
        else:                                      # a real NaN in a complex sample: the real parts only
            assert np.all(np.isnan(got[r, p:p + T].real)) and same_bits(got[r].imag, clean[r].imag)


# ---- 4. state ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_set_taps_history_and_reset(torch, geom, kind):
    tile, group = geom
    T0, T1, T2 = 33, group, 70
    n = 300
    x = make_rows(kind, 2, 4 * n, seed=8)
    t0, t1, t2 = make_taps(1, T0)[0], make_taps(1, T1)[0], make_taps(1, T2)[0]
    xt = torch.from_numpy(x).cuda()
    op = ops.RowFir(kind, t0, nchan=2, max_block=16)
    firs = []
    for c in range(2):
        f = ops.Fir(t0, complex_data=bool(kind))
        f.set_mode(ops.Fir.DIRECT)
        firs.append(f)

    def step(k):
        y = op.process_batch(xt[:, k * n:(k + 1) * n]).cpu().numpy()
        for c in range(2):
            assert same_bits(y[c], firs[c].process(xt[c, k * n:(k + 1) * n].contiguous()).cpu().numpy()), (k, c)
            assert same_bits(op.get_history(c), firs[c].get_history()), (k, c)
        return y

    first = step(0)
    op.set_taps(t1)                                # a shorter filter in mid-stream: the newest samples stay
    for f in firs:
        f.set_taps(t1)
    assert op.ntaps == T1
    step(1)
    op.set_taps(t2)                                # a longer one: the older part of the history is zero
    for f in firs:
        f.set_taps(t2)
    step(2)
    op.set_taps(make_taps(1, T2, seed=21)[0], 1)   # one channel, the same count
    firs[1].set_taps(make_taps(1, T2, seed=21)[0])
    step(3)
    assert capi.load().qdsp_hip_rowfir_set_taps(op._h, 1, t1.ctypes.data_as(C.POINTER(C.c_float)), T1) == EINVAL      # another count
    # get / set round trip, one channel at a time
    h0, h1 = op.get_history(0), op.get_history(1)
    assert h0.shape == (T2 - 1,) and not same_bits(h0, h1)
    op.set_history(h1, 0)
    assert same_bits(op.get_history(0), h1) and same_bits(op.get_history(1), h1)
    # count == 0 launches nothing and keeps the history
    op.process_batch(xt[:, :0], count=0)
    assert same_bits(op.get_history(0), h1)
    # reset: zero history, the first call's bits again (with the first taps)
    op.set_taps(t0)
    op.reset()
    assert not op.get_history(1).any()
    assert same_bits(op.process_batch(xt[:, :n]).cpu().numpy(), first)


@pytest.mark.parametrize("kind", [0, 1])
def test_entry_points_give_the_same_bits(torch, kind):
    T, n = 25, 3000
    taps, x = make_taps(1, T)[0], make_rows(kind, 1, n, seed=12)[0]
    want, _ = fir_direct(torch, kind, taps, x)
    xt = torch.from_numpy(x).cuda()
    cuts = [0, 1, 700, n]
    host = ops.RowFir(kind, taps, max_block=4096)
    assert same_bits(np.concatenate([host.process(x[a:b]) for a, b in zip(cuts, cuts[1:])]), want)
    devp = ops.RowFir(kind, taps, max_block=4096)
    assert same_bits(np.concatenate([devp.process(xt[a:b].contiguous()).cpu().numpy() for a, b in zip(cuts, cuts[1:])]), want)
    HOSTL, DEVL = 0, 1
    for il in (HOSTL, DEVL):
        for ol in (HOSTL, DEVL):
            e = ops.RowFir(kind, taps, max_block=4096)
            yh, yd = np.zeros(n, NP[kind]), torch.zeros(n, dtype=xt.dtype, device="cuda")
            torch.cuda.synchronize()
            for a, b in zip(cuts, cuts[1:]):
                src = x[a:b].ctypes.data if il == HOSTL else xt[a:b].data_ptr()
                dst = yh[a:b].ctypes.data if ol == HOSTL else yd[a:b].data_ptr()
                assert e.process_ex(src, il, b - a, dst, ol) == 0
            assert same_bits(yh if ol == HOSTL else yd.cpu().numpy(), want), (il, ol)
    assert host.time_dev(xt, torch.empty_like(xt), 2) > 0.0
    # the completion event of a deferred host output (qdsp_hip_set_done_event takes the new kinds)
    L_ = capi.load()
    ev = C.c_void_p()
    capi.check(L_.qdsp_hip_event_create(0, C.byref(ev)))
    for e, ref in ((ops.RowFir(kind, taps, max_block=4096), want[:700]), (ops.DelayImag(max_block=4096), None)):
        if ref is None and not kind:
            continue
        hy = np.zeros(700, NP[kind])
        assert e._fn("process_ex")(e._h, x.ctypes.data, 0, 700, hy.ctypes.data, 3) == EINVAL      # deferred, but no event yet
        e.set_done_event(ev.value)
        assert e.process_ex(x.ctypes.data, 0, 700, hy.ctypes.data, 3) == 0                         # host out, deferred
        capi.check(L_.qdsp_hip_event_wait(ev))
        assert same_bits(hy, ref if ref is not None else delay_imag_ref(x[:700])[0])
    capi.check(L_.qdsp_hip_event_destroy(ev))


# ---- 5. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors(torch):
    L_ = capi.load()
    h = C.c_void_p()
    t = (C.c_float * 5000)(*([0.5] * 5000))
    for kind, nchan, ntaps, mb in ((2, 1, 3, 16), (-1, 1, 3, 16), (0, 0, 3, 16), (0, 65536, 3, 16), (0, 1, 0, 16), (0, 1, 4097, 16), (0, 1, 3, -1)):
        assert L_.qdsp_hip_rowfir_create(C.byref(h), 0, kind, nchan, t, ntaps, mb) == EINVAL and not h, (kind, nchan, ntaps, mb)
    assert L_.qdsp_hip_rowfir_create(C.byref(h), 0, 1, 1, None, 3, 16) == EINVAL
    assert L_.qdsp_hip_rowfir_create(C.byref(h), 0, 1, 2, t, 4096, 16) == 0 and h
    assert L_.qdsp_hip_rowfir_ntaps(h) == 4096 and L_.qdsp_hip_rowfir_ntaps(None) == EINVAL
    assert L_.qdsp_hip_rowfir_set_taps(h, 2, t, 4096) == EINVAL and L_.qdsp_hip_rowfir_set_taps(h, -2, t, 4096) == EINVAL
    assert L_.qdsp_hip_rowfir_set_taps(h, 0, t, 4095) == EINVAL and L_.qdsp_hip_rowfir_set_taps(h, -1, t, 4097) == EINVAL
    assert L_.qdsp_hip_rowfir_set_taps(h, -1, None, 3) == EINVAL and L_.qdsp_hip_rowfir_set_taps(h, -1, t, 3) == 0
    buf = (C.c_float * 16)()
    assert L_.qdsp_hip_rowfir_get_history(h, 2, buf) == EINVAL and L_.qdsp_hip_rowfir_set_history(h, -1, buf) == EINVAL
    x = torch.zeros(256, dtype=torch.complex64, device="cuda")
    y = torch.zeros(256, dtype=torch.complex64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    run = lambda i, n, si, o, so: L_.qdsp_hip_rowfir_process_batch_dev(h, i, n, si, o, so, s)   # noqa: E731
    assert run(x.data_ptr(), 64, 64, x.data_ptr(), 64) == EINVAL                 # in place
    assert run(x.data_ptr(), 64, 128, x.data_ptr() + 8 * 100, 128) == EINVAL     # overlapping spans (row 1 of the input)
    assert run(x.data_ptr(), 64, 63, y.data_ptr(), 64) == EINVAL                 # stride < count
    assert run(x.data_ptr(), 64, 64, y.data_ptr(), 63) == EINVAL
    assert run(x.data_ptr() + 4, 64, 64, y.data_ptr(), 64) == EINVAL             # not aligned to the sample
    assert run(x.data_ptr(), 64, 64, y.data_ptr() + 4, 64) == EINVAL
    assert run(x.data_ptr(), -1, 64, y.data_ptr(), 64) == EINVAL and run(None, 64, 64, y.data_ptr(), 64) == EINVAL
    assert run(None, 0, 0, None, 0) == 0                                        # count 0: nothing to do
    assert run(x.data_ptr(), 64, 128, y.data_ptr(), 128) == 0
    hx = np.zeros(64, np.complex64)
    assert L_.qdsp_hip_rowfir_process_ex(h, hx.ctypes.data, 0, 8, hx.ctypes.data, 0) == EINVAL       # two channels: no host path
    L_.qdsp_hip_rowfir_destroy(h)
    h1 = C.c_void_p()
    assert L_.qdsp_hip_rowfir_create(C.byref(h1), 0, 1, 1, t, 3, 16) == 0
    hy = np.zeros(64, np.complex64)
    assert L_.qdsp_hip_rowfir_process_ex(h1, hx.ctypes.data, 0, 17, hy.ctypes.data, 0) == ESIZE      # count > max_block on a host side
    assert L_.qdsp_hip_rowfir_process_ex(h1, hx.ctypes.data, 0, 16, hy.ctypes.data, 4) == EINVAL
    assert L_.qdsp_hip_rowfir_process_ex(h1, hx.ctypes.data, 0, 16, hy.ctypes.data, 0) == 0
    L_.qdsp_hip_rowfir_destroy(h1)
    L_.qdsp_hip_rowfir_destroy(None)


# ---- 6. DelayImag ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [1, 3, 65])
def test_delay_imag_is_delay_imag_ref(torch, geom, nchan):
    """The same cuts and layouts against delay_imag_ref, bit for bit: NaN payloads, infinities and signed zeros pass unchanged."""
    tile, _ = geom
    sizes = [0, 1, 2, tile - 1, tile, tile + 1, 2 * tile + 5]
    n = sum(sizes)
    x = make_rows(1, nchan, n, seed=60 + nchan)
    w = x.view(np.uint32).reshape(nchan, n, 2)
    w[:, 5, 1] = 0x7FC12345                         # a NaN with a payload, -0.0, an infinity
    w[:, tile, 1] = 0x80000000
    w[:, tile + 1, 0] = 0xFF800000
    op = ops.DelayImag(nchan=nchan, max_block=16)
    got = run_calls(torch, op, padded(torch, x), sizes, 1)
    assert op.last_kernel()["name"] == "delay_imag_kernel"
    for c in range(nchan):
        want, last = delay_imag_ref(x[c])
        assert same_bits(got[c], want), c
        assert same_bits(op.get_state(c), last), c
    one = ops.DelayImag(nchan=nchan, max_block=16)
    assert same_bits(run_calls(torch, one, padded(torch, x), [n], 1), got)


def test_delay_imag_state_entry_points_and_errors(torch):
    n = 1000
    x = make_rows(1, 2, n, seed=4)
    xt = torch.from_numpy(x).cuda()
    op = ops.DelayImag(nchan=2, max_block=16)
    assert op.get_state(0) == 0 and op.get_state(1) == 0
    op.set_state(2.5, 1)
    op.set_state(-0.0, 0)
    assert op.get_state(1) == F32(2.5) and np.signbit(op.get_state(0))
    y = op.process_batch(xt).cpu().numpy()
    assert same_bits(y[1], delay_imag_ref(x[1], 2.5)[0]) and same_bits(y[0], delay_imag_ref(x[0], -0.0)[0])
    op.process_batch(xt[:, :0], count=0)            # count 0 keeps the state
    assert same_bits(op.get_state(0), x[0, -1].imag)
    op.set_state(1.0)
    assert op.get_state(0) == 1 and op.get_state(1) == 1
    op.reset()
    assert same_bits(op.process_batch(xt).cpu().numpy()[0], delay_imag_ref(x[0])[0])
    # one row: host, device and the block-graph entry point
    want = delay_imag_ref(x[0])[0]
    for path in ("host", "device", "ex"):
        e = ops.DelayImag(max_block=4096)
        if path == "host":
            got = np.concatenate([e.process(x[0, :300]), e.process(x[0, 300:])])
        elif path == "device":
            got = np.concatenate([e.process(xt[0, :300].contiguous()).cpu().numpy(), e.process(xt[0, 300:].contiguous()).cpu().numpy()])
        else:
            got = np.zeros(n, np.complex64)
            assert e.process_ex(x[0].ctypes.data, 0, n, got.ctypes.data, 0) == 0
        assert same_bits(got, want), path
    L_ = capi.load()
    s = torch.cuda.current_stream().cuda_stream
    yt = torch.zeros_like(xt)
    run = lambda i, k, si, o, so: L_.qdsp_hip_delay_imag_process_batch_dev(op._h, i, k, si, o, so, s)   # noqa: E731
    assert run(xt.data_ptr(), 100, n, xt.data_ptr(), n) == EINVAL                # in place
    assert run(xt.data_ptr(), 100, n, xt.data_ptr() + 8 * 50, n) == EINVAL       # overlapping
    assert run(xt.data_ptr() + 4, 100, n, yt.data_ptr(), n) == EINVAL and run(xt.data_ptr(), 100, 99, yt.data_ptr(), n) == EINVAL
    assert run(xt.data_ptr(), 100, n, yt.data_ptr(), n) == 0
    v = C.c_float()
    assert L_.qdsp_hip_delay_imag_get_state(op._h, 2, C.byref(v)) == EINVAL and L_.qdsp_hip_delay_imag_set_state(op._h, 2, 0.0) == EINVAL
    h = C.c_void_p()
    assert L_.qdsp_hip_delay_imag_create(C.byref(h), 0, 0, 16) == EINVAL and not h
    L_.qdsp_hip_delay_imag_destroy(None)
