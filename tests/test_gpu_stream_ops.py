"""The host path that the per-row operators share (qdsp_amd/csrc/stream_op.*): *_process_ex under every pair of link codes, its
error codes, and the harness helpers that take any handle (qdsp_hip_set_done_event, qdsp_hip_last_kernel,
qdsp_hip_time_process_dev), for every handle kind behind that path.  The kernels have their own tests; here two consecutive blocks
through each pair of links must give the bits of the same two blocks through *_process on another fresh handle (the second block:
carried state is part of the comparison).  2053 samples are one full tile of 256 x 8 plus a ragged tail of 5: the smallest count
that takes both the 16-byte and the scalar path of the loads and stores; 1 is the smallest call there is."""
import ctypes as C

import numpy as np
import pytest

from qdsp_amd import capi, ops

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
HOST, DEVICE, PIPELINED, DEFERRED = 0, 1, 2, 3
MAXB = 4096
COUNTS = (2053, 1)
LINKS = [(i, o) for i in (HOST, DEVICE, PIPELINED) for o in (HOST, DEVICE, PIPELINED, DEFERRED)]


class Kind:
    """One handle kind: how to make it, floats per input / output sample, its entry-point family and its kernel at these sizes."""

    def __init__(self, name, make, fin, fout, kernel, nchan2=True):
        self.name, self._make, self.fin, self.fout, self.kernel, self.nchan2 = name, make, fin, fout, kernel, nchan2

    def make(self, nchan=1):
        kw = {"nchan": nchan} if self.nchan2 else {}
        return self._make(max_block=MAXB, **kw)

    def __repr__(self):
        return self.name


KINDS = [
    Kind("fm", lambda **k: ops.FmDemod(250e3, 75e3, **k), 2, 1, "fm_demod_kernel"),
    Kind("fm_stereo", lambda **k: ops.FmDemod(250e3, 75e3, stereo=True, **k), 2, 2, "fm_demod_kernel"),
    Kind("am", lambda **k: ops.AmDemod(**k), 2, 1, "am_sub_kernel"),
    Kind("ssb", lambda **k: ops.SsbDemod(48_000.0, 3_000.0, 0, **k), 2, 1, "ssb_demod_kernel", nchan2=False),
    Kind("deemp_mono", lambda **k: ops.Deemp(48e3, 50e-6, stereo=False, **k), 1, 1, "deemp_row_kernel"),
    Kind("deemp_stereo", lambda **k: ops.Deemp(48e3, 50e-6, stereo=True, **k), 2, 2, "deemp_row_kernel"),
    Kind("squelch", lambda **k: ops.Squelch(-50.0, **k), 2, 2, "level_row_kernel"),
    Kind("agc", lambda **k: ops.Agc(1.0, 48e3, **k), 1, 1, "level_row_kernel"),
    Kind("stereo_fm", lambda **k: ops.StereoFmDemod(250e3, 75e3, **k), 2, 2, "stereo_mix_kernel"),
    Kind("ffagc_real", lambda **k: ops.FeedForwardAgc("real", window=16, **k), 1, 1, "ff_agc_kernel"),
    Kind("ffagc_complex", lambda **k: ops.FeedForwardAgc("complex", window=16, **k), 2, 2, "ff_agc_kernel"),
    Kind("cagc", lambda **k: ops.ComplexAgc(**k), 2, 2, "cagc_row_kernel"),
    Kind("costas", lambda **k: ops.CostasLoop(2, 0.01, **k), 2, 2, "costas_kernel"),
]
IDS = [k.name for k in KINDS]
FFAGC = ("ffagc_real", "ffagc_complex")


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def event():
    L = capi.load()
    ev = C.c_void_p()
    capi.check(L.qdsp_hip_event_create(0, C.byref(ev)))
    yield ev
    capi.check(L.qdsp_hip_event_destroy(ev))


def blocks(kind, n):
    """Two input blocks of n samples, as floats."""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    return [rng.standard_normal(n * kind.fin).astype(np.float32) for _ in range(2)]


_REF = {}


def reference(kind, n):
    """(return code, output floats) of the two blocks through *_process on a fresh handle; computed once per (kind, n)."""
    if (kind.name, n) not in _REF:
        op, res = kind.make(), []
        for x in blocks(kind, n):
            y = np.zeros(n * kind.fout, np.float32)
            rc = op._fn("process")(op._h, x.ctypes.data, n, y.ctypes.data)
            assert rc >= 0, (kind, n, rc)
            res.append((rc, y))
        op.close()
        _REF[kind.name, n] = res
    return _REF[kind.name, n]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- 1. every pair of links gives the bits of the host path ---------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_every_link_pair_matches_the_host_path(torch, event, kind, n):
    want = reference(kind, n)
    if kind.name in FFAGC:
        assert [rc for rc, _ in want] == ([2038, 2053] if n == 2053 else [0, 0])
    else:
        assert [rc for rc, _ in want] == [0, 0]
    xs = blocks(kind, n)
    xd = [torch.from_numpy(x).cuda() for x in xs]
    L = capi.load()
    for il, ol in LINKS:
        op = kind.make()
        if ol == DEFERRED:
            assert L.qdsp_hip_set_done_event(op._h, event) == 0
        for b in range(2):
            yh = np.zeros(n * kind.fout, np.float32)
            yd = torch.zeros(n * kind.fout, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            src = xs[b].ctypes.data if il == HOST else xd[b].data_ptr()
            dst = yh.ctypes.data if ol in (HOST, DEFERRED) else yd.data_ptr()
            rc = op._fn("process_ex")(op._h, src, il, n, dst, ol)
            if ol == DEFERRED:
                assert L.qdsp_hip_event_wait(event) == 0
            if ol in (DEVICE, PIPELINED):
                torch.cuda.synchronize()
                yh = yd.cpu().numpy()
            wrc, wy = want[b]
            assert rc == wrc, (kind, n, il, ol, b, rc)
            assert np.array_equal(bits(yh), bits(wy)), (kind, n, il, ol, b)
        if n > 1 or kind.name not in FFAGC:          # (FeedForwardAGC emits nothing, and launches nothing but its history copy)
            assert op.last_kernel()["name"] == kind.kernel, (kind, op.last_kernel())
        op.close()


# ---- 2. error codes through each kind's own entry points ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_process_ex_error_codes(torch, event, kind):
    L = capi.load()
    n = MAXB + 1
    x = np.zeros(n * kind.fin, np.float32)
    y = np.zeros(n * kind.fout, np.float32)
    xd = torch.zeros(n * kind.fin, dtype=torch.float32, device="cuda")
    yd = torch.zeros(n * kind.fout, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    op = kind.make()
    ex = op._fn("process_ex")
    hp, dp = (x.ctypes.data, y.ctypes.data), (xd.data_ptr(), yd.data_ptr())
    assert op.last_kernel()["name"] == ""
    for il, ol in ((-1, HOST), (3, HOST), (7, HOST), (HOST, -1), (HOST, 4)):
        assert ex(op._h, hp[0], il, 10, hp[1], ol) == EINVAL, (il, ol)
    assert ex(op._h, hp[0], HOST, 10, hp[1], DEFERRED) == EINVAL, "deferred without an event"
    assert ex(op._h, hp[0], HOST, -1, hp[1], HOST) == EINVAL
    assert ex(op._h, None, HOST, 10, hp[1], HOST) == EINVAL
    assert L.qdsp_hip_set_done_event(op._h, event) == 0
    for il, ol in LINKS:                              # one count beyond max_block: refused wherever a side is on the host
        if il == HOST or ol in (HOST, DEFERRED):
            assert ex(op._h, hp[0] if il == HOST else dp[0], il, n, hp[1] if ol in (HOST, DEFERRED) else dp[1], ol) == ESIZE, (il, ol)
    for il, ol in LINKS:                              # no count but nothing else wrong: 0, before any work
        assert ex(op._h, hp[0] if il == HOST else dp[0], il, 0, hp[1] if ol in (HOST, DEFERRED) else dp[1], ol) == 0, (il, ol)
    assert ex(op._h, None, HOST, 0, None, HOST) == 0
    assert op.last_kernel()["name"] == "", "nothing has been launched so far"
    if kind.name in FFAGC:
        assert ex(op._h, hp[0], HOST, 10, None, HOST) == 0 and op.fill() == 10, "a call that emits nothing takes a null out"
        assert ex(op._h, hp[0], HOST, 10, None, HOST) == EINVAL and op.fill() == 10, "5 outputs and nowhere to put them"
        assert ex(op._h, hp[0], HOST, 10, hp[1], HOST) == 5 and op.fill() == 15
        want = n
    else:
        assert ex(op._h, hp[0], HOST, 10, None, HOST) == EINVAL
        want = 0
    assert ex(op._h, dp[0], DEVICE, n, dp[1], DEVICE) == want, "device to device: max_block does not bound it"
    torch.cuda.synchronize()
    assert op.last_kernel()["name"] == kind.kernel
    op.close()
    if kind.nchan2:
        two = kind.make(nchan=2)
        for il, ol in LINKS[:3]:
            assert two._fn("process_ex")(two._h, hp[0], il, 10, hp[1], ol) == EINVAL, "the block-graph path is one channel"
        assert two._fn("process")(two._h, hp[0], 10, hp[1]) == EINVAL
        two.close()


# ---- 3. the helpers that take any handle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_done_event_last_kernel_and_time(torch, event, kind, n):
    L = capi.load()
    op = kind.make()
    xd = torch.from_numpy(blocks(kind, n)[0]).cuda()
    yd = torch.zeros(n * kind.fout, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert L.qdsp_hip_set_done_event(op._h, event) == 0
    assert L.qdsp_hip_set_done_event(op._h, None) == 0
    assert op.last_kernel() == {"name": "", "grid": 0, "block": 0, "lds_bytes": 0}
    ms = C.c_float(-1.0)
    stream = torch.cuda.current_stream().cuda_stream
    args = (xd.data_ptr(), n, yd.data_ptr(), stream)
    assert L.qdsp_hip_time_process_dev(op._h, *args, 0, C.byref(ms)) == EINVAL
    assert L.qdsp_hip_time_process_dev(op._h, *args, -1, C.byref(ms)) == EINVAL
    assert L.qdsp_hip_time_process_dev(op._h, *args, 2, None) == EINVAL
    assert op.last_kernel()["name"] == "" and ms.value == -1.0
    assert L.qdsp_hip_time_process_dev(op._h, None, n, yd.data_ptr(), stream, 2, C.byref(ms)) == EINVAL, "the launch's own refusal comes through"
    assert op.last_kernel()["name"] == ""
    assert L.qdsp_hip_time_process_dev(op._h, *args, 2, C.byref(ms)) == 0 and ms.value > 0.0
    if kind.name in FFAGC:
        assert op.fill() == min(2 * n, 15)
    if n > 1 or kind.name not in FFAGC:
        assert op.last_kernel()["name"] == kind.kernel and op.last_kernel()["block"] in (64, 256)
    op.close()


def test_helpers_refuse_other_handles(torch):
    L = capi.load()
    m = ops.Math(ops.Math.ADD, max_block=16)
    op = KINDS[0].make()
    op.close()
    ms, g = C.c_float(), C.c_int()
    name = C.create_string_buffer(32)
    for h in (m._h, op._h, None):
        assert L.qdsp_hip_set_done_event(h, None) == EINVAL
        assert L.qdsp_hip_last_kernel(h, name, 32, C.byref(g), C.byref(g), C.byref(g)) == EINVAL
        assert L.qdsp_hip_time_process_dev(h, None, 0, None, None, 2, C.byref(ms)) == EINVAL
    m.close()


# ---- 4. handle kinds do not mix ------------------------------------------------------------------------------------------------------
def test_every_family_refuses_every_other_kind(torch):
    L = capi.load()
    x = np.zeros(32, np.float32)
    y = np.zeros(32, np.float32)
    made = [(k, k.make()) for k in KINDS]
    families = sorted({op._prefix for _, op in made})
    assert len(families) == 9
    for kind, op in made:
        for fam in families:
            rc = getattr(L, fam + "_process_ex")(op._h, x.ctypes.data, HOST, 10, y.ctypes.data, HOST)
            assert rc == (0 if fam == op._prefix else EINVAL), (kind, fam, rc)   # (10 samples: FeedForwardAGC emits none yet)
    for _, op in made:
        op.close()
