"""PskDemod and MskDemod on the GPU (qdsp_amd/csrc/psk_chain.cpp).  A chain handle against the composition of the existing operators
called one after the other -- ComplexAgc -> one Fir in DIRECT mode per row -> CostasLoop -> delay_imag_ref -> MmClockRecovery, and
FmDemod -> MmClockRecovery -- bit for bit: symbols, counts, every stage's state read through stage(), and the tap_dev rows; the
entry points against each other; NaN locality; reset; argument errors; the C++ mirror's harness; and the one test that says the
chain demodulates (tests/_psk_ref.py: the convergence condition the CPU test asserts on the numpy chain)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _mmcr_ref as M
import _psk_ref as P
from qdsp_amd import capi, ops

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "psk_check")
NTAPS = 32
SR = 48000.0
HOSTL, DEVL, PIPE, DEFER = 0, 1, 2, 3
SENT = 8589934592.0                   # 2^33: a float no symbol of these inputs is


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def tile():
    return ops.RowFir.tile()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def call_sizes(tile):
    """0, 1, 6, T - 1, 700 and 2 TILE + 5 samples; with max_block 1024 the last call grows the scratch rows in mid-stream."""
    return [0, 1, 6, NTAPS - 1, 700, 2 * tile + 5]


def row_params(nchan):
    """Per row: baud rate (2.3 to 5.9 samples per symbol), roll-off, AGC rate, loop bandwidth, the clock's gains and limit, deviation."""
    r = np.arange(nchan)
    return dict(baud=(SR / (2.3 + 0.45 * (r % 9))).astype(F32), alpha=(0.32 + 0.01 * (r % 5)).astype(F32),
                agc_rate=(1e-3 * (1 + r % 4)).astype(F32), bw=(0.004 + 0.001 * (r % 3)).astype(F32),
                g_omega=(2.5e-5 * (1 + r % 2)).astype(F32), g_mu=(0.01 + 0.002 * (r % 3)).astype(F32), rel=(0.005 + 0.001 * (r % 2)).astype(F32),
                dev=(SR / (4 + r % 3)).astype(F32))


_SIG = {}


def rows_of(nchan, n):
    """nchan rows of n samples: QPSK-like pulses at each row's symbol rate plus noise, at differing amplitudes (shared, never changed)."""
    if (nchan, n) not in _SIG:
        par = row_params(nchan)
        x = np.stack([M.signal(1, float(F32(SR) / par["baud"][c]), int(n / 2.2) + 8, seed=100 + c)[:n] * F32(0.05 * (1 + c % 7)) for c in range(nchan)])
        assert x.shape == (nchan, n) and x.dtype == np.complex64
        x.setflags(write=False)
        _SIG[(nchan, n)] = x
    return _SIG[(nchan, n)]


def padded(torch, x, lead=1):
    """The rows of x in a tensor whose row stride is odd and whose rows start `lead` samples in: only sample-aligned."""
    nchan, n = x.shape
    stride = n + lead + 2
    stride += 1 - stride % 2
    buf = torch.zeros((nchan, stride), dtype=torch.complex64, device="cuda")
    buf[:, lead:lead + n] = torch.from_numpy(np.array(x)).cuda()          # (a copy: the shared rows are read-only)
    return buf[:, lead:lead + n]


def make_psk(order, offset, nchan, **kw):
    p = row_params(nchan)
    return ops.PskDemod(order, offset, SR, p["baud"], NTAPS, p["alpha"], p["agc_rate"], p["bw"], p["g_omega"], p["g_mu"], p["rel"], nchan=nchan,
                        max_block=kw.pop("max_block", 1024), **kw)


def make_msk(nchan, **kw):
    p = row_params(nchan)
    return ops.MskDemod(SR, p["dev"], p["baud"], p["g_omega"], p["g_mu"], p["rel"], nchan=nchan, max_block=kw.pop("max_block", 1024), **kw)


class PskComposition:
    """The separate handles doing the same work, one call after the other; the delay is the numpy definition."""

    def __init__(self, torch, order, offset, nchan):
        p = row_params(nchan)
        self.torch, self.nchan, self.offset = torch, nchan, offset
        self.agc = ops.ComplexAgc(1.0, 65535.0, p["agc_rate"], nchan=nchan, max_block=16)
        self.taps = [ops.rrc_taps(NTAPS, SR, p["baud"][c], p["alpha"][c]) for c in range(nchan)]
        self.firs = []
        for c in range(nchan):
            f = ops.Fir(self.taps[c], complex_data=True, max_block=16)
            f.set_mode(ops.Fir.DIRECT)
            self.firs.append(f)
        self.costas = ops.CostasLoop(order, p["bw"], nchan=nchan, max_block=16)
        self.last_im = np.zeros(nchan, F32)
        self.clock = ops.MmClockRecovery(ops.MmClockRecovery.COMPLEX, (F32(SR) / p["baud"]).astype(F32), p["g_omega"], p["g_mu"], p["rel"], nchan=nchan,
                                         max_block=16)

    def call(self, xv):
        """One call over the rows xv [nchan, n]: (symbol rows, counts, the stage outputs)."""
        torch, n = self.torch, xv.shape[1]
        if n == 0:
            return np.zeros((self.nchan, 0), np.complex64), np.zeros(self.nchan, np.int32), {}
        a = self.agc.process_batch(xv)
        f = torch.stack([self.firs[c].process(a[c].contiguous()) for c in range(self.nchan)])
        c_ = self.costas.process_batch(f)
        stages = {"agc": a.cpu().numpy(), "costas": c_.cpu().numpy()}
        d = c_
        if self.offset:
            dn = np.empty((self.nchan, n), np.complex64)
            for c in range(self.nchan):
                dn[c], self.last_im[c] = P.delay_imag_ref(stages["costas"][c], self.last_im[c])
            stages["delay"] = dn
            d = torch.from_numpy(dn).cuda()
        rows, cnt = self.clock.process_batch(d)
        return rows.cpu().numpy(), cnt.cpu().numpy(), stages


def check_psk_states(chain, comp, label):
    agc, rrc, costas, clock = (chain.stage(w) for w in (chain.AGC, chain.RRC, chain.COSTAS, chain.CLOCK))
    for c in range(chain.nchan):
        assert agc.get_gain(c) == comp.agc.get_gain(c), (label, "agc gain", c)
        assert same_bits(rrc.get_history(c), comp.firs[c].get_history()), (label, "rrc history", c)
        assert costas.get_state(c) == comp.costas.get_state(c), (label, "costas state", c)
        assert costas.gains(c) == comp.costas.gains(c), (label, "costas gains", c)
        got, want = clock.get_state(c), comp.clock.get_state(c)
        assert same_bits(np.asarray(got, np.float64), np.asarray(want, np.float64)), (label, "clock state", c, got, want)
        if comp.offset:
            assert same_bits(chain.stage(chain.DELAY).get_state(c), comp.last_im[c]), (label, "lastIm", c)


# ---- 1. the chain is the composition of the existing operators -----------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [1, 17, 33])
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("order", [2, 4, 8])
def test_psk_chain_is_the_composition(torch, tile, order, offset, nchan):
    sizes = call_sizes(tile)
    n = sum(sizes)
    xv = padded(torch, rows_of(nchan, n))
    chain, comp = make_psk(order, offset, nchan), PskComposition(torch, order, offset, nchan)
    assert chain.stage(chain.RRC).ntaps == NTAPS
    for c in sorted({0, nchan - 1}):
        assert same_bits(np.concatenate([chain.stage(chain.RRC).get_history(c)]), np.zeros(NTAPS - 1, np.complex64))
    a = 0
    for k, s in enumerate(sizes):
        no = chain.out_size(s)
        assert no == comp.clock.out_size(s)
        guard = torch.full((nchan, no + 17 - no % 2), SENT, dtype=torch.complex64, device="cuda")      # (odd stride)
        out = guard[:, 8:8 + no]
        rows, cnt = chain.process_batch(xv[:, a:a + s], out=out, count=s)
        want_rows, want_cnt, stages = comp.call(xv[:, a:a + s])
        cnt = cnt.cpu().numpy()
        assert np.array_equal(cnt, want_cnt) and np.array_equal(chain.counts(), want_cnt), (k, s, cnt, want_cnt)
        rows = rows.cpu().numpy()
        for c in range(nchan):
            assert same_bits(rows[c, :cnt[c]], want_rows[c, :cnt[c]]), (k, s, c)
        g = guard.cpu().numpy()
        for c in range(nchan):                   # nothing written outside a row's symbols
            assert np.all(g[c, :8] == SENT) and np.all(g[c, 8 + cnt[c]:] == SENT), ("sentinels", k, c)
        if s:
            assert chain.last_kernel()["name"] == "mm_clock_kernel"
            assert chain.tap(chain.RRC) is None                         # (the Costas loop has run over them in place)
            assert same_bits(chain.tap(chain.COSTAS, s).cpu().numpy(), stages["costas"]), ("costas rows", k)
            if offset:
                assert same_bits(chain.tap(chain.DELAY, s).cpu().numpy(), stages["delay"]), ("delay rows", k)
                assert chain.tap(chain.AGC) is None                     # (the delay stage has reused them)
            else:
                assert same_bits(chain.tap(chain.AGC, s).cpu().numpy(), stages["agc"]), ("agc rows", k)
            assert chain.tap(chain.COSTAS).data_ptr() % 16 == 0 and chain.tap(chain.COSTAS).stride(0) % 2 == 0
        check_psk_states(chain, comp, (k, s))
        a += s


@pytest.mark.parametrize("nchan", [1, 17, 33])
def test_msk_chain_is_the_composition(torch, tile, nchan):
    sizes = call_sizes(tile)
    n = sum(sizes)
    p = row_params(nchan)
    xv = padded(torch, rows_of(nchan, n))
    chain = make_msk(nchan)
    fm = ops.FmDemod(SR, p["dev"], nchan=nchan, max_block=16)
    clock = ops.MmClockRecovery(ops.MmClockRecovery.REAL, (F32(SR) / p["baud"]).astype(F32), p["g_omega"], p["g_mu"], p["rel"], nchan=nchan, max_block=16)
    a = 0
    for k, s in enumerate(sizes):
        rows, cnt = chain.process_batch(xv[:, a:a + s])
        cnt = cnt.cpu().numpy()
        if s:
            m = fm.process_batch(xv[:, a:a + s])
            want_rows, want_cnt = clock.process_batch(m)
            want_rows, want_cnt = want_rows.cpu().numpy(), want_cnt.cpu().numpy()
            assert same_bits(chain.tap(chain.FM, s).cpu().numpy(), m.cpu().numpy()), ("fm rows", k)
        else:
            want_rows, want_cnt = np.zeros((nchan, 0), F32), np.zeros(nchan, np.int32)
        assert rows.dtype == torch.float32 and np.array_equal(cnt, want_cnt) and np.array_equal(chain.counts(), want_cnt), (k, s)
        rows = rows.cpu().numpy()
        for c in range(nchan):
            assert same_bits(rows[c, :cnt[c]], want_rows[c, :cnt[c]]), (k, s, c)
            assert same_bits(chain.stage(chain.FM).get_phase(c), fm.get_phase(c)), (k, c)
            assert same_bits(np.asarray(chain.stage(chain.CLOCK).get_state(c)), np.asarray(clock.get_state(c))), (k, c)
        a += s


# ---- 2. the entry points -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["psk4", "oqpsk", "msk"])
def test_entry_points_give_the_same_bits(torch, which):
    n, cuts = 3000, [0, 1, 7, 700, 3000]
    x = rows_of(1, n)[0]
    xt = torch.from_numpy(np.array(x)).cuda()
    make = (lambda: make_msk(1, max_block=4096)) if which == "msk" else (lambda: make_psk(4, which == "oqpsk", 1, max_block=4096))
    sym = np.float32 if which == "msk" else np.complex64
    ref = make()
    rows, cnt = ref.process_batch(xt.view(1, -1))
    whole = rows.cpu().numpy()[0, :int(cnt.cpu().numpy()[0])]          # one call
    assert whole.dtype == sym and len(whole) > n / 2.4 - 20
    got = []
    d = make()
    for a, b in zip(cuts, cuts[1:]):
        r, c = d.process_batch(xt[a:b].view(1, -1))
        got.append(r.cpu().numpy()[0, :int(c.cpu().numpy()[0])])
    batch = np.concatenate(got)                                        # the cut calls
    # (the AGC stage is an FP64 scan whose last bits may depend on the cuts: every path is compared at the same cuts)
    assert len(batch) == len(whole)
    for path in ("host", "device"):
        e = make()
        parts = [e.process(x[a:b]) if path == "host" else e.process(xt[a:b].contiguous()).cpu().numpy() for a, b in zip(cuts, cuts[1:])]
        assert same_bits(np.concatenate(parts), batch), path
        e.reset()
        again = e.process(x) if path == "host" else e.process(xt).cpu().numpy()
        assert same_bits(again, whole), (path, "after reset")
    for il in (HOSTL, DEVL, PIPE):
        for ol in (HOSTL, DEVL):
            e = make()
            parts = []
            for a, b in zip(cuts, cuts[1:]):
                cap = max(e.out_size(b - a), 1)
                yh = np.zeros(cap, sym)
                yd = torch.zeros(cap, dtype=torch.float32 if which == "msk" else torch.complex64, device="cuda")
                src = x[a:b].ctypes.data if il == HOSTL else xt[a:b].data_ptr()
                torch.cuda.synchronize()
                no = e.process_ex(src, il, b - a, yh.ctypes.data if ol == HOSTL else yd.data_ptr(), ol)
                parts.append(yh[:no].copy() if ol == HOSTL else yd[:no].cpu().numpy())
            assert same_bits(np.concatenate(parts), batch), (il, ol)
    e = make()
    y = np.zeros(n, sym)
    for ol in (PIPE, DEFER, 4, -1):                 # links that would hand over before the count is known
        assert e._fn("process_ex")(e._h, x.ctypes.data, HOSTL, 10, y.ctypes.data, ol) == EINVAL, ol
    assert e._fn("process_ex")(e._h, x.ctypes.data, HOSTL, 4097, y.ctypes.data, HOSTL) == ESIZE
    assert same_bits(e.process(x), whole)            # (the refused calls moved nothing)
    out = torch.zeros(n, dtype=torch.float32 if which == "msk" else torch.complex64, device="cuda")
    assert e.time_dev(xt, out, 2) > 0.0


# ---- 3. NaN locality and reset -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["psk", "msk"])
def test_a_nan_stays_in_its_row_and_reset_replays(torch, which):
    nchan, n, r = 17, 1500, 5
    x = rows_of(nchan, n)
    make = (lambda: make_msk(nchan)) if which == "msk" else (lambda: make_psk(4, True, nchan))

    def run(chain, rows):
        out, cnt = chain.process_batch(torch.from_numpy(np.array(rows)).cuda())
        return out.cpu().numpy(), cnt.cpu().numpy()

    chain = make()
    clean, ccnt = run(chain, x)
    bad = x.copy()
    bad[r, 400] = complex(np.nan, 0.25)
    other = make()
    got, gcnt = run(other, bad)
    for c in range(nchan):
        if c == r:
            assert gcnt[c] < ccnt[c] or not same_bits(got[c, :gcnt[c]], clean[c, :ccnt[c]])
        else:
            assert gcnt[c] == ccnt[c] and same_bits(got[c, :gcnt[c]], clean[c, :ccnt[c]]), c
    second, scnt = run(chain, x)                     # the state moved on ...
    assert not all(same_bits(second[c, :scnt[c]], clean[c, :ccnt[c]]) for c in range(nchan) if scnt[c] == ccnt[c])
    chain.reset()                                    # ... and reset replays the first call's bits
    assert not chain.counts().any()
    again, acnt = run(chain, x)
    assert np.array_equal(acnt, ccnt)
    for c in range(nchan):
        assert same_bits(again[c, :acnt[c]], clean[c, :ccnt[c]]), c
    other.reset()                                    # the stopped row runs again
    again, acnt = run(other, x)
    assert np.array_equal(acnt, ccnt) and same_bits(again[r, :acnt[r]], clean[r, :ccnt[r]])


# ---- 4. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors(torch):
    L_ = capi.load()
    h = C.c_void_p()
    t = (C.c_float * 8)(*([0.125] * 8))
    g, m, r = 2.5e-5, 0.01, 0.005
    psk = lambda order, offset, nchan, ntaps, omega, taps=t, bw=0.004: L_.qdsp_hip_psk_create(   # noqa: E731
        C.byref(h), 0, order, offset, nchan, 64, taps, ntaps, 1e-3, bw, omega, g, m, r)
    for args in ((3, 0, 1, 8, 4.0), (4, 2, 1, 8, 4.0), (4, -1, 1, 8, 4.0), (4, 0, 0, 8, 4.0), (4, 0, 1, 0, 4.0), (4, 0, 1, 4097, 4.0),
                 (4, 0, 1, 8, 0.5), (4, 0, 1, 8, float("nan"))):
        assert psk(*args) == EINVAL and not h, args
    assert psk(4, 0, 1, 8, 4.0, taps=None) == EINVAL and psk(4, 0, 1, 8, 4.0, bw=-1.0) == EINVAL and not h
    assert L_.qdsp_hip_msk_create(C.byref(h), 0, 1, 64, 0.0, 6000.0, 4.0, g, m, r) == EINVAL and not h      # sample rate
    assert L_.qdsp_hip_msk_create(C.byref(h), 0, 1, 64, 48000.0, 6000.0, 1.0, g, m, r) == EINVAL and not h  # a step below one sample
    assert L_.qdsp_hip_msk_create(C.byref(h), 0, 0, 64, 48000.0, 6000.0, 4.0, g, m, r) == EINVAL and not h
    assert psk(4, 0, 2, 8, 4.0) == 0 and h
    s, st = C.c_void_p(), C.c_int64()
    assert L_.qdsp_hip_psk_stage(h, 3, C.byref(s)) == EINVAL              # _DELAY on a chain without offset
    assert L_.qdsp_hip_psk_stage(h, 5, C.byref(s)) == EINVAL and L_.qdsp_hip_psk_stage(h, -1, C.byref(s)) == EINVAL
    assert L_.qdsp_hip_psk_stage(h, 0, None) == EINVAL and L_.qdsp_hip_msk_stage(h, 0, C.byref(s)) == EINVAL       # the other kind
    assert L_.qdsp_hip_psk_stage(h, 4, C.byref(s)) == 0 and s
    assert L_.qdsp_hip_mmcr_set_omega(s, 1, 0.5) == EINVAL and L_.qdsp_hip_mmcr_set_omega(s, 1, 10.7) == 0        # the stage's own rule
    assert L_.qdsp_hip_psk_out_size(h, 100) == 34 and L_.qdsp_hip_psk_out_size(h, -1) == EINVAL
    assert L_.qdsp_hip_psk_tap_dev(h, 4, C.byref(s), C.byref(st)) == EINVAL and L_.qdsp_hip_psk_tap_dev(h, 3, C.byref(s), C.byref(st)) == EINVAL
    assert L_.qdsp_hip_psk_tap_dev(h, 2, None, C.byref(st)) == EINVAL
    assert L_.qdsp_hip_psk_tap_dev(h, 2, C.byref(s), C.byref(st)) == 0 and not s                                 # before the first call
    x = torch.zeros(256, dtype=torch.complex64, device="cuda")
    y = torch.zeros(256, dtype=torch.complex64, device="cuda")
    cs = torch.cuda.current_stream().cuda_stream
    run = lambda i, n, si, o, so: L_.qdsp_hip_psk_process_batch_dev(h, i, n, si, o, so, None, cs)   # noqa: E731
    assert run(x.data_ptr(), 64, 63, y.data_ptr(), 64) == EINVAL and run(None, 64, 64, y.data_ptr(), 64) == EINVAL
    assert run(x.data_ptr(), -1, 64, y.data_ptr(), 64) == EINVAL and run(x.data_ptr(), 64, 64, None, 64) == EINVAL
    hx, hy = np.zeros(64, np.complex64), np.zeros(64, np.complex64)
    assert L_.qdsp_hip_psk_process_ex(h, hx.ctypes.data, 0, 8, hy.ctypes.data, 0) == EINVAL                      # two channels: no host path
    cnt = (C.c_int * 2)(5, 5)
    assert L_.qdsp_hip_psk_get_counts(h, None) == EINVAL and L_.qdsp_hip_psk_get_counts(h, cnt) == 0 and list(cnt) == [0, 0]
    assert run(x.data_ptr(), 64, 128, y.data_ptr(), 128) == 0
    assert L_.qdsp_hip_psk_get_counts(h, cnt) == 0 and cnt[0] == 16 and 5 <= cnt[1] <= 7
    assert L_.qdsp_hip_msk_destroy(h) is None and L_.qdsp_hip_psk_reset(h) == 0          # (the other kind's destroy leaves it alone)
    L_.qdsp_hip_psk_destroy(h)
    L_.qdsp_hip_psk_destroy(None)
    with pytest.raises(capi.QdspHipError):
        make_psk(4, False, 1).stage(ops.PskDemod.DELAY)
    with pytest.raises(capi.QdspHipError):
        ops.PskDemod(4, False, 48000.0, 48000.0)      # a rate ratio below the clock stage's parameter rule


# ---- 5. the C++ mirror ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST, "build/psk_check"], stdout=subprocess.DEVNULL, timeout=300)
    return BIN


@pytest.mark.parametrize("link", ["dev", "host"])
@pytest.mark.parametrize("mode", ["psk2", "psk4", "psk8", "oqpsk", "msk"])
def test_psk_check_files_are_the_operators(torch, harness, tmp_path, mode, link):
    n, block = 6000, 1000
    x = np.ascontiguousarray(rows_of(1, n)[0])
    x.tofile(tmp_path / "x.bin")
    sr, baud, alpha, rate, bw, g, m, r, dev = 48000.0, 12000.0, 0.35, 2e-3, 0.005, 5e-5, 0.012, 0.006, 6000.0
    f = lambda v: repr(float(F32(v)))               # noqa: E731
    if mode == "msk":
        extra = [f(dev), f(g), f(m), f(r)]
        op = ops.MskDemod(sr, dev, baud, F32(g), F32(m), F32(r), max_block=block)
        sym = np.float32
    else:
        extra = ["31", f(alpha), f(rate), f(bw), f(g), f(m), f(r)]
        order, offset = {"psk2": (2, False), "psk4": (4, False), "psk8": (8, False), "oqpsk": (4, True)}[mode]
        op = ops.PskDemod(order, offset, sr, baud, 31, F32(alpha), F32(rate), F32(bw), F32(g), F32(m), F32(r), max_block=block)
        sym = np.complex64
    p = subprocess.run([harness, mode, link, "x.bin", "y.bin", str(block), f(sr), f(baud)] + extra, cwd=tmp_path, check=True, timeout=180,
                       capture_output=True, text=True)
    assert "graph ok" in p.stdout and f"{'host' if link == 'host' else 'device'} link" in p.stdout
    y = np.fromfile(tmp_path / "y.bin", dtype=sym)
    want = np.concatenate([op.process(x[a:a + block]) for a in range(0, n, block)])
    assert len(want) > n / 4 - 5 and same_bits(y, want)


# ---- 6. the chain demodulates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntaps", [31, 32])
@pytest.mark.parametrize("order", [4, 2])
def test_convergence(torch, order, ntaps):
    """QPSK and BPSK at 4 samples per symbol through 31 and 32 RRC taps, alpha 0.32; 6000 symbols at RMS 0.05 with a carrier of
    2e-3 rad per sample plus a fixed phase, a fractional timing offset and noise at 0.05 of the RMS; default loop parameters.  Over
    the second half of the symbols less the last 250 every decision equals the sent symbol for one rotation of the constellation
    and one delay, and the Costas frequency read back lies within 5e-4 of 2e-3.  (The CPU test asserts the same on the numpy chain.)"""
    x, sent = P.psk_signal(order, 6000)
    op = ops.PskDemod(order, False, 4.0, 1.0, ntaps, 0.32, max_block=len(x))
    y = op.process(x)
    freq, _ = op.stage(op.COSTAS).get_state(0)
    ok, rep = P.converged(y, freq, sent, order)
    print(order, ntaps, rep)
    assert rep["compared"] == 2750 and ok, rep
