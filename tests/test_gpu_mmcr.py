"""MMClockRecovery on the GPU against its numpy definition (tests/_mmcr_ref.py: mm_ref), bit for bit: symbols, counts and the state
read back; call cuts and entry points; a row in a batch against the row alone; NaN locality; the interpolator table; the C++
mirror's harness.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _mmcr_ref as M
from qdsp_amd import capi, ops

pytestmark = pytest.mark.gpu

EINVAL = -10001
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "clock_check")
ROWS, SLOTS = 16, 32
SENT = 0x4B1DF00D                      # a finite float (1.0350605e7) no output of these inputs has
NP = {0: np.float32, 1: np.complex64}
G_OMEGA, G_MU, REL = 0.01 * 0.01 / 4, 0.01, 0.005


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def round_len(rows_in_wave: int) -> int:
    """Samples per row and round of a wave with that many rows (mmcr.hip.h)."""
    s = 2
    while rows_in_wave * s * 2 <= SLOTS:
        s *= 2
    return 64 * s


def chunks_of(nchan: int):
    """The round lengths of a launch over nchan rows: the full waves' and the last wave's."""
    ls = {round_len(nchan % ROWS or ROWS)}
    if nchan > ROWS:
        ls.add(round_len(ROWS))
    return sorted(ls)


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def row_params(nchan, L):
    """Per row: omega (1.02: every step 1; 2; 4; 10.7; one above the round length), gains and limit, differing within a wave."""
    omegas = [1.02, 2.0, 10.7, 1.5 * L + 0.3, 4.0]
    out = []
    for r in range(nchan):
        om = omegas[r % 5]
        g_mu = 0.01 if om < 1.5 else (0.005, 0.01, 0.02)[r % 3]
        out.append((om, (2.5e-5, 1e-4)[r % 2], g_mu, 0.005 if om < 1.5 else (0.005, 0.02)[(r // 5) % 2]))
    return out


def signals(kind, pars, n, seed):
    """One row per parameter set: symbols at the row's omega, a timing offset per row, noise."""
    rows = []
    for r, p in enumerate(pars):
        sps = p[0]
        x = M.signal(kind, sps, int(n / sps) + 2, seed * 1000 + r, offset=(0.1 + 0.13 * r) % 1.0 * min(sps, 8.0))
        rows.append(x[:n])
    return np.stack(rows)


def make(kind, pars, n):
    cols = list(zip(*pars))
    return ops.MmClockRecovery(kind, np.asarray(cols[0], F32), np.asarray(cols[1], F32), np.asarray(cols[2], F32), np.asarray(cols[3], F32),
                               nchan=len(pars), max_block=max(n, 1))


def ref_rows(x, kind, pars, states, taps):
    """mm_ref over one call of every row; `states` (a list, None at the start) is replaced."""
    outs = []
    for r, p in enumerate(pars):
        y, states[r] = M.mm_ref(x[r], kind, M.params(*p), states[r], taps)
        outs.append(y)
    return outs


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_state(d, r, st):
    mu, dyn, nxt = d.get_state(r)
    if np.isnan(st["mu"]):
        assert np.isnan(mu), r
    else:
        assert F32(mu) == F32(st["mu"]) and F32(dyn) == F32(st["dyn"]) and nxt == st["next"], (r, mu, dyn, nxt, st["mu"], st["dyn"], st["next"])


# ---- 1. bit-identity with mm_ref ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("nchan", [1, 15, 16, 17, 65])
def test_symbols_counts_and_state_are_mm_ref(torch, kind, nchan):
    """Rows with omega 1.02, 2, 10.7, 4 and one above the round length side by side in a wave, each with its own gains and limit;
    calls of 0, 1, 6, 7, 8, L - 1, L, L + 1 and 2 L + 5 samples one after the other on one handle."""
    L = chunks_of(nchan)[0]
    counts = [0, 1, 6, 7, 8, L - 1, L, L + 1, 2 * L + 5]
    n = sum(counts)
    pars = row_params(nchan, L)
    x = signals(kind, pars, n, seed=7 + kind)
    xt = dev(torch, x)
    d = make(kind, pars, n)
    taps = d.interp_taps()
    assert d.out_size(L) == L and d.out_size(0) == 0                # (a row of omega 1.02 is always there: steps of 1)
    states = [None] * nchan
    a = 0
    for c in counts:
        rows, cnt = d.process_batch(xt[:, a:a + c])
        assert d.last_kernel()["name"] == "mm_clock_kernel" or c == 0
        rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
        want = ref_rows(x[:, a:a + c], kind, pars, states, taps)
        assert [len(w) for w in want] == list(cnt), (c, cnt)
        assert np.array_equal(d.counts(), cnt)
        for r in range(nchan):
            assert same_bits(rows[r, :cnt[r]], want[r]), (c, r)
        a += c
    for r in sorted({0, nchan - 1, min(3, nchan - 1), (nchan - 1) // ROWS * ROWS}):
        check_state(d, r, states[r])


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("omega", [1.02, 2.0, 10.7, "above"])
def test_every_row_at_one_omega(torch, kind, omega):
    """16 rows in lockstep: all steps 1 (omega 1.02), 2, 10.7, and an omega above the round length (rounds that emit nothing)."""
    nchan, L = 16, round_len(16)
    om = 2.5 * L + 0.25 if omega == "above" else omega
    n = 2 * L + 5 if omega != "above" else 8 * L + 3
    pars = [(om, G_OMEGA, G_MU, REL)] * nchan
    x = signals(kind, pars, n, seed=31)
    d = make(kind, pars, n)
    taps = d.interp_taps()
    rows, cnt = d.process_batch(dev(torch, x))
    rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
    states = [None] * nchan
    want = ref_rows(x, kind, pars, states, taps)
    assert [len(w) for w in want] == list(cnt)
    if omega == 1.02:
        assert cnt.min() >= n / 1.03
    if omega == "above":
        assert 3 <= cnt.max() <= 4
    for r in range(nchan):
        assert same_bits(rows[r, :cnt[r]], want[r]), r
        check_state(d, r, states[r])


# ---- 2. call cuts and entry points -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nchan", [(0, 1), (1, 1), (0, 17), (1, 17)])
def test_cuts_and_entry_points_give_the_same_bits(torch, kind, nchan):
    Ls = chunks_of(nchan)
    sizes = [s for L in Ls for s in (1, 6, 7, 8, L - 1, L + 1)]
    n = sum(sizes) + Ls[-1] // 2 + 11
    cuts = [0] + list(np.cumsum(sizes)) + [n]
    pars = row_params(nchan, Ls[0]) if nchan > 1 else [(4.0, G_OMEGA, G_MU, REL)]
    x = signals(kind, pars, n, seed=11 + nchan)
    xt = dev(torch, x)
    one = make(kind, pars, n)
    rows, cnt = one.process_batch(xt)
    rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
    whole = [rows[r, :cnt[r]] for r in range(nchan)]
    st0 = [one.get_state(r) for r in range(nchan)]
    if nchan == 1:
        want, _ = M.mm_ref(x[0], kind, M.params(*pars[0]), None, one.interp_taps())
        assert same_bits(whole[0], want)

    d = make(kind, pars, n)
    got = [[] for _ in range(nchan)]
    for a, b in zip(cuts, cuts[1:]):
        rows, cnt = d.process_batch(xt[:, a:b])
        rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
        for r in range(nchan):
            got[r].append(rows[r, :cnt[r]].copy())
    for r in range(nchan):
        assert same_bits(np.concatenate(got[r]), whole[r]), r
        assert same_bits(np.asarray(d.get_state(r)), np.asarray(st0[r])), r
    if nchan > 1:
        return

    # one row: process() on host and device tensors ...
    for path in ("host", "device"):
        e = make(kind, pars, n)
        parts = [e.process(x[0, a:b]) if path == "host" else e.process(xt[0, a:b]).cpu().numpy() for a, b in zip(cuts, cuts[1:])]
        assert same_bits(np.concatenate(parts), whole[0]) and e.get_state(0) == st0[0], path
        e.reset()
        again = e.process(x[0]) if path == "host" else e.process(xt[0]).cpu().numpy()
        assert same_bits(again, whole[0]) and e.get_state(0) == st0[0], path
    # ... and process_ex with every accepted pair of links; the links that would hand over before the count is known are refused
    HOSTL, DEVL, PIPE, DEFER = 0, 1, 2, 3
    for il in (HOSTL, DEVL, PIPE):
        for ol in (HOSTL, DEVL):
            e = make(kind, pars, n)
            parts = []
            for a, b in zip(cuts, cuts[1:]):
                cap = max(e.out_size(b - a), 1)
                yh = np.zeros(cap, NP[kind])
                yd = torch.zeros(cap, dtype=xt.dtype, device="cuda")
                src = x[0, a:b].ctypes.data if il == HOSTL else xt[0, a:b].data_ptr()
                torch.cuda.synchronize()
                no = e.process_ex(src, il, b - a, yh.ctypes.data if ol == HOSTL else yd.data_ptr(), ol)
                parts.append(yh[:no].copy() if ol == HOSTL else yd[:no].cpu().numpy())
            assert same_bits(np.concatenate(parts), whole[0]) and e.get_state(0) == st0[0], (il, ol)
    e = make(kind, pars, n)
    y = np.zeros(n, NP[kind])
    L_ = capi.load()
    for ol in (PIPE, DEFER, 4, -1):
        assert L_.qdsp_hip_mmcr_process_ex(e._h, x[0].ctypes.data, HOSTL, 10, y.ctypes.data, ol) == EINVAL, ol
    assert e.get_state(0) == (0.5, 4.0, 0)


# ---- 3. a row in a batch equals the row alone --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_rows_of_a_batch_equal_the_rows_alone(torch, kind):
    """The first and last row of the first and last wave of 65 rows, on odd strides and an offset base, with sentinels after every
    row's count and after its out_size slots."""
    nchan, L = 65, round_len(16)
    n = 2 * L + 5
    pars = row_params(nchan, L)
    x = signals(kind, pars, n, seed=5)
    d = make(kind, pars, n)
    cap = d.out_size(n)
    in_stride, out_stride, in_off, out_off = n + 3, cap + 5, 1, 3
    dt = torch.complex64 if kind else torch.float32
    buf = torch.zeros(nchan * in_stride + in_off, dtype=dt, device="cuda")
    xin = buf[in_off:].as_strided((nchan, n), (in_stride, 1))
    xin.copy_(dev(torch, x))
    words = 2 if kind else 1
    obuf = torch.full(((nchan * out_stride + out_off) * words,), SENT, dtype=torch.int32, device="cuda").view(torch.float32)
    obuf = torch.view_as_complex(obuf.view(-1, 2)) if kind else obuf
    out = obuf[out_off:].as_strided((nchan, out_stride), (out_stride, 1))
    rows, cnt = d.process_batch(xin, out=out)
    assert rows.shape == (nchan, cap)
    cnt = cnt.cpu().numpy()
    raw = obuf.cpu().numpy().view(np.uint32).reshape(-1, words)
    assert np.all(raw[:out_off] == SENT)
    for r in range(nchan):
        row = raw[out_off + r * out_stride: out_off + (r + 1) * out_stride]
        assert np.all(row[cnt[r]:] == SENT), r                      # nothing behind the row's count, nor behind its out_size slots
        assert not np.any(np.all(row[:cnt[r]] == SENT, axis=1)), r
    got = out.cpu().numpy()
    for r in (0, 15, 64 - 16, 63, 64):
        alone = make(kind, [pars[r]], n)
        y = alone.process(dev(torch, x[r])).cpu().numpy()
        assert len(y) == cnt[r] and same_bits(got[r, :cnt[r]], y), r
        assert alone.get_state(0) == d.get_state(r), r


# ---- 4. NaN and Inf locality -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("poison", ["nan", "inf"])
def test_nan_and_inf_stay_in_their_row(torch, kind, poison):
    nchan, L = 5, round_len(5)
    n = L + 300                                                      # the poisoned sample lies in the second round
    pars = [(4.0, G_OMEGA, G_MU, REL)] * nchan
    x = signals(kind, pars, 2 * n, seed=17)
    clean = make(kind, pars, 2 * n)
    taps = clean.interp_taps()
    rows0, cnt0 = clean.process_batch(dev(torch, x[:, :n]))
    rows0, cnt0 = rows0.cpu().numpy(), cnt0.cpu().numpy()
    bad = x.copy()
    bad[2, L + 100] = np.nan if poison == "nan" else np.inf
    d = make(kind, pars, 2 * n)
    rows, cnt = d.process_batch(dev(torch, bad[:, :n]))
    rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
    for r in (0, 1, 3, 4):
        assert cnt[r] == cnt0[r] and same_bits(rows[r, :cnt[r]], rows0[r, :cnt0[r]]), r
        assert d.get_state(r) == clean.get_state(r), r
    want, st = M.mm_ref(bad[2, :n], kind, M.params(*pars[2]), None, taps)
    assert cnt[2] == len(want)
    got = rows[2, :cnt[2]]
    fin = np.isfinite(want.view(F32)).reshape(len(want), -1).all(axis=1)
    assert same_bits(got[fin], want[fin]) and np.array_equal(np.isnan(got.view(F32)), np.isnan(want.view(F32)))
    assert np.array_equal(np.isinf(got.view(F32)), np.isinf(want.view(F32)))
    first = int(np.argmin(fin))
    assert first > 0 and same_bits(got[:first], rows0[2, :first])   # up to the poisoned window the row is its clean self
    check_state(d, 2, st)
    if poison == "nan":
        assert cnt[2] == first + 1 and np.isnan(d.get_state(2)[0])  # the NaN symbol is written, then the row stops
        rows, cnt = d.process_batch(dev(torch, bad[:, n:]))
        assert cnt.cpu().numpy()[2] == 0 and np.isnan(d.get_state(2)[0])
        assert min(cnt.cpu().numpy()[[0, 1, 3, 4]]) > 0
        d.reset()                                                    # revives it
        rows, cnt = d.process_batch(dev(torch, x[:, :n]))
        rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
        assert cnt[2] == cnt0[2] and same_bits(rows[2, :cnt[2]], rows0[2, :cnt0[2]])
        d.set_state(0.25, 4.0, 3, chan=2)
        assert d.get_state(2) == (0.25, 4.0, 3)


# ---- 5. the table ------------------------------------------------------------------------------------------------------------------
def test_interp_taps_are_the_closed_form_and_can_be_replaced(torch):
    kind, n = 1, 700
    pars = [(4.0, G_OMEGA, G_MU, REL)]
    x = signals(kind, pars, n, seed=3)
    d = make(kind, pars, n)
    taps = d.interp_taps()
    assert same_bits(taps, M.lib_taps())
    y0 = d.process(x[0])
    rng = np.random.default_rng(1)
    other = (M.lib_taps() * (1 + 1e-3 * rng.standard_normal((129, 8)))).astype(F32)
    d.reset()
    d.set_interp_taps(other)
    assert same_bits(d.interp_taps(), other)
    y1 = d.process(x[0])
    want, st = M.mm_ref(x[0], kind, M.params(*pars[0]), None, other)
    assert same_bits(y1, want) and not same_bits(y1, y0[:len(y1)])
    check_state(d, 0, st)
    bad = other.copy()
    bad[5, 5] = np.nan
    L_ = capi.load()
    assert L_.qdsp_hip_mmcr_set_interp_taps(d._h, bad.ctypes.data_as(C.POINTER(C.c_float))) == EINVAL


def test_parameter_rule_and_argument_errors(torch):
    L_ = capi.load()
    h = C.c_void_p()
    mk = lambda *p: L_.qdsp_hip_mmcr_create(C.byref(h), 0, 0, 1, 1000, *p)
    assert mk(1.0, G_OMEGA, G_MU, REL) == EINVAL and not h
    for p in ((4.0, G_OMEGA, G_MU, 1.0), (float("nan"), G_OMEGA, G_MU, REL), (4.0, float("inf"), G_MU, REL), (4.0, G_OMEGA, float("nan"), REL),
              (0.0, G_OMEGA, G_MU, REL), (2.0 ** 20, G_OMEGA, G_MU, REL)):
        assert mk(*p) == EINVAL, p
    assert L_.qdsp_hip_mmcr_create(C.byref(h), 0, 2, 1, 1000, 4.0, G_OMEGA, G_MU, REL) == EINVAL
    assert mk(1.02, G_OMEGA, G_MU, REL) == 0 and h
    assert L_.qdsp_hip_mmcr_set_omega(h, 0, 1.0) == EINVAL and L_.qdsp_hip_mmcr_set_gains(h, 0, G_OMEGA, 0.5) == EINVAL
    assert L_.qdsp_hip_mmcr_set_limit(h, 0, 0.5) == EINVAL and L_.qdsp_hip_mmcr_set_omega(h, 1, 4.0) == EINVAL
    assert L_.qdsp_hip_mmcr_set_state(h, 0, 1.0, 1.02, 0) == EINVAL and L_.qdsp_hip_mmcr_set_state(h, 0, 0.5, 1.02, -1) == EINVAL
    assert L_.qdsp_hip_mmcr_out_size(h, 100) == 100
    assert L_.qdsp_hip_mmcr_set_omega(h, 0, 10.7) == 0 and L_.qdsp_hip_mmcr_out_size(h, 100) == 10
    x = torch.zeros(64, device="cuda")
    y = torch.zeros(64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert L_.qdsp_hip_mmcr_process_batch_dev(h, x.data_ptr(), 64, 64, y.data_ptr(), 6, None, s) == EINVAL      # out_stride < out_size
    assert L_.qdsp_hip_mmcr_process_batch_dev(h, x.data_ptr(), 64, 64, x.data_ptr(), 64, None, s) == EINVAL     # in place
    assert L_.qdsp_hip_mmcr_process_batch_dev(h, x.data_ptr() + 2, 60, 60, y.data_ptr(), 64, None, s) == EINVAL  # alignment
    assert L_.qdsp_hip_mmcr_process_batch_dev(h, x.data_ptr(), 64, 64, y.data_ptr(), 7, None, s) == 0
    L_.qdsp_hip_mmcr_destroy(h)


# ---- 6. the C++ mirror -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST, "build/clock_check"], stdout=subprocess.DEVNULL, timeout=300)
    return BIN


@pytest.mark.parametrize("kind,link", [(0, "dev"), (0, "host"), (1, "dev"), (1, "host")])
def test_clock_check_files_are_mm_ref(torch, harness, tmp_path, kind, link):
    n, block, omega = 6000, 1000, 4.0
    x = signals(kind, [(omega, G_OMEGA, G_MU, REL)], n, seed=23 + kind)[0]
    x.tofile(tmp_path / "x.bin")
    g, m, r = (repr(float(F32(v))) for v in (G_OMEGA, G_MU, REL))
    p = subprocess.run([harness, "c" if kind else "f", link, "x.bin", "y.bin", str(block), repr(omega), g, m, r], cwd=tmp_path, check=True,
                       timeout=180, capture_output=True, text=True)
    assert "graph ok" in p.stdout and f"{'host' if link == 'host' else 'device'} link" in p.stdout
    y = np.fromfile(tmp_path / "y.bin", dtype=NP[kind])
    d = make(kind, [(omega, G_OMEGA, G_MU, REL)], n)
    want, _ = M.mm_ref(x, kind, M.params(omega, G_OMEGA, G_MU, REL), None, d.interp_taps())
    assert len(want) > n / omega - 3 and same_bits(y, want)
