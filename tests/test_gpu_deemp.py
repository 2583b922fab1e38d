"""BFMDeemp on the GPU (qdsp_hip_deemp_*, ops.Deemp, dsp::BFMDeemp) against the exact recurrence of the reference's float
coefficients (tests/test_deemp_cpu.py: deemp_exact, sequential in np.longdouble).  Bound 1, for every output:
    |y_gpu - truth| <= 0.5 ulp32(truth) + 2^-40 E,     E = the same filter over |x| from |state|
(one final rounding, plus 2^13 FP64 epsilons of reassociation relative to the sum of the absolute terms).  A reassociated scan
cannot repeat the float loop of the reference bit for bit, so the reference enters as |y_gpu - y_ref| <= |y_ref - truth| + bound
and, for rows of at least 4096 samples, max |y_gpu - truth| <= max |y_ref - truth|."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from qdsp_amd import capi, ops
from test_deemp_cpu import (ALPHAS, INPUTS, LD, ROW_TILES, SIZES, TILE, _same_bits, case_table, check_against_truth, deemp_alpha,
                            deemp_bound, deemp_envelope, deemp_exact, deemp_ref, make_input)

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -10001, -10003
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "demod_check")
ROW, SCAN = "deemp_row_kernel", "deemp_scan_kernel"


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def cuts_of(n, sizes=(1, 7, 4096, 65_537)):
    c = [0]
    for s in sizes:
        c.append(min(n, c[-1] + s))
    return c + [n]


def form_of(n):
    return ROW if -(-n // TILE) <= ROW_TILES else SCAN


def meets_bound(y, x, alpha, state=0.0, label=""):
    """Bound 1 for one call over columns x from the exact `state`; returns the exact state after it."""
    truth, st = deemp_exact(x, alpha, state)
    check_against_truth(y, truth, deemp_envelope(x, alpha, state), None, label)
    return st


# ---- 1. accuracy against the exact recurrence ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_accuracy_against_the_exact_recurrence(torch, n):
    x, al, ref, truth, env = case_table(n)
    names = list(ALPHAS)
    for ai, name in enumerate(names):
        sr, tau = ALPHAS[name]
        mono = ops.Deemp(sr, tau, stereo=False, max_block=n)
        assert _same_bits([mono.alpha()], [al[3 * ai]])
        got = {}
        for k in range(3):
            mono.reset()
            y = mono.process(torch.from_numpy(x[:, 3 * ai + k].copy()).cuda()).cpu().numpy()
            assert mono.last_kernel()["name"] == form_of(n)
            got[f"mono {INPUTS[k]}"] = (3 * ai + k, y)
            if k == 0:                      # the host entry point runs the same launch
                mono.reset()
                assert _same_bits(mono.process(x[:, 3 * ai]), y)
        st = ops.Deemp(sr, tau, stereo=True, max_block=n)
        for l, r in ((0, 1), (2, 0)):
            st.reset()
            xs = np.ascontiguousarray(x[:, [3 * ai + l, 3 * ai + r]])
            y = st.process(torch.from_numpy(xs).cuda()).cpu().numpy()
            assert y.shape == (n, 2) and st.last_kernel()["name"] == form_of(n)
            got[f"stereo l {INPUTS[l]}"] = (3 * ai + l, y[:, 0])
            got[f"stereo r {INPUTS[r]}"] = (3 * ai + r, y[:, 1])
            # both components run the same arithmetic as a mono row
            assert _same_bits(y[:, 0], got[f"mono {INPUTS[l]}"][1]) and _same_bits(y[:, 1], got[f"mono {INPUTS[r]}"][1])
        for what, (k, y) in got.items():
            label = f"n={n} {name} {what}"
            ratio, e_gpu, e_ref = check_against_truth(y, truth[:, k], env[:, k], ref[:, k], label)
            if n >= 4096:
                assert e_gpu <= e_ref, label


# ---- 2. call boundaries ---------------------------------------------------------------------------------------------------------------
def test_call_boundaries_and_state(torch):
    n = 400_001
    sr, tau = ALPHAS["240k_75us"]
    al = deemp_alpha(sr, tau)
    x = np.stack([make_input("gauss", n, sr, 3), make_input("tone", n, sr)], axis=1)
    truth, _ = deemp_exact(x, al)
    env = deemp_envelope(x, al)
    xt = torch.from_numpy(x).cuda()
    cuts = cuts_of(n)
    for path in ("host", "device"):
        one = ops.Deemp(sr, tau, max_block=n)
        y1 = one.process(x) if path == "host" else one.process(xt).cpu().numpy()
        check_against_truth(y1, truth, env, None, f"{path} one call")
        d = ops.Deemp(sr, tau, max_block=n)
        st = np.zeros(2, LD)
        pieces = []
        for a, b in zip(cuts, cuts[1:]):
            y = d.process(x[a:b]) if path == "host" else d.process(xt[a:b]).cpu().numpy()
            st = meets_bound(y, x[a:b], al, st, f"{path} [{a}, {b})")
            pieces.append(y)
        yr = np.concatenate(pieces)
        check_against_truth(yr, truth, env, None, f"{path} ragged")
        assert _same_bits(d.get_state(), yr[-1]) and _same_bits(one.get_state(), y1[-1])
    # set_state + process == a fresh filter started from that state
    a_, b_ = ops.Deemp(sr, tau), ops.Deemp(sr, tau)
    a_.process(xt[:5000])
    a_.set_state(0.375, -1.5)
    b_.set_state(0.375, -1.5)
    assert _same_bits(a_.process(xt[5000:90_000]).cpu().numpy(), b_.process(xt[5000:90_000]).cpu().numpy())
    b_.set_state(0.375, -1.5)
    meets_bound(b_.process(xt[:3000]).cpu().numpy(), x[:3000], al, np.asarray([0.375, -1.5], LD), "from the float state")
    b_.reset()
    assert b_.get_state() == (0, 0)
    assert _same_bits(b_.process(xt[:3000]).cpu().numpy(), ops.Deemp(sr, tau).process(xt[:3000]).cpu().numpy())
    # count 0 keeps the state, count 1 works
    m = ops.Deemp(sr, tau, stereo=False)
    m.set_state(0.5)
    assert len(m.process(np.zeros(0, np.float32))) == 0 and m.get_state() == np.float32(0.5)
    y = m.process(np.asarray([2.0], np.float32))
    meets_bound(y, np.asarray([2.0], np.float32), al, 0.5, "count 1")
    assert _same_bits([m.get_state()], y)


# ---- 3. batch on the real producer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stereo", [True, False])
def test_batch_on_channelizer_and_fm_output(torch, stereo):
    nchan, M, SR = 64, 64, 250_000.0
    taps = O.lowpass_taps_f64(256, 1.0 / 64.0)
    incs = [ops.phase_delta(1.0, -(c - 31.5) / 64.0) for c in range(nchan)]
    chn = ops.Channelizer(taps, 1, M, incs, max_block=0)
    fm = ops.FmDemod(SR / M, 1_000.0, stereo=stereo, nchan=nchan)
    rates = np.asarray([SR / M * (1 + c % 5) for c in range(nchan)], np.float32)
    taus = np.asarray([(50e-6 if c % 2 else 75e-6) * (1 + c % 3) for c in range(nchan)], np.float32)
    al = np.asarray([deemp_alpha(rates[c], taus[c]) for c in range(nchan)], np.float32)
    nc = 2 if stereo else 1
    for pad in (37, 0):                     # rows padded by an odd number of samples: the scalar path; unpadded: the vector path
        de = ops.Deemp(rates, taus, stereo=stereo, nchan=nchan)
        singles = [ops.Deemp(float(rates[c]), float(taus[c]), stereo=stereo) for c in (0, 17, 63)]
        st = np.zeros(nchan * nc, LD)
        for call, n in enumerate((64 * 4096, 64 * 40_000)):
            x = ops.synth_iq(n, first_sample=call * 10**7, seed=5)
            no = chn.out_size(n)
            yc = chn.process(x)
            fbuf = torch.zeros((nchan, no + pad, 2) if stereo else (nchan, no + pad), dtype=torch.float32, device="cuda")
            f = fm.process_batch(yc, fbuf)
            obuf = torch.zeros_like(fbuf)
            y = de.process_batch(f, obuf)
            assert de.last_kernel()["name"] == form_of(no)
            fh, yh = f.cpu().numpy().reshape(nchan, no, nc), y.cpu().numpy().reshape(nchan, no, nc)
            if pad:
                assert float(obuf[:, no:].abs().max()) == 0, "the padding is not written"
            cols = lambda a: a.transpose(1, 0, 2).reshape(no, nchan * nc)      # one column per channel and component
            st = meets_bound(cols(yh), cols(fh), np.repeat(al, nc), st, f"pad {pad} call {call}")
            for s, c in zip(singles, (0, 17, 63)):      # same tiling, same order: the same bits
                ys = s.process(f[c].contiguous()).cpu().numpy().reshape(no, nc)
                assert _same_bits(ys, yh[c]), (pad, call, c)


# ---- 4. non-finite input ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [TILE, 3 * TILE + 5, 40 * TILE + 1001])
def test_non_finite_input_stays_in_its_lane_and_call(torch, n):
    sr, tau = ALPHAS["48k_50us"]
    al = deemp_alpha(sr, tau)
    x = np.stack([make_input("gauss", n, sr, 1), make_input("gauss", n, sr, 2)], axis=1)
    x2 = np.stack([make_input("gauss", 5000, sr, 3), make_input("gauss", 5000, sr, 4)], axis=1)
    ks = sorted({5, (n // TILE // 2) * TILE + 777 if n > TILE else 1000, n - 3})
    for bad in (np.nan, np.inf, -np.inf):
        for k in ks:
            xb = x.copy()
            xb[k, 0] = bad
            d = ops.Deemp(sr, tau)
            y = d.process(torch.from_numpy(xb).cuda()).cpu().numpy()
            label = f"n={n} {bad} at {k}"
            fin = np.isfinite(y[:, 0])
            assert np.all(fin[:k]) and not np.any(fin[k:]), label
            if np.isnan(bad):
                assert np.all(np.isnan(y[k:, 0])), label
            meets_bound(y[:k, 0], x[:k, 0], al, 0.0, label + " l before")
            st_r = meets_bound(y[:, 1], x[:, 1], al, 0.0, label + " r")
            y2 = d.process(torch.from_numpy(x2).cuda()).cpu().numpy()        # the next call is clean, l from state 0
            meets_bound(y2, x2, al, np.asarray([0, st_r], LD), label + " next call")
    # signed zeros and subnormals in: finite out
    xz = x.copy()
    xz[::3, 0] = -0.0
    xz[1::3, 0] = 1e-45
    xz[2::3, 0] = -3e-39
    xz[::2, 1] = 0.0
    y = ops.Deemp(sr, tau).process(torch.from_numpy(xz).cuda()).cpu().numpy()
    assert np.all(np.isfinite(y))
    meets_bound(y, xz, al, 0.0, f"n={n} zeros and subnormals")


# ---- 5. bypass, 6. in place, 7. determinism ------------------------------------------------------------------------------------------
def test_bypass_copies_and_keeps_the_state(torch):
    sr, tau = ALPHAS["48k_50us"]
    nchan, n = 3, 70_001
    x = torch.randn((nchan, n + 5, 2), device="cuda")
    d = ops.Deemp(sr, tau, nchan=nchan)
    d.process_batch(x[:, :1000])
    before = [d.get_state(c) for c in range(nchan)]
    d.bypass(True)
    out = torch.zeros((nchan, n + 3, 2), device="cuda")
    y = d.process_batch(x, out, count=n)
    assert torch.equal(y.view(torch.int32), x[:, :n].view(torch.int32)) and float(out[:, n:].abs().max()) == 0
    assert [d.get_state(c) for c in range(nchan)] == before
    m = ops.Deemp(sr, tau, stereo=False, max_block=n)
    m.bypass(True)
    xh = make_input("gauss", n, sr)
    xh[7] = np.nan
    assert _same_bits(m.process(xh), xh) and m.get_state() == 0
    d.bypass(False)
    ref = ops.Deemp(sr, tau, nchan=nchan)
    ref.process_batch(x[:, :1000])
    assert torch.equal(d.process_batch(x[:, 1000:5000]), ref.process_batch(x[:, 1000:5000]))


@pytest.mark.parametrize("n", [TILE * ROW_TILES - 4, 1_000_003])     # even row stride: vector path; odd: scalar
def test_in_place_equals_out_of_place(torch, n):
    sr, tau = ALPHAS["240k_75us"]
    nchan = 4
    x = torch.randn((nchan, n + 2, 2), device="cuda")
    a, b = ops.Deemp(sr, tau, nchan=nchan), ops.Deemp(sr, tau, nchan=nchan)
    want = a.process_batch(x, count=n)
    assert a.last_kernel()["name"] == form_of(n)
    buf = x.clone()
    got = b.process_batch(buf, buf, count=n)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert [a.get_state(c) for c in range(nchan)] == [b.get_state(c) for c in range(nchan)]
    # the same buffer with another stride is not "in place"
    L = capi.load()
    assert L.qdsp_hip_deemp_process_batch_dev(b._h, buf.data_ptr(), 100, n + 2, buf.data_ptr(), n + 4, None) == EINVAL


def test_same_call_twice_gives_the_same_bits(torch):
    sr, tau = ALPHAS["tiny"]
    nchan, n = 64, 100_003
    x = torch.randn((nchan, n), device="cuda")
    d = ops.Deemp(sr, tau, stereo=False, nchan=nchan)
    d.set_state(0.125)
    y1 = d.process_batch(x).clone()
    assert d.last_kernel()["name"] == SCAN
    d.set_state(0.125)
    y2 = d.process_batch(x)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))


# ---- 8. argument errors, harness helpers ---------------------------------------------------------------------------------------------
def test_argument_errors(torch):
    L = capi.load()
    h = C.c_void_p()
    for kind, nchan, mb in ((2, 1, 10), (-1, 1, 10), (0, 0, 10), (1, 70_000, 10), (0, 1, -5)):
        assert L.qdsp_hip_deemp_create(C.byref(h), 0, kind, nchan, mb) == EINVAL
    two = ops.Deemp(48e3, 50e-6, nchan=2, max_block=100)
    one = ops.Deemp(48e3, 50e-6, max_block=100)
    mono = ops.Deemp(48e3, 50e-6, stereo=False, max_block=100)
    x = np.zeros((101, 2), np.float32)
    y = np.zeros((101, 2), np.float32)
    assert L.qdsp_hip_deemp_process(one._h, x.ctypes.data, 101, y.ctypes.data) == ESIZE
    assert L.qdsp_hip_deemp_process(one._h, x.ctypes.data, -1, y.ctypes.data) == EINVAL
    assert L.qdsp_hip_deemp_process(two._h, x.ctypes.data, 10, y.ctypes.data) == EINVAL            # host path: one channel
    assert L.qdsp_hip_deemp_process_ex(one._h, x.ctypes.data, 7, 10, y.ctypes.data, 0) == EINVAL
    assert L.qdsp_hip_deemp_process_ex(one._h, x.ctypes.data, 0, 10, y.ctypes.data, 3) == EINVAL    # deferred without an event
    inf, nan = float("inf"), float("nan")
    for sr, tau in ((0.0, 50e-6), (-48e3, 50e-6), (inf, 50e-6), (nan, 50e-6), (48e3, -1e-6), (48e3, inf), (48e3, nan)):
        assert L.qdsp_hip_deemp_set(one._h, 0, sr, tau) == EINVAL, (sr, tau)
    assert L.qdsp_hip_deemp_set(two._h, 2, 48e3, 50e-6) == EINVAL
    assert L.qdsp_hip_deemp_set(two._h, -1, 48e3, 0.0) == 0 and two.alpha(1) == 1
    p = C.c_float()
    assert L.qdsp_hip_deemp_get_state(two._h, 2, C.byref(p), C.byref(p)) == EINVAL
    assert L.qdsp_hip_deemp_get_state(one._h, 0, C.byref(p), None) == EINVAL
    assert L.qdsp_hip_deemp_get_state(mono._h, 0, C.byref(p), None) == 0
    assert L.qdsp_hip_deemp_get_alpha(two._h, -1, C.byref(p)) == EINVAL
    assert L.qdsp_hip_deemp_set_state(two._h, 5, 0.0, 0.0) == EINVAL
    xt = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    yt = torch.zeros((1000, 2), dtype=torch.float32, device="cuda")
    bd = L.qdsp_hip_deemp_process_batch_dev
    assert bd(two._h, xt.data_ptr(), 400, 399, yt.data_ptr(), 400, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 400, 400, yt.data_ptr(), 300, None) == EINVAL
    assert bd(two._h, xt.data_ptr() + 4, 10, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), 10, 10, yt.data_ptr() + 4, 10, None) == EINVAL
    assert bd(mono._h, xt.data_ptr() + 2, 10, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, xt.data_ptr(), -1, 10, yt.data_ptr(), 10, None) == EINVAL
    assert bd(two._h, None, 10, 10, yt.data_ptr(), 10, None) == EINVAL
    # handle kinds do not mix
    fm = ops.FmDemod(250e3, 75e3)
    ssb = ops.SsbDemod(48_000.0, 3_000.0, 0)
    assert L.qdsp_hip_deemp_process_dev(fm._h, xt.data_ptr(), 10, yt.data_ptr(), None) == EINVAL
    assert L.qdsp_hip_deemp_process_dev(ssb._h, xt.data_ptr(), 10, yt.data_ptr(), None) == EINVAL
    assert L.qdsp_hip_deemp_reset(fm._h) == EINVAL and L.qdsp_hip_deemp_set_bypass(fm._h, 1) == EINVAL
    assert L.qdsp_hip_demod_process_dev(one._h, xt.data_ptr(), 10, yt.data_ptr(), None) == EINVAL
    assert L.qdsp_hip_demod_reset(one._h) == EINVAL
    assert L.qdsp_hip_ssb_cf32_process_dev(one._h, xt.data_ptr(), 10, yt.data_ptr(), None) == EINVAL
    torch.cuda.synchronize()


def test_done_event_and_time(torch):
    L = capi.load()
    ev = C.c_void_p()
    capi.check(L.qdsp_hip_event_create(0, C.byref(ev)))
    for stereo in (True, False):
        d = ops.Deemp(48e3, 50e-6, stereo=stereo)
        x = torch.randn((1 << 20, 2) if stereo else (1 << 20,), device="cuda")
        assert L.qdsp_hip_set_done_event(d._h, ev) == 0
        assert d.time_dev(x, torch.empty_like(x), 3) > 0
        assert d.last_kernel()["name"] == SCAN and d.last_kernel()["grid"] == 512
    capi.check(L.qdsp_hip_event_destroy(ev))


# ---- 9. the block graph ------------------------------------------------------------------------------------------------------------------
N, BLOCK, DECIM = 240_000, 24_000, 10
VFO_ARGS = ["300000", "2400000", "240000", "200000"]    # offset, inSR, outSR, bandwidth: 2.4 Msps -> 240 ksps


@pytest.fixture(scope="module")
def graph(tmp_path_factory):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL, timeout=300)
    d = tmp_path_factory.mktemp("deempgraph")
    O.synth_iq(0, N, seed=42).tofile(d / "x.cf32")
    subprocess.run([BIN, "vfo", str(d / "x.cf32"), str(d / "v.cf32"), str(BLOCK)] + VFO_ARGS, check=True, timeout=180,
                   capture_output=True, text=True)
    v = np.fromfile(d / "v.cf32", dtype=np.complex64)
    assert len(v) == N // DECIM
    return d, v


@pytest.mark.parametrize("link", ["dev", "host"])
def test_fm_then_bfmdeemp_blocks(graph, link):
    d, v = graph
    out = d / f"deemp_{link}.bin"
    r = subprocess.run([BIN, "deemp", link, str(d / "x.cf32"), str(out), str(BLOCK)] + VFO_ARGS + ["75000", "50e-6"],
                       check=True, timeout=180, capture_output=True, text=True)
    assert "graph ok" in r.stdout and f"{link if link == 'host' else 'device'} link" in r.stdout
    y = np.fromfile(out, dtype=np.float32).reshape(-1, 2)
    assert len(y) == len(v)
    vb = BLOCK // DECIM
    fm = ops.FmDemod(240_000.0, 75_000.0, stereo=True, max_block=vb)
    de = ops.Deemp(240_000.0, 50e-6, max_block=vb)
    al = deemp_alpha(240_000.0, 50e-6)
    st = np.zeros(2, LD)
    for a in range(0, len(v), vb):          # one run() per VFO output block
        f = fm.process(v[a:a + vb])
        assert _same_bits(y[a:a + vb], de.process(f)), a
        st = meets_bound(y[a:a + vb], f, al, st, f"{link} block at {a}")


# ---- 10. a full-size call ----------------------------------------------------------------------------------------------------------------
def test_full_size_call(torch):
    n = (1 << 28) + 12_345
    sr, tau = ALPHAS["240k_75us"]
    al = deemp_alpha(sr, tau)
    b = float(np.float32(np.float32(1) - al))
    run_in = int(math.ceil(-60 * math.log(2) / math.log(b))) + 1       # b^run_in < 2^-60: the filter has forgotten what came before
    assert b ** run_in < 2.0 ** -60
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand(n, device="cuda", generator=g) - 0.25
    d = ops.Deemp(sr, tau, stereo=False)
    y = d.process(x)
    torch.cuda.synchronize()
    assert d.last_kernel()["name"] == SCAN
    for a in (0, n // 2 - 777, n - 70_001):
        w = min(n, a + 70_001)
        s = max(a - run_in, 0)
        xw = x[s:w].cpu().numpy()
        # started from 0 a run-in before the window: the filter forgets, the state there (|y| <= max |x| = 0.75) has decayed
        # to less than 0.75 * 2^-60 by the window's first sample
        truth, _ = deemp_exact(xw, al)
        env = deemp_envelope(xw, al)
        err = np.abs(y[a:w].cpu().numpy().astype(LD) - truth[a - s:])
        bound = deemp_bound(truth[a - s:], env[a - s:]) + (LD(2.0) ** -60 if s else LD(0))
        assert np.all(err <= bound), (a, float(np.max(err / bound)))
    assert _same_bits([d.get_state()], y[-1:].cpu().numpy())
    del x, y
    torch.cuda.empty_cache()
