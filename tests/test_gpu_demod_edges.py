"""The demodulators' kernels (qdsp_amd/csrc/demod.hip) at their edges, against the restatements tests/test_demod_cpu.py pins:
FM mono and stereo at every count next to a lane (8 samples) and a workgroup (2048) in the four row layouts that each switch
one input of the 16-byte-access decision off, the carried phase after each; AM against the two-candidate rule of
`am_candidates` (|x| bit for bit, the mean within an ulp of exact) up to and past the 1024-partials cap on a batch;
non-finite samples confined to their channel; the state calls on a batch in mid-stream; SSB at odd and even counts, on
its scalar path, with the NCO calls in mid-stream and across the kernel's grid-stride loop.  Every output buffer is
pre-filled with a sentinel: what a call does not own keeps it."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle as O
from qdsp_amd import capi, ops
from test_demod_cpu import (_same_bits, am_cancellation_row, am_candidates_of_mag, am_mag, am_ref, am_row_ok, fm_ref_rows,
                            phasor_speeds)

pytestmark = pytest.mark.gpu

SR = 250_000.0
DEVS = np.asarray([75_000.0, 12_500.0, 3_000.0], np.float32)
EINVAL = -10001
SENT = 0x4B1DF00D                      # a finite float (1.0350605e7) no demodulator output of these inputs has
LANE, TILE = 8, 2048                   # kDemodSpl, kDemodNT * kDemodSpl
AM_CAP = 1024 * TILE                   # kAmMaxParts workgroups: both AM kernels loop above this many samples per channel
FM_COUNTS = [1, 2, 7, 8, 9, 15, 16, 17, 2039, 2040, 2041, 2047, 2048, 2049, 2055, 2056, 2057, 4095, 4096, 4097]
AM_COUNTS = [1, 2, 7, 8, 9, 2047, 2048, 2049, 4097]
AM_BIG_COUNTS = [AM_CAP, AM_CAP + 1, AM_CAP + 2047, AM_CAP + 2049, 2 * AM_CAP + 5]
SECOND = 19                            # the call after: its first output shows the carried phase
LAYOUTS = ("aligned", "in_stride_odd", "base_offset", "out_stride_off")


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def rand_rows(nchan, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nchan, n)) + 1j * rng.standard_normal((nchan, n))).astype(np.complex64)


def geometry(layout, width, stereo):
    """(in_stride, out_stride, in_offset, out_offset) in samples / output elements for rows of up to `width` samples.  Each
    layout but the first fails one input of the kernels' `vec` rule and stays within the header's alignment (input 8 bytes;
    output 4, stereo 8)."""
    w4 = (width + 3) // 4 * 4 + 4
    ins, outs, io, oo = w4, w4, 0, 0
    if layout == "in_stride_odd":
        ins += 1
    elif layout == "base_offset":
        io, oo = 1, 1                  # 8 bytes; 4 bytes (stereo: 8)
    elif layout == "out_stride_off":
        outs += 1 if stereo else 2     # odd float2 rows; float rows = 2 (mod 4)
    else:
        assert layout == "aligned"
    return ins, outs, io, oo


class Batch:
    """`nchan` rows on the device in one of the four layouts; the output, guard bands included, starts as SENT everywhere.
    run() launches one call, checks that nothing outside the rows' first max(count so far) elements has changed, and returns
    the call's rows as (nchan, count) float32 (stereo: (nchan, count, 2))."""

    def __init__(self, torch, nchan, width, layout, stereo=False):
        self.torch, self.nchan, self.of = torch, nchan, 2 if stereo else 1
        self.ins, self.outs, self.io, self.oo = geometry(layout, width, stereo)
        self.x = torch.zeros(self.io + nchan * self.ins + 8, dtype=torch.complex64, device="cuda")
        self.y = torch.full(((self.oo + nchan * self.outs + 64) * self.of,), SENT, dtype=torch.int32, device="cuda")
        assert self.x.data_ptr() % 16 == 0 and self.y.data_ptr() % 16 == 0
        self.written = 0
        self.kept = None

    def load(self, rows):
        rows = rows if self.torch.is_tensor(rows) else self.torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        n = rows.shape[1]
        assert rows.shape[0] == self.nchan and n <= self.ins
        self.x[self.io:self.io + self.nchan * self.ins].view(self.nchan, self.ins)[:, :n] = rows
        return n

    def run(self, op, rows):
        n = self.load(rows)
        assert n <= self.outs
        rc = capi.load().qdsp_hip_demod_process_batch_dev(op._h, self.x.data_ptr() + 8 * self.io, n, self.ins,
                                                          self.y.data_ptr() + 4 * self.of * self.oo, self.outs,
                                                          self.torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        h = self.y.cpu().numpy()
        lo, hi = self.oo * self.of, (self.oo + self.nchan * self.outs) * self.of
        body = h[lo:hi].reshape(self.nchan, self.outs, self.of)
        before = self.written
        self.written = max(self.written, n)
        assert np.all(h[:lo] == SENT), "wrote before the first row"
        assert np.all(h[hi:] == SENT), "wrote past the last row"
        assert np.all(body[:, self.written:] == SENT), "wrote between count and out_stride"
        if before > n:                                 # the longer call before: its outputs past this count stand
            assert np.array_equal(body[:, n:before], self.kept[:, n:before]), "wrote past count"
        self.kept = body[:, :self.written].copy()
        y = body[:, :n].copy().view(np.float32)
        return y if self.of == 2 else y[:, :, 0]


# ---- 1. FM: counts x layouts, bit for bit ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fm_rows():
    return rand_rows(3, FM_COUNTS[-1] + SECOND, 41)


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
@pytest.mark.parametrize("count", FM_COUNTS)
def test_fm_counts_and_layouts(torch, fm_rows, count, stereo):
    for nchan in (1, 3):
        sp = phasor_speeds(SR, DEVS[:nchan])
        x1, x2 = fm_rows[:nchan, :count], fm_rows[:nchan, count:count + SECOND]
        want1, p1 = fm_ref_rows(x1, sp)
        want2, p2 = fm_ref_rows(x2, sp, p1)
        for layout in LAYOUTS:
            d = ops.FmDemod(SR, DEVS[:nchan], stereo=stereo, nchan=nchan, max_block=0)
            b = Batch(torch, nchan, max(count, SECOND), layout, stereo)
            for k, (x, want, p) in enumerate(((x1, want1, p1), (x2, want2, p2))):
                y = b.run(d, x)
                where = (count, nchan, layout, k)
                if stereo:
                    assert _same_bits(y[:, :, 0], want) and _same_bits(y[:, :, 1], want), where
                else:
                    assert _same_bits(y, want), where
                assert _same_bits([d.get_phase(c) for c in range(nchan)], p), where
            assert d.last_kernel()["name"] == "fm_demod_kernel"


def test_fm_widest_batch(torch):
    nchan, count = 65_535, 9                           # kDemodMaxChan: grid.y at its limit
    devs = (1_000.0 + np.arange(nchan)).astype(np.float32)
    sp = phasor_speeds(SR, devs)
    assert len(np.unique(sp)) > 65_000
    x = rand_rows(nchan, count + 2, 43)
    d = ops.FmDemod(SR, devs, nchan=nchan, max_block=0)
    b = Batch(torch, nchan, count, "aligned")
    want, p = fm_ref_rows(x[:, :count], sp)
    assert _same_bits(b.run(d, x[:, :count]), want)
    assert _same_bits([d.get_phase(c) for c in (0, 1, 32_768, 65_534)], p[[0, 1, 32_768, 65_534]])
    assert _same_bits(b.run(d, x[:, count:]), fm_ref_rows(x[:, count:], sp, p)[0])
    h = C.c_void_p()
    assert capi.load().qdsp_hip_demod_create(C.byref(h), 0, 0, nchan + 1, 0) == EINVAL and not h


# ---- 2. AM: |x| bit for bit, one mean per row within an ulp of exact -------------------------------------------------------
def am_rows(nchan, n, seed):
    """Unit noise; the cancellation row; noise at another scale."""
    x = rand_rows(nchan, n, seed)
    x[1] = am_cancellation_row(n, seed + 1)
    if nchan > 2:
        x[2] *= np.float32(37.5)
    return x


def check_am(y, mags, where, cands=None):
    for c in range(len(mags)):
        cc = cands[c] if cands else am_candidates_of_mag(mags[c])
        if not am_row_ok(y[c], cc):
            m = mags[c]
            got = np.float32(np.median(m.astype(np.float64) - y[c].astype(np.float64)))
            bad = int(np.sum((m - got).astype(np.float32).view(np.uint32) != y[c].view(np.uint32)))
            pytest.fail(f"{where} channel {c}: mean about {got!r}, candidates {[a for a, _ in cc]}, {bad} samples differ from |x| - that")


@pytest.fixture(scope="module")
def am_small():
    x = am_rows(3, AM_COUNTS[-1] + SECOND, 51)
    return x, am_mag(x)


@pytest.mark.parametrize("count", AM_COUNTS)
def test_am_counts_and_layouts(torch, am_small, count):
    x, m = am_small
    for layout in LAYOUTS:
        d = ops.AmDemod(nchan=3, max_block=0)
        b = Batch(torch, 3, max(count, SECOND), layout)
        check_am(b.run(d, x[:, :count]), m[:, :count], (count, layout))
        assert d.last_kernel()["name"] == "am_sub_kernel" and d.last_kernel()["grid"] == -(-count // TILE)
        # no state: the next call on the handle subtracts its own mean
        check_am(b.run(d, x[:, count:count + SECOND]), m[:, count:count + SECOND], (count, layout, "second call"))


@pytest.fixture(scope="module")
def am_big(torch):
    x = am_rows(2, AM_BIG_COUNTS[-1], 61)
    x[0] *= np.float32(3)
    return torch.from_numpy(x).cuda(), am_mag(x)


@pytest.mark.parametrize("count", AM_BIG_COUNTS)
def test_am_around_the_partials_cap(torch, am_big, count):
    xt, m = am_big
    mags = m[:, :count]
    cands = [am_candidates_of_mag(r) for r in mags]
    for layout in ("aligned", "base_offset"):          # 16-byte and scalar accesses in both kernels' loops
        d = ops.AmDemod(nchan=2, max_block=0)
        b = Batch(torch, 2, count, layout)
        y = b.run(d, xt[:, :count])
        assert d.last_kernel()["grid"] == 1024
        check_am(y, mags, (count, layout), cands)
        del b
    check_am(Batch(torch, 2, 4097, "aligned").run(d, xt[:, 5:4102]), m[:, 5:4102], (count, "the call after"))


# ---- 3. non-finite samples stay in their channel ---------------------------------------------------------------------------
POISON = [complex(np.nan, 0.5), complex(np.inf, 0.5), complex(-np.inf, 0.5), complex(0.5, np.nan), complex(0.5, np.inf), complex(0.5, -np.inf)]


def poison_positions(count):
    return [0, LANE - 1, LANE, TILE - 1, TILE, count - 1]


@pytest.mark.parametrize("count", [2049, 4096])
@pytest.mark.parametrize("kind", ["fm", "fm_stereo", "am"])
def test_non_finite_samples_do_not_cross_channels(torch, kind, count):
    stereo = kind == "fm_stereo"
    x = am_rows(3, count + SECOND, 71) if kind == "am" else rand_rows(3, count + SECOND, 71)
    sp = phasor_speeds(SR, DEVS)
    new = (lambda: ops.AmDemod(nchan=3, max_block=0)) if kind == "am" else (lambda: ops.FmDemod(SR, DEVS, stereo=stereo, nchan=3, max_block=0))
    mono = (lambda y: y[:, :, 0]) if stereo else (lambda y: y)
    for layout in ("aligned", "in_stride_odd"):
        d = new()
        b = Batch(torch, 3, count, layout, stereo)
        clean1, clean2 = b.run(d, x[:, :count]), b.run(d, x[:, count:])
        for pos in poison_positions(count):
            for bad in POISON:
                where = (kind, count, layout, pos, bad)
                xp = x.copy()
                xp[1, pos] = bad
                d = new()
                b = Batch(torch, 3, count, layout, stereo)
                y1, y2 = b.run(d, xp[:, :count]), b.run(d, xp[:, count:])
                for c in (0, 2):
                    assert np.array_equal(y1[c].view(np.uint32), clean1[c].view(np.uint32)), where
                    assert np.array_equal(y2[c].view(np.uint32), clean2[c].view(np.uint32)), where
                if kind == "am":
                    with np.errstate(all="ignore"):
                        want1 = am_ref(xp[1, :count])[0]
                    assert not np.any(np.isfinite(want1))
                    assert np.array_equal(np.isnan(y1[1]), np.isnan(want1)) and _same_bits(y1[1], want1), where
                    assert np.array_equal(y2[1].view(np.uint32), clean2[1].view(np.uint32)), where
                    continue
                want1, p1 = fm_ref_rows(xp[1:2, :count], sp[1:2])
                want2, _ = fm_ref_rows(xp[1:2, count:], sp[1:2], p1)
                for ch in ((0, 1) if stereo else (0,)):
                    g1 = y1[1, :, ch] if stereo else y1[1]
                    g2 = y2[1, :, ch] if stereo else y2[1]
                    assert np.array_equal(np.isnan(g1), np.isnan(want1[0])) and _same_bits(g1, want1[0]), where
                    assert np.array_equal(np.isnan(g2), np.isnan(want2[0])) and _same_bits(g2, want2[0]), where
                assert not np.isfinite(want1[0, pos]) and int(np.sum(~np.isfinite(want1[0]))) == (2 if pos < count - 1 else 1)
                assert _same_bits([d.get_phase(c) for c in range(3)], fm_ref_rows(xp[:, count:], sp)[1]), where
                if pos == count - 1:                   # the poisoned phase is carried into one output of the next call
                    assert np.isnan(p1[0]) and not np.isfinite(mono(y2)[1, 0]) and np.all(np.isfinite(mono(y2)[1, 1:])), where
                else:
                    assert np.all(np.isfinite(mono(y2)[1])), where


# ---- 4. state calls on a batch in mid-stream -------------------------------------------------------------------------------
STATE_COUNTS = (2049, 5, 4097)
SCHEDULES = {
    "set_fm+set_phase(2), set_phase(-1)": ((("set_fm", 1, 48_000.0, 5_000.0), ("set_phase", 2, 1.25)), (("set_phase", -1, -2.5),)),
    "reset, set_fm(-1)+set_phase(0)": ((("reset",),), (("set_fm", -1, 192_000.0, 75_000.0), ("set_phase", 0, 3.0))),
}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_fm_state_calls_on_a_batch_mid_stream(torch, stereo, schedule):
    x = rand_rows(3, sum(STATE_COUNTS), 81)
    d = ops.FmDemod(SR, DEVS, stereo=stereo, nchan=3, max_block=0)
    sp, ph = phasor_speeds(SR, DEVS), np.zeros(3, np.float32)
    at = 0
    for k, n in enumerate(STATE_COUNTS):
        rows = x[:, at:at + n]
        at += n
        want, ph = fm_ref_rows(rows, sp, ph)
        y = Batch(torch, 3, n, LAYOUTS[k], stereo).run(d, rows)
        assert _same_bits(y[:, :, 0] if stereo else y, want) and (not stereo or _same_bits(y[:, :, 1], want)), (k, n)
        assert _same_bits([d.get_phase(c) for c in range(3)], ph), (k, n)
        for name, *args in (SCHEDULES[schedule][k] if k < 2 else ()):
            chans = slice(None) if args and args[0] < 0 else slice(args[0], args[0] + 1) if args else None
            if name == "set_fm":
                d.set_fm(args[1], args[2], args[0])
                sp = sp.copy()
                sp[chans] = phasor_speeds(args[1], [args[2]])[0]
            elif name == "set_phase":
                d.set_phase(args[1], args[0])
                ph = ph.copy()
                ph[chans] = np.float32(args[1])
            else:
                d.reset()
                ph = np.zeros(3, np.float32)
            assert _same_bits([d.get_phase(c) for c in range(3)], ph), (k, name, args)


# ---- 5. SSB ------------------------------------------------------------------------------------------------------------------
SSB_COUNTS = [1, 2, 3, 255, 256, 257, 511, 512, 513, 100_001]
SSB_INC = ops.ssb_phase_delta(48_000.0, 2_700.0, ops.SsbDemod.USB)


def ssb_run(torch, s, xt, in_off, out_off):
    """One qdsp_hip_ssb_cf32_process_dev call on buffers `in_off` samples / `out_off` floats past a 16-byte boundary."""
    n = xt.numel()
    xin = torch.zeros(n + in_off + 2, dtype=torch.complex64, device="cuda")
    xin[in_off:in_off + n] = xt
    y = torch.full((n + out_off + 64,), SENT, dtype=torch.int32, device="cuda")
    assert xin.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    rc = capi.load().qdsp_hip_ssb_cf32_process_dev(s._h, xin.data_ptr() + 8 * in_off, n, y.data_ptr() + 4 * out_off,
                                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    h = y.cpu().numpy()
    assert np.all(h[:out_off] == SENT) and np.all(h[out_off + n:] == SENT), "wrote outside [0, count)"
    return h[out_off:out_off + n].view(np.float32)


@pytest.fixture(scope="module")
def ssb_input(torch):
    return ops.synth_iq(SSB_COUNTS[-1] + SECOND, seed=91)


@pytest.mark.parametrize("volk_gain", [True, False], ids=["volk_gain", "unit_gain"])
@pytest.mark.parametrize("count", SSB_COUNTS)
def test_ssb_counts_and_alignments(torch, ssb_input, count, volk_gain):
    cuts = (ssb_input[:count], ssb_input[count:count + SECOND])
    xl = ops.Xlator(phase_inc=SSB_INC, max_block=0)
    xl.set_volk_gain(volk_gain)
    want = [xl.process(c).cpu().numpy().real for c in cuts]
    for in_off, out_off in ((0, 0), (1, 0), (0, 1)):   # 16-byte loads and 8-byte stores; input on 8 bytes; output on 4
        s = ops.SsbDemod(phase_inc=SSB_INC, max_block=0)
        s.set_volk_gain(volk_gain)
        for c, w in zip(cuts, want):
            assert _same_bits(ssb_run(torch, s, c, in_off, out_off), w), (count, in_off, out_off, len(w))
        assert s.last_kernel()["name"] == "ssb_demod_kernel"
        assert s.get_phase() == xl.get_phase()


def test_ssb_nco_calls_mid_stream(torch, ssb_input):
    s, xl = ops.SsbDemod(phase_inc=SSB_INC, max_block=0), ops.Xlator(phase_inc=SSB_INC, max_block=0)
    old = ops.SsbDemod(phase_inc=SSB_INC, max_block=0)          # never told of anything
    at = [0]

    def both(n, what):
        x = ssb_input[at[0]:at[0] + n]
        at[0] += n
        y, w = s.process(x).cpu().numpy(), xl.process(x).cpu().numpy()
        assert _same_bits(y, w.real), what
        assert s.get_phase() == xl.get_phase(), what
        return x, y

    x, y = both(1001, "first call")
    assert _same_bits(y, old.process(x).cpu().numpy())
    # set_phase_inc: from the next call on
    inc2 = ops.phase_delta(48_000.0, -7_000.0)
    s.set_phase_inc(*inc2)
    xl.set_phase_inc(*inc2)
    assert s.get_phase() == xl.get_phase() == old.get_phase()
    x, y = both(513, "after set_phase_inc")
    yo = old.process(x).cpu().numpy()
    assert y[0] == yo[0] and not np.array_equal(y[1:], yo[1:]) and s.get_phase() != old.get_phase()
    # set_phase: the call after it is a fresh block's first call from that phase
    s.set_phase(0.6, -0.8)
    xl.set_phase(0.6, -0.8)
    assert s.get_phase() == xl.get_phase() and abs(s.get_phase() - (0.6 - 0.8j)) < 1e-6
    x, y = both(255, "after set_phase")
    fresh = ops.SsbDemod(phase_inc=inc2, max_block=0)
    fresh.set_phase(0.6, -0.8)
    assert _same_bits(y, fresh.process(x).cpu().numpy()) and s.get_phase() == fresh.get_phase()
    # advance(n): n samples processed and thrown away
    s.advance(777)
    xl.process(ssb_input[at[0]:at[0] + 777])
    at[0] += 777
    assert s.get_phase() == xl.get_phase() != fresh.get_phase()
    both(300, "after advance")


def test_ssb_across_the_stride_loop(torch):
    n = (1 << 27) + 515                                # 256 Ki workgroups of 256 pairs cover 2^27 samples: 258 lanes go round again
    w = 70_001
    x = ops.synth_iq(n, seed=93)
    s, xl = ops.SsbDemod(phase_inc=SSB_INC, max_block=0), ops.Xlator(phase_inc=SSB_INC, max_block=0)
    s.set_volk_gain(True)
    xl.set_volk_gain(True)
    y = s.process(x)
    assert s.last_kernel()["grid"] == 256 * 1024
    z = xl.process(x)
    assert s.get_phase() == xl.get_phase()
    o = O.Xlator(1.0, 0.0, exact=True, volk_gain=True)
    o.delta[:] = SSB_INC
    dt = math.atan2(float(o.delta[1]), float(o.delta[0])) / (2.0 * math.pi)
    for a in (0, (1 << 26) - 35_000, (1 << 27) - 2 * w, (1 << 27) - w + 1, n - w):
        yw = y[a:a + w].cpu().numpy()
        assert _same_bits(yw, z[a:a + w].cpu().numpy().real), a
        a0 = a - a % 512                               # the oracle's gain sawtooth counts from the start of its call
        o.turns = C.c_double((a0 * dt) % 1.0)
        wo = o.process(x[a0:a + w].cpu().numpy())[a - a0:]
        err = float(np.abs(yw - wo.real).max())
        print(f"window at {a}: max |ssb - exact-phase oracle| = {err:.3e}")
        assert err < 6e-7, a
    del x, y, z
    torch.cuda.empty_cache()
