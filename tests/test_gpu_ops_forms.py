"""The three entry forms of every per-row operator class of qdsp_amd.ops -- a numpy array (the host entry point), a 1-D tensor
(*_process_dev) and a 2-D tensor (`process_batch`) -- at the sizes where the PYTHON path can go wrong, not the kernels': 1 and 2
channels, calls of 0, 1 and 70 samples, rows padded by 3 samples, and a batch passed with count = shape[1] - 1.  Nothing here has
a numeric reference: every result is compared bit for bit with the first call of a fresh handle of the same kind through the same
form, computed once per case.  Per class and channel count:

  (a) a call of 0 samples returns an empty result of the class's output dtype and trailing shape on each form and does not move
      the state: the next call equals a fresh handle's first call;
  (b) a caller's `out` (and `counts`) larger than needed comes back as a view of that very storage of the documented extent, with
      nothing written beyond it (a sentinel fill); padded input and output rows and an explicit `count` give the same values;
  (c) a wrong input dtype, a wrong number of rows, a non-unit inner stride, a short `out`, an `out` of the wrong dtype, a `counts`
      or `in_counts` of the wrong dtype or length, and the 1-D form on a handle of more than one channel (where the class reads
      it as one row) raise AssertionError and launch nothing: the next call again equals a fresh handle's first call."""
import numpy as np
import pytest

from qdsp_amd import capi, ops

pytestmark = pytest.mark.gpu

C64, F32, U8 = np.complex64, np.float32, np.uint8
MAXB, N, PAD = 256, 70, 3
SYNC = np.array([1, 0, 1, 1], U8)
FRAME = 16
FIXED, RET, COUNTS = "n", "returned", "counts"      # how many outputs a call yields: n / out_size(n), the call returns the count /
#                                                     out_size(n) slots and a count per row


class Case:
    """One kind of one class: how to make it, the sample type of each side (dtype and trailing shape), its output-count rule,
    whether its batch form takes `in_counts`, whether its 1-D form reads more than one channel's rows back to back (`flat`), whether the library has a
    batch entry point for it (`batch`; SsbDemod has none: its process_batch checks its arguments and the C call then refuses)."""

    def __init__(self, name, make, din, dout, tin=(), tout=(), rule=FIXED, in_counts=False, flat=False, nchans=(1, 2), batch=True):
        self.name, self.make, self.din, self.dout, self.tin, self.tout = name, make, din, dout, tin, tout
        self.rule, self.in_counts, self.flat, self.nchans, self.batch = rule, in_counts, flat, nchans, batch


TAPS5 = np.array([0.1, -0.2, 0.5, 0.3, -0.1], F32)
CASES = [
    Case("fm", lambda n: ops.FmDemod(250e3, 75e3, nchan=n, max_block=MAXB), C64, F32, flat=True),
    Case("fm_stereo", lambda n: ops.FmDemod(250e3, 75e3, stereo=True, nchan=n, max_block=MAXB), C64, F32, tout=(2,), flat=True),
    Case("am", lambda n: ops.AmDemod(nchan=n, max_block=MAXB), C64, F32, flat=True),
    Case("ssb", lambda n: ops.SsbDemod(48_000.0, 3_000.0, 0, max_block=MAXB), C64, F32, flat=True, nchans=(1,), batch=False),
    Case("deemp_mono", lambda n: ops.Deemp(48e3, 50e-6, stereo=False, nchan=n, max_block=MAXB), F32, F32),
    Case("deemp_stereo", lambda n: ops.Deemp(48e3, 50e-6, stereo=True, nchan=n, max_block=MAXB), F32, F32, tin=(2,), tout=(2,)),
    Case("squelch", lambda n: ops.Squelch(-50.0, nchan=n, max_block=MAXB), C64, C64),
    Case("agc", lambda n: ops.Agc(1.0, 48e3, nchan=n, max_block=MAXB), F32, F32),
    Case("stereo_fm", lambda n: ops.StereoFmDemod(250e3, 75e3, nchan=n, pilot_taps=TAPS5, max_block=MAXB), C64, F32, tout=(2,), flat=True),
    Case("ffagc_real", lambda n: ops.FeedForwardAgc("real", nchan=n, max_block=MAXB, window=8), F32, F32, rule=RET),
    Case("ffagc_complex", lambda n: ops.FeedForwardAgc("complex", nchan=n, max_block=MAXB, window=8), C64, C64, rule=RET),
    Case("cagc", lambda n: ops.ComplexAgc(nchan=n, max_block=MAXB), C64, C64),
    Case("costas", lambda n: ops.CostasLoop(4, 0.01, nchan=n, max_block=MAXB), C64, C64),
    Case("mmcr_real", lambda n: ops.MmClockRecovery("real", 4.0, nchan=n, max_block=MAXB), F32, F32, rule=COUNTS),
    Case("mmcr_complex", lambda n: ops.MmClockRecovery("complex", 4.0, nchan=n, max_block=MAXB), C64, C64, rule=COUNTS),
    Case("rowfir_real", lambda n: ops.RowFir("real", TAPS5, nchan=n, max_block=MAXB), F32, F32),
    Case("rowfir_complex", lambda n: ops.RowFir("complex", TAPS5, nchan=n, max_block=MAXB), C64, C64),
    Case("delay_imag", lambda n: ops.DelayImag(nchan=n, max_block=MAXB), C64, C64),
    Case("psk", lambda n: ops.PskDemod(4, False, 48000.0, 12000.0, nchan=n, max_block=MAXB), C64, C64, rule=COUNTS),
    Case("msk", lambda n: ops.MskDemod(48000.0, 6000.0, 12000.0, nchan=n, max_block=MAXB), C64, F32, rule=COUNTS),
    Case("threshold", lambda n: ops.Threshold(nchan=n, max_block=MAXB), F32, U8, in_counts=True),
    Case("deframer_bytes", lambda n: ops.Deframer(FRAME, SYNC, "bytes", nchan=n, max_block=MAXB), U8, U8, rule=COUNTS, in_counts=True),
    Case("deframer_float", lambda n: ops.Deframer(FRAME, SYNC, "float", nchan=n, max_block=MAXB), F32, U8, rule=COUNTS, in_counts=True),
]
PARAMS = [pytest.param(c, n, id=f"{c.name}-{n}") for c in CASES for n in c.nchans]


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def rows(case, nchan, n):
    """(nchan, n) + case.tin input samples; the deframer kinds get the sync word every FRAME + 4 bits, so that frames come out."""
    rng = np.random.default_rng(len(case.name) * 100 + nchan)
    shape = (nchan, n) + case.tin
    if case.name.startswith("deframer"):
        bits = rng.integers(0, 2, shape).astype(U8)
        for s in range(0, n - len(SYNC), FRAME + len(SYNC)):
            bits[:, s:s + len(SYNC)] = SYNC
        return bits if case.din is U8 else ((bits.astype(F32) * 2 - 1) * F32(0.75)).astype(F32)
    if case.din is C64:
        return (0.5 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(C64)
    return (0.5 * rng.standard_normal(shape)).astype(F32)


def other(dt):
    return F32 if dt is not F32 else C64


SENTINEL = {C64: -77.25 + 3j, F32: -77.25, U8: 0xA5}


class Forms:
    """The calls of one (case, nchan), results brought to the host: a list of arrays whose bits are compared (for a count per row:
    the counts, then each row's counted part)."""

    def __init__(self, torch, case, nchan):
        self.t, self.case, self.nchan = torch, case, nchan
        self.per = getattr(self.fresh(), "frame_bytes", 1)      # elements per output: a Deframer's frame is frame_bytes of them

    def fresh(self):
        return self.case.make(self.nchan)

    def dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).cuda()

    def tdt(self, dt):
        return getattr(self.t, np.dtype(dt).name)

    def full(self, shape, dt):
        return self.t.full(tuple(shape), SENTINEL[dt], dtype=self.tdt(dt), device="cuda")

    def val(self, r):
        if isinstance(r, tuple):
            out, counts = r[0].cpu().numpy(), r[1].cpu().numpy()
            assert counts.dtype == np.int32 and counts.shape == (self.nchan,), (counts.dtype, counts.shape)
            return [counts] + [out[c, :counts[c] * self.per].copy() for c in range(self.nchan)]
        return [r.cpu().numpy() if hasattr(r, "cpu") else np.asarray(r)]

    def cap(self, n):
        """The slots per row a call of n samples needs, in elements of the output dtype."""
        return n if self.case.rule == FIXED else self.fresh().out_size(n) * self.per


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("case,nchan", PARAMS)
def test_three_forms(torch, case, nchan):
    F = Forms(torch, case, nchan)
    tdt_in, tdt_out = F.tdt(case.din), F.tdt(case.dout)
    X = rows(case, nchan, N + 1)
    x = np.ascontiguousarray(X[:, :N])
    xd, one_row = F.dev(x), nchan == 1 or case.flat
    cap, cap1, cap0 = F.cap(N), F.cap(1), F.cap(0)
    assert cap >= 2 and cap0 <= cap1 <= cap, (cap0, cap1, cap)
    flat_in = xd.reshape((nchan * N,) + case.tin)           # the 1-D form's input: the one row, or the rows back to back
    bad = []

    def check(ok, what):
        if not ok:
            bad.append(what)

    # the first call of a fresh handle through each form: what everything below is compared with
    ref_batch = F.val(F.fresh().process_batch(xd)) if case.batch else None
    ref_dev = F.val(F.fresh().process(flat_in)) if one_row else None
    ref_host = F.val(F.fresh().process(x[0])) if nchan == 1 else None
    if case.batch:
        r1 = F.fresh().process(xd[:, :1].contiguous())
        rows1 = r1[0] if isinstance(r1, tuple) else r1
        check(rows1.dtype == tdt_out and tuple(rows1.shape) == (nchan, cap1) + case.tout, f"a call of 1 sample: {rows1.dtype} {tuple(rows1.shape)}")
        if case.rule == FIXED and one_row:
            check(same([ref_dev[0].reshape((nchan, N) + case.tout)], ref_batch), "the 1-D form and the batch form differ")
    else:
        with pytest.raises(capi.QdspHipError):
            F.fresh().process_batch(xd)

    def unmoved(op, what):
        got, want = (F.val(op.process_batch(xd)), ref_batch) if case.batch else (F.val(op.process(flat_in)), ref_dev)
        check(same(got, want), f"{what}: the next call is not a fresh handle's first call")

    # ---- (a) a call of 0 samples, each form
    if case.batch:
        op = F.fresh()
        r0 = op.process(torch.empty((nchan, 0) + case.tin, dtype=tdt_in, device="cuda"))
        if case.rule == COUNTS:
            check(tuple(r0[0].shape) == (nchan, cap0) and r0[0].dtype == tdt_out and not r0[1].cpu().numpy().any(), f"count 0, batch: {tuple(r0[0].shape)} {r0[0].dtype}")
        else:
            check(tuple(r0.shape) == (nchan, 0) + case.tout and r0.dtype == tdt_out, f"count 0, batch: {tuple(r0.shape)} {r0.dtype}")
        unmoved(op, "count 0, batch")
    empty_shape = (0, F.per) if F.per > 1 else (0,) + case.tout
    if one_row:
        op = F.fresh()
        r0 = op.process(torch.empty((0,) + case.tin, dtype=tdt_in, device="cuda"))
        check(tuple(r0.shape) == empty_shape and r0.dtype == tdt_out, f"count 0, 1-D: {tuple(r0.shape)} {r0.dtype}")
        check(same(F.val(op.process(flat_in)), ref_dev), "count 0, 1-D: the next call is not a fresh handle's first call")
    if nchan == 1:
        op = F.fresh()
        r0 = op.process(np.empty((0,) + case.tin, dtype=case.din))
        check(isinstance(r0, np.ndarray) and r0.shape == empty_shape and r0.dtype == case.dout, f"count 0, numpy: {r0.shape} {r0.dtype}")
        check(same(F.val(op.process(x[0])), ref_host), "count 0, numpy: the next call is not a fresh handle's first call")

    # ---- (b) a caller's out: the batch form, rows padded on both sides, `count` below shape[1]
    if case.batch:
        buf = torch.zeros((nchan, N + 1 + PAD) + case.tin, dtype=tdt_in, device="cuda")
        buf[:, :N + 1] = F.dev(X)
        xin = buf[:, :N + 1]                                     # stride(0) = count + 1 + PAD samples; count = shape[1] - 1
        out = F.full((nchan, cap + 5) + case.tout, case.dout)
        kw = {"counts": torch.full((nchan,), -1, dtype=torch.int32, device="cuda")} if case.rule == COUNTS else {}
        r = F.fresh().process_batch(xin, out, count=N, **kw)
        got = r[0] if isinstance(r, tuple) else r
        extent = cap if case.rule != RET else ref_batch[0].shape[1]
        check(got.data_ptr() == out.data_ptr() and got.stride() == out.stride() and tuple(got.shape) == (nchan, extent) + case.tout,
              f"out, batch: not the (nchan, {extent}) view of the caller's rows: {tuple(got.shape)} {got.stride()}")
        check(bool((out[:, cap:] == SENTINEL[case.dout]).all()), "out, batch: written beyond the documented extent")
        check(same(F.val(r), ref_batch), "out, batch (padded rows, count = shape[1] - 1): not the contiguous call's values")
        if kw:
            check(r[1].data_ptr() == kw["counts"].data_ptr(), "out, batch: the caller's counts did not come back")
        padded = torch.zeros((nchan, N + PAD) + case.tin, dtype=tdt_in, device="cuda")
        padded[:, :N] = xd
        check(same(F.val(F.fresh().process(padded[:, :N])), ref_batch), "padded rows through process(): not the contiguous call's values")
    if one_row:                                              # ... and the 1-D form
        out = F.full((nchan * cap + 5,) + case.tout, case.dout)
        r = F.fresh().process(flat_in, out)
        check(r.data_ptr() == out.data_ptr() and same(F.val(r), ref_dev), "out, 1-D: not a view of the caller's storage with the call's values")
        check(bool((out[nchan * cap:] == SENTINEL[case.dout]).all()), "out, 1-D: written beyond the documented extent")

    # ---- (c) refusals: AssertionError before anything is launched
    op = F.fresh()

    def refused(what, call):
        try:
            call()
        except AssertionError:
            return
        except Exception as e:  # noqa: BLE001
            bad.append(f"{what}: {type(e).__name__} instead of AssertionError: {e}")
            return
        bad.append(f"{what}: accepted")

    wrong_in = torch.zeros((nchan, N) + case.tin, dtype=F.tdt(other(case.din)), device="cuda")
    refused("input dtype, batch", lambda: op.process_batch(wrong_in))
    refused("rows", lambda: op.process_batch(torch.zeros((nchan + 1, N) + case.tin, dtype=tdt_in, device="cuda")))
    refused("inner stride", lambda: op.process_batch(torch.zeros((nchan, 2 * N) + case.tin, dtype=tdt_in, device="cuda")[:, ::2]))
    refused("short out, batch", lambda: op.process_batch(xd, F.full((nchan, cap - 1) + case.tout, case.dout)))
    refused("out dtype, batch", lambda: op.process_batch(xd, F.full((nchan, cap) + case.tout, other(case.dout))))
    for name in (["counts"] if case.rule == COUNTS else []) + (["in_counts"] if case.in_counts else []):
        refused(f"{name} dtype", lambda: op.process_batch(xd, **{name: torch.zeros(nchan, dtype=torch.int64, device="cuda")}))
        refused(f"{name} length", lambda: op.process_batch(xd, **{name: torch.zeros(nchan + 1, dtype=torch.int32, device="cuda")}))
    if one_row:
        refused("input dtype, 1-D", lambda: op.process(wrong_in.reshape((nchan * N,) + case.tin)))
        refused("short out, 1-D", lambda: op.process(flat_in, F.full((nchan * cap - 1,) + case.tout, case.dout)))
        refused("out dtype, 1-D", lambda: op.process(flat_in, F.full((nchan * cap,) + case.tout, other(case.dout))))
    else:
        refused("1-D form, more than one channel", lambda: op.process(flat_in))
    unmoved(op, "refusals")
    assert not bad, f"{case.name}, nchan {nchan}:\n  " + "\n  ".join(bad)
