"""Running one call sequence three ways: the harness of tests/test_gpu_async_order.py (a plain helper module).

include/qdsp_hip.h promises that every *_process_dev is asynchronous on the caller's stream and that every setter, getter, reset
and call-time table rebuild waits for what is in flight.  On torch's default stream -- HIP's legacy null stream, handle 0, implicitly
ordered against every blocking copy and every other blocking stream -- and with a synchronise after every call, neither half of
that promise is exercised.  Here a scenario (a list of steps on fresh handles) runs

    "null"    on the default stream, torch.cuda.synchronize() after every step: the way the rest of the suite runs;
    "serial"  on a non-blocking side stream, stream.synchronize() after every step, the host side of every step timed;
    "async"   on the same kind of stream with NO synchronisation by the test until the end, and a bounded busy period (`hold`)
              queued in front of the calls, so that every step starts while earlier work is provably still queued.

A step is a `Call` (a process* call: asynchronous, returns device tensors) or a `Host` action (setter, getter, reset, configure,
close: must wait for the queue by itself).  A step that drains the queue -- every Host action does, and a Call that rebuilds a table
at call time does too -- leaves the event recorded in front of it complete on return; the harness then queues the next hold.  Before
every Host action of an async run the queue must still be busy (`Window.assert_open`) and must hold a library call, not the hold
alone: an action whose window was already closed has tested nothing, so the run is abandoned (`ClosedWindow`), repeated once on
fresh handles with four times the holds, and fails if that is not enough.  A Call that finds the queue empty gets a new hold in
front of it (holds are sized up to the next Host action; steps that do not drain the queue can follow one another for longer).

The hold in front of a step is a measurement: 4 x the host time the serial run needed from that step to the next Host action, at
least 5 ms, at most 100 ms.  It is bounded by a cycle / op count; nothing here waits on a flag."""
import os
import time

import numpy as np

HOLD_MIN_MS, HOLD_CAP_MS, HOLD_FACTOR, RERUN_FACTOR = 5.0, 100.0, 4.0, 4.0
RECORDS = []          # one entry per scenario run through run_modes: what write_report() lists


class ClosedWindow(AssertionError):
    """A step of an async run found the queue already empty: it raced nothing."""


def _torch():
    import torch

    return torch


def side_stream():
    """A non-blocking stream of torch's; the premise of the module as checked facts."""
    torch = _torch()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0, "torch.cuda.Stream() gave the null stream"
    assert torch.cuda.default_stream().cuda_stream == 0, "torch's default stream is not HIP's null stream (handle 0)"
    return s


# ---- the hold -------------------------------------------------------------------------------------------------------------------
_CAL = {}


def _calibrate():
    """("sleep", cycles per ms) of torch.cuda._sleep, or ("ops", ops per ms, buffer) of a chain of element-wise torch ops on a
    preallocated tensor where _sleep is unusable; timed once with two events."""
    torch = _torch()
    if "cal" in _CAL:
        return _CAL["cal"]
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cal = None
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(100_000)        # (first launch: the kernel is loaded)
            for cycles in (2_000_000, 20_000_000):
                e0.record()
                torch.cuda._sleep(cycles)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if ms >= 1.0:
                    cal = ("sleep", cycles / ms)
                    break
    except Exception:  # noqa: BLE001  (no _sleep in this torch: the op chain)
        cal = None
    if cal is None:
        buf = torch.zeros(1 << 22, dtype=torch.float32, device="cuda")
        with torch.cuda.stream(s):
            buf.add_(1.0)
            nops = 400
            e0.record()
            for _ in range(nops):
                buf.add_(1.0)
            e1.record()
            e1.synchronize()
        cal = ("ops", nops / max(e0.elapsed_time(e1), 1e-3), buf)
    s.synchronize()
    _CAL["cal"] = cal
    return cal


def hold(stream, ms):
    """Queue a busy period of about `ms` milliseconds on `stream`: everything queued behind it has not run while it lasts."""
    torch = _torch()
    cal = _calibrate()
    with torch.cuda.stream(stream):
        if cal[0] == "sleep":
            torch.cuda._sleep(max(1, int(ms * cal[1])))
        else:
            for _ in range(max(1, int(ms * cal[1]))):
                cal[2].add_(1.0)


class Window:
    """An event behind the work queued on `stream` so far.  While it has not completed, that work is still queued or running."""

    def __init__(self, stream):
        self.ev = _torch().cuda.Event()
        self.ev.record(stream)

    def is_open(self):
        return not self.ev.query()

    def assert_open(self, what=""):
        if self.ev.query():
            raise ClosedWindow(f"nothing was in flight any more before {what}")


# ---- steps ------------------------------------------------------------------------------------------------------------------------
class Call:
    """A process* call.  fn() returns a tensor, a tuple of tensors, or None; `handle`: whose last_kernel() names the kernel;
    `expect`: the names it may have."""
    racing = False

    def __init__(self, label, fn, handle=None, expect=None):
        self.label, self.fn, self.handle, self.expect = label, fn, handle, expect


class Host:
    """A host action that must order itself against the queue.  fn() returns None or a value (getters).  `op`, `method`: what the
    coverage check counts as raced (None: nothing)."""
    racing = True

    def __init__(self, label, fn, op=None, method=None):
        self.label, self.fn, self.op, self.method = label, fn, op, method


def H(op, method, *args, **kw):
    """The Host action op.method(*args, **kw)."""
    plain = args and all(isinstance(a, (int, float, bool)) for a in args)
    return Host(f"{type(op).__name__}.{method}{args if plain else ''}", lambda: getattr(op, method)(*args, **kw), op, method)


class Result:
    def __init__(self):
        self.outputs = []      # (label, list of numpy arrays) per step, in order
        self.kernels = []      # (label, kernel name) per Call with a handle
        self.host_ms = []      # serial: host time of every step
        self.holds = []        # async: (step index, ms) of every hold queued
        self.drained = []      # async: per step, whether it left the queue empty
        self.raced = []        # async: (op, method) of every Host action that ran with its window open
        self.steps = []


def _np(v):
    """A step's value as a list of numpy arrays (device tensors are copied to the host: call after the final synchronise)."""
    torch = _torch()
    if v is None:
        return []
    if isinstance(v, torch.Tensor):
        return [v.detach().cpu().numpy().copy()]
    if isinstance(v, (tuple, list)):
        return [a for x in v for a in _np(x)]
    return [np.asarray(v)]


def bits(a):
    """The bytes of an array, for a bit-for-bit comparison (NaNs and signed zeros included)."""
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8) if a.size else np.zeros(0, np.uint8)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def _plan_holds(steps, host_ms, scale):
    """Hold in front of step k, should the queue be empty there: the serial host time from step k to the next Host action
    (inclusive; to the end if there is none), times 4, within [5, 100] ms, times `scale` (the rerun)."""
    out = []
    for k in range(len(steps)):
        t = 0.0
        for j in range(k, len(steps)):
            t += host_ms[j] if host_ms is not None else 0.0
            if steps[j].racing:
                break
        out.append(min(max(HOLD_FACTOR * t, HOLD_MIN_MS), HOLD_CAP_MS) * scale)
    return out


def run(scenario, mode, host_ms=None, scale=1.0):
    """Run `scenario()` -- a callable that creates fresh handles and device inputs (on the default stream) and returns the steps --
    in `mode`.  Returns a Result; every output stays referenced until the final synchronise."""
    torch = _torch()
    assert mode in ("null", "serial", "async"), mode
    res = Result()
    steps = res.steps = scenario()
    torch.cuda.synchronize()
    raw = []

    def kernel_of(st):
        if not st.racing and st.handle is not None:
            res.kernels.append((st.label, st.handle.last_kernel()["name"]))

    if mode == "null":
        for st in steps:
            raw.append(st.fn())
            kernel_of(st)
            torch.cuda.synchronize()
    else:
        side = side_stream()
        side.wait_stream(torch.cuda.default_stream())
        holds = _plan_holds(steps, host_ms, scale) if mode == "async" else None
        with torch.cuda.stream(side):
            queued_calls = 0
            if mode == "async":
                hold(side, holds[0])
                res.holds.append((0, holds[0]))
            for k, st in enumerate(steps):
                if mode == "serial":
                    t0 = time.perf_counter()
                    raw.append(st.fn())
                    res.host_ms.append((time.perf_counter() - t0) * 1e3)
                    kernel_of(st)
                    side.synchronize()
                    continue
                w = Window(side)
                if st.racing:
                    w.assert_open(f"step {k} ({st.label})")
                    assert queued_calls > 0, f"step {k} ({st.label}): only the hold is queued, no library call to race with"
                elif not w.is_open():
                    # a hold is sized up to the next Host action; a run of steps that do not drain the queue (set_mode, a staged
                    # retune, set_history_dev and the calls between them) can outlast it.  A Call needs no open window of its
                    # own -- the next Host action does -- so the queue is simply held again, in front of this call.
                    queued_calls = 0
                    hold(side, holds[k])
                    res.holds.append((k, holds[k]))
                    w = Window(side)
                raw.append(st.fn())
                drained = bool(w.ev.query())
                kernel_of(st)
                res.drained.append(drained)
                if st.racing:
                    res.raced.append((st.op, st.method))
                if drained:
                    queued_calls = 0
                    if k + 1 < len(steps):
                        hold(side, holds[k + 1])
                        res.holds.append((k + 1, holds[k + 1]))
                elif not st.racing:
                    queued_calls += 1
            side.synchronize()
        torch.cuda.synchronize()
    for st, v in zip(steps, raw):
        res.outputs.append((st.label, _np(v)))
    for st, (_, name) in zip([s for s in steps if not s.racing and s.handle is not None], res.kernels):
        if st.expect is not None:
            assert name in st.expect, f"{mode}: {st.label} ran {name}, expected one of {sorted(st.expect)}"
    return res


def run_modes(name, scenario):
    """The three runs of one scenario: (null, serial, async).  The async run is repeated once with four times the holds if a
    window was closed; a second closed window fails (ClosedWindow is an AssertionError)."""
    null = run(scenario, "null")
    serial = run(scenario, "serial")
    rerun = False
    try:
        asy = run(scenario, "async", serial.host_ms)
    except ClosedWindow:
        rerun = True
        asy = run(scenario, "async", serial.host_ms, scale=RERUN_FACTOR)
    RECORDS.append({"name": name, "labels": [s.label for s in serial.steps], "racing": [s.racing for s in serial.steps],
                    "host_ms": serial.host_ms, "holds": asy.holds, "drained": asy.drained, "rerun": rerun})
    return null, serial, asy


def assert_same(name, a, b, what):
    """Two Results agree bit for bit: every output, every getter value, every count, every kernel name."""
    assert a.kernels == b.kernels, f"{name}: kernels differ, {what}: {a.kernels} / {b.kernels}"
    assert len(a.outputs) == len(b.outputs)
    for i, ((la, va), (lb, vb)) in enumerate(zip(a.outputs, b.outputs)):
        assert la == lb and len(va) == len(vb), (name, what, i, la, lb)
        for j, (x, y) in enumerate(zip(va, vb)):
            if not same_bits(x, y):
                x, y = np.asarray(x), np.asarray(y)
                where = ""
                if x.shape == y.shape and x.dtype == y.dtype and x.size:
                    bad = np.flatnonzero(bits(x) != bits(y)) // max(x.dtype.itemsize, 1)
                    where = f": {len(np.unique(bad))} of {x.size} elements, first at {np.unique(bad)[:4].tolist()}"
                raise AssertionError(f"{name}: step {i} ({la}), value {j} differs, {what}{where}")


def write_report(path):
    """The measured host times and the holds used, per scenario."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    cal = _CAL.get("cal")
    with open(path, "w") as f:
        f.write("# tests/test_gpu_async_order.py: per scenario, the host time of every step in the serial run (ms; * = racing host action),\n"
                "# the hold queued in front of it in the async run (ms, where the queue was empty there), whether the step drained the queue,\n"
                "# and whether the scenario needed the one permitted rerun with four times the holds.\n")
        if cal:
            f.write(f"# hold: {cal[0]}, {cal[1]:.1f} {'cycles' if cal[0] == 'sleep' else 'ops'} per ms\n")
        for r in RECORDS:
            holds = dict(r["holds"])
            f.write(f"\n{r['name']}: rerun {'yes' if r['rerun'] else 'no'}, {sum(r['racing'])} racing actions, "
                    f"holds {sum(holds.values()):.1f} ms in all\n")
            for k, (lab, racing, ms) in enumerate(zip(r["labels"], r["racing"], r["host_ms"])):
                h = f"{holds[k]:7.2f}" if k in holds else "      -"
                d = ("drained" if r["drained"][k] else "queued") if k < len(r["drained"]) else "?"
                f.write(f"  {k:3d} {'*' if racing else ' '} host {ms:8.3f}  hold {h}  {d:8s} {lab}\n")
