#!/usr/bin/env python3
"""Rates of FeedForwardAGC (qdsp_amd/csrc/ff_agc.hip) on device-resident rows, beside the level blocks' two-launch form.

    python scripts/bench_ff_agc.py                 # writes profiles/ff_agc_rates.txt
    python scripts/bench_ff_agc.py --kernel-run 2  # 200 launches of the W=1024 and level legs of shape 2 only, nothing written: for a
                                                   # rocprofv3 --kernel-trace --stats run, which times level_apply_kernel on its own
                                                   # (profiles/ff_agc_kernel_stats.txt)

Shapes: one row of 10^6 samples, 64 rows of 4096 and 64 rows of 65536; complex and float rows.  Legs per shape:
  ffagc W=1024   ff_agc_kernel in its steady state (1023 samples held, so every call emits as many samples as it takes in)
  ffagc W=1      the same kernel with no halo and no doubling pass (stage, combine, divide, store): what is left of a tile when
                 the LDS maxima are taken away; 1 - t(W=1) / t(W=1024) is the share of the call spent on the halo and the maxima
  squelch / agc  the level blocks at the same shape with QDSP_HIP_LEVEL_ROW_TILES=0: level_partial_kernel + level_apply_kernel,
                 i.e. the row read twice and written once in two launches.  The pass that scales and stores is level_apply_kernel;
                 the events around a call cannot time it alone, so the level legs are the PAIR of launches: the apply pass by
                 itself is faster, and every "of the rate of" figure below is an upper bound on the ratio against that pass
Timing: qdsp_hip_time_process_dev, i.e. back-to-back launches queued from C with HIP events on the launch stream around them, in
windows of >= `--window` s after a warm-up, the legs alternated over `--repeats` rounds; min and spread (max / min - 1) of the
per-call time.  Bytes are algorithmic, from shapes: every sample read once and written once (complex 8 + 8, float 4 + 4), for
every leg alike; fractions are of 8 TB/s (MI355X HBM peak).  The inputs of the 64-row shapes stay in the caches between calls."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "ff_agc_rates.txt")
KNOB = "QDSP_HIP_LEVEL_ROW_TILES"
SHAPES = ((1, 1_000_000), (64, 4096), (64, 65536))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds per timed window")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--kernel-run", type=int, default=None, metavar="SHAPE", help="index into SHAPES: launch that shape's legs only")
    args = ap.parse_args()

    import torch

    from qdsp_amd import capi, ops

    assert torch.cuda.is_available(), "bench_ff_agc needs the GPU"
    big = max(c * n for c, n in SHAPES)
    g = torch.Generator(device="cuda").manual_seed(1)
    xc = torch.view_as_complex(torch.randn((big, 2), device="cuda", generator=g))
    xf = torch.randn(big, device="cuda", generator=g)
    oc, of = torch.empty_like(xc), torch.empty_like(xf)

    legs = {}   # name -> (operator, input, output, samples per call, bytes per sample, expected kernel)
    for nchan, rows in SHAPES if args.kernel_run is None else SHAPES[args.kernel_run:args.kernel_run + 1]:
        n, shape = nchan * rows, f"{nchan}x{rows}"
        for kind, x, out, per in (("complex", xc, oc, 16.0), ("real", xf, of, 8.0)):
            for w in (1024, 1) if args.kernel_run is None else (1024,):
                legs[f"ffagc {kind} W={w} {shape}"] = (ops.FeedForwardAgc(kind, nchan=nchan, max_block=0, window=w), x[:n], out[:n], n, per, "ff_agc_kernel")
        legs[f"squelch two {shape}"] = (ops.Squelch(-50.0, nchan=nchan, max_block=0), xc[:n], oc[:n], n, 16.0, "level_apply_kernel")
        legs[f"agc two {shape}"] = (ops.Agc(10.0, 48e3, nchan=nchan, max_block=0), xf[:n], of[:n], n, 8.0, "level_apply_kernel")

    L = capi.load()
    stream = torch.cuda.current_stream().cuda_stream
    capi.setenv(KNOB, "0")

    def window(name, iters):
        op, x, out, n, per, kern = legs[name]
        ms = C.c_float()
        capi.check(L.qdsp_hip_time_process_dev(op._h, x.data_ptr(), n // op.nchan, out.data_ptr(), stream, iters, C.byref(ms)), name)
        assert op.last_kernel()["name"] == kern, (name, op.last_kernel())
        return float(ms.value)

    if args.kernel_run is not None:
        for name in legs:
            window(name, 200)
        capi.setenv(KNOB, None)
        return
    iters = {}
    for name in legs:
        window(name, 20)                          # (the first call of an ffagc leg fills the history)
        t = window(name, 50)
        iters[name] = max(50, int(args.window * 1e3 / max(t, 1e-4)) + 1)
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name in legs:
            times[name].append(window(name, iters[name]))
    capi.setenv(KNOB, None)
    for name, (op, *_rest) in legs.items():
        if name.startswith("ffagc"):
            assert op.fill() == op.window - 1, name
        if name.startswith("squelch"):
            assert all(op.is_open(c) for c in range(op.nchan)), name      # the copy was timed, not the memset

    lines = ["# scripts/bench_ff_agc.py: per-call us (min over %d alternated windows of >= %.2f s of back-to-back launches, HIP events), spread = max/min - 1"
             % (args.repeats, args.window),
             "# ffagc = ff_agc_kernel (one launch); squelch / agc two = level_partial_kernel + level_apply_kernel (%s=0)" % KNOB,
             "# bytes: algorithmic, every sample read once and written once (complex 16 B, float 8 B per sample); frac = bytes / min time / 8 TB/s",
             "%-34s %10s %10s %8s %10s %7s" % ("leg", "samples", "us", "spread", "GB/s", "frac")]
    res = {}
    for name, (op, x, out, n, per, kern) in legs.items():
        t = min(times[name])
        res[name] = t
        gbs = n * per / (t * 1e-3) / 1e9
        lines.append("%-34s %10d %10.3f %7.1f%% %10.1f %7.3f" % (name, n, t * 1e3, 100 * (max(times[name]) / t - 1), gbs, gbs * 1e9 / PEAK))
    for nchan, rows in SHAPES:
        shape = f"{nchan}x{rows}"
        for kind, level in (("complex", "squelch"), ("real", "agc")):
            t, t1, tl = res[f"ffagc {kind} W=1024 {shape}"], res[f"ffagc {kind} W=1 {shape}"], res[f"{level} two {shape}"]
            lines.append("# %s %s: ffagc W=1024 runs at %.3f of the rate of %s's two launches (at most that of level_apply_kernel alone); halo and LDS maxima: %.2f of its call (W=1: %.3f us)"
                         % (kind, shape, tl / t, level, 1.0 - t1 / t, t1 * 1e3))
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        with open(os.environ.get("BENCH_FF_AGC_OUT", OUT), "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
