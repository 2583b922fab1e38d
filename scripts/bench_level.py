#!/usr/bin/env python3
"""Rates of the two forms of the level blocks (qdsp_amd/csrc/level.hip: Squelch, AGC) on device-resident rows.

    python scripts/bench_level.py                  # writes profiles/level_rates.txt

Legs: Squelch (rows open: every sample copied) and AGC at 64 rows of 2048, 4096, 6144 and 8192 samples -- 1 to 4 tiles, the sizes
the one-launch form serves -- each in the one-launch form (level_row_kernel) and, with QDSP_HIP_LEVEL_ROW_TILES=0, in the
two-launch form (level_partial_kernel + level_apply_kernel); the AM demodulator (am_partial_kernel + am_sub_kernel), which has the
two-launch shape, on the same rows; and one row of 2^24 samples (always two launches) for all three.
Timing: qdsp_hip_time_process_dev, i.e. back-to-back launches queued from C with HIP events on the launch stream around them, in
windows of >= `--window` s after a warm-up, the legs alternated over `--repeats` rounds; min and spread (max / min - 1) of the
per-call time.  At the 64-row shapes a call is a few microseconds: what is compared is the rate at which a stream of such calls
drains, launch cost included -- the cost the one-launch form is there to halve.  Bytes are algorithmic, from shapes: every sample
read once and written once (Squelch 16 B, AGC 8 B, AM 8 B in + 4 B out); fractions are of 8 TB/s (MI355X HBM peak)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "level_rates.txt")
KNOB = "QDSP_HIP_LEVEL_ROW_TILES"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()

    import torch

    from qdsp_amd import capi, ops

    assert torch.cuda.is_available(), "bench_level needs the GPU"
    nchan, big = 64, 1 << 24
    g = torch.Generator(device="cuda").manual_seed(1)
    xc = torch.view_as_complex(torch.randn((big, 2), device="cuda", generator=g))
    xf = torch.randn(big, device="cuda", generator=g)
    oc, of = torch.empty_like(xc), torch.empty_like(xf)

    legs = {}   # name -> (operator, input, output, samples per call, bytes per sample, knob value, expected kernel)

    def add(name, op, x, out, n, per, knob, kern):
        legs[name] = (op, x[:n], out[:n], n, per, knob, kern)

    for rows in (2048, 4096, 6144, 8192):
        n = nchan * rows
        for form, knob, kern in (("row", None, "level_row_kernel"), ("two", "0", "level_apply_kernel")):
            add(f"squelch 64x{rows} {form}", ops.Squelch(-50.0, nchan=nchan, max_block=0), xc, oc, n, 16.0, knob, kern)
            add(f"agc 64x{rows} {form}", ops.Agc(10.0, 48e3, nchan=nchan, max_block=0), xf, of, n, 8.0, knob, kern)
        add(f"am 64x{rows} two", ops.AmDemod(nchan=nchan, max_block=0), xc, of, n, 12.0, None, "am_sub_kernel")
    add("squelch 1x2^24 two", ops.Squelch(-50.0, max_block=0), xc, oc, big, 16.0, None, "level_apply_kernel")
    add("agc 1x2^24 two", ops.Agc(10.0, 48e3, max_block=0), xf, of, big, 8.0, None, "level_apply_kernel")
    add("am 1x2^24 two", ops.AmDemod(max_block=0), xc, of, big, 12.0, None, "am_sub_kernel")

    import ctypes as C

    L = capi.load()
    stream = torch.cuda.current_stream().cuda_stream

    def window(name, iters):
        op, x, out, n, per, knob, kern = legs[name]
        capi.setenv(KNOB, knob)
        rows = n // op.nchan                  # samples per row: process_dev takes the nchan rows back to back
        assert op.nchan * rows <= x.numel() and op.nchan * rows <= out.numel()
        ms = C.c_float()
        capi.check(L.qdsp_hip_time_process_dev(op._h, x.data_ptr(), rows, out.data_ptr(), stream, iters, C.byref(ms)), name)
        t = float(ms.value)
        assert op.last_kernel()["name"] == kern, (name, op.last_kernel())
        return t

    iters = {}
    for name in legs:
        window(name, 20)
        t = window(name, 50)
        iters[name] = max(50, int(args.window * 1e3 / max(t, 1e-4)) + 1)
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name in legs:
            times[name].append(window(name, iters[name]))
    capi.setenv(KNOB, None)
    for name, (op, *_rest) in legs.items():
        if name.startswith("squelch"):
            assert all(op.is_open(c) for c in range(op.nchan)), name      # the copy was timed, not the memset

    lines = ["# scripts/bench_level.py: per-call us (min over %d alternated windows of >= %.2f s of back-to-back launches, HIP events), spread = max/min - 1"
             % (args.repeats, args.window),
             "# row = level_row_kernel (one launch); two = level_partial_kernel + level_apply_kernel (%s=0), or am_partial_kernel + am_sub_kernel" % KNOB,
             "# bytes: algorithmic, every sample read once and written once (squelch 16 B, agc 8 B, am 12 B per sample); frac = bytes / min time / 8 TB/s",
             "%-24s %10s %10s %8s %10s %7s" % ("leg", "samples", "us", "spread", "GB/s", "frac")]
    res = {}
    for name, (op, x, out, n, per, knob, kern) in legs.items():
        t = min(times[name])
        res[name] = t
        gbs = n * per / (t * 1e-3) / 1e9
        lines.append("%-24s %10d %10.3f %7.1f%% %10.1f %7.3f" % (name, n, t * 1e3, 100 * (max(times[name]) / t - 1), gbs, gbs * 1e9 / PEAK))
    for kind in ("squelch", "agc"):
        for rows in (2048, 4096, 6144, 8192):
            r, t = res[f"{kind} 64x{rows} row"], res[f"{kind} 64x{rows} two"]
            lines.append("# %s 64x%d (%d tiles): one launch takes %.3f of the two-launch form's time" % (kind, rows, rows // 2048, r / t))
    for rows in (4096, 8192):
        lines.append("# squelch two-launch form against AM's two launches, 64x%d, per byte: %.3f of its rate"
                     % (rows, (16.0 / res[f"squelch 64x{rows} two"]) / (12.0 / res[f"am 64x{rows} two"])))
    lines.append("# one row of 2^24, per byte against AM: squelch %.3f, agc %.3f of its rate"
                 % ((16.0 / res["squelch 1x2^24 two"]) / (12.0 / res["am 1x2^24 two"]), (8.0 / res["agc 1x2^24 two"]) / (12.0 / res["am 1x2^24 two"])))
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        with open(os.environ.get("BENCH_LEVEL_OUT", OUT), "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
