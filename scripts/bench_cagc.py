#!/usr/bin/env python3
"""Rates of ComplexAGC (qdsp_amd/csrc/cagc.hip) on device-resident rows, next to the stereo de-emphasis scan.

    python scripts/bench_cagc.py                   # writes profiles/cagc_rates.txt

Legs: ops.ComplexAgc (cagc_partial_kernel + cagc_scan_kernel + cagc_serial_kernel, which returns at once) at 64 rows of 65 536
samples and at one row of 2^24; ops.Deemp(stereo=True) (deemp_partial_kernel + deemp_scan_kernel) on the same rows in the same
process -- it moves the same 16 bytes per sample and composes two FP64 components where ComplexAGC composes three; the 64-row call
again with one sample of one row out of the scan's domain (rate |x| > 1), so that this row takes the serial float loop while the
other 63 are scanned; and one row of 65 536 samples in and out of the domain, which gives the serial path's time per sample.
Timing: qdsp_hip_time_process_dev, i.e. back-to-back launches queued from C with HIP events on the launch stream around them, in
windows of >= `--window` s after a warm-up, the legs alternated over `--repeats` rounds; min and spread (max / min - 1) of the
per-call time.  Bytes are algorithmic, from shapes: every sample read once and written once, 16 B; fractions are of 8 TB/s
(MI355X HBM peak)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "cagc_rates.txt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()

    import torch

    from qdsp_amd import capi, ops

    assert torch.cuda.is_available(), "bench_cagc needs the GPU"
    nchan, rows, big = 64, 65_536, 1 << 24
    g = torch.Generator(device="cuda").manual_seed(1)
    xc = torch.view_as_complex(torch.randn((big, 2), device="cuda", generator=g)) * 0.5      # rate |x| <= 1 by a wide margin
    bad = xc[:nchan * rows].clone()
    bad[5 * rows + 12_345] = 5000.0                     # row 5: rate |x| = 5
    oc = torch.empty_like(xc)

    legs = {}   # name -> (operator, input, output, samples per call, expected kernel)

    def add(name, op, x, n, kern):
        legs[name] = (op, x[:n], oc[:n], n, kern)

    add("cagc 64x65536", ops.ComplexAgc(nchan=nchan, max_block=0), xc, nchan * rows, "cagc_scan_kernel")
    add("deemp stereo 64x65536", ops.Deemp(48e3, 50e-6, stereo=True, nchan=nchan, max_block=0), xc, nchan * rows, "deemp_scan_kernel")
    add("cagc 1x2^24", ops.ComplexAgc(max_block=0), xc, big, "cagc_scan_kernel")
    add("deemp stereo 1x2^24", ops.Deemp(48e3, 50e-6, stereo=True, max_block=0), xc, big, "deemp_scan_kernel")
    add("cagc 64x65536 row 5 serial", ops.ComplexAgc(nchan=nchan, max_block=0), bad, nchan * rows, "cagc_scan_kernel")
    add("cagc 1x65536", ops.ComplexAgc(max_block=0), xc, rows, "cagc_scan_kernel")
    add("cagc 1x65536 serial", ops.ComplexAgc(max_block=0), bad[5 * rows:], rows, "cagc_scan_kernel")

    L = capi.load()
    stream = torch.cuda.current_stream().cuda_stream

    def window(name, iters):
        op, x, out, n, kern = legs[name]
        per_row = n // op.nchan               # process_dev takes the nchan rows back to back
        ms = C.c_float()
        capi.check(L.qdsp_hip_time_process_dev(op._h, x.data_ptr(), per_row, out.data_ptr(), stream, iters, C.byref(ms)), name)
        assert op.last_kernel()["name"] == kern, (name, op.last_kernel())
        return float(ms.value)

    iters = {}
    for name in legs:
        window(name, 5)
        t = window(name, 20)
        iters[name] = max(20, int(args.window * 1e3 / max(t, 1e-4)) + 1)
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name in legs:
            times[name].append(window(name, iters[name]))
    # what was timed: the scanned rows hold a gain the scan keeps in its domain, the serial rows went through the float loop
    import numpy as np

    assert all(0 <= legs["cagc 64x65536"][0].get_gain(c) <= 1e5 for c in range(nchan))
    gs = legs["cagc 1x65536 serial"][0].get_gain()
    assert np.isnan(gs) or float(np.float32(gs)) == gs, gs

    lines = ["# scripts/bench_cagc.py: per-call us (min over %d alternated windows of >= %.2f s of back-to-back launches, HIP events), spread = max/min - 1"
             % (args.repeats, args.window),
             "# cagc = cagc_partial_kernel + cagc_scan_kernel + cagc_serial_kernel; deemp = deemp_partial_kernel + deemp_scan_kernel, stereo_t rows",
             "# bytes: algorithmic, every sample read once and written once, 16 B per sample; frac = bytes / min time / 8 TB/s",
             "%-30s %10s %12s %8s %10s %7s" % ("leg", "samples", "us", "spread", "GB/s", "frac")]
    res = {}
    for name, (op, x, out, n, kern) in legs.items():
        t = min(times[name])
        res[name] = t
        gbs = n * 16.0 / (t * 1e-3) / 1e9
        lines.append("%-30s %10d %12.3f %7.1f%% %10.1f %7.3f" % (name, n, t * 1e3, 100 * (max(times[name]) / t - 1), gbs, gbs * 1e9 / PEAK))
    for shape in ("64x65536", "1x2^24"):
        lines.append("# %s: cagc takes %.3f of the stereo de-emphasis scan's time (expected: at most 1.5, the ratio of the FP64 composition work)"
                     % (shape, res[f"cagc {shape}"] / res[f"deemp stereo {shape}"]))
    lines.append("# 64x65536 with row 5 out of the domain: %.3f of the all-scanned call's time"
                 % (res["cagc 64x65536 row 5 serial"] / res["cagc 64x65536"]))
    serial = (res["cagc 1x65536 serial"] - res["cagc 1x65536"]) * 1e3 / (rows / 1000.0)
    lines.append("# serial path (cagc_serial_kernel, one wave): %.1f us per 1000 samples (the 1x65536 legs: serial - scanned, both"
                 " with the check pass and the scan launch)" % serial)
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        with open(os.environ.get("BENCH_CAGC_OUT", OUT), "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
