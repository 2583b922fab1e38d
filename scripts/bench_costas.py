#!/usr/bin/env python3
"""Rates of CostasLoop (qdsp_amd/csrc/costas.hip) on device-resident rows, next to ComplexAGC's one-wave serial path.

    python scripts/bench_costas.py                   # writes profiles/costas_rates.txt

Legs: ops.CostasLoop of each order (costas_kernel<2 / 4 / 8>, one row per lane) at 1, 64 and 256 rows of 65 536 samples; and, as the
yardstick for a per-sample float feedback loop on this GPU, ops.ComplexAgc on one row of 65 536 samples in and out of its scan's
domain (bench_cagc.py's pair of legs: the difference is cagc_serial_kernel, one wave walking one row).  Recorded per leg: per-call
time, ns per sample of a row (the time of a step of the lockstep walk), aggregate Msamples/s; per order the time of 64 rows over the
time of one row.  Also the accuracy figure of tests/test_gpu_costas.py: per order the worst e_gpu / e_ref over the cases of
tests/test_costas_cpu.py (max |y - truth| of the kernel over that of the reference's float loop).
Timing: qdsp_hip_time_process_dev, i.e. back-to-back launches queued from C with HIP events on the launch stream around them, in
windows of >= `--window` s after a warm-up, the legs alternated over `--repeats` rounds; min and spread (max / min - 1) of the
per-call time."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "profiles", "costas_rates.txt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from qdsp_amd import capi, ops

    assert torch.cuda.is_available(), "bench_costas needs the GPU"
    rows, shapes = 65_536, (1, 64, 256)
    g = torch.Generator(device="cuda").manual_seed(1)
    ang = torch.rand((max(shapes) * rows,), device="cuda", generator=g) * (2 * np.pi)
    xc = torch.polar(torch.ones_like(ang), ang) + 0.05 * torch.view_as_complex(torch.randn((max(shapes) * rows, 2), device="cuda", generator=g))
    bad = (xc[:rows] * 0.5).clone()
    bad[12_345] = 5000.0                                # ComplexAGC: rate |x| = 5, out of the scan's domain
    oc = torch.empty_like(xc)

    legs = {}   # name -> (operator, input, output, samples per call, expected kernel)
    for order in (2, 4, 8):
        for nchan in shapes:
            legs[f"costas<{order}> {nchan}x65536"] = (ops.CostasLoop(order, 0.004, nchan=nchan, max_block=0), xc[:nchan * rows],
                                                     oc[:nchan * rows], nchan * rows, "costas_kernel")
    legs["cagc 1x65536"] = (ops.ComplexAgc(max_block=0), (xc[:rows] * 0.5).clone(), oc[:rows], rows, "cagc_scan_kernel")
    legs["cagc 1x65536 serial"] = (ops.ComplexAgc(max_block=0), bad, oc[:rows], rows, "cagc_scan_kernel")

    L = capi.load()
    stream = torch.cuda.current_stream().cuda_stream

    def window(name, iters):
        op, x, out, n, kern = legs[name]
        ms = C.c_float()
        capi.check(L.qdsp_hip_time_process_dev(op._h, x.data_ptr(), n // op.nchan, out.data_ptr(), stream, iters, C.byref(ms)), name)
        assert op.last_kernel()["name"] == kern, (name, op.last_kernel())
        return float(ms.value)

    iters = {}
    for name in legs:
        window(name, 2)
        t = window(name, 3)
        iters[name] = max(3, int(args.window * 1e3 / max(t, 1e-4)) + 1)
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name in legs:
            times[name].append(window(name, iters[name]))
    for name, (op, *_rest) in legs.items():               # what was timed: loops whose state stayed finite
        if name.startswith("costas"):
            assert all(np.all(np.isfinite(op.get_state(c))) for c in (0, op.nchan - 1)), name

    # the accuracy figure of the GPU test
    from test_costas_cpu import case_table, deviation

    t = case_table()
    worst = {}
    for order in (2, 4, 8):
        cols = [k for k, o in enumerate(t["order"]) if o == order]
        d = ops.CostasLoop(order, t["bw"][cols], nchan=len(cols), max_block=0)
        y = d.process_batch(torch.from_numpy(np.ascontiguousarray(t["x"][:, cols].T)).cuda()).cpu().numpy().T
        worst[order] = max((deviation(y[:, i], t["truth"], k) / t["e_ref"][k], t["names"][k]) for i, k in enumerate(cols))

    lines = ["# scripts/bench_costas.py: per-call us (min over %d alternated windows of >= %.2f s of back-to-back launches, HIP events), spread = max/min - 1"
             % (args.repeats, args.window),
             "# costas<ORDER> = costas_kernel<ORDER>, one row per lane, 16 rows per wave, one wave per workgroup; ns/step = time / samples of a row",
             "# cagc = cagc_partial_kernel + cagc_scan_kernel + cagc_serial_kernel (one row; `serial`: the row takes the one-wave float loop)",
             "%-30s %10s %12s %8s %10s %12s" % ("leg", "samples", "us", "spread", "ns/step", "Msamples/s")]
    res = {}
    for name, (op, x, out, n, kern) in legs.items():
        tm = min(times[name])
        res[name] = tm
        lines.append("%-30s %10d %12.3f %7.1f%% %10.2f %12.2f" % (name, n, tm * 1e3, 100 * (max(times[name]) / tm - 1),
                                                                 tm * 1e6 / rows, n / (tm * 1e-3) / 1e6))
    for order in (2, 4, 8):
        lines.append("# costas<%d>: 64 rows take %.3f of one row's time, 256 rows %.3f (expected near 1: the lanes run in lockstep)"
                     % (order, res[f"costas<{order}> 64x65536"] / res[f"costas<{order}> 1x65536"],
                        res[f"costas<{order}> 256x65536"] / res[f"costas<{order}> 1x65536"]))
    serial = (res["cagc 1x65536 serial"] - res["cagc 1x65536"]) * 1e6 / rows
    lines.append("# yardstick, cagc_serial_kernel (one wave, one row, float): %.1f ns per sample (the cagc legs: serial - scanned)" % serial)
    for order in (2, 4, 8):
        lines.append("# costas<%d> accuracy: worst e_gpu / e_ref over the cases of tests/test_costas_cpu.py %.4f (%s); the test allows 4"
                     % (order, worst[order][0], worst[order][1]))
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        with open(os.environ.get("BENCH_COSTAS_OUT", OUT), "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
