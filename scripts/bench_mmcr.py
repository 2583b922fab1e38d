#!/usr/bin/env python3
"""Rates of MMClockRecovery (qdsp_amd/csrc/mmcr.hip) on device-resident rows, next to CostasLoop and a device copy.

    python scripts/bench_mmcr.py                     # writes profiles/mmcr_rates.txt

Legs: ops.MmClockRecovery on float and complex rows (mm_clock_kernel<float / float2>, one row per lane) at 64 and 1024 rows of
1 000 000 samples, 4 samples per symbol; as reference points on the same run ops.CostasLoop(4) (costas_kernel<4>, the same
one-row-per-lane arrangement, one serial step per sample where the clock recovery takes one per symbol) at the same shapes, and a
device-to-device copy of the complex rows' bytes.  Recorded per leg: per-call time, ns per input sample of a row, ns per symbol of a
row (the time of a step of the lockstep walk, staging included), aggregate input Msamples/s.
Timing: qdsp_hip_time_process_dev, i.e. back-to-back launches queued from C with HIP events on the launch stream around them, after
a warm-up call, the legs alternated over `--repeats` rounds of `--iters` launches; min and spread (max / min - 1) of the per-call
time."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "mmcr_rates.txt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2, help="launches per timed window")
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from qdsp_amd import capi, ops

    assert torch.cuda.is_available(), "bench_mmcr needs the GPU"
    n, shapes, sps = args.samples, (64, 1024), 4
    g = torch.Generator(device="cuda").manual_seed(1)
    nsym = n // sps + 1
    pulse = torch.tensor([0.38, 0.92, 0.92, 0.38], device="cuda")

    def rows_of(cplx):
        """64 rows of QPSK / +-1 symbols at 4 samples per symbol under a half-sine pulse plus noise, repeated to 1024 rows."""
        parts = 2 if cplx else 1
        sym = torch.randint(0, 2, (64, nsym, parts), device="cuda", generator=g).float() * 2 - 1
        x = (sym[:, :, None, :] * pulse[None, None, :, None]).reshape(64, nsym * sps, parts)[:, :n]
        x = x + 0.05 * torch.randn(x.shape, device="cuda", generator=g)
        x = torch.view_as_complex(x.contiguous()) if cplx else x[..., 0].contiguous()
        return x.repeat(max(shapes) // 64, 1).contiguous()

    xf, xc = rows_of(False), rows_of(True)
    of, oc = torch.empty_like(xf), torch.empty_like(xc)

    legs = {}   # name -> (operator, input, output, rows, expected kernel)
    for nchan in shapes:
        legs[f"mmcr<float> {nchan}x{n}"] = (ops.MmClockRecovery(0, float(sps), nchan=nchan, max_block=0), xf[:nchan], of[:nchan], nchan, "mm_clock_kernel")
        legs[f"mmcr<complex> {nchan}x{n}"] = (ops.MmClockRecovery(1, float(sps), nchan=nchan, max_block=0), xc[:nchan], oc[:nchan], nchan, "mm_clock_kernel")
        legs[f"costas<4> {nchan}x{n}"] = (ops.CostasLoop(4, 0.004, nchan=nchan, max_block=0), xc[:nchan], oc[:nchan], nchan, "costas_kernel")

    L = capi.load()
    stream = torch.cuda.current_stream().cuda_stream

    def window(name, iters):
        op, x, out, nchan, kern = legs[name]
        ms = C.c_float()
        capi.check(L.qdsp_hip_time_process_dev(op._h, x.data_ptr(), n, out.data_ptr(), stream, iters, C.byref(ms)), name)
        assert op.last_kernel()["name"] == kern, (name, op.last_kernel())
        return float(ms.value)

    def copy_ms(nchan, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            oc[:nchan].copy_(xc[:nchan])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for name in legs:
        window(name, 1)
    times = {k: [] for k in legs}
    copies = {s: [] for s in shapes}
    for _ in range(args.repeats):
        for name in legs:
            times[name].append(window(name, args.iters))
        for s in shapes:
            copies[s].append(copy_ms(s, 5))
    symbols = {}
    for name, (op, x, out, nchan, kern) in legs.items():   # what was timed: loops that kept running, at about n / sps symbols per call
        if name.startswith("mmcr"):
            assert all(np.isfinite(op.get_state(c)[0]) for c in (0, nchan - 1)), name
            cnt = op.counts()
            assert cnt.min() > 0.98 * n / sps and cnt.max() < 1.02 * n / sps, (name, cnt.min(), cnt.max())
            symbols[name] = float(cnt.mean())

    lines = ["# scripts/bench_mmcr.py: per-call us (min over %d alternated windows of %d back-to-back launches, HIP events), spread = max/min - 1"
             % (args.repeats, args.iters),
             "# mmcr<T> = mm_clock_kernel<T>, costas<4> = costas_kernel<4>: one row per lane, 16 rows per wave, one wave per workgroup; rows of %d samples, %d samples per symbol"
             % (n, sps),
             "# ns/sample = time / samples of a row; ns/symbol = time / symbols of a row (mmcr: one serial step per symbol; costas: per sample)",
             "%-30s %12s %12s %8s %10s %10s %12s" % ("leg", "samples", "us", "spread", "ns/sample", "ns/symbol", "Msamples/s")]
    res = {}
    for name, (op, x, out, nchan, kern) in legs.items():
        tm = min(times[name])
        res[name] = tm
        per_sym = tm * 1e6 / symbols[name] if name in symbols else tm * 1e6 / n
        lines.append("%-30s %12d %12.1f %7.1f%% %10.2f %10.2f %12.2f" % (name, nchan * n, tm * 1e3, 100 * (max(times[name]) / tm - 1), tm * 1e6 / n,
                                                                       per_sym, nchan * n / (tm * 1e-3) / 1e6))
    for s in shapes:
        tm = min(copies[s])
        lines.append("%-30s %12d %12.1f %7.1f%% %10s %10s %12.2f" % (f"copy {s}x{n} complex", s * n, tm * 1e3, 100 * (max(copies[s]) / tm - 1), "-", "-",
                                                                   s * n / (tm * 1e-3) / 1e6))
    for s in shapes:
        lines.append("# %d rows: mmcr<complex> takes %.3f of costas<4>'s time per input sample, mmcr<float> %.3f; the copy of the same bytes %.4f"
                     % (s, res[f"mmcr<complex> {s}x{n}"] / res[f"costas<4> {s}x{n}"], res[f"mmcr<float> {s}x{n}"] / res[f"costas<4> {s}x{n}"],
                        min(copies[s]) / res[f"costas<4> {s}x{n}"]))
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        with open(os.environ.get("BENCH_MMCR_OUT", OUT), "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
