#!/usr/bin/env python3
"""QDSP_HIP_FFT_NT across filter lengths: the LDS-DMA FIR (fir_fft_dma_kernel, asked for by mode) on 2^log2n samples at several tap
counts, the policies interleaved in ONE process as scripts/ab_env.py does, median / min / max of the kernel time per (taps, policy).
The overlap (taps - 1 rounded up to even) decides whether a segment's row requests and stores cover whole 128-byte lines.

    python scripts/ab_fft_nt_taps.py --taps 63,65,129,256,1000,1025 --nt 0,1,2,3 [--rounds 11] [--log2n 27]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from qdsp_amd import capi, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taps", default="63,65,129,256,1000,1025")
    ap.add_argument("--nt", default="0,1,2,3", help="QDSP_HIP_FFT_NT values; 'd' = unset (the default)")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log2n", type=int, default=27)
    a = ap.parse_args()
    n = 1 << a.log2n
    x = ops.synth_iq(n, seed=1234)
    out = torch.empty(n + 8, dtype=torch.complex64, device="cuda")
    policies = a.nt.split(",")
    for ntaps in [int(t) for t in a.taps.split(",")]:
        op = ops.Fir(bench.lowpass_taps(ntaps, 1.0 / 16.0), max_block=0)
        op.set_mode(op.FFT)
        for _ in range(3):
            op.time_dev(x, out, 20)
        times = {p: [] for p in policies}
        for _ in range(a.rounds):
            for p in policies:
                capi.setenv("QDSP_HIP_FFT_NT", None if p == "d" else p)
                op.process(x, out)
                times[p].append(op.time_dev(x, out, a.iters))
                assert op.last_kernel()["name"] == "fir_fft_dma_kernel", op.last_kernel()
        capi.setenv("QDSP_HIP_FFT_NT", None)
        ov = (ntaps - 1 + 1) & ~1
        for p in policies:
            t = times[p]
            print(f"taps {ntaps:5d} overlap {ov:5d} (mod 16: {ov % 16:2d})  QDSP_HIP_FFT_NT={p}  median {statistics.median(t):.4f} ms  min {min(t):.4f}  max {max(t):.4f}", flush=True)
        op.close()


if __name__ == "__main__":
    main()
