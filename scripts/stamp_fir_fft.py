#!/usr/bin/env python3
"""Where a wave of fir_fft_dmapk_kernel spends its time: the diagnostic build of the kernel (template parameter STAMPS) sums
s_memtime ticks per phase of its segment loop; this script runs it on the bench workload and prints the share of each phase.
Each workgroup also leaves its first tick, its tick at loop entry and its last tick on the constant-rate clock (s_memrealtime, 100 MHz,
the same on every CU) and the ids of the CU it ran on: the launch's timeline -- the prologue's share of a slot's time, the gap between a
workgroup's end and its successor's start on a slot, and how long the chip runs partly empty at the start and at the end.

    python scripts/stamp_fir_fft.py [--log2n 27]

(Needs the diagnostic build of the library: make -C qdsp_amd/csrc -B DIAG=1.)
The device buffer is handed over through QDSP_HIP_FFT_STAMPS=<device pointer> (read by launch_fft only for this purpose)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from qdsp_amd import capi, ops  # noqa: E402

WORDS = 24          # kFftStampWords (fft_fir.hip.h): 16 per-phase sums, three 64-bit ticks, HW_ID, XCC_ID
TICK_US = 0.01      # s_memrealtime: 100 MHz


def timeline(w, slots_per_cu=4):
    """w: [nwg][WORDS] int64 (unsigned words).  Prints the reduction described above."""
    import numpy as np

    t_first = w[:, 16] | (w[:, 17] << 32)
    t_loop = w[:, 18] | (w[:, 19] << 32)
    t_last = w[:, 20] | (w[:, 21] << 32)
    cu = (w[:, 23] << 8) | ((w[:, 22] >> 8) & 0xFF)      # XCC_ID, then HW_ID's CU / SH / SE fields
    t0, t1 = int(t_first.min()), int(t_last.max())
    span = (t1 - t0) * TICK_US
    life = (t_last - t_first).astype(np.float64)
    pro = (t_loop - t_first).astype(np.float64)
    ncu = len(np.unique(cu))
    slots = ncu * slots_per_cu
    print(f"timeline: {len(w)} workgroups on {ncu} CUs, first tick to last tick {span:.1f} us")
    print(f"  prologue (first tick -> loop entry): mean {pro.mean() * TICK_US:.2f} us, median {np.median(pro) * TICK_US:.2f} us = "
          f"{100.0 * pro.sum() / life.sum():.2f} % of the workgroups' time (mean workgroup {life.mean() * TICK_US:.1f} us)")
    first_round = np.sort(t_first)[: min(slots, len(w))]
    print(f"  prologue of the first {len(first_round)} workgroups (all slots start at once): mean "
          f"{pro[np.argsort(t_first)[:len(first_round)]].mean() * TICK_US:.2f} us; of the later ones "
          f"{(pro[np.argsort(t_first)[len(first_round):]].mean() * TICK_US if len(w) > len(first_round) else float('nan')):.2f} us")
    # hand-over gaps: per CU, each start after the first `slots_per_cu` takes over the slot of the earliest end not yet taken
    gaps = []
    for c in np.unique(cu):
        m = cu == c
        starts, ends = np.sort(t_first[m]), np.sort(t_last[m])
        for i, s_ in enumerate(starts[slots_per_cu:]):
            gaps.append(int(s_) - int(ends[i]))
    if gaps:
        g = np.array(gaps, dtype=np.float64) * TICK_US
        print(f"  end of a workgroup -> first tick of its successor on the slot: median {np.median(g):.2f} us, mean {g.mean():.2f} us, "
              f"p90 {np.percentile(g, 90):.2f} us ({len(g)} hand-overs; x {len(g) / slots:.1f} per slot = {g.mean() * len(g) / slots:.1f} us per slot)")
    full_at = int(np.sort(t_first)[min(slots, len(w)) - 1])
    last_start = int(t_first.max())
    first_free = int(t_last[t_last >= last_start].min())
    tail = (t1 - first_free) * TICK_US
    busy_tail = np.clip(t_last - first_free, 0, None).sum() * TICK_US
    print(f"  start: {(full_at - t0) * TICK_US:.2f} us until {min(slots, len(w))} workgroups have started")
    print(f"  end: {tail:.2f} us between the first slot that finds no successor and the last tick = {100.0 * tail / span:.1f} % of the launch, "
          f"slots busy {100.0 * busy_tail / (slots * tail) if tail > 0 else 0.0:.0f} % on average in it")
    res = (np.minimum(t_last, t1) - t_first).sum() * TICK_US / (slots * span)
    print(f"  workgroup slots occupied over the launch: {100.0 * res:.1f} %")


PHASES = ["wait for DMA (vmcnt)", "read raw + pass A + write (in place)", "barrier 1", "read + pass B", "barrier 2", "write layout 2", "barrier 3",
          "read + pass C, x Hf, pass C'", "barrier 4", "write layout 2", "barrier 5", "read + pass B'", "barrier 6", "write layout 1", "barrier 7",
          "read, request next DMA, pass A', stores, loop"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    a = ap.parse_args()
    n = 1 << a.log2n
    os.environ["QDSP_HIP_FFT_DMA"] = "2"
    x = ops.synth_iq(n, seed=1234)
    out = torch.empty(n, dtype=torch.complex64, device="cuda")
    op = bench.make_op(ops, "fir256", 0)
    if hasattr(capi, "reload_env"):
        capi.reload_env()
    for _ in range(3):
        op.time_dev(x, out, 20)
    grid = op.last_kernel()["grid"]
    stamps = torch.zeros(grid * WORDS, dtype=torch.int32, device="cuda")
    os.environ["QDSP_HIP_FFT_STAMPS"] = str(stamps.data_ptr())
    if hasattr(capi, "reload_env"):
        capi.reload_env()
    ms = op.time_dev(x, out, 1)
    torch.cuda.synchronize()
    os.environ.pop("QDSP_HIP_FFT_STAMPS")
    words = stamps.view(grid, WORDS)[: grid - 1].cpu().numpy().astype("int64") & 0xFFFFFFFF      # (the last workgroup hands over the history)
    s = torch.from_numpy(words[:, :16].astype("float64"))
    tot = s.sum(dim=1)
    print(f"diagnostic launch {ms:.4f} ms, grid {grid}; mean ticks per workgroup-wave {tot.mean():.0f} (s_memtime ticks = shader cycles)")
    order = [15] + list(range(15))
    names = {15: PHASES[15]}
    names.update({i: PHASES[i] for i in range(15)})
    for i in [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]:
        print(f"  {names[i]:48s} {100.0 * s[:, i].sum() / tot.sum():5.1f} %")
    timeline(words)
    op.close()


if __name__ == "__main__":
    main()
