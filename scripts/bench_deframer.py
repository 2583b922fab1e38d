#!/usr/bin/env python3
"""Rates of Threshold and Deframer (qdsp_amd/csrc/deframe.hip) on device-resident rows, next to a device copy of the same bytes.

    python scripts/bench_deframer.py                 # writes profiles/deframer_rates.txt

Legs, at 64 rows of 1 000 000 symbols: ops.Deframer on uint8 rows (kind 0) and on float soft symbols (kind 1), a 32-bit sync word
and frames of 2048 bits, on a stream that holds one frame after the other (locked: every frame starts with the word) and on one that
never holds the word (the match map and the search alone: nothing is packed); ops.Threshold on the float rows; and a device-to-device
copy of the input rows' bytes.  Recorded per leg: per-call time, input bytes/s, frames/s, and the input rate as a fraction of the
copy ceiling of profiles/r01_micro_copy_bw.txt (5758 GB/s read+write, i.e. 2879 GB/s of input at one read and one write per byte;
the deframer reads its input and writes an eighth of it, so its own bound is reading the input once: 6246 GB/s, the read-only
figure of the same file).
Timing: HIP events on the launch stream around `--iters` back-to-back calls, after a warm-up call, the legs alternated over
`--repeats` rounds; min and spread (max / min - 1) of the per-call time."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "deframer_rates.txt")
COPY_GBS, READ_GBS = 5758.0, 6246.0     # profiles/r01_micro_copy_bw.txt: best copy16 (read+write) and best read16 (read only)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from qdsp_amd import ops

    assert torch.cuda.is_available(), "bench_deframer needs the GPU"
    n, nchan, fl = args.samples, 64, 2048
    rng = np.random.default_rng(1)
    sync = rng.integers(0, 2, 32).astype(np.uint8)
    sync[0] = 1
    bits = rng.integers(0, 2, (nchan, n)).astype(np.uint8)
    locked = bits.copy()
    for r in range(nchan):
        for p in range(int(rng.integers(0, fl)), n - 32, fl):
            locked[r, p:p + 32] = sync
    # no run of 32 bytes equals the word: break every accidental hit
    free = bits.copy()
    for r in range(nchan):
        while True:
            hits = np.flatnonzero((np.lib.stride_tricks.sliding_window_view(free[r], 32) == sync[None, :]).all(axis=1))
            if hits.size == 0:
                break
            free[r, hits] ^= 1
    mag = rng.uniform(0.1, 2.0, (nchan, n)).astype(np.float32)
    rows = {}
    for name, b in (("locked", locked), ("no sync", free)):
        rows[name, 0] = torch.from_numpy(b).cuda()
        rows[name, 1] = torch.from_numpy(np.where(b > 0, mag, -mag).astype(np.float32)).cuda()

    legs = {}   # name -> (call, input tensor, expected kernel, operator)
    for kind, tag in ((0, "uint8"), (1, "float")):
        for name in ("locked", "no sync"):
            d = ops.Deframer(fl, sync, kind, nchan=nchan, max_block=n)
            x = rows[name, kind]
            out = torch.empty((nchan, d.out_size(n) * d.frame_bytes), dtype=torch.uint8, device="cuda")
            legs[f"deframer {tag} {name}"] = (lambda it, d=d, x=x, out=out: d.time_dev(x, out, it), x, "deframe_match_kernel", d)
    thr = ops.Threshold(nchan=nchan, max_block=n)
    tx = rows["locked", 1]
    tout = torch.empty((nchan, n), dtype=torch.uint8, device="cuda")
    legs["threshold float"] = (lambda it: thr.time_dev(tx, tout, it), tx, "threshold_kernel", thr)

    def copy_ms(x, iters):
        y = torch.empty_like(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        y.copy_(x)
        e0.record()
        for _ in range(iters):
            y.copy_(x)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for name, (fn, x, kern, op) in legs.items():
        fn(1)
        assert op.last_kernel()["name"] == kern, (name, op.last_kernel())
    times = {k: [] for k in legs}
    copies = {0: [], 1: []}
    for _ in range(args.repeats):
        for name, (fn, x, kern, op) in legs.items():
            times[name].append(fn(args.iters))
        for kind in (0, 1):
            copies[kind].append(copy_ms(rows["locked", kind], args.iters))
    frames = {}
    # what was timed: a locked stream gives about n / frame_len frames per row and call (the rows are replayed call after call, so
    # each call first loses the lock of the one before: up to five saved frames, then the search)
    for name, (fn, x, kern, op) in legs.items():
        if name.startswith("deframer"):
            c = op.counts()
            if "locked" in name:
                assert c.min() >= n // fl - 8 and c.max() <= n // fl + 1, (name, c.min(), c.max())
            else:
                assert c.max() == 0, (name, c.max())
            frames[name] = float(c.sum())

    lines = ["# scripts/bench_deframer.py: per-call us (min over %d alternated windows of %d back-to-back calls, HIP events), spread = max/min - 1"
             % (args.repeats, args.iters),
             "# deframer = deframe_match_kernel + deframe_walk_kernel + deframe_pack_kernel per call; %d rows of %d symbols, sync 32 bits, frames of %d bits"
             % (nchan, n, fl),
             "# locked: one frame after the other, each starting with the word; no sync: the word never occurs (match map and search only)",
             "# of copy = input bytes/s over the %.0f GB/s copy ceiling (read+write) of profiles/r01_micro_copy_bw.txt; of read = over its %.0f GB/s read-only figure"
             % (COPY_GBS, READ_GBS),
             "%-28s %12s %10s %8s %12s %12s %9s %9s" % ("leg", "bytes in", "us", "spread", "GB/s in", "frames/s", "of copy", "of read")]
    for name, (fn, x, kern, op) in legs.items():
        tm = min(times[name])
        nbytes = x.numel() * x.element_size()
        gbs = nbytes / (tm * 1e-3) / 1e9
        lines.append("%-28s %12d %10.1f %7.1f%% %12.1f %12.3e %9.3f %9.3f" % (name, nbytes, tm * 1e3, 100 * (max(times[name]) / tm - 1), gbs,
                                                                            frames.get(name, 0.0) / (tm * 1e-3), gbs / COPY_GBS, gbs / READ_GBS))
    for kind, tag in ((0, "uint8"), (1, "float")):
        tm = min(copies[kind])
        x = rows["locked", kind]
        nbytes = x.numel() * x.element_size()
        gbs = nbytes / (tm * 1e-3) / 1e9
        lines.append("%-28s %12d %10.1f %7.1f%% %12.1f %12s %9.3f %9.3f" % (f"copy {tag} rows", nbytes, tm * 1e3, 100 * (max(copies[kind]) / tm - 1), gbs, "-",
                                                                          gbs / COPY_GBS, gbs / READ_GBS))
    thr_tm, thr_x = min(times["threshold float"]), legs["threshold float"][1]
    lines.append("# threshold float: %d MB read and %d MB written per call, %.0f GB/s in all.  The same input rows are replayed call after call and may"
                 % (thr_x.numel() * 4 // 1000000, thr_x.numel() // 1000000, thr_x.numel() * 5 / (thr_tm * 1e-3) / 1e9))
    lines.append("# partly be served by the Infinity Cache (256 MB), so its fractions are upper figures, not an HBM rate; the same holds for the copies.")
    lines.append("# The deframer's split by kernel, and what is supposed about where its time goes: EXPERIMENTS.md (Threshold and Deframer).")
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        with open(os.environ.get("BENCH_DEFRAMER_OUT", OUT), "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
