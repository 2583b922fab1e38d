#!/usr/bin/env python3
"""Rate of the Reed-Solomon decoder (qdsp_amd/csrc/rs.hip) as FalconRS on device-resident rows, next to a device copy.

    python scripts/bench_rs.py                   # writes profiles/rs_rates.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_rs.py --quick --no-write
    python scripts/bench_rs.py --stats DIR/.../*_results.db    # appends the split by kernel to profiles/rs_rates.txt (no GPU)

Shape: 64 rows x 256 frames of 1279 bytes (five interleaved RS(255, 239) codewords behind a 4-byte sync word), 81 920 codewords per
call.  Three legs: clean frames (the all-zero-syndrome shortcut), 4 errors in every codeword, 8 errors in every codeword (the most
the code corrects; every frame is kept in all three).  Recorded per leg: per-call time, codewords/s, bytes in + out per second and
that as a fraction of the copy ceiling of profiles/r01_micro_copy_bw.txt (5758 GB/s read+write).
Timing: HIP events on the launch stream around `--iters` back-to-back calls, after a warm-up call, the legs alternated over
`--repeats` rounds; min and spread (max / min - 1) of the per-call time."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "profiles", "rs_rates.txt")
COPY_GBS = 5758.0     # profiles/r01_micro_copy_bw.txt: best copy16 (read+write)
NCHAN, NFRAMES = 64, 256
LEGS = (("clean", 0), ("4 errors / codeword", 4), ("8 errors / codeword", 8))
KERNELS = ("rs_decode_kernel", "rs_scan_kernel", "rs_pack_kernel")


def kernel_split(db, quick_iters):
    """The three kernels' durations per leg from the database of a traced --quick run: one warm-up call per leg first, then the legs
    one after the other, quick_iters calls each, so the launches are told apart by their order."""
    import sqlite3
    import statistics

    con = sqlite3.connect(db)
    cols = [r[1] for r in con.execute("pragma table_info(kernels)")]
    order = next((c for c in ("start", "start_timestamp", "dispatch_id", "id") if c in cols), None)
    rows = con.execute("select name, duration from kernels" + (f" order by {order}" if order else "")).fetchall()
    seq = [(next(k for k in KERNELS if k in name), dur * 1e-3) for name, dur in rows if any(k in name for k in KERNELS)]
    per, warm = 3 * quick_iters, 3 * len(LEGS)
    assert len(seq) == warm + per * len(LEGS), (len(seq), per)
    lines = ["# split by kernel: rocprofv3 --kernel-trace --stats of `bench_rs.py --quick` (a run of its own; %d timed calls per leg, the"
             % quick_iters, "# warm-up call left out), median us per launch"]
    lines.append("%-24s %12s %12s %12s %10s" % ("leg", *KERNELS, "sum"))
    for i, (leg, _) in enumerate(LEGS):
        part = seq[warm + i * per: warm + (i + 1) * per]
        med = [statistics.median([d for k, d in part if k == kern]) for kern in KERNELS]
        lines.append("%-24s %12.1f %12.1f %12.1f %10.1f" % (leg, *med, sum(med)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
    ap.add_argument("--quick", action="store_true", help="a warm-up call per leg, then the legs one after the other, 5 calls each (for a traced run)")
    ap.add_argument("--stats", metavar="DB", help="append the split by kernel from the database of a traced --quick run; no GPU")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    out_path = os.environ.get("BENCH_RS_OUT", OUT)
    quick_iters = 5
    if args.stats:
        lines = kernel_split(args.stats, quick_iters)
        print("\n".join(lines))
        with open(out_path, "a") as fo:
            fo.write("\n".join(lines) + "\n")
        return

    import numpy as np
    import torch

    import _rs_ref as R
    from qdsp_amd import fec, ops

    assert torch.cuda.is_available(), "bench_rs needs the GPU"
    lay = R.falcon_layout()
    rng = np.random.default_rng(1)
    # 256 distinct frames, every row a rotation of them (the definition decodes 1280 codewords per leg, not 81 920)
    base = lay.encode(rng.integers(0, 256, (NFRAMES, 5, lay.code.k)).astype(np.uint8))
    base[:, :4] = [0x1A, 0xCF, 0xFC, 0x1D]
    legs = {}
    for name, ne in LEGS:
        fr = base.copy()
        for f in range(NFRAMES):
            for c in range(5):
                pos = rng.choice(255, ne, replace=False)
                fr[f, 4 + pos * 5 + c] ^= rng.integers(1, 256, ne).astype(np.uint8)
        want, good, errs = lay.decode(fr)
        assert good.all() and (errs == ne).all()
        rows = np.stack([np.roll(fr, r, axis=0).reshape(-1) for r in range(NCHAN)])
        x = torch.from_numpy(rows).cuda()
        d = fec.FalconRs(nchan=NCHAN, max_block=NFRAMES)
        out = torch.empty((NCHAN, NFRAMES * lay.frame_out), dtype=torch.uint8, device="cuda")
        y, counts = d.process_batch(x, out)                       # warm-up, and the check of what is timed
        assert counts.cpu().tolist() == [NFRAMES] * NCHAN and d.last_kernel()["name"] == "rs_decode_kernel"
        assert y[3].cpu().numpy().tobytes() == np.roll(want, 3, axis=0).tobytes()
        legs[name] = (d, x, out)

    if args.quick:
        for name, (d, x, out) in legs.items():
            print(name, "%.1f us" % (d.time_dev(x, out, quick_iters) * 1e3))
        return

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

    times = {k: [] for k in legs}
    copies = []
    for _ in range(args.repeats):
        for name, (d, x, out) in legs.items():
            times[name].append(d.time_dev(x, out, args.iters))
        copies.append(copy_ms(legs["clean"][1], args.iters))
    nin, nout = NCHAN * NFRAMES * lay.frame_in, NCHAN * NFRAMES * lay.frame_out
    ncw = NCHAN * NFRAMES * 5
    lines = ["# scripts/bench_rs.py: per-call us (min over %d alternated windows of %d back-to-back calls, HIP events), spread = max/min - 1"
             % (args.repeats, args.iters),
             "# FalconRs = rs_decode_kernel + rs_scan_kernel + rs_pack_kernel per call; %d rows x %d frames of %d bytes in, %d bytes out,"
             % (NCHAN, NFRAMES, lay.frame_in, lay.frame_out),
             "# %d codewords of RS(255, 239) per call, every frame kept; of copy = (bytes in + out)/s over the %.0f GB/s copy ceiling"
             % (ncw, COPY_GBS),
             "# (read+write) of profiles/r01_micro_copy_bw.txt",
             "%-24s %12s %12s %10s %8s %14s %12s %9s" % ("leg", "bytes in", "bytes out", "us", "spread", "codewords/s", "GB/s in+out", "of copy")]
    for name in legs:
        tm = min(times[name])
        gbs = (nin + nout) / (tm * 1e-3) / 1e9
        lines.append("%-24s %12d %12d %10.1f %7.1f%% %14.3e %12.1f %9.4f" % (name, nin, nout, tm * 1e3, 100 * (max(times[name]) / tm - 1),
                                                                           ncw / (tm * 1e-3), gbs, gbs / COPY_GBS))
    tm = min(copies)
    gbs = 2 * nin / (tm * 1e-3) / 1e9
    lines.append("%-24s %12d %12d %10.1f %7.1f%% %14s %12.1f %9.4f" % ("copy of the input rows", nin, nin, tm * 1e3, 100 * (max(copies) / tm - 1), "-", gbs,
                                                                     gbs / COPY_GBS))
    lines.append("# The 21 MB of input are replayed call after call and fit the Infinity Cache, so the copy's figure is an upper one, not an HBM rate.")
    lines.append("# What is supposed about where the decoder's time goes: EXPERIMENTS.md (Reed-Solomon decoder).")
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        with open(out_path, "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
