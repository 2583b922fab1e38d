#!/usr/bin/env python3
"""Rate of FalconPacketSync (qdsp_amd/csrc/fpkt.hip) on device-resident rows, next to a device copy of the same bytes timed in the
same run.

    python scripts/bench_fpkt.py                  # writes profiles/fpkt_rates.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_fpkt.py --quick --no-write
    python scripts/bench_fpkt.py --stats DIR/.../*_results.db    # appends the split by kernel to profiles/fpkt_rates.txt (no GPU)

Shape: 64 rows x 256 frames, 1275 bytes apart (what FalconRs leaves), 1195 of them read.  Two legs: a realistic stream, packets
of a few hundred bytes and a few of more than a frame; and the worst case of the walk and of the offset table, every frame filled
with three-byte packets (396 walked packets and a three-byte residue that the next frame completes: 397 packets per frame).
Recorded per leg: per-call time, frames/s, packets per call, bytes in + out per second and that as a fraction of the copy ceiling of
profiles/r01_micro_copy_bw.txt (5758 GB/s read+write).  Every call replays the same rows, so it begins with a counter break: the
packet pending behind a call's last frame is carried (the carry is written) and dropped by the next call's first frame.
Timing: HIP events on the launch stream around `--iters` back-to-back calls, after a warm-up call, the legs alternated over
`--repeats` rounds; min and spread (max / min - 1) of the per-call time."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "profiles", "fpkt_rates.txt")
COPY_GBS = 5758.0     # profiles/r01_micro_copy_bw.txt: best copy16 (read+write)
NCHAN, NFRAMES, STRIDE = 64, 256, 1275
LEGS = ("realistic", "three-byte packets")
KERNELS = ("fpkt_walk_kernel", "fpkt_scan_kernel", "fpkt_pack_kernel")


def kernel_split(db, quick_iters):
    """The three kernels' durations per leg from the database of a traced --quick run: the checked call and a warm-up call per leg
    first, then the legs one after the other, quick_iters calls each, so the launches are told apart by their order."""
    import sqlite3
    import statistics

    con = sqlite3.connect(db)
    cols = [r[1] for r in con.execute("pragma table_info(kernels)")]
    order = next((c for c in ("start", "start_timestamp", "dispatch_id", "id") if c in cols), None)
    rows = con.execute("select name, duration from kernels" + (f" order by {order}" if order else "")).fetchall()
    seq = [(next(k for k in KERNELS if k in name), dur * 1e-3) for name, dur in rows if any(k in name for k in KERNELS)]
    per, warm = 3 * quick_iters, 2 * 3 * len(LEGS)
    assert len(seq) == warm + per * len(LEGS), (len(seq), per)
    lines = ["# split by kernel: rocprofv3 --kernel-trace --stats of `bench_fpkt.py --quick` (a run of its own; %d timed calls per leg, the"
             % quick_iters, "# checked call and the warm-up call left out), median us per launch"]
    lines.append("%-24s %18s %18s %18s %10s" % ("leg", *KERNELS, "sum"))
    for i, leg in enumerate(LEGS):
        part = seq[warm + i * per: warm + (i + 1) * per]
        med = [statistics.median([d for k, d in part if k == kern]) for kern in KERNELS]
        lines.append("%-24s %18.1f %18.1f %18.1f %10.1f" % (leg, *med, sum(med)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
    ap.add_argument("--quick", action="store_true", help="a warm-up call per leg, then the legs one after the other, 5 calls each (for a traced run)")
    ap.add_argument("--stats", metavar="DB", help="append the split by kernel from the database of a traced --quick run; no GPU")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    out_path = os.environ.get("BENCH_FPKT_OUT", OUT)
    quick_iters = 5
    if args.stats:
        lines = kernel_split(args.stats, quick_iters)
        print("\n".join(lines))
        with open(out_path, "a") as fo:
            fo.write("\n".join(lines) + "\n")
        return

    import numpy as np
    import torch

    import _fpkt_ref as R
    from qdsp_amd import falcon, ops

    assert torch.cuda.is_available(), "bench_fpkt needs the GPU"
    rng = np.random.default_rng(1)
    # one stream of 256 frames per leg; row r is the stream rotated by 4 r frames and renumbered, so that the rows differ in where
    # their packets lie and every row's counters run on (the definition walks 2 rows, not 64)
    real = R.random_stream(rng, NFRAMES, stride=STRIDE, mean=300, big=0.02, breaks=0.0, zero=0.0, ctr0=1, fill=True)
    three = np.zeros((NFRAMES, STRIDE), np.uint8)
    data = np.tile(np.array([0x00, 0x01, 0x5A], np.uint8), R.DATA // 3)
    three[:, R.HEADER:R.FRAME] = data
    for f in range(NFRAMES):
        three[f, :R.HEADER] = np.frombuffer(R.make_header(1 + f, 0), np.uint8)

    def rows_of(base):
        rows = []
        for r in range(NCHAN):
            fr = np.roll(base, -4 * r, axis=0).copy()
            for f in range(NFRAMES):
                fr[f, :R.HEADER] = np.frombuffer(R.make_header(1 + f, R.parse_header(fr[f])[1]), np.uint8)
            rows.append(fr)
        return np.stack(rows)

    nb, npk = R.out_size(NFRAMES), R.out_packets(NFRAMES)
    legs = {}
    for name, base in zip(LEGS, (real, three)):
        hx = rows_of(base)
        x = torch.from_numpy(hx.reshape(NCHAN, -1)).cuda()
        op = falcon.FalconPacketSync(STRIDE, nchan=NCHAN, max_block=NFRAMES)
        out = torch.empty((NCHAN, nb), dtype=torch.uint8, device="cuda")
        offs = torch.empty((NCHAN, npk + 1), dtype=torch.int32, device="cuda")
        cnt = torch.empty(NCHAN, dtype=torch.int32, device="cuda")
        op.process_batch(x, out, offs, counts=cnt)
        torch.cuda.synchronize()
        tot = op.counts()
        for r in (0, 5):
            wo, wf, _ = R.serial_row(hx[r])
            assert tot[0, r] == len(wf) - 1 and tot[1, r] == len(wo), (name, r)
            assert np.array_equal(offs[r, :len(wf)].cpu().numpy(), wf) and out[r, :len(wo)].cpu().numpy().tobytes() == wo, (name, r)
        assert op.last_kernel()["name"] == "fpkt_pack_kernel"
        legs[name] = (op, x, out, offs, cnt, int(tot[0].sum()), int(tot[1].sum()))

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def call(name):
        op, x, out, offs, cnt, _, _ = legs[name]
        return lambda: op.process_batch(x, out, offs, counts=cnt)

    if args.quick:
        for name in LEGS:
            call(name)()
        for name in LEGS:
            events(call(name), quick_iters)
        torch.cuda.synchronize()
        print("quick run done")
        return

    times = {k: [] for k in LEGS}
    copies = {k: [] for k in LEGS}
    for _ in range(args.repeats):
        for name in LEGS:
            call(name)()
            times[name].append(events(call(name), args.iters))
            src = legs[name][1]
            dst = torch.empty_like(src)
            dst.copy_(src)
            copies[name].append(events(lambda: dst.copy_(src), args.iters))
            del dst
    nin = NCHAN * NFRAMES * R.FRAME
    lines_out = ["# scripts/bench_fpkt.py: per-call us (min over %d alternated windows of %d back-to-back calls, HIP events), spread = max/min - 1"
                 % (args.repeats, args.iters),
                 "# FalconPacketSync = fpkt_walk_kernel + fpkt_scan_kernel + fpkt_pack_kernel per call, %d rows x %d frames %d bytes apart, %d read"
                 % (NCHAN, NFRAMES, STRIDE, R.FRAME),
                 "# of each; bytes out: the packets and 4 bytes of offset per packet; of copy = (bytes in + out)/s over the %.0f GB/s copy ceiling"
                 % COPY_GBS,
                 "# (read+write) of profiles/r01_micro_copy_bw.txt; each leg's copy is a device copy of its input rows, timed in the same run",
                 "%-26s %10s %10s %10s %10s %8s %10s %12s %9s" % ("leg", "bytes in", "bytes out", "packets", "us", "spread", "Mframes/s", "GB/s in+out", "of copy")]
    for name in LEGS:
        _, _, _, _, _, pk, by = legs[name]
        nout = by + 4 * pk
        tm = min(times[name])
        gbs = (nin + nout) / (tm * 1e-3) / 1e9
        lines_out.append("%-26s %10d %10d %10d %10.1f %7.1f%% %10.2f %12.1f %9.4f" % (name, nin, nout, pk, tm * 1e3, 100 * (max(times[name]) / tm - 1),
                                                                                 NCHAN * NFRAMES / (tm * 1e-3) / 1e6, gbs, gbs / COPY_GBS))
        tc = min(copies[name])
        full = NCHAN * NFRAMES * STRIDE
        gbs = 2 * full / (tc * 1e-3) / 1e9
        lines_out.append("%-26s %10d %10d %10s %10.1f %7.1f%% %10.2f %12.1f %9.4f" % ("  copy of its input rows", full, full, "-", tc * 1e3,
                                                                                 100 * (max(copies[name]) / tc - 1), NCHAN * NFRAMES / (tc * 1e-3) / 1e6, gbs,
                                                                                 gbs / COPY_GBS))
    lines_out.append("# 21 MB in and about as much out per call: both legs and their copies are replayed call after call and fit the 256 MiB Infinity")
    lines_out.append("# Cache, so these are upper figures, and at tens of microseconds per call the three launches' own overhead is part of them.")
    lines_out.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines_out) + "\n"
    print(txt)
    if not args.no_write:
        with open(out_path, "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
