#!/usr/bin/env python3
"""Rates of HrptDemux, TipDemux and HirsDemux (qdsp_amd/csrc/noaa.hip) on device-resident rows, each next to a device copy of the
same bytes timed in the same run.

    python scripts/bench_noaa.py                  # writes profiles/noaa_rates.txt

Shapes: HrptDemux 64 rows x 256 frames of 13863 bytes (227 MB in, 335 MB of AVHRR lines out: above the 256 MiB Infinity Cache, so
its figure is an HBM one), every fourth frame with TIP and every fourth with AIP minor frames; a second leg writes the AVHRR planes
alone.  TipDemux and HirsDemux 64 rows x 4096 items (27 MB in / 19 MB out and 9.4 MB in / about 10 MB out: these two fit the
cache).  Recorded per leg: per-call time, bytes in + out per second, and that as a fraction of the copy ceiling of
profiles/r01_micro_copy_bw.txt (5758 GB/s read+write).
Timing: HIP events on the launch stream around `--iters` back-to-back calls, after a warm-up call, the legs alternated over
`--repeats` rounds; min and spread (max / min - 1) of the per-call time."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "profiles", "noaa_rates.txt")
COPY_GBS = 5758.0     # profiles/r01_micro_copy_bw.txt: best copy16 (read+write)
NCHAN, NFRAMES, NITEMS = 64, 256, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    out_path = os.environ.get("BENCH_NOAA_OUT", OUT)

    import numpy as np
    import torch

    import _noaa_ref as R
    from qdsp_amd import noaa, ops

    assert torch.cuda.is_available(), "bench_noaa needs the GPU"
    rng = np.random.default_rng(1)

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    # ---- HrptDemux: 8 distinct frames checked against the definition, the rows rotations of their repetition ----
    base = rng.integers(0, 256, (8, R.FRAME_BYTES)).astype(np.uint8)
    base[:, 7] = (base[:, 7] & 0xF9) | (np.array([1, 0, 3, 2, 1, 0, 3, 2], np.uint8) << 1)
    row = np.tile(base, (NFRAMES // 8, 1))
    x = torch.from_numpy(np.stack([np.roll(row, r, axis=0).reshape(-1) for r in range(NCHAN)])).cuda()
    hr = noaa.HrptDemux(nchan=NCHAN, max_block=NFRAMES)
    av = torch.empty((NCHAN, 5, NFRAMES, 2048), dtype=torch.uint16, device="cuda")
    tip = torch.empty((NCHAN, NFRAMES * 520), dtype=torch.uint8, device="cuda")
    aip = torch.empty_like(tip)
    tc = torch.empty(NCHAN, dtype=torch.int32, device="cuda")
    ac = torch.empty_like(tc)
    hr.process_batch(x, avhrr=av, tip=tip, aip=aip, tip_counts=tc, aip_counts=ac)
    wav, wtip, waip, _ = R.hrpt_demux_fast(np.roll(row, 3, axis=0)[:16])
    assert np.array_equal(av[3, :, :16].cpu().numpy(), wav) and tc.cpu().tolist() == [5 * NFRAMES // 4] * NCHAN == ac.cpu().tolist()
    assert np.array_equal(tip[3, :wtip.size].cpu().numpy(), wtip.ravel()) and np.array_equal(aip[3, :waip.size].cpu().numpy(), waip.ravel())
    assert hr.last_kernel()["name"] == "hrpt_avhrr_kernel"
    hin = NCHAN * NFRAMES * R.FRAME_BYTES
    hav = NCHAN * NFRAMES * 5 * 2048 * 2
    hmf = 2 * NCHAN * (NFRAMES // 4) * 520

    # ---- TipDemux ----
    mf = torch.from_numpy(rng.integers(0, 256, (NCHAN, NITEMS * 104)).astype(np.uint8)).cuda()
    tp = noaa.TipDemux(nchan=NCHAN, max_block=NITEMS)
    rec = torch.empty((NCHAN, NITEMS * 74), dtype=torch.uint8, device="cuda")
    rc = torch.empty(NCHAN, dtype=torch.int32, device="cuda")
    tp.process_batch(mf, rec, counts=rc)
    assert np.array_equal(rec[5].cpu().numpy().reshape(-1, 74), R.tip_demux(mf[5].cpu().numpy())) and tp.last_kernel()["name"] == "tip_kernel"

    # ---- HirsDemux on packets 36 bytes apart whose elements count 0 .. 55 round and round ----
    pk = rng.integers(0, 256, (NITEMS, 36)).astype(np.uint8)
    el = (np.arange(NITEMS) % 56).astype(np.uint8)
    pk[:, 2] = (pk[:, 2] & 0xE0) | (el >> 1)
    pk[:, 3] = (pk[:, 3] & 0x7F) | ((el & 1) << 7)
    px = torch.from_numpy(np.stack([np.roll(pk, 56 * r, axis=0).reshape(-1) for r in range(NCHAN)])).cuda()
    hi = noaa.HirsDemux(36, nchan=NCHAN, max_block=NITEMS)
    lines = torch.empty((NCHAN, 20, NITEMS + 1, 56), dtype=torch.uint16, device="cuda")
    lc = torch.empty(NCHAN, dtype=torch.int32, device="cuda")
    hi.process_batch(px, lines, counts=lc)
    want = R.HirsFast().process(pk.ravel())
    nl = want.shape[1]
    assert int(lc[0]) == nl and np.array_equal(lines[0, :, :nl].cpu().numpy(), want) and hi.last_kernel()["name"] == "hirs_pack_kernel"
    nl = int(lc.sum()) // NCHAN                   # (a rotated row breaks one line more)
    hi.reset()

    legs = {
        "HrptDemux (all outputs)": (lambda: hr.process_batch(x, avhrr=av, tip=tip, aip=aip, tip_counts=tc, aip_counts=ac), hin, hav + hmf, x),
        "HrptDemux (AVHRR only)": (lambda: hr.process_batch(x, avhrr=av, tip=False, aip=False, tip_counts=False, aip_counts=False), hin, hav, x),
        "TipDemux": (lambda: tp.process_batch(mf, rec, counts=rc), NCHAN * NITEMS * 104, NCHAN * NITEMS * 74, mf),
        "HirsDemux": (lambda: hi.process_batch(px, lines, counts=lc), NCHAN * NITEMS * 36, NCHAN * nl * 20 * 56 * 2, px),
    }
    times = {k: [] for k in legs}
    copies = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name, (fn, _, _, src) in legs.items():
            times[name].append(events(fn, args.iters))
            dst = torch.empty_like(src)
            copies[name].append(events(lambda: dst.copy_(src), args.iters))
            del dst
    lines_out = ["# scripts/bench_noaa.py: per-call us (min over %d alternated windows of %d back-to-back calls, HIP events), spread = max/min - 1"
                 % (args.repeats, args.iters),
                 "# HrptDemux = hrpt_avhrr_kernel + hrpt_scan_kernel + hrpt_gather_kernel per call, %d rows x %d frames of %d bytes; TipDemux ="
                 % (NCHAN, NFRAMES, R.FRAME_BYTES),
                 "# tip_kernel, HirsDemux = hirs_scan_kernel + hirs_pack_kernel, %d rows x %d items each; of copy = (bytes in + out)/s over the"
                 % (NCHAN, NITEMS),
                 "# %.0f GB/s copy ceiling (read+write) of profiles/r01_micro_copy_bw.txt; each leg's copy is a device copy of its input rows,"
                 % COPY_GBS,
                 "# timed in the same run",
                 "%-28s %12s %12s %10s %8s %12s %9s" % ("leg", "bytes in", "bytes out", "us", "spread", "GB/s in+out", "of copy")]
    for name, (_, nin, nout, _) in legs.items():
        tm = min(times[name])
        gbs = (nin + nout) / (tm * 1e-3) / 1e9
        lines_out.append("%-28s %12d %12d %10.1f %7.1f%% %12.1f %9.4f" % (name, nin, nout, tm * 1e3, 100 * (max(times[name]) / tm - 1), gbs, gbs / COPY_GBS))
        tc_ = min(copies[name])
        gbs = 2 * nin / (tc_ * 1e-3) / 1e9
        lines_out.append("%-28s %12d %12d %10.1f %7.1f%% %12.1f %9.4f" % ("  copy of its input rows", nin, nin, tc_ * 1e3, 100 * (max(copies[name]) / tc_ - 1), gbs,
                                                                       gbs / COPY_GBS))
    lines_out.append("# HrptDemux moves 227 MB in and 335 MB out per call, more than the 256 MiB Infinity Cache: an HBM figure.  TipDemux (27 MB in, 19 MB")
    lines_out.append("# out) and HirsDemux (9.4 MB in, 10 MB out) are replayed call after call and fit the cache: theirs and their copies' are upper figures.")
    lines_out.append("# What the AVHRR kernel's figure is supposed to be limited by: EXPERIMENTS.md (NOAA demultiplexers).  No counter run is recorded.")
    lines_out.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines_out) + "\n"
    print(txt)
    if not args.no_write:
        with open(out_path, "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
