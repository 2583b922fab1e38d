#!/usr/bin/env python3
"""Rate of the Viterbi decoder (qdsp_amd/csrc/viterbi.hip) on device-resident rows.

    python scripts/bench_viterbi.py                  # writes profiles/viterbi_rates.txt

Soft input, rate 1/2, k = 7 (0161, 0127) and k = 9 (0767, 0545), two shapes of about the same decoded bits: 64 rows x 16 frames of
8168 sets (1020 decoded bytes a frame: few, long frames, 1024 waves) and 64 rows x 256 frames of 526 sets (65 decoded bytes: many
short frames, 16384 waves).  Frames are encodings of random messages with Gaussian noise (sigma 60 on the 0 .. 255 scale), sixteen
different ones dealt over the rows; one frame per leg is checked against the numpy definition first.  Recorded per leg: per-call
time and decoded Mbit/s (decoded bits of a call over its time).  Timing: HIP events on the launch stream around `--iters`
back-to-back calls, after a warm-up call, the legs alternated over `--repeats` rounds; min and spread (max / min - 1)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "profiles", "viterbi_rates.txt")
NCHAN = 64
LEGS = (("k=7, 16 x 8168 sets", 7, 16, 8168), ("k=9, 16 x 8168 sets", 9, 16, 8168), ("k=7, 256 x 526 sets", 7, 256, 526),
        ("k=9, 256 x 526 sets", 9, 256, 526))
# the reference's own decoder, one thread, portable build at -O2, one soft frame of 8168 sets (the issue that asked for this kernel)
CPU_MS = {7: 2.8, 9: 9.6}
DISTINCT = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    out_path = os.environ.get("BENCH_VITERBI_OUT", OUT)

    import numpy as np
    import torch

    import _viterbi_ref as V
    from qdsp_amd import ops, viterbi

    assert torch.cuda.is_available(), "bench_viterbi needs the GPU"
    rng = np.random.default_rng(1)
    legs = {}
    for name, order, nframes, sets in LEGS:
        poly = V.CODES[(2, order)]
        base = np.stack([V.make_input(2, order, poly, sets, True, V.KIND_CODED, 900 + i) for i in range(DISTINCT)])
        pick = rng.integers(0, DISTINCT, (NCHAN, nframes))
        hx = base[pick]                                            # (NCHAN, nframes, 2 sets)
        x = torch.from_numpy(hx.reshape(NCHAN, -1)).cuda()
        op = viterbi.ViterbiDecoder(2, order, poly, sets, soft=True, nchan=NCHAN, max_block=nframes)
        out = torch.empty((NCHAN, nframes * op.frame_out_bytes), dtype=torch.uint8, device="cuda")
        op.process_batch(x, out=out)
        torch.cuda.synchronize()
        want, _, _ = V.decode(2, order, poly, base[:2], sets, True)
        got = out.cpu().numpy().reshape(NCHAN, nframes, -1)
        for r, f in ((0, 0), (NCHAN - 1, nframes - 1), (17, nframes // 2)):
            if pick[r, f] < 2:
                assert got[r, f].tobytes() == want[pick[r, f]].tobytes(), (name, r, f)
        where = np.argwhere(pick < 2)[:4]
        assert len(where) and all(got[r, f].tobytes() == want[pick[r, f]].tobytes() for r, f in where), name
        assert op.last_kernel()["name"] == "viterbi_decode_kernel"
        legs[name] = (op, x, out, NCHAN * nframes * (sets - order + 1), op.last_kernel())

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def call(name):
        op, x, out, _, _ = legs[name]
        return lambda: op.process_batch(x, out=out)

    times = {k[0]: [] for k in LEGS}
    for _ in range(args.repeats):
        for name, *_ in LEGS:
            call(name)()
            times[name].append(events(call(name), args.iters))
    lines = ["# scripts/bench_viterbi.py: per-call us (min over %d alternated windows of %d back-to-back calls, HIP events), spread = max/min - 1"
             % (args.repeats, args.iters),
             "# viterbi_decode_kernel, one launch per call, soft input, rate 1/2, %d rows; Mbit/s = decoded bits of a call over its time" % NCHAN,
             "%-24s %8s %8s %12s %12s %8s %12s %8s" % ("leg", "waves", "grid", "bits out", "us", "spread", "Mbit/s", "LDS/WG")]
    for name, order, nframes, sets in LEGS:
        _, _, _, nbits, lk = legs[name]
        tm = min(times[name])
        lines.append("%-24s %8d %8d %12d %12.1f %7.1f%% %12.1f %8d" % (name, NCHAN * nframes, lk["grid"], nbits, tm * 1e3, 100 * (max(times[name]) / tm - 1),
                                                                     nbits / (tm * 1e-3) / 1e6, lk["lds_bytes"]))
    lines.append("# for orientation, the reference's own decoder on one CPU thread (portable build, -O2), one soft frame of 8168 sets:")
    for order, ms in CPU_MS.items():
        lines.append("#   k=%d: %.1f ms a frame, %.2f Mbit/s" % (order, ms, (8168 - order + 1) / (ms * 1e-3) / 1e6))
    lines.append("# The input rows (17 MB a call) are replayed call after call and fit the 256 MiB Infinity Cache; the kernel is bound by its")
    lines.append("# serial add-compare-select steps, not by memory.")
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        with open(out_path, "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
