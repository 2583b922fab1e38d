#!/usr/bin/env python3
"""Throughput of the demodulators (qdsp_amd/csrc/demod.hip) and of the de-emphasis scan (deemp.hip) on device-resident synthetic IQ.

    python scripts/bench_demod.py                  # writes profiles/deemp_rates.txt (r05_demod_rates.txt: the run before the de-emphasis legs)
    python scripts/bench_demod.py --quick --no-write   # a few launches of every kernel (for a rocprofv3 --kernel-trace run)

Legs: FM, FM stereo, AM and SSB on 2^27-sample calls and on reference-sized 1e6-sample calls; xlate_cf32 on the same input
(SSB is its NCO with half the store bytes); chan64 (BASELINE configs[4]: 64 channels, 256 taps, decimate 64) on a 2^27-sample
input alone and followed by a batched 64-channel FM demodulator on its device output, and by FM stereo + the batched de-emphasis;
deemp_stereo / deemp_mono: the de-emphasis scan alone on the FM legs' outputs (16 B / 8 B per sample algorithmic; at these sizes the
scan runs as two passes and reads its input twice, so it moves 24 B / 12 B).  Timing: HIP events on the launch stream
around windows of >= 0.5 s after a warm-up, the legs alternated over `--repeats` rounds; min and spread (max / min - 1) of the
per-call time.  Bytes are algorithmic, from shapes: 8 B read + 4 B written per sample (FM, AM, SSB), 8 + 8 (FM stereo, xlate).
Fractions are of 8 TB/s (MI355X HBM peak).  Kernel times proper come from a separate rocprofv3 --kernel-trace --stats run."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "deemp_rates.txt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--quick", action="store_true", help="3 launches per leg, no timing windows (profiler runs)")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--stats", metavar="DB", help="summarise the kernels of a rocprofv3 --kernel-trace database of a --quick run instead")
    args = ap.parse_args()
    if args.stats:
        return kernel_stats(args.stats)

    import torch

    import oracle as O
    from qdsp_amd import ops

    assert torch.cuda.is_available(), "bench_demod needs the GPU"
    big, ref = 1 << 27, 1_000_000
    x = ops.synth_iq(big, seed=1)
    f_out = torch.empty(big, dtype=torch.float32, device="cuda")
    s_out = torch.empty((big, 2), dtype=torch.float32, device="cuda")
    c_out = torch.empty(big, dtype=torch.complex64, device="cuda")
    fm, fms, am = ops.FmDemod(250e3, 75e3, max_block=0), ops.FmDemod(250e3, 75e3, stereo=True, max_block=0), ops.AmDemod(max_block=0)
    ssb = ops.SsbDemod(48e3, 2.7e3, ops.SsbDemod.USB, max_block=0)
    xl = ops.Xlator(phase_inc=ops.ssb_phase_delta(48e3, 2.7e3, ops.SsbDemod.USB), max_block=0)
    taps = O.lowpass_taps_f64(256, 1.0 / 64.0)
    incs = [ops.phase_delta(1.0, -(c - 31.5) / 64.0) for c in range(64)]
    chn = ops.Channelizer(taps, 1, 64, incs, max_block=0)
    nco = chn.out_size(big)
    ch_out = torch.empty((64, nco + 8), dtype=torch.complex64, device="cuda")
    chan_fm = ops.FmDemod(250e3 / 64, 5e3, nchan=64, max_block=0)
    fm_ch_out = torch.empty((64, nco), dtype=torch.float32, device="cuda")
    chan_fms = ops.FmDemod(250e3 / 64, 5e3, stereo=True, nchan=64, max_block=0)
    chan_de = ops.Deemp(250e3 / 64, 50e-6, nchan=64, max_block=0)
    fms_ch_out = torch.empty((64, nco, 2), dtype=torch.float32, device="cuda")
    de_ch_out = torch.empty((64, nco, 2), dtype=torch.float32, device="cuda")
    de_s, de_m = ops.Deemp(250e3, 50e-6, max_block=0), ops.Deemp(250e3, 50e-6, stereo=False, max_block=0)
    fms.process(x, s_out)          # what the de-emphasis legs read: FM audio
    fm.process(x, f_out)
    ds_in, dm_in = s_out.clone(), f_out.clone()
    ds_out, dm_out = torch.empty_like(s_out), torch.empty_like(f_out)

    def leg(op, n, out):
        xi = x[:n]
        return lambda: op.process(xi, out[:n])

    def chan_only():
        chn.process(x, ch_out)

    def chan_fm_leg():
        y = chn.process(x, ch_out)
        chan_fm.process_batch(y, fm_ch_out)

    def chan_fms_deemp_leg():
        y = chn.process(x, ch_out)
        chan_de.process_batch(chan_fms.process_batch(y, fms_ch_out), de_ch_out)

    def deemp_leg(op, src, dst, n):
        return lambda: op.process(src[:n], dst[:n])

    legs = {}
    for n, tag in ((big, "2^27"), (ref, "1e6")):
        legs[f"fm {tag}"] = (leg(fm, n, f_out), n, 12.0)
        legs[f"fm_stereo {tag}"] = (leg(fms, n, s_out), n, 16.0)
        legs[f"am {tag}"] = (leg(am, n, f_out), n, 12.0)
        legs[f"ssb {tag}"] = (leg(ssb, n, f_out), n, 12.0)
        legs[f"xlate {tag}"] = (leg(xl, n, c_out), n, 16.0)
        legs[f"deemp_stereo {tag}"] = (deemp_leg(de_s, ds_in, ds_out, n), n, 16.0)
        legs[f"deemp_mono {tag}"] = (deemp_leg(de_m, dm_in, dm_out, n), n, 8.0)
    legs["chan64 2^27"] = (chan_only, big, 16.0 * (1 + 1 / 64))           # (bench.py's chan64 bytes: input + 64 outputs of 1/64)
    legs["chan64+fm 2^27"] = (chan_fm_leg, big, None)
    legs["chan64+fm_stereo+deemp 2^27"] = (chan_fms_deemp_leg, big, None)

    if args.quick:
        for f, _, _ in legs.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        print("quick: every leg launched 3 times")
        return

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(f, iters):
        ev0.record()
        for _ in range(iters):
            f()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / iters

    iters = {}
    for name, (f, n, _) in legs.items():
        for _ in range(3):
            f()
        t = window(f, 3)
        iters[name] = max(3, int(args.window * 1e3 / max(t, 1e-3)) + 1)
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name, (f, n, _) in legs.items():
            times[name].append(window(f, iters[name]))

    lines = ["# scripts/bench_demod.py: per-call ms (min over %d alternated windows of >= %.1f s, HIP events), spread = max/min - 1" % (args.repeats, args.window),
             "# bytes: algorithmic (FM / AM / SSB 12 B, FM stereo / xlate 16 B per sample); frac = bytes / min time / 8 TB/s",
             "# deemp: 16 B (stereo) / 8 B (mono) per sample algorithmic; both sizes run the two-pass form, which reads its input twice",
             "%-28s %12s %10s %8s %10s %7s" % ("leg", "samples", "ms", "spread", "GB/s", "frac")]
    res = {}
    for name, (f, n, b) in legs.items():
        t = min(times[name])
        spread = max(times[name]) / t - 1
        res[name] = t
        if b is None:
            lines.append("%-28s %12d %10.4f %7.1f%% %10s %7s" % (name, n, t, 100 * spread, "-", "-"))
        else:
            gbs = n * b / (t * 1e-3) / 1e9
            lines.append("%-28s %12d %10.4f %7.1f%% %10.1f %7.3f" % (name, n, t, 100 * spread, gbs, gbs * 1e9 / PEAK))
    fm_add = res["chan64+fm 2^27"] - res["chan64 2^27"]
    lines.append("# chan64 -> batched 64-channel FM: +%.4f ms over chan64 alone (%.1f %%); the FM kernel's own bytes: %d samples x 12 B"
                 % (fm_add, 100 * fm_add / res["chan64 2^27"], 64 * nco))
    de_add = res["chan64+fm_stereo+deemp 2^27"] - res["chan64 2^27"]
    lines.append("# chan64 -> batched FM stereo -> batched de-emphasis: +%.4f ms over chan64 alone (%.1f %%)" % (de_add, 100 * de_add / res["chan64 2^27"]))
    for tag in ("2^27", "1e6"):
        lines.append("# deemp_stereo against fm_stereo, same algorithmic bytes (%s): %.3f of its rate" % (tag, res[f"fm_stereo {tag}"] / res[f"deemp_stereo {tag}"]))
    for tag in ("2^27", "1e6"):
        s_gbs = 12.0 / res[f"ssb {tag}"]
        x_gbs = 16.0 / res[f"xlate {tag}"]
        lines.append("# ssb against xlate_cf32 on equal bytes (%s): %.3f" % (tag, s_gbs / x_gbs))
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        out = os.environ.get("BENCH_DEMOD_OUT", OUT)
        with open(out, "w") as fo:
            fo.write(txt)


def kernel_stats(db):
    """Per kernel and launch shape of a `rocprofv3 --kernel-trace --stats -- python scripts/bench_demod.py --quick` run: launches,
    min / median duration, and -- for the 2^27-sample launches -- the fraction of 8 TB/s on the leg's algorithmic bytes."""
    import sqlite3
    import statistics

    rows = sqlite3.connect(db).execute("select name, grid_x, grid_y, workgroup_x, vgpr_count, scratch_size, lds_size, duration from kernels").fetchall()
    groups = {}
    for name, gx, gy, wx, vgpr, scratch, lds, dur in rows:
        short = name.replace("void ", "").split("(")[0]
        if not any(k in short for k in ("demod", "am_", "xlate_kernel", "chan_uniform", "deemp")):
            continue
        groups.setdefault((short, gx, gy, wx, vgpr, scratch, lds), []).append(dur * 1e-3)   # (ns)
    lines = ["# rocprofv3 --kernel-trace --stats of scripts/bench_demod.py --quick (3 launches per leg); durations in us",
             "# (grid_x counts work-items here; frac: 2^27-sample launches only, FM / AM / SSB 12 B, FM stereo / xlate 16 B per sample)",
             "%-44s %10s %4s %5s %6s %7s %4s %10s %10s %6s" % ("kernel", "grid_x", "ny", "vgpr", "scratch", "lds", "n", "min_us", "med_us", "frac")]
    for (short, gx, gy, wx, vgpr, scratch, lds), d in sorted(groups.items()):
        frac = "-"
        if gy == 1 and gx == (1 << 24) and "fm_demod" in short:          # 8 samples per work-item
            frac = "%.3f" % ((1 << 27) * (16.0 if "<true>" in short else 12.0) / (min(d) * 1e-6) / PEAK)
        elif gy == 1 and gx == (1 << 26) and ("ssb_demod" in short or "xlate_kernel" in short):   # 2 per work-item
            frac = "%.3f" % ((1 << 27) * (12.0 if "ssb" in short else 16.0) / (min(d) * 1e-6) / PEAK)
        lines.append("%-44s %10d %4d %5d %6d %7d %4d %10.1f %10.1f %6s" % (short, gx, gy, vgpr, scratch, lds, len(d), min(d),
                                                                          statistics.median(d), frac))
    for nc, by in ((2, 16.0), (1, 8.0)):
        de = [min(d) for (short, gx, gy, *_), d in groups.items()
              if gy == 1 and short in (f"qk::deemp_partial_kernel<{nc}>", f"qk::deemp_scan_kernel<{nc}>") and gx >= 1023 * 256]
        if len(de) == 2:
            lines.append("# de-emphasis (%d floats per sample) at 2^27 samples, both passes: %.1f us, frac %.3f on %d B per sample"
                         % (nc, sum(de), (1 << 27) * by / (sum(de) * 1e-6) / PEAK, int(by)))
    am = [min(d) for (short, gx, gy, *_), d in groups.items() if short.startswith("qk::am_") and gy == 1 and gx == 1024 * 256]
    if len(am) == 2:
        lines.append("# AM at 2^27 samples, both passes: %.1f us, frac %.3f" % (sum(am), (1 << 27) * 12.0 / (sum(am) * 1e-6) / PEAK))
    txt = "\n".join(lines) + "\n"
    print(txt)
    out = os.path.join(ROOT, "profiles", "deemp_kernel_stats.txt")
    with open(out, "w") as fo:
        fo.write(txt)


if __name__ == "__main__":
    main()
