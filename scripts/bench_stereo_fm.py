#!/usr/bin/env python3
"""StereoFMDemod on device-resident rows: the one-handle form (qdsp_amd/csrc/stereo_fm.hip) against the same work composed from
the operators the library had before it.

    python scripts/bench_stereo_fm.py              # writes profiles/stereo_fm_rates.txt

Shapes: 64 channels x 4096 and x 65536 samples, pilot filters of 193 and 1001 taps.  Legs, in one process, alternated round by round:
  handle       ops.StereoFmDemod: fm_demod_kernel + pilot_fir_kernel + stereo_mix_kernel, queued back to back from C
               (qdsp_hip_time_process_dev), HIP events on the launch stream around `iters` calls.
  handle T=1   the same handle with a one-tap filter: the same three launches with the filter's FMAs taken out.  The difference to
               `handle` is taken as pilot_fir_kernel's time for its FMAs; nchan * count * T / that = its FMA rate.
  composed     batched ops.FmDemod, 64 ops.Fir(real) calls (one handle and one call per channel), batched ops.Agc, the matrix as
               torch element-wise operations -- issued from Python as a user of those operators would, events around `iters` rounds.
  composed dev the sum of the composition's device times, each operator timed on its own as back-to-back launches queued from C (64 x
               one FIR row + FmDemod + Agc) plus the torch matrix: a lower bound of the composition without any host cost.
Windows of >= `--window` s after a warm-up; median, min and spread (max / min - 1) over `--repeats` alternated rounds."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "stereo_fm_rates.txt")
NCHAN = 64
FMAC_CYCLES = 3.99        # profiles/r03_micro_valu_rate.txt: v_fmac_f32, 4 waves/SIMD, cycles per instruction per SIMD at 2.4 GHz
CUS, CLOCK = 256, 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds per timed window")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    import oracle as O
    from qdsp_amd import ops

    import ctypes as C

    from qdsp_amd import capi

    assert torch.cuda.is_available(), "bench_stereo_fm needs the GPU"
    L = capi.load()
    stream = torch.cuda.current_stream().cuda_stream

    def queued(op, x, out, rows, iters):
        """ms per call of `iters` back-to-back process_dev calls on rows of `rows` samples, queued from C, HIP events around them"""
        ms = C.c_float()
        capi.check(L.qdsp_hip_time_process_dev(op._h, x.data_ptr(), rows, out.data_ptr(), stream, iters, C.byref(ms)), "time_process_dev")
        return float(ms.value)

    fs, dev = 250_000.0, 75_000.0
    g = torch.Generator(device="cuda").manual_seed(1)
    legs, shapes = {}, []
    for count in (4096, 65536):
        ph = torch.cumsum(torch.randn((NCHAN, count), device="cuda", generator=g) * 0.3, dim=1)
        x = torch.polar(torch.ones_like(ph), ph).contiguous()
        for T in (193, 1001):
            taps = O.blackman_bandpass_taps(1000.0, 19000.0, fs, T)
            shape = f"64x{count} T={T}"
            shapes.append((shape, count, T))
            out = torch.empty((NCHAN, count, 2), dtype=torch.float32, device="cuda")
            sfm = ops.StereoFmDemod(fs, dev, nchan=NCHAN, pilot_taps=taps, max_block=0)
            sf1 = ops.StereoFmDemod(fs, dev, nchan=NCHAN, pilot_taps=np.ones(1, np.float32), max_block=0)
            fm = ops.FmDemod(fs, dev, nchan=NCHAN, max_block=0)
            firs = [ops.Fir(taps, complex_data=False, max_block=0) for _ in range(NCHAN)]
            agc = ops.Agc(20.0, fs, nchan=NCHAN, max_block=0)
            m = torch.empty((NCHAN, count), dtype=torch.float32, device="cuda")
            f = torch.empty_like(m)
            p = torch.empty_like(m)

            def matrix(m=m, p=p, out=out):
                s = m * (p * p)
                torch.add(m, s, out=out[:, :, 0])
                torch.sub(m, s, out=out[:, :, 1])

            def composed(x=x, m=m, f=f, p=p, fm=fm, firs=firs, agc=agc, matrix=matrix):
                fm.process_batch(x, out=m)
                for c in range(NCHAN):
                    firs[c].process(m[c], out=f[c])
                agc.process_batch(f, out=p)
                matrix()

            def events(fn, iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / iters

            def composed_dev(iters, x=x, m=m, f=f, p=p, fm=fm, firs=firs, agc=agc, matrix=matrix, events=events, count=count):
                t = queued(fm, x, m, count, iters) + NCHAN * queued(firs[0], m[0], f[0], count, iters) + queued(agc, f, p, count, iters)
                return t + events(matrix, iters)

            legs[shape + " handle"] = lambda iters, sfm=sfm, x=x, out=out, count=count: queued(sfm, x, out, count, iters)
            legs[shape + " handle T=1"] = lambda iters, sf1=sf1, x=x, out=out, count=count: queued(sf1, x, out, count, iters)
            legs[shape + " composed"] = lambda iters, composed=composed, events=events: events(composed, iters)
            legs[shape + " composed dev"] = composed_dev

    iters = {}
    for name, leg in legs.items():
        leg(3)
        t = leg(5)
        iters[name] = max(5, min(2000, int(args.window * 1e3 / max(t, 1e-3)) + 1))
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name, leg in legs.items():
            times[name].append(leg(iters[name]))

    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["# scripts/bench_stereo_fm.py: ms per call of 64 rows (median, min, spread = max/min - 1 over %d alternated windows of >= %.2f s)"
             % (args.repeats, args.window),
             "# handle: ops.StereoFmDemod, three launches queued from C; composed: FmDemod + 64 x Fir(real) + Agc + torch matrix issued from Python;",
             "# composed dev: the sum of those operators' device times, each queued from C on its own (no host cost: a lower bound of the composition)",
             "%-32s %10s %10s %8s" % ("leg", "median ms", "min ms", "spread")]
    for name in legs:
        v = times[name]
        lines.append("%-32s %10.4f %10.4f %7.1f%%" % (name, med[name], min(v), 100 * (max(v) / min(v) - 1)))
    fracs = {}
    peak = CUS * 4 * 64 / FMAC_CYCLES * CLOCK          # FMAs per second: 256 CUs x 4 SIMDs x 64 lanes per v_fmac_f32 of 3.99 cycles
    for shape, count, T in shapes:
        h, c, cd, h1 = (med[f"{shape} {k}"] for k in ("handle", "composed", "composed dev", "handle T=1"))
        worst = max(max(times[f"{shape} handle"]), 0.0)
        best_other = min(min(times[f"{shape} composed"]), min(times[f"{shape} composed dev"]))
        lines.append("# %s: handle %.4f ms = %.3f of composed (%.4f), %.3f of composed dev (%.4f); slowest handle window %.4f %s fastest composed window %.4f"
                     % (shape, h, h / c, c, h / cd, cd, worst, "<" if worst < best_other else ">=", best_other))
        fir_ms = max(h - h1, 1e-6)
        rate = NCHAN * count * T / (fir_ms * 1e-3)
        lines.append("#   pilot_fir_kernel's FMAs: %.4f ms (handle - handle T=1) -> %.2f TFMA/s = %.2f of the v_fmac_f32 issue rate (%.1f TFMA/s at 2.4 GHz, "
                     "r03_micro_valu_rate.txt); grid: %d workgroups on %d CUs"
                     % (fir_ms, rate / 1e12, rate / peak, peak / 1e12, NCHAN * -(-count // 2048), CUS))
        fracs[shape] = rate / peak
    best = max(fracs, key=fracs.get)
    lines.append("# estimate from instruction counts (not measured): per 12 taps a wave issues 96 v_fmac_f32 (about 384 cycles of its SIMD) and 3 ds_read_b128")
    lines.append("#   (2-way conflict: 24 LDS cycles, 96 per CU for its four SIMDs), i.e. the LDS would be a quarter as busy as the VALU")
    if fracs[best] >= 0.5:
        lines.append("# bound, from the measured rate: at %s the FMAs run at %.2f of the v_fmac_f32 issue rate -- the VALU bounds pilot_fir_kernel there (no LDS"
                     % (best, fracs[best]))
        lines.append("#   limit could leave the VALU more than half busy); shapes with a smaller fraction: %s"
                     % (", ".join("%s %.2f" % (k, v) for k, v in fracs.items() if k != best) or "none"))
    else:
        lines.append("# bound, from the measured rate: the FMAs reach at most %.2f of the v_fmac_f32 issue rate (%s): neither the VALU nor, by the estimate above, the"
                     % (fracs[best], best))
        lines.append("#   LDS bounds pilot_fir_kernel at these shapes; what does (staging, waits per 12 taps, grid size) is not resolved by this run")
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        with open(os.environ.get("BENCH_STEREO_FM_OUT", OUT), "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
