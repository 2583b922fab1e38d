#!/usr/bin/env python3
"""PSKDemod / MSKDemod on device-resident rows: the one-call chains (qdsp_amd/csrc/psk_chain.cpp) and their stages, next to the
same work composed from the separate handles.  Numbers only: nothing here promises a speed-up, the serial loops (Costas, M&M: one
row per lane) bound the chain.

    python scripts/bench_psk.py              # writes profiles/psk_rates.txt

Shape: 64 rows x 65536 samples, QPSK at 4 samples per symbol, RRC filters of 32 and 361 taps; MSK at 4 samples per symbol.
Legs, in one process, alternated round by round; every one is `iters` back-to-back calls queued from C (qdsp_hip_time_process_dev),
HIP events on the launch stream around them:
  chain          ops.PskDemod / ops.MskDemod: every stage in one call
  <stage>        the stage's operator on its own: ops.ComplexAgc, ops.RowFir, ops.CostasLoop, ops.DelayImag, ops.MmClockRecovery,
                 ops.FmDemod
  rowfir T=1     RowFir with a one-tap filter: the same launch with the filter's FMAs taken out.  The difference to `rowfir` is taken
                 as row_fir_kernel's time for its FMAs; 2 nchan count T / that = its FMA rate.
  fir x64        one single-stream ops.Fir in DIRECT mode on one row, times 64: the FIR stage of the composition without host cost
  composed       the composition issued from Python as a user of the separate operators would (events around `iters` rounds):
                 ComplexAgc, 64 x Fir DIRECT, CostasLoop, MmClockRecovery
Windows of >= `--window` s after a warm-up; median, min and spread (max / min - 1) over `--repeats` alternated rounds."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "psk_rates.txt")
NCHAN, COUNT = 64, 65536
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

    from qdsp_amd import capi, ops

    assert torch.cuda.is_available(), "bench_psk needs the GPU"
    L = capi.load()
    stream = torch.cuda.current_stream().cuda_stream

    def queued(op, x, out, iters):
        ms = C.c_float()
        capi.check(L.qdsp_hip_time_process_dev(op._h, x.data_ptr(), COUNT, out.data_ptr(), stream, iters, C.byref(ms)), "time_process_dev")
        return float(ms.value)

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    g = torch.Generator(device="cuda").manual_seed(1)
    sym = (torch.randint(0, 2, (NCHAN, COUNT // 4), device="cuda", generator=g) * 2 - 1) + 1j * (torch.randint(0, 2, (NCHAN, COUNT // 4), device="cuda", generator=g) * 2 - 1)
    x = (0.05 * sym.repeat_interleave(4, dim=1) + 0.005 * torch.randn((NCHAN, COUNT), dtype=torch.complex64, device="cuda", generator=g)).to(torch.complex64).contiguous()
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    yf = torch.empty((NCHAN, COUNT), dtype=torch.float32, device="cuda")
    zf = torch.empty_like(yf)
    kw = dict(nchan=NCHAN, max_block=0)

    legs, fir_shapes = {}, []
    for T in (32, 361):
        taps = ops.rrc_taps(T, 4.0, 1.0, 0.32)
        for offset in ((False, True) if T == 32 else (False,)):
            name = f"psk4{' offset' if offset else ''} T={T}"
            chain = ops.PskDemod(4, offset, 4.0, 1.0, T, **kw)
            legs[name + " chain"] = lambda iters, op=chain: queued(op, x, y, iters)
        rowfir = ops.RowFir(1, taps, **kw)
        legs[f"T={T} rowfir"] = lambda iters, op=rowfir: queued(op, x, y, iters)
        fir = ops.Fir(taps, complex_data=True, max_block=0)
        fir.set_mode(ops.Fir.DIRECT)
        legs[f"T={T} fir x64"] = lambda iters, op=fir: NCHAN * queued(op, x[0], y[0], iters)
        fir_shapes.append(T)
        firs = []
        for _ in range(NCHAN):
            f = ops.Fir(taps, complex_data=True, max_block=0)
            f.set_mode(ops.Fir.DIRECT)
            firs.append(f)
        agc_c, costas_c = ops.ComplexAgc(1.0, 65535.0, 1e-3, **kw), ops.CostasLoop(4, 0.004, **kw)
        clock_c = ops.MmClockRecovery(1, 4.0, **kw)

        def composed(firs=firs, agc_c=agc_c, costas_c=costas_c, clock_c=clock_c):
            agc_c.process_batch(x, out=y)
            for c in range(NCHAN):
                firs[c].process(y[c], out=z[c])
            costas_c.process_batch(z, out=z)
            clock_c.process_batch(z, out=y)

        legs[f"psk4 T={T} composed"] = lambda iters, fn=composed: events(fn, iters)
    one = ops.RowFir(1, np.ones(1, np.float32), **kw)
    legs["rowfir T=1"] = lambda iters, op=one: queued(op, x, y, iters)
    stage_ops = {"cagc": ops.ComplexAgc(1.0, 65535.0, 1e-3, **kw), "costas<4>": ops.CostasLoop(4, 0.004, **kw), "delay_imag": ops.DelayImag(**kw),
                 "mmcr complex": ops.MmClockRecovery(1, 4.0, **kw)}
    for name, op in stage_ops.items():
        legs[name] = lambda iters, op=op: queued(op, x, y, iters)
    msk = ops.MskDemod(4.0, 1.0, 1.0, **kw)
    fm, clock_f = ops.FmDemod(4.0, 1.0, **kw), ops.MmClockRecovery(0, 4.0, **kw)
    legs["msk chain"] = lambda iters: queued(msk, x, yf, iters)
    legs["fm"] = lambda iters: queued(fm, x, yf, iters)
    legs["mmcr float"] = lambda iters: queued(clock_f, yf, zf, iters)

    iters = {}
    for name, leg in legs.items():
        leg(2)
        t = leg(3)
        iters[name] = max(3, min(2000, int(args.window * 1e3 / max(t, 1e-3)) + 1))
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name, leg in legs.items():
            times[name].append(leg(iters[name]))

    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["# scripts/bench_psk.py: ms per call of %d rows x %d samples (median, min, spread = max/min - 1 over %d alternated windows of >= %.2f s)"
             % (NCHAN, COUNT, args.repeats, args.window),
             "# chain: one call of ops.PskDemod / ops.MskDemod; the other legs: one operator on its own, queued from C; fir x64: 64 times one",
             "# single-stream Fir in DIRECT mode on one row; composed: ComplexAgc + 64 x Fir DIRECT + CostasLoop + MmClockRecovery issued from Python",
             "%-28s %10s %10s %8s" % ("leg", "median ms", "min ms", "spread")]
    for name in legs:
        v = times[name]
        lines.append("%-28s %10.4f %10.4f %7.1f%%" % (name, med[name], min(v), 100 * (max(v) / min(v) - 1)))
    peak = CUS * 4 * 64 / FMAC_CYCLES * CLOCK          # FMAs per second: 256 CUs x 4 SIMDs x 64 lanes per v_fmac_f32 of 3.99 cycles
    for T in fir_shapes:
        stages = med["cagc"] + med[f"T={T} rowfir"] + med["costas<4>"] + med["mmcr complex"]
        dev = med["cagc"] + med[f"T={T} fir x64"] + med["costas<4>"] + med["mmcr complex"]
        ch, co = med[f"psk4 T={T} chain"], med[f"psk4 T={T} composed"]
        lines.append("# psk4 T=%d: chain %.4f ms; the sum of its stages on their own %.4f; composition: %.4f issued from Python, %.4f as the sum of its "
                     "operators' device times (FIR stage: 64 x Fir DIRECT %.4f against rowfir %.4f)"
                     % (T, ch, stages, co, dev, med[f"T={T} fir x64"], med[f"T={T} rowfir"]))
        lines.append("#   the one-call chain is %s than the composition issued from Python (%.3f of it) and %s than the sum of its device times (%.3f of it)"
                     % ("faster" if ch < co else "SLOWER", ch / co, "faster" if ch < dev else "SLOWER", ch / dev))
        fir_ms = max(med[f"T={T} rowfir"] - med["rowfir T=1"], 1e-6)
        rate = 2.0 * NCHAN * COUNT * T / (fir_ms * 1e-3)
        lines.append("#   row_fir_kernel's FMAs: %.4f ms (rowfir - rowfir T=1) -> %.2f TFMA/s = %.2f of the v_fmac_f32 issue rate (%.1f TFMA/s at 2.4 GHz, "
                     "r03_micro_valu_rate.txt); grid: %d workgroups on %d CUs" % (fir_ms, rate / 1e12, rate / peak, peak / 1e12, NCHAN * -(-COUNT // ops.RowFir.tile()), CUS))
    lines.append("# psk4 offset T=32: chain %.4f ms (delay_imag on its own %.4f)" % (med["psk4 offset T=32 chain"], med["delay_imag"]))
    lines.append("# msk: chain %.4f ms; fm %.4f + mmcr float %.4f = %.4f" % (med["msk chain"], med["fm"], med["mmcr float"], med["fm"] + med["mmcr float"]))
    lines.append("# estimate from instruction counts (not measured): complex rows, per 12 taps a wave issues 96 v_pk_fma_f32 (192 FMAs, about 384 cycles of its")
    lines.append("#   SIMD; 768 as v_fmac_f32) and 6 ds_read_b128 (4-way conflict: 96 LDS cycles, 384 per CU for its four SIMDs), i.e. the LDS would be as busy")
    lines.append("#   as the VALU; the packed form's own issue rate is 2.0 on the scale above")
    lines.append("# device: %s" % ops.device_info(0))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if not args.no_write:
        with open(os.environ.get("BENCH_PSK_OUT", OUT), "w") as fo:
            fo.write(txt)


if __name__ == "__main__":
    main()
