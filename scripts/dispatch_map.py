"""Which kernel family serves which call: one line per (settings, class, interp, decim, taps) with the family at each rung of a ladder of
call sizes.  Uses qdsp_amd.ops and last_kernel() only, so it runs on any revision of the library; two revisions dispatch alike exactly when
their outputs are the same text.  tests/golden/dispatch_map.txt is such an output (tests/fake_hip/select_selftest.cpp recomputes it on
the CPU from qdsp_amd/csrc/select.cpp, tests/test_gpu_dispatch_map.py compares a part of it with the library's calls).  On the GPU box:

    python scripts/dispatch_map.py [--sha REVISION] > map.txt

A line reads `settings class L M taps | count=family count=family ... end=count`: a family is written where it changes along the ladder and
holds up to the next entry; `end` is the last rung the row ran (rows with interp > decim stop at 2^25).  Names are folded the way
tests/conftest.py kname() folds them.  Settings: `default`; `parity` = the five variables tests/conftest.py gives test_gpu_parity; and
`setting7` = QDSP_HIP_DECIM_SETTING=7 on one decimation-8 row: the committed decim_table.inc holds settings 1-6 and 8 but no 7, so no
row under the default settings can meet it.
Classes: fir_c / fir_r (FIR on complex / real data), dec_c / vfo / dec_r (integer decimator, fused VFO, real decimator), rat_c / rat_r
(rational resampler; `taps` = interp x taps per phase), xlate (the bare mixer: the grid of the issue misses its family, this row adds it),
and fir_c / dec_c again with set_mode DIRECT and FFT (class name + `:direct` / `:fft`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LADDER = sorted([1 << k for k in (6, 10, 12, 14, 16, 18)] + [1 << k for k in range(19, 28)] + [1_000_000])
FIR_TAPS = (2, 7, 8, 24, 31, 63, 96, 127, 256, 321, 401, 769, 770, 1024, 1025, 2049, 2050)
DECIMS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 25, 50, 64, 128, 200)
DEC_TAPS = (16, 64, 104, 128, 160, 256, 401, 1024)
RATIOS = ((2, 1), (3, 2), (2, 3), (4, 3), (5, 8), (3, 8), (10, 7), (10, 3), (6, 1), (8, 3), (33, 32), (147, 160), (160, 147), (24, 125))
TAPS_PER_PHASE = (8, 16, 24, 40)
PARITY = {"QDSP_HIP_MF_MIN_COUNT": "0", "QDSP_HIP_RM_MIN_COUNT": "0", "QDSP_HIP_FFT1K_MAX_COUNT": "0", "QDSP_HIP_NO_LM_SMALL_CALL_RULE": "1",
          "QDSP_HIP_DECIM_SETTING": "0"}
MODE_ROWS = (("fir_c", 1, 1, 127), ("dec_c", 1, 8, 128))
SETTINGS = (("default", {}, None), ("parity", PARITY, None), ("setting7", {"QDSP_HIP_DECIM_SETTING": "7"}, (("dec_c", 1, 8, 128, 0),)))


def rows():
    """(class, interp, decim, taps, mode) in the order of the map."""
    for cls in ("fir_c", "fir_r"):
        for t in FIR_TAPS:
            yield cls, 1, 1, t, 0
    for cls in ("dec_c", "vfo", "dec_r"):
        for m in DECIMS:
            for t in DEC_TAPS:
                yield cls, 1, m, t, 0
    for cls in ("rat_c", "rat_r"):
        for l, m in RATIOS:
            for p in TAPS_PER_PHASE:
                yield cls, l, m, l * p, 0
    yield "xlate", 1, 1, 0, 0
    for cls, l, m, t in MODE_ROWS:
        for mode in (1, 2):
            yield cls, l, m, t, mode


def ladder_of(interp, decim):
    return [c for c in LADDER if c <= (1 << 25) or interp <= decim]


def fold(name):
    return "fir_fft_kernel" if name in ("fir_fft_dma_kernel", "fir_fft_dmapk_kernel") else name


def lowpass(ntaps, cutoff):
    k = np.arange(ntaps) - (ntaps - 1) / 2.0
    return (2 * cutoff * np.sinc(2 * cutoff * k) * np.hamming(ntaps)).astype(np.float32)


def make_op(ops, cls, interp, decim, taps, mode):
    base = cls
    if base == "xlate":
        return ops.Xlator(phase_inc=ops.phase_delta(1.0, 0.1234), max_block=0)
    h = lowpass(taps, 0.45 / max(interp, decim)) * interp
    if base in ("fir_c", "fir_r"):
        op = ops.Fir(h, complex_data=base == "fir_c", max_block=0)
    elif base == "vfo":
        op = ops.Vfo(h, interp, decim, ops.phase_delta(1.0, 0.1234), max_block=0)
    else:
        op = ops.Resampler(h, interp, decim, complex_data=base.endswith("_c"), max_block=0)
    if mode:
        op.set_mode(mode)
    return op


def format_row(settings, cls, interp, decim, taps, mode, families, counts):
    name = cls + {0: "", 1: ":direct", 2: ":fft"}[mode]
    parts, prev = [], None
    for c, f in zip(counts, families):
        if f != prev:
            parts.append(f"{c}={f}")
            prev = f
    return f"{settings} {name} {interp} {decim} {taps} | {' '.join(parts)} end={counts[-1]}"


def parse_row(line):
    """A line of the map back into (settings, class, interp, decim, taps, mode, [(count, family) at every rung the row ran])."""
    head, body = line.split(" | ")
    settings, name, interp, decim, taps = head.split()
    cls, _, m = name.partition(":")
    entries = dict(e.split("=") for e in body.split())
    end, rungs, fam = int(entries.pop("end")), [], None
    for c in LADDER:
        if c > end:
            break
        fam = entries.get(str(c), fam)
        rungs.append((c, fam))
    return settings, cls, int(interp), int(decim), int(taps), {"": 0, "direct": 1, "fft": 2}[m], rungs


def main():
    import torch

    from qdsp_amd import capi, ops

    sha = sys.argv[sys.argv.index("--sha") + 1] if "--sha" in sys.argv else "unknown"
    print(f"# dispatch map of {sha}: scripts/dispatch_map.py, one MI355X")
    gen = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(2 * LADDER[-1], dtype=torch.float32, device="cuda", generator=gen) * 0.25
    xc = torch.view_as_complex(x.view(-1, 2))
    out = torch.empty(2 * (6 * (1 << 25) + 16), dtype=torch.float32, device="cuda")
    outc = torch.view_as_complex(out.view(-1, 2))
    seen = set()
    for settings, env, only in SETTINGS:
        for k in PARITY:
            capi.setenv(k, env.get(k))
        for cls, interp, decim, taps, mode in only or rows():
            op = make_op(ops, cls, interp, decim, taps, mode)        # (after the settings: a handle's tables follow them)
            real = cls.endswith("_r")
            counts, fams = ladder_of(interp, decim), []
            for c in counts:
                op.process(x[:c] if real else xc[:c], out if real else outc)
                fams.append(fold(op.last_kernel()["name"]))
            torch.cuda.synchronize()
            op.close()
            seen.update(fams)
            print(format_row(settings, cls, interp, decim, taps, mode, fams, counts), flush=True)
    for k in PARITY:
        capi.setenv(k, None)
    print("families: " + " ".join(sorted(seen)), file=sys.stderr)


if __name__ == "__main__":
    main()
