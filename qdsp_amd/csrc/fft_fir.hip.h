// fft_fir.hip.h -- overlap-save fast convolution for long complex FIRs (gfx950).
//
// Why: direct form costs 2*ntaps FMAs per complex sample (1024 FLOP at 256 taps against 16
// algorithmic bytes: FP32-compute-bound at ~30 % of the HBM roofline).  A
// 4096-point overlap-save block costs ~135 FLOP per sample, which puts the filter back
// under the HBM roof.  Same operator, same state, same boundary (FIR<complex_t>::run,
// src/dsp/filter.h:51-74); results differ from the k-ordered FP32 sum only by FP32 FFT
// rounding (~3e-7 RMS relative, tests/test_gpu_parity.py) -- inside the 1e-5 bar.
//
// One workgroup = 256 lanes = one 4096-point block at a time, persistent over blocks.
//   x (F samples, H = ntaps-1 of them overlap) --A--> --B--> --C--> * Hf --C'--> --B'--> --A'--> y
// F = 16*16*16: three radix-16 passes done in registers (16 points per lane), separated by
// LDS transposes; the inverse runs the same passes backwards, so no bit-reversal pass
// exists: Hf is stored in the digit-reversed order pass C leaves the spectrum in.
// Per-lane constants (pass twiddles, Hf slice) are loaded once per workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include "kconst.h"      // kFftN

namespace qk {

constexpr int kFftNT = 256;
constexpr int kFftRow1 = 272;   // layout 1: [k0][n1*16 + n0], row padded 256 -> 272 elements
constexpr int kFftRow2 = 17;    // layout 2: [k0*16 + k1][n0], row padded 16 -> 17 elements
constexpr int kFftLdsElems = 16 * kFftRow1;  // 4352 >= 256*17 = 4352

constexpr int kFftStampWords = 24;   // per workgroup: 16 per-phase sums, first / loop-entry / last tick (64-bit each), HW_ID, XCC_ID

struct FftArgs {
    const float2* in;
    float2* out;
    const float2* hist;       // H raw samples preceding in[0] (fused VFO: de-rotated by the caller from the rotated form the handle keeps)
    float2* hist_raw_next;    // fused VFO: where the hand-over also leaves the next call's history un-rotated (or nullptr)
    const float2* hist_keep;  // the same H samples in the form the handle keeps them (rotated for the fused VFO): source of the hand-over
    float2* hist_next;
    const float2* Hf;         // [256][16]: Hf[(k0*16+k1)*16 + k2] = FFT(taps reversed)[k0 + 16 k1 + 256 k2] / F
    const float2* TA;         // [256][16]: exp(-j 2pi t k / 4096)
    const float2* TB;         // [16][16] : exp(-j 2pi lo k / 256)
    const float2* HfT;        // [16][256]: Hf entry-major, HfT[k*256 + t] == Hf[t*16 + k] -- a wave reads 512 contiguous bytes per entry
    const float2* TAT;        // [16][256]: TA entry-major, TAT[k*256 + element] == TA[element*16 + k]
    int tbl;                  // 1: the kernels read HfT / TAT (the default); 0: Hf / TA (QDSP_HIP_FFT_TBL=0, kept for the A/B of the two layouts)
    long long count;          // input samples of this call
    long long nout;           // outputs of this call
    int H;                    // history length (ntaps-1 for the FIR, taps per phase for the resampler)
    int dec;                  // 1, 2, 4, 8, 16: decimation handled by pruning the inverse transform
    int decm;                 // dec == 1 only: keep every decm-th output of the full inverse
    unsigned decm_inv;        // floor(2^32 / decm) + 1: x / decm == (x * decm_inv) >> 32 for x < 2^32 / decm (0: divide)
    int strided;              // dec == 1 only: resampler semantics -- y[n'] sits at stream position n'*decm - 1 (0 = FIR: y[n] at n)
    int rot;                  // 1: fused VFO -- Hf holds the spectrum of taps * exp(j k dphase), outputs are rotated
    int ov;                   // leading invalid elements of a segment (multiple of dec)
    int seg_shift;            // segment b starts at stream position b*L - seg_shift
    int L;                    // stream positions covered per segment = 4096 - ov
    int nblocks;
    int nwg;                  // persistent workgroups (grid = nwg + 1; the last one hands over history)
    int n_long, rounds;       // the LDS-DMA kernels: workgroups below n_long take segments w, w + n_long, ... (at most `rounds` of them);
                              // the nwg - n_long after them take short contiguous runs (fft_taper_tier); n_long == nwg: no short ones
    int vec;                  // 1: in/out 16-byte aligned and segments start on even samples -> float4 path
    int grouped;              // dec >= 4: 1 = fir_fft_dec_kernel (groups of dec segments), 0 = one segment per workgroup
    int m_shift;              // fir_fft1k_kernel, strided: log2(decm) when decm is a power of two <= 64 (a lane keeps all or none of its 16 elements), else -1
    int abl;                  // diagnostic builds of fir_fft_dmapk_kernel: ablation mask (0: the product)
    unsigned* stamps;         // diagnostic build of fir_fft_dmapk_kernel only: [grid][kFftStampWords] per-phase tick sums + timeline (nullptr: off)
    int nt;                   // the LDS-DMA kernels (both; a template parameter of each): bit 0 = non-temporal DMA of rows 1-14 of an interior segment
                              // (rows 0 and 15 hold the overlap a neighbour reads as well), bit 1 = non-temporal 16-byte stores.  QDSP_HIP_FFT_NT, or by
                              // the overlap: 3 up to 256, 2 above, 0 where segments do not start on 64-byte boundaries (launch_fft, qdsp_hip.hip)
    int dma;                  // 1: fir_fft_dma_kernel (FIR<complex_t>, 16-byte aligned in / out, overlap <= 2048): segments arrive by LDS-DMA
    int real2;                // 1: real samples (4-byte in/out/hist); block b = real segments 2b (re) and 2b+1 (im)
    // NCO (rot only).  x[j] exp(j phi(j)) filtered by h == exp(j phi(p - (N-1))) * (x filtered by
    // h[k] exp(j k dphase)) at output position p: the input is never rotated, only the KEPT outputs are.
    unsigned long long phase_in0;   // phase of in[0] (history hand-over, de-rotation of the history)
    unsigned long long phase0;      // phase_in0 - (ntaps-1)*dphase: output at position p gets phase0 + p*dphase
    unsigned long long dphase;
    double2 rot_step;         // exp(j 2pi nwg*L*dphase): block b -> b + nwg (per-segment kernel); x dec for the grouped kernel
    float2 wtab[16];          // exp(j 2pi 256*n2*dphase)
    float gm1;                // |phase_inc| - 1 (VOLK magnitude sawtooth: a real scale of the input samples), 0 = off
};

// Tapered grid of the LDS-DMA kernels.  `slots` workgroups are resident at a time; a grid of equal workgroups ends with slots that find
// no successor while others still work through a whole one.  Here the first min(nblocks, slots) workgroups are long -- `rounds`
// stride-n_long segments each, three quarters of the whole rounds the call has, so the front stays compact and they pay one prologue
// -- and the rest of the segments goes to short workgroups in tiers: every workgroup of a tier takes `len` consecutive segments,
// len = 1/(2 slots) of what is left, rounded up, so the runs shrink to single segments at the end and the dispatcher hands them to
// whichever slot frees up first.  A function of nblocks and slots alone (2^27 samples at 256 taps: 34 953 segments = 1024 x 26 and
// 3 209 short workgroups of 5, 2 and 1); host (grid size) and kernel (a workgroup's run) walk the same tiers.
// (the long workgroups' share, measured at 2^27 samples in one process: 17 / 26 / 30 / 32 / 33 of the 34 rounds 0.430 / 0.423 / 0.426 /
// 0.439 / 0.443 ms -- the slots drift apart by more than a few segments, and only short workgroups even that out)
inline int fft_taper_rounds(int nblocks, int slots) {
    if (nblocks <= slots) return 1;
    return nblocks / slots - nblocks / (4 * slots);
}
// one tier: `rem` segments are left; returns the tier's run length and sets its workgroup count
__host__ __device__ inline int fft_taper_tier(int rem, int slots, int& cnt) {
    const int len = (rem + 2 * slots - 1) / (2 * slots);
    cnt = (rem + len - 1) / len;
    if (cnt > slots) cnt = slots;
    return len;
}
inline int fft_taper_short_count(int nblocks, int slots, int rounds) {
    const int n_long = nblocks < slots ? nblocks : slots;
    int rem = nblocks - rounds * n_long, total = 0;
    while (rem > 0) {
        int cnt;
        const int len = fft_taper_tier(rem, slots, cnt);
        total += cnt;
        rem -= cnt * len;
    }
    return total;
}

// fft1k_fir.hip: 1024-point segments, one wave each (reference-sized calls).  Same FftArgs; Hf / TA / TB point at
// that kernel's own tables (entry-major: [16][64] spectrum in its pass-C order, [16][64] W1024^(l ka), [16][4] W64^(j kb1)),
// wtab[i] = exp(j 2pi 64 i dphase), nblocks segments = the grid minus the hand-over workgroup.
constexpr int kFft1kN = 1024;
constexpr int kFft1kPitch = 84;
int launch_fir_fft1k(const FftArgs& a, hipStream_t stream);

// Defined in fft_fir.hip (its own translation unit: built with -fno-slp-vectorize, see there).
int launch_fir_fft(const FftArgs& a, int grid, hipStream_t stream);

}  // namespace qk
