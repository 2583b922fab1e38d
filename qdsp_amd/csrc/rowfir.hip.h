// rowfir.hip.h -- FIR<float | complex_t> (src/dsp/filter.h:51-74) over nchan channel rows, and DelayImag (src/dsp/processing.h:300-344),
// the two stages PSKDemod needs in batched form (gfx950).  Both are ordinary launches with blockIdx.y = channel and a tile of
// kDemodNT lanes x kDemodSpl consecutive samples, as in demod.hip / stereo_fm.hip.
//   row_fir_kernel<NC>   y[c][i] = sum_k taps[c][k] x[c][i - (T - 1) + k], direct form, NC = floats per sample (1 float rows, 2
//                        complex_t rows; the taps are real).  It is pilot_fir_kernel (stereo_fm.hip.h) without the maximum and with
//                        taps per channel: a workgroup stages its kRowFirTile + T - 1 inputs in LDS (the halo from the carried
//                        history where the tile starts before sample T - 1 of the call); a lane keeps a sliding register window of
//                        12 samples over its 8 consecutive outputs and refills four samples of it per four taps.  The taps are read
//                        with a wave-uniform index (blockIdx.y is the channel: scalar loads).  Every output component is the chain
//                        acc = fmaf(taps[k], x, acc), k = 0 .. T - 1 from +0.0f -- no zero taps are padded in, the last T % 12 taps
//                        run the same chain one LDS sample per FMA -- so its bits depend on the taps and the T samples under them
//                        alone: the bits of qdsp_hip_fir_cf32 / _f32 in QDSP_HIP_FIR_DIRECT mode.
//                        LDS reads, by the bank rule of ds_read_b128 (four groups of 16 lanes, bank = (byte address / 4) mod 64):
//                          float rows    a lane's window advances 32 bytes per lane: lane l reads the 16-byte slots 2 l + k / 4, in a
//                                        lane group two lanes meet on every other slot (2-way, pilot_fir_kernel's count): 8 LDS
//                                        cycles per wave and read against the 32 FMAs (128 VALU cycles) that follow it.
//                          complex rows  the window advances 64 bytes per lane: lane l covers banks 16 l .. 16 l + 3 (mod 64), so
//                                        lanes l and l + 4 meet; a group ({0-3, 12-15, 20-27}, ...) holds four lanes of every
//                                        residue mod 4: 4-way, 16 LDS cycles per wave and read.  One read brings two complex samples
//                                        = 2 taps x 8 outputs x 2 components = 32 FMAs: 128 VALU cycles of that wave's SIMD as
//                                        v_fmac_f32, 64 as the 16 v_pk_fma_f32 the kernel issues (re and im of a sample as one
//                                        two-wide fma, fused per component: the same bits).  With the four SIMDs of a CU reading at
//                                        once that is 64 LDS cycles per 128 or 64 VALU cycles: half as busy as the VALU in the
//                                        scalar form, as busy as it in the packed one.  Measured at 361 taps (profiles/
//                                        psk_rates.txt, EXPERIMENTS.md): the scalar form at 0.95 of the v_fmac_f32 issue rate, the
//                                        packed one at 1.5 of it -- 0.75 of its own.  The plain map stays: a padded or swizzled image
//                                        costs every read its address arithmetic, and the filter is 0.3 % of a chain's time.
//                        The workgroups over the last T - 1 samples write the next history (slot cur ^ 1; readers see slot cur): a
//                        tile may read the history another tile rewrites.  No workgroup waits for another.
//   delay_imag_kernel    out[i] = {in[i].re, in[i - 1].im}, in[-1].im = the row's carried lastIm (slot cur; the lane that holds the
//                        call's last sample writes slot cur ^ 1).  Bit copies only: the samples move as 32-bit integers.
#pragma once
#include "demod.hip.h"

namespace qk {

constexpr int kRowFirMaxTaps = 4096;                               // the pilot filter's cap
constexpr int kRowFirTile = kDemodNT * kDemodSpl;                  // outputs per workgroup
constexpr int kRowFirLds = kRowFirTile + kRowFirMaxTaps + 16;      // samples: the tile, the halo, and the window's read-ahead
constexpr int kRowFirGroup = 12;                                   // taps per unrolled group of the tap loop

struct RowFirArgs {
    const float* in;            // rows of NC floats per sample, in_stride samples apart
    float* out;                 // out_stride samples apart; never overlaps in
    const float* taps;          // [nchan][T]
    const float* hist;          // [nchan][T - 1] samples, slot cur: the last T - 1 inputs before this call
    float* hist_next;           // slot cur ^ 1
    long long count, in_stride, out_stride;
    int T;
    int tiles;
    int vec;                    // 1: every output row 16-byte aligned
};

struct DelayImagArgs {
    const uint2* in;            // complex_t rows as pairs of 32-bit words
    uint2* out;
    const unsigned* last;       // [nchan] slot cur
    unsigned* last_next;        // [nchan] slot cur ^ 1
    long long count, in_stride, out_stride;
};

}  // namespace qk

namespace qh {

struct RowFir : StreamOp {
    static constexpr OpKind kKind = OpKind::RowFir;
    int kind = 0;                          // 0 float rows, 1 complex_t rows
    int ntaps = 0;
    float* d_taps = nullptr;               // [nchan][ntaps]
    float* d_hist[2] = {nullptr, nullptr}; // [nchan][ntaps - 1] samples; read from slot cur, written to cur ^ 1
    int cur = 0;
    std::vector<float> taps;               // [nchan][ntaps]
};

struct DelayImagOp : StreamOp {
    static constexpr OpKind kKind = OpKind::DelayImag;
    unsigned* d_last[2] = {nullptr, nullptr};   // [nchan] lastIm, as bits
    int cur = 0;
};

}  // namespace qh
