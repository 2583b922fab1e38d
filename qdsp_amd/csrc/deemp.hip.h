// deemp.hip.h -- BFMDeemp (src/dsp/filter.h:90-173), the 50 / 75 us de-emphasis filter, as a batched parallel scan (gfx950).
//   y[i] = alpha x[i] + (1 - alpha) y[i-1] is one affine map y -> A y + B per sample, (A, B) = (b, a x[i]); affine maps compose
//   associatively, (A2, B2) o (A1, B1) = (A2 A1, A2 B1 + B2), so a row is a prefix scan.  a = (double)alpha and
//   b = (double)(float)(1.0f - alpha) are the reference's own float coefficients; the composition runs in FP64 and every output is
//   rounded to float once (a reassociated scan cannot repeat the reference's float loop bit for bit; it is held to the exact
//   recurrence instead: tests/test_gpu_deemp.py).
//   Tile = kDemodNT lanes x kDemodSpl consecutive samples.  A lane folds its samples into one pair; the 64 pairs of a wave are
//   scanned by cross-lane moves; the four wave totals go through a few LDS words (one barrier pair per tile); the lane replays its
//   samples from its exclusive prefix.  The scan of a tile and the tiles -> chunks geometry are scan.hip.h (cagc.hip uses them too).
//     deemp_row_kernel      short rows, one launch: one workgroup per channel walks the row tile by tile
//     deemp_partial_kernel  long rows, pass 1: workgroup g folds the T tiles of chunk g into one FP64 pair (the last chunk is skipped:
//                           nothing follows it)
//     deemp_scan_kernel     long rows, pass 2: workgroup g folds the pairs of the chunks before it onto the carried state (Horner,
//                           at most kAmMaxParts - 1 of them, the same order in every workgroup), then scans and stores chunk g
//   No workgroup waits for another: the two passes are two ordinary launches on one stream.  The state (FP64 per channel and
//   component) is double-buffered like the FM phase: read from slot cur, written to cur ^ 1 by the lane that owns the last sample.
//   A state that is not finite reads as 0 (the reference's NaN rule, extended to +-Inf: see include/qdsp_hip.h).
#pragma once
#include "demod.hip.h"

namespace qk {

constexpr int kDeempRowTiles = 16;   // rows of at most this many tiles take the one-launch form

struct DeempArgs {
    const float* in;            // rows of float (mono) or float2 {l, r} (stereo); may alias out exactly (in place)
    float* out;
    const float* alpha;         // [nchan]
    const double* state;        // [nchan][NC] (slot cur)
    double* state_next;         // [nchan][NC] (slot cur ^ 1)
    double* part;               // [nchan][G][1 + NC]: A, B per component, of chunk g
    long long count, in_stride, out_stride;   // samples
    long long T;                // tiles per chunk
    int G;                      // chunks per channel
    int vec;                    // 1: every row 16-byte aligned
};

}  // namespace qk

namespace qh {

struct Deemp : StreamOp {
    static constexpr OpKind kKind = OpKind::Deemp;
    int kind = 0;                          // QDSP_HIP_DEEMP_MONO / _STEREO
    bool bypass = false;
    double* d_state[2] = {nullptr, nullptr};
    int cur = 0;
    float* d_alpha = nullptr;
    std::vector<float> alpha;
    double* d_part = nullptr;
};

}  // namespace qh
