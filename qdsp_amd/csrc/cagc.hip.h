// cagc.hip.h -- ComplexAGC (src/dsp/processing.h:235-298), the per-sample feedback AGC on complex samples, as a batched clamped
// prefix scan (gfx950).
//   out[i] = in[i] g;  g += (setPoint - |out[i]|) rate;  if (g > maxGain) g = maxGain.   While g >= 0, |in[i] g| = |in[i]| g, so a
//   sample is the map g -> min(a_i g + b, c) with a_i = 1 - rate |in[i]|, b = setPoint rate, c = maxGain.  For a >= 0 these maps
//   are closed under composition and associative,
//       (a2, b2, c2) o (a1, b1, c1) = (a2 a1,  a2 b1 + b2,  min(a2 c1 + b2, c2)),
//   so a row is a prefix scan: deemp.hip.h with a third component for the clamp.  out[i] takes the gain before sample i, the
//   exclusive prefix a lane holds anyway.  r, setPoint, maxGain are the reference's floats widened; |x| = sqrt(re^2 + im^2) and
//   a = fma(-r, |x|, 1) in FP64; every output is (float)(x g), the FP64 product rounded to float.  A reassociated FP64 scan
//   cannot repeat the reference's float loop bit for bit; it is held to the exact recurrence instead (tests/test_gpu_cagc.py).
//   The identity that pads ragged tiles and stands left of lane 0 is (1, 0, DBL_MAX), not (1, 0, +inf): a sample with a == 0
//   exactly (rate |x| == 1) would meet it as 0 * inf.  A maxGain of +inf is clamped to DBL_MAX for the same reason.
//   Tile = kDemodNT lanes x kDemodSpl consecutive samples, scanned as in deemp.hip.h: the same tile_scan and chunk geometry
//   (scan.hip.h), here over Clamp maps.
//     cagc_row_kernel      short rows, one launch: one workgroup per channel sweeps the row once to check the domain, then tile by tile
//     cagc_partial_kernel  long rows, pass 1: workgroup g folds the T tiles of chunk g into one FP64 triple and records whether
//                          every sample of the chunk is in the domain
//     cagc_scan_kernel     long rows, pass 2: workgroup g folds the triples of the chunks before it onto the carried gain (at most
//                          kAmMaxParts - 1, the same order in every workgroup), then scans and stores chunk g
//     cagc_serial_kernel   the rows out of the domain (below), one wave each; returns at once for every other row
//   No workgroup waits for another: ordinary launches on one stream.  The gain (FP64 per channel, 1 at creation) is double-buffered:
//   read from slot cur, written to cur ^ 1 by the lane that owns the last sample.
//   The domain.  The scan is the reference's recurrence only while the gain cannot turn negative and no sample poisons it.  A row
//   is in the domain for a call if the carried gain is finite and >= 0, 0 <= b < inf, c >= 0, rate >= 0, and every sample is
//   finite with a_i >= 0 (rate |x| <= 1).  (rate >= 0 and b < inf are added to what the algebra needs: a_i > 1 overflows the
//   product of a chunk, b = inf meets a == 0.)  Pass 1 records this per chunk with ordinary vector stores; the scan writes nothing
//   to a row that fails, state included; the host never waits on the decision.
//   The serial path.  cagc_serial_kernel runs a failed row with the reference's loop in FP32: every product and sum rounded
//   separately, no contraction, correctly rounded sqrtf, from (float) of the carried gain.  Outputs and the gain (widened back into
//   the state) are the float loop's bit for bit: NaN, Inf and negative gains behave as in the reference.  It is serial: one
//   wave, one sample after the other (loads and stores are 64 samples wide) -- 110 us per 1000 samples measured
//   (profiles/cagc_rates.txt), some 10 000 times the scan's time per sample of a full batch, and a call lasts as long as its
//   slowest row: 64 rows of 65 536 take 44 us scanned and 7.4 ms with one of them here.  It is there so that such a row is right,
//   not fast.
#pragma once
#include "demod.hip.h"

namespace qk {

constexpr int kCagcRowTiles = 16;   // rows of at most this many tiles take the one-launch form
constexpr int kCagcPart = 4;        // doubles per chunk: a, b, c, out-of-domain flag

struct CagcArgs {
    const float* in;            // rows of complex_t {re, im}; may alias out exactly (in place)
    float* out;
    const float* par;           // [nchan][3]: setPoint, maxGain, rate
    const double* state;        // [nchan] gain (slot cur)
    double* state_next;         // [nchan] (slot cur ^ 1)
    double* part;               // [nchan][G][kCagcPart]
    long long count, in_stride, out_stride;   // samples
    long long T;                // tiles per chunk
    int G;                      // chunks per channel
    int vec;                    // 1: every row 16-byte aligned
};

}  // namespace qk

namespace qh {

struct Cagc : StreamOp {
    static constexpr OpKind kKind = OpKind::Cagc;
    double* d_state[2] = {nullptr, nullptr};
    int cur = 0;
    float* d_par = nullptr;
    std::vector<float> par;                // [nchan][3]
    double* d_part = nullptr;
};

}  // namespace qh
