// ff_agc.hip.h -- FeedForwardAGC<T> (src/dsp/processing.h:147-233) over nchan channel rows (gfx950).  With the stream of all samples
// ever handed in, x[0], x[1], ..., and the window W (the reference: 1024)
//   y[p] = x[p] / level[p],   level[p] = max(1e-4f, max over j in [0, W) of a(x[p + j]))
//   float rows:     a(v) = fabsf(v)
//   complex_t rows: a(v) = r + 0.4f * r with r = fabsf(v.re) (fastAmplitude, types.h:58-63, takes both of its magnitudes from
//                   re: kept as it stands), product and sum each rounded; y = {re / level, im / level}
// under the reference's predicate `val > level` from 1e-4f: a NaN never wins, +Inf does.  a is non-decreasing in r (a rounded
// product and a rounded sum of non-decreasing operands), so the kernel takes the window maximum of r = fabsf(re) -- a NaN staged
// as +0.0f, which never wins either -- and applies a once per output: max(1e-4f, a(max r)) is the reference's level exactly.
// The maximum of NaN-free floats is exact in any order; the division is the IEEE one.
//
// ff_agc_kernel, grid (tiles [+ 1], nchan), kDemodNT lanes, one workgroup per kFfAgcTile consecutive outputs of one row.  The row
// it works on is [history | in]: the channel's `fill` <= W - 1 samples not yet output (slot cur), then the call's `count`.
//   stage    r of its kFfAgcTile + W - 1 samples into LDS, lane-strided; a lane keeps its own 8 samples in registers, so the
//            input is read once (plus the halo)
//   maxima   by doubling: M_j[p] = max r[p .. p + 2^j), M_(j+1)[p] = max(M_j[p], M_j[p + 2^j]), ping-pong between two LDS
//            arrays, 16 bytes per lane and instruction on consecutive addresses (no bank conflict); the first pass forms M_2
//            from r directly.  With k = floor(log2 W) the window is max(M_k[p], M_k[p + W - 2^k]): the offset combine, which
//            also applies a and the floor 1e-4f.
//   store    y = x / level from the registers.  Rows that are not 16-byte aligned: 4 or 8 bytes per lane, lane-strided.
//            Aligned rows: the quotients pass through LDS once more and leave as 16 bytes per lane.  Same arithmetic, same bits.
// Chosen over the block prefix / suffix scheme (van Herk, Gil-Werman): its two running maxima per block of W are serial chains of
// W steps, and a tile of 2048 + 1023 samples holds three such blocks -- six chains for 256 lanes; run in parallel each chain is
// itself a log2 W scan.  Doubling keeps every lane busy in every pass.  Per tile, with L = (kFfAgcTile + W - 1) rounded up to 4:
// LDS 2 * L * 4 bytes (24576 at W = 1024, 49152 at 4096); barriers 1 (stage) + max(k - 1, k > 0) (passes) + 1 (combine), and
// 2 more on the 16-byte store path: 11 / 13 at W = 1024.
// Measured (profiles/ff_agc_rates.txt, W = 1024): 64 rows of 65536 take 30.5 us complex / 29.3 us float (2.2 / 1.1 TB/s of samples read
// once and written once); the same kernel at W = 1 takes 12.1 / 7.7 us, so the halo and the maxima are 0.6 / 0.74 of the call: the
// tile's LDS work, the same for 4- and 8-byte samples, sets the time, not memory.
// The last workgroup of a row (blockIdx.x == tiles, present when the next fill > 0) writes the next history -- the last fill'
// samples of [history | in] -- into slot cur ^ 1.  No workgroup waits for another; a call that emits nothing is that copy alone.
#pragma once
#include "demod.hip.h"

namespace qk {

constexpr int kFfAgcTile = kDemodNT * kDemodSpl;   // outputs per workgroup
constexpr int kFfAgcMaxWindow = 4096;              // (the staged halo of pilot_fir_kernel)
constexpr int kFfAgcReal = 0;                      // KIND: float rows
constexpr int kFfAgcComplex = 1;                   // KIND: complex_t rows

struct FfAgcArgs {
    const float* in;            // rows of float / float2, in_stride samples apart
    float* out;                 // rows of `nout` outputs, out_stride samples apart; never overlaps in
    const float* hist;          // [nchan][hstride] slot cur: the `fill` samples not yet output, oldest first
    float* hist_next;           // [nchan][hstride] slot cur ^ 1
    long long count, in_stride, out_stride;   // samples
    long long nout;             // outputs of this call: max(0, fill + count - (W - 1))
    int W, k;                   // k = floor(log2 W)
    int fill, fill_next;
    int hstride;                // samples
    int tiles;                  // ceil(nout / kFfAgcTile)
    int L;                      // floats per LDS array
    int vec;                    // 1: every output row 16-byte aligned
};

// floats per LDS array / dynamic LDS bytes of a launch
constexpr int ff_agc_L(int W) { return (kFfAgcTile + W - 1 + 3) & ~3; }
constexpr int ff_agc_lds(int W) { return 2 * ff_agc_L(W) * (int)sizeof(float); }

}  // namespace qk

namespace qh {

struct FfAgc : StreamOp {
    static constexpr OpKind kKind = OpKind::FfAgc;
    int kind = 0;                          // qk::kFfAgcReal / kFfAgcComplex
    int window = 1024;
    float* d_hist[2] = {nullptr, nullptr}; // read from slot cur, written to cur ^ 1
    int cur = 0;
    int fill = 0;                          // samples held, the same for every row
};

}  // namespace qh
