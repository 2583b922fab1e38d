// level.hip.h -- the two level blocks of src/dsp/processing.h that are one reduction over a call plus one pass over it (gfx950):
//   Squelch (processing.h:424-489)  the mean of |x| over the call decides whether the call is copied or zeroed
//   AGC     (processing.h:83-145)   the call is scaled by 1 / level; level decays in dB between calls and follows the call's maximum
//   Tile = kDemodNT lanes x kDemodSpl consecutive samples, blockIdx.y = channel, as in demod.hip / deemp.hip.
//     level_row_kernel      rows of at most kLevelRowTiles tiles, one launch: one workgroup per channel loads the whole row into
//                           registers (every lane its samples of every tile), reduces, applies the result to the samples it still
//                           holds and stores them: the input is read once
//     level_partial_kernel  long rows, pass 1: grid (G, nchan), lanes stride over the row as in am_partial_kernel; one FP64 partial
//                           per workgroup (Squelch: sum of |x|; AGC: the maximum, exact in FP64)
//     level_apply_kernel    long rows, pass 2: every workgroup folds its channel's G partials in the same order, derives the call's
//                           scalar (open / 1 / level) and stores its share of the row; workgroup 0 writes the next state
//   No workgroup waits for another: the two passes are two ordinary launches on one stream.  The state (AGC: float level; Squelch:
//   the decision of the last call, an int) is double-buffered like the FM phase: read from slot cur, written to cur ^ 1.
//   Squelch: sum of am_mag(x) in FP64 in a fixed tree order, mean = (float)(sum / count), open = 10.0f * log10f(mean) >= level
//   (the rule of am_sub_kernel: VOLK's float accumulator depends on the host's SIMD width).  AGC: the maximum under the
//   reference's predicate x > m from -inf (a NaN never wins; exact, whatever the order).
#pragma once
#include "demod.hip.h"

namespace qk {

constexpr int kLevelRowTiles = 4;   // rows of at most this many tiles take the one-launch form: 32 (AGC) / 64 (Squelch) VGPRs of samples
constexpr int kLevelSquelch = 0;    // KIND: float2 rows
constexpr int kLevelAgc = 1;        // KIND: float rows

struct LevelArgs {
    const float* in;            // rows of float2 (Squelch) or float (AGC); may alias out exactly (in place)
    float* out;
    const float* param;         // [nchan] Squelch: level in dB; AGC: fallRate / sampleRate
    const void* state;          // [nchan] slot cur: AGC float level (Squelch: not read)
    void* state_next;           // [nchan] slot cur ^ 1: AGC float level, Squelch int open
    double* part;               // [nchan][G]
    long long count, in_stride, out_stride;   // samples
    int tiles;                  // level_row_kernel: tiles of a row, <= kLevelRowTiles
    int G;                      // workgroups per channel of the two-pass form
    int vec;                    // 1: every row 16-byte aligned
};

// ---- device helpers shared by level.hip and stereo_fm.hip ----
// a workgroup's maximum of one float per lane under the reference's predicate (block_sum's tree)
__device__ __forceinline__ float block_max(float m, float* red) {
    const int t = threadIdx.x;
    red[t] = m;
    __syncthreads();
#pragma unroll
    for (int w = kDemodNT / 2; w > 0; w >>= 1) {
        if (t < w && red[t + w] > red[t]) red[t] = red[t + w];
        __syncthreads();
    }
    return red[0];
}

// AGC::run, the decay and the peak (processing.h:123-127): the inner expression in float, pow(10, float) in double
__device__ __forceinline__ float agc_level(float level, float cfr, long long count, float peak) {
#pragma clang fp contract(off)
    const float e = ((10.0f * log10f(level)) - (cfr * (float)count)) / 10.0f;
    level = (float)pow(10.0, (double)e);
    if (peak > level) level = peak;
    return level;
}

}  // namespace qk

namespace qh {

struct Level : StreamOp {
    static constexpr OpKind kKind = OpKind::Level;
    int kind = 0;                          // qk::kLevelSquelch / kLevelAgc
    void* d_state[2] = {nullptr, nullptr}; // 4 bytes per channel
    int cur = 0;
    float* d_param = nullptr;
    std::vector<float> param;              // Squelch: level; AGC: fall / rate
    std::vector<float> fall, rate;         // AGC
    double* d_part = nullptr;
};

}  // namespace qh
