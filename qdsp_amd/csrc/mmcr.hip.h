// mmcr.hip.h -- MMClockRecovery<float | complex_t> (src/dsp/clock_recovery.h:68-243), the Mueller & Mueller symbol-timing loop of
// PSKDemod and MSKDemod, batched with one row per lane (gfx950).  Per symbol and row, with x the row's stream since the last reset:
//   idx = round(mu 128);  y = sum_k x[pos - 7 + k] taps[idx][k];  e = the type's phase error of y, clamped to +-1;
//   dynOmega = clamp(dynOmega + gainOmega e, omegaMin, omegaMax);  mu += dynOmega + muGain e;  pos += floor(mu);  mu -= floor(mu).
//   The step to the next symbol depends on the symbol just formed, so a row is serial; rows are independent and run as in
//   costas.hip.h: a wave takes 16 of them, lane r < 16 walking row r, all 64 lanes moving the data.
//   mm_clock_kernel<T>: grid = ceil(nchan / 16) workgroups of one wave.  A wave with R rows works in rounds of L = 64 S samples per
//   row, S = the largest power of two with R S <= 32 (R = 16: L = 128; one row: L = 2048):
//     load    R S instructions, each 64 consecutive samples of one row, into registers; issued for round c + 1 before round c is
//             walked, so they are in flight during the walk
//     stage   the registers go to the input image behind a halo of 7 samples: row pitch L + 7 samples, odd, so that the walk's
//             reads (lane = row, same sample index) fall into 16 different banks
//     walk    lane r forms the symbols whose window ends inside the round from the image and the table (129 x 8 floats, in LDS) and
//             puts them into consecutive slots of the output image (pitch L + 1): at steps of 1 the output slot overtakes the
//             window, so the walk cannot run in place.  Then it moves the last 7 samples of its row into the halo of the next round
//             (only lane r reads or writes row r between the two barriers).  A row whose step exceeds L emits nothing in some rounds.
//     store   row by row, the round's symbols go from the output image to global memory at the row's running count, coalesced
//   Arithmetic: the eight products of a symbol are exact in FP64 and are added in tap order in FP64 (an FMA chain: with an exact
//   product it rounds as the sum does), the sum is rounded to float once; everything behind it is the reference's float code,
//   every operation rounded on its own (this file is compiled with contraction off).
//   A NaN phase error stops its row: the symbol is written, nothing follows, and the row's carried mu is NaN, which is also what
//   marks a stopped row at the next call.  The clamps are v_min / v_max and drop the NaN, so the chain only ever sees finite numbers;
//   the window index is taken only while 0 <= next < n, idx is clamped to 0 .. 128, the step to >= 1, and a symbol is stored only
//   while the row's count is below `cap`.
//   The state ([nchan][kMmcrState] floats) is double-buffered: read from slot cur, written to cur ^ 1.
#pragma once
#include "demod.hip.h"

namespace qk {

constexpr int kMmcrLanes = 64;                                   // one wave per workgroup
constexpr int kMmcrRows = 16;                                    // rows per workgroup: one per lane of the wave's first quarter
constexpr int kMmcrSlots = 32;                                   // staging instructions per round, 64 samples of one row each
constexpr int kMmcrHalo = 7;                                     // samples in front of a round: the interpolator spans 8
constexpr int kMmcrSteps = 128, kMmcrTaps = 8;                   // the table: (kMmcrSteps + 1) rows of kMmcrTaps
constexpr int kMmcrTable = (kMmcrSteps + 1) * kMmcrTaps;         // 1032 floats
constexpr int kMmcrImgIn = kMmcrSlots * 64 + kMmcrRows * kMmcrHalo;   // samples of the input image: R (L + 7), R L <= 32 * 64
constexpr int kMmcrImgOut = kMmcrSlots * 64 + kMmcrRows;              // of the output image: R (L + 1)
// a row's state, in floats: mu, dynOmega, next (an int), unused, the detector (float rows: lastOutput; complex rows: p0, p1, c0,
// c1), the last 7 samples
constexpr int kMmcrState = 32, kMmcrStDet = 4, kMmcrStHist = 12;
constexpr int kMmcrPar = 4;                                      // a row's parameters: gainOmega, muGain, omegaMin, omegaMax

struct MmcrArgs {
    const void* in;             // rows of float or complex_t
    void* out;                  // rows of symbols; never aliases in
    const float* taps;          // [129][8], 16-byte aligned
    const float* par;           // [nchan][kMmcrPar]
    const float* state;         // [nchan][kMmcrState] (slot cur)
    float* state_next;          // (slot cur ^ 1)
    int* counts;                // [nchan] symbols of this call
    long long count, in_stride, out_stride;   // samples
    int cap;                    // symbols a row may store
    int nchan;
};

}  // namespace qk

namespace qh {

struct Mmcr : StreamOp {
    static constexpr OpKind kKind = OpKind::Mmcr;
    int kind = 0;                          // 0 float rows, 1 complex_t rows
    float* d_state[2] = {nullptr, nullptr};
    int cur = 0;
    float* d_par = nullptr;
    float* d_taps = nullptr;
    int* d_counts = nullptr;
    int* h_count = nullptr;                // pinned: row 0's count of the last process_ex call
    std::vector<float> par;                // [nchan][kMmcrPar]
    std::vector<float> omega, rel;         // [nchan]
    std::vector<float> taps;               // [129][8]
    int64_t min_step = 1;                  // floor(min over rows of omegaMin - |muGain|)
};

}  // namespace qh
