// costas.hip.h -- CostasLoop<ORDER> (src/dsp/pll.h:47-102), the carrier-recovery loop of PSKDemod, batched with one row per lane
// (gfx950).  Per sample and row:
//   out = vco * in;  e = error<ORDER>(out) clamped to +-1;  freq = clamp(freq + beta e, +-1);  phase += freq + alpha e, wrapped into
//   [-T, T] with T the reference's float 2 pi;  vco = (cos(-phase), sin(-phase)).
//   The error detectors of orders 4 and 8 are discontinuous, so nothing composes along a row: a row is serial.  Rows are
//   independent, so a wave takes 16 of them, lane r < 16 walking row r, all in lockstep.  Only the first quarter of the wave
//   walks: the step time grows with the number of 16-lane groups that hold an active lane (measured with 64, 32 and 16 rows on a
//   wave: EXPERIMENTS.md; the kept form: profiles/costas_rates.txt).  All 64 lanes move the data.
//   costas_kernel<ORDER>: grid = ceil(nchan / 16) workgroups of one wave.  A wave with R rows (16 but for the last) works in rounds
//   of L = 64 S samples per row, S = the largest power of two with R S <= 64 (R = 16: L = 256; one row: L = 4096), so that a round
//   stages about the same bytes whatever R is:
//     load    R S instructions, each 64 lanes x 8 bytes of one row (512 contiguous bytes), into registers; issued for round c + 1
//             before round c is walked, so they are in flight during the walk
//     stage   the registers go to the LDS image, row pitch L + 1 samples: odd in 8-byte units, so the walk's ds_read_b64 (lane = row,
//             same sample index) hits 16 different bank pairs
//     walk    lane r runs samples 0 .. n - 1 of row r from the image and writes each output over its input
//     store   the image goes back to global memory the way it came, 512 contiguous bytes per instruction
//   Rows are read and written with 8-byte accesses only, so every row layout takes the same path; in place works because round c is
//   stored after rounds c and c + 1 have been read.
//   Arithmetic: alpha and beta are the reference's floats (its mixed float / double formula, on the host); frequency and phase are
//   carried in FP64, and the mix, the error, both clamps, the wrap and the sine / cosine are FP64; each output is rounded to float
//   once.  The sine and cosine are this file's own: |phase| <= T always, so one multiple k of pi / 2 (|k| <= 4) is taken off and two
//   Taylor polynomials on [-pi / 4, pi / 4] are evaluated by Estrin's scheme (truncation < 7e-12); no table, no large-argument path.
//   The wrap is one conditional step each way: for the alpha of a finite bandwidth >= 0, |freq + alpha e| <= 1.83 < T.
//   The chain: clamps are v_min / v_max, which drop a NaN; the reference's compare-and-assign clamps keep it.  So a NaN error is
//   recorded in a flag off the chain instead: from that sample on the row's outputs are NaN and its carried state is NaN, as in the
//   reference, while the chain itself only ever sees finite numbers.  A carried frequency or phase that is not finite reads as 0.
//   The state ([nchan][2] FP64: frequency, phase) is double-buffered: read from slot cur, written to cur ^ 1.
#pragma once
#include "demod.hip.h"

namespace qk {

constexpr int kCostasLanes = 64;                                 // one wave per workgroup
constexpr int kCostasRows = 16;                                  // rows per workgroup: one per lane of the wave's first quarter
constexpr int kCostasSlots = 64;                                 // staging instructions per round, 512 bytes of one row each
constexpr int kCostasImg = kCostasSlots * 64 + kCostasRows;      // float2 slots of the LDS image: R (L + 1), R L <= 64 * 64

struct CostasArgs {
    const float2* in;           // rows of complex_t; may alias out exactly (in place)
    float2* out;
    const float* par;           // [nchan][2]: alpha, beta
    const double* state;        // [nchan][2]: frequency, phase (slot cur)
    double* state_next;         // (slot cur ^ 1)
    long long count, in_stride, out_stride;   // samples
    int nchan;
};

}  // namespace qk

namespace qh {

struct Costas : StreamOp {
    static constexpr OpKind kKind = OpKind::Costas;
    int order = 2;
    double* d_state[2] = {nullptr, nullptr};
    int cur = 0;
    float* d_par = nullptr;
    std::vector<float> par;                // [nchan][2]
};

}  // namespace qh
