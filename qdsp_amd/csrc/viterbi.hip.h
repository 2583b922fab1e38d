// viterbi.hip.h -- libcorrect's convolutional decoder (src/libcorrect/convolutional: correct_convolutional_decode[_soft] on a fresh
// object), batched over channel rows x terminated frames (gfx950).  include/qdsp_hip.h states the definition.  One launch:
//   viterbi_decode_kernel<ORDER, RATE, SOFT>  one wave per frame, kVitWaves frames per workgroup, a grid-stride loop over
//                     rows x frames; the waves of a workgroup never synchronise with each other.
//     states        2^(ORDER-1) states, state s in lane s & 63, register s >> 6 (ORDER 6: lanes 32 .. 63 idle).  With that map the
//                   two predecessors of state lane + 64 k, (s >> 1) and (s >> 1) | 2^(ORDER-2), sit in ONE lane,
//                   (lane >> 1) + 32 (k & 1), in registers k >> 1 and (k >> 1) + half: packed as a 16-bit pair they come by one
//                   cross-lane read per state (ORDER <= 7: one register, two reads), and no lane takes a branch of its own.
//     branches      a lane's two labels per state are constants in registers: as 0 / 255 byte masks (soft), so a branch metric
//                   is one v_sad_u8 of the step's packed symbols against the mask with the path metric as the addend, or as
//                   bits (hard: v_bcnt of the XOR).  Each sum is cut to 16 bits before the compare, as the uint16_t of the C code.
//     symbols       64 steps a block: every lane loads one ALIGNED dword of the block's bytes (the next block's load is issued
//                   before this block's steps), lane u then builds step u's packed symbols from two cross-lane reads and a
//                   shift by the frame's misalignment; a step costs one v_readlane.  Nothing is read bytewise from memory.
//     phases        warm-up (low predecessor only, nothing recorded), inner (tie: low), tail (tie: high).  Set 0 leaves the
//                   metrics at zero: the C code's first error_buffer_swap after a reset changes nothing (it takes the read side
//                   from the index before moving it), so what set 0 wrote is overwritten by set 1, which reads zeros.  The tail computes
//                   every state; the reference only every skip-th, but neither it nor this kernel reads the others again:
//                   searches stride by skip, a traceback from a multiple of skip stays on multiples of the earlier skips.
//     decisions     one ballot per step and register, stored in an LDS ring of 20 ORDER slices.
//     bookkeeping   the fresh object's counters are functions of the step number alone: renormalise every
//                   floor(65535 / (255 RATE)) steps, trace back at 20 ORDER, then every 15 ORDER steps; both use one search,
//                   a wave min-reduction on metric << 16 | state.
//     traceback     lane l loads slices l, l + 64, l + 128 steps back (their addresses do not depend on the path); the serial part
//                   is a chain in registers: select the 64-bit word by state >> 6, v_readlane, shift.  The emitted bits go
//                   to an LDS bit ring at their absolute positions, are packed to bytes (a byte may span two tracebacks: 15 ORDER
//                   is no multiple of 8), staged in LDS at their global address mod 64 and stored as aligned dwords; bytes only at
//                   the frame's unaligned ends.
// Bounds: a wave reads the frame's frame_in bytes through aligned dwords that hold at least one of them and writes exactly
// frame_out = (sets - ORDER + 1) / 8 bytes; frames f >= the row's count are skipped.  LDS per wave: 160 ORDER SPL + 320 bytes.
#pragma once
#include "stream_op.h"

namespace qk {

constexpr int kVitWaves = 4;                      // frames per workgroup
constexpr int kVitMaxGrid = 4096;                 // workgroups of a launch; the grid-stride loop serves the rest

struct VitArgs {
    const unsigned char* in;    // rows of frames, frame_in bytes each
    const int* in_counts;       // [nchan] or null: every row has nframes
    unsigned char* out;         // rows of frames, frame_out bytes each
    long long in_stride, out_stride;   // bytes
    int nchan, nframes, sets, frame_in, frame_out;
    unsigned poly[3];
};

}  // namespace qk

namespace qh {

// No per-row stream operator (nothing is carried from call to call): the StreamOp head is embedded for the host path only, and the
// handle is known by viterbi.hip's own set of live addresses, not by the per-row table.
struct Viterbi : StreamOp {
    int rate = 2, order = 7, sets = 0, soft = 1;
    int frame_in = 0, frame_out = 0;
    unsigned poly[3] = {0, 0, 0};
};

// the last launch of h if it is a live decoder, else null (qdsp_hip_last_kernel)
const Launch* viterbi_last(void* h);

}  // namespace qh
