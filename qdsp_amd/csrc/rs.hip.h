// rs.hip.h -- Reed-Solomon decoding of interleaved frames (FalconRS: src/dsp/falcon_fec.h), batched over channel rows x frames
// (gfx950).  The algebra is libcorrect's correct_reed_solomon_decode, bit for bit (include/qdsp_hip.h states it).  Three launches:
//   rs_decode_kernel  grid (nframes, nchan), one wave per codeword: the I waves of a frame share a workgroup, so the frame's verdict
//                     is one LDS flag.  exp / log and the two byte maps sit in LDS (1280 bytes); the frame is staged once, through
//                     the input map and de-interleaved, from ALIGNED dword loads (the frame's bytes are picked out of the words
//                     around them: frames are skip + 255 I bytes long, so most start misaligned).  Per wave:
//                       syndromes  a lane takes coefficients 4 lane .. 4 lane + 3 and walks the roots with running exponents; four
//                                  syndromes to a dword, each dword XOR-reduced over the wave in six steps;
//                       locator    libcorrect's Berlekamp-Massey, serial in its num_roots steps: lane j holds coefficient j of the
//                                  locator and of the last locator, the discrepancy is a wave XOR-reduction, the shift by the delay
//                                  one cross-lane read.  Orders, delay and the coefficients above an order are tracked as the C
//                                  code tracks them (its order is a maximum, not a degree; stale coefficients stay);
//                       roots      four passes of 64 elements, counted and ranked by ballot; a count != order fails the codeword;
//                       values     lane m forms coefficient m of S Lambda mod x^num_roots, then lane r serves root r: position,
//                                  Omega / Lambda' and the XOR into the staged codeword.
//                     A good frame goes to its scratch slot already re-interleaved, through the output map and the XOR sequence
//                     (expanded to the frame's length on the host), with one flag byte per frame.
//   rs_scan_kernel    one workgroup per row: the exclusive scan of the good flags (ballots, 256 frames a step) gives every good
//                     frame its slot, and the row its count.
//   rs_pack_kernel    grid (nframes, nchan): a good frame is copied to its slot: bytes up to the destination's first 16-byte
//                     boundary, 16-byte stores built from aligned dword loads of the scratch slot, bytes at the end.
// Multiplication is by table: exp[log a + log b] from LDS (a shift-and-reduce product in VALU is the unmeasured alternative).
// Bounds: a workgroup reads its frame's bytes [f * frame_in + skip, + 255 I) of the row and the aligned words that hold them;
// f < the row's frame count <= nframes; scratch, flags and slots are [nchan][nframes]; the pack writes slot < count <= nframes.
#pragma once
#include "demod.hip.h"
#include "rs_tables.h"

namespace qk {

constexpr int kRsMaxDepth = qrs::kMaxDepth;
constexpr int kRsTab = 1280;                      // exp[512] log[256] in_map[256] out_map[256]; the expanded XOR sequence follows
constexpr int kRsScanNT = 256;
constexpr int kRsPackNT = 128;
constexpr int kRsSlotPad = 16;                    // bytes behind a scratch slot's 16-byte multiple (the pack reads whole dwords)

struct RsArgs {
    const unsigned char* in;    // rows of frames, frame_in bytes each
    const int* in_counts;       // [nchan] or null: every row has nframes
    unsigned char* out;
    const unsigned char* tab;   // kRsTab bytes, then xor_full[frame_out]
    unsigned char* scratch;     // [nchan][nframes][slot]
    unsigned char* good;        // [nchan][nframes]
    int* slots;                 // [nchan][nframes]: the frame's output slot, -1 dropped
    int* counts;                // [nchan]
    int* errs;                  // [nchan][nframes * depth] or null
    long long in_stride, out_stride;   // bytes
    int nframes, depth, skip, nroots, k;
    int g0, gap, gap_inv, fpow;        // (gap * first_root) % 255, gap, its inverse mod 255, (first_root - 1) mod 255
    int frame_in, frame_out, slot;     // bytes
};

}  // namespace qk

namespace qh {

struct Rs : StreamOp {
    static constexpr OpKind kKind = OpKind::Rs;
    qrs::Params p;
    qrs::Field field;
    std::vector<unsigned char> tab;     // host copy of the device tables
    int slot = 0;
    unsigned char* d_tab = nullptr;
    unsigned char* d_scratch = nullptr; // for calls of up to scratch_frames frames per row
    unsigned char* d_good = nullptr;
    int* d_slots = nullptr;
    int64_t scratch_frames = 0;
    int* d_counts = nullptr;
    int* h_count = nullptr;             // pinned: row 0's count of the last process_ex call
};

}  // namespace qh
