// deframe.hip.h -- Threshold (src/dsp/processing.h:554-610) and Deframer (src/dsp/deframing.h), batched over channel rows (gfx950).
//   threshold_kernel      out[i] = in[i] > 0.0f as one byte per float.  A lane takes 16 consecutive outputs behind the row's first
//                         16-byte boundary of the OUTPUT: one 16-byte store, and four 16-byte loads where the inputs under it are
//                         aligned too (else sixteen 4-byte loads); the bytes in front of the boundary and the last, partial group go
//                         one by one.  The compare is done on the bit pattern (0 < bits <= 0x7f800000), so it does not depend on
//                         the denormal mode: NaN, -0.0f, +0.0f and negative denormals give 0, positive denormals and +Inf give 1.
//   Deframer, per row with B = the row's carried tail (the last sync_len bytes before the call; zeros after create / reset)
//   followed by the call's n bytes -- the reference's work buffer: position i of the call has frame bit B[i] and
//   match(i) = (B[i .. i + sync_len) == sync word).  Three launches on the call's stream:
//   deframe_match_kernel  grid (ceil(count / 1024), nchan), 256 lanes: a tile of 1024 positions plus a halo of sync_len - 1 bytes is
//                         staged in LDS (float rows are thresholded on the way in), every lane compares at its position (the word's
//                         first eight bytes at once, from three aligned LDS words; only a position that passes goes on byte by byte,
//                         leaving at the first byte that differs) and a wave's 64 results go out as one ballot word.  Tile 0 also writes
//                         the row's next tail, B[n .. n + sync_len).
//   deframe_walk_kernel   one wave per row, serial in EVENTS only: while reading it adds min(frame_len - bits_read, remaining) at
//                         once; after a frame it tests one bit of the match words; while searching the 64 lanes look at 64 words
//                         (4096 positions) per step and take the first set bit.  The words pass through LDS in chunks of 2048.  It
//                         writes the start position of every frame that ends in the call (negative: the frame began in an earlier
//                         call), the frame in progress at the end, the per-row frame count and the new state.
//   deframe_pack_kernel   one lane per output byte: frame m, byte b gathers B[start + 8 b + k] << (7 - k), k = 0 .. 7, truncated to a
//                         byte as the reference's `|=` into a uint8_t does.  A frame that began earlier takes the bytes it already
//                         has from the row's carry buffer (ceil(frame_len / 8) bytes) and ORs the rest in; the frame in progress at
//                         the end of the call goes to the carry buffer the same way.
//   State, tail and carry are double-buffered (read from slot cur, written to cur ^ 1): lanes of other workgroups still read the old
//   ones while one writes the new.  Every index is bounded by the row's byte count n <= count: the stage reads B below n + sync_len,
//   i.e. inputs below n; the walk reads words below ceil(n / 64) and stores at most `cap` starts; the pack reads B[j] for 0 <= j < n.
#pragma once
#include "demod.hip.h"

namespace qk {

constexpr int kThrNT = 256;                       // lanes per workgroup of threshold_kernel
constexpr int kThrPer = 16;                       // outputs per lane: one 16-byte store
constexpr int kDfNT = 256;                        // lanes per workgroup of the match and pack kernels
constexpr int kDfTile = 1024;                     // positions per workgroup of deframe_match_kernel
constexpr int kDfMaxSync = 256;                   // bytes of the longest sync word
constexpr int kDfWalkWords = 2048;                // match words per LDS chunk of deframe_walk_kernel (131072 positions)
constexpr int kDfWalkBatch = 8;                   // words a lane loads at once while it fills a chunk
constexpr int kDfState = 4;                       // ints per row: bits_read, bad, after, unused
constexpr int kDfMeta = 4;                        // ints per row and call: frames, a frame is in progress, its start, its bits so far

struct ThresholdArgs {
    const float* in;
    unsigned char* out;
    const int* in_counts;       // [nchan] or null
    long long count, in_stride, out_stride;
};

struct DeframeArgs {
    const void* in;             // rows of uint8_t (kind 0) or float (kind 1)
    const int* in_counts;       // [nchan] or null: every row has `count`
    unsigned char* out;         // rows of frames, frame_bytes each, back to back
    const unsigned char* sync;  // [sync_len]
    const unsigned char* tail;  // [nchan][sync_len] (slot cur)
    unsigned char* tail_next;
    const unsigned char* carry; // [nchan][frame_bytes] (slot cur)
    unsigned char* carry_next;
    const int* state;           // [nchan][kDfState] (slot cur)
    int* state_next;
    unsigned long long* words;  // [nchan][wstride] match bits, bit (i & 63) of word i >> 6
    int* starts;                // [nchan][cap + 1]
    int* meta;                  // [nchan][kDfMeta]
    int* counts;                // [nchan] frames of this call
    long long in_stride, out_stride, wstride;   // elements, bytes, words
    int count, cap, frame_len, frame_bytes, sync_len, nchan;
};

}  // namespace qk

namespace qh {

struct Threshold : StreamOp {
    static constexpr OpKind kKind = OpKind::Threshold;
};

struct Deframer : StreamOp {
    static constexpr OpKind kKind = OpKind::Deframer;
    int kind = 0;                          // 0 uint8_t rows, 1 float rows thresholded on load
    int frame_len = 0, frame_bytes = 0, sync_len = 0;
    std::vector<unsigned char> sync;
    unsigned char* d_sync = nullptr;
    unsigned char* d_tail[2] = {nullptr, nullptr};
    unsigned char* d_carry[2] = {nullptr, nullptr};
    int* d_state[2] = {nullptr, nullptr};
    int cur = 0;
    unsigned long long* d_words = nullptr; // scratch for calls of up to scratch_count bytes per row
    int* d_starts = nullptr;
    int64_t scratch_count = 0;
    int* d_meta = nullptr;
    int* d_counts = nullptr;
    int* h_count = nullptr;                // pinned: row 0's frame count of the last process_ex call
};

}  // namespace qh
