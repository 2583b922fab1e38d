// fpkt.hip.h -- dsp::FalconPacketSync (src/dsp/falcon_packet.h) batched over channel rows (gfx950): the last block of the Falcon 9
// chain, behind FalconRs.  The reference's loop carries lastCounter, packetRead and a 16 KiB packet from frame to frame;
// include/qdsp_hip.h states it and its closed form.  What makes it parallel: the walk over a frame's packet headers starts with
// nothing pending whatever came before, so a frame's own packets, their end e and its tail T (-1, or the 1191 - e bytes that begin
// a packet it cannot finish) depend on the frame alone; what crosses frames is the counter check and the pending length, and a
// pending run holds at most 13 continuation frames under the cap of 16392 bytes, so every frame finds its incoming length by
// looking back over at most 14 frames.
//   fpkt_walk_kernel  grid (nframes, nchan), one wave per frame.  Bytes 0 .. 1194 go to LDS from the aligned dwords around them
//                     (frames begin at any byte; no dword is read that holds no byte of the frame).  The wave walks the chain of
//                     length fields out of LDS with a wave-uniform position (at most 396 dependent steps, a handful on real
//                     streams); lane l keeps bits 32 l .. 32 l + 31 of the map of packet starts in a register.  Out: the frame's
//                     summary {ctr, pkt | e << 16, T, packets} and the 1191-bit map of starts (40 dwords).
//                     The serial walk was built, not the parallel one (next(i) for all 1191 positions and the chain marked by
//                     pointer doubling in about 11 rounds of 1191 LDS gathers each): on a realistic stream, packets of a few
//                     hundred bytes, the walk is under ten steps a frame and the launch takes 8 us of the call's 38 at 64 rows x
//                     256 frames, a third of the pack launch.  Its worst case is measured too and is bad: frames filled with
//                     three-byte packets take 396 steps each and the launch 238 us of 264 (profiles/fpkt_rates.txt); there the
//                     parallel walk would win, and it stays the open alternative (EXPERIMENTS.md).
//   fpkt_scan_kernel  one workgroup per row, 256 frames a pass.  Frame f looks back to the nearest non-continuation frame g (or the
//                     carried state) for its incoming length in_f and the number k of continuation frames between; it emits a
//                     pending packet if in_f >= 0 and in_f + pkt_f <= 16392.  Two exclusive prefix sums (packets, bytes) give
//                     every frame its first packet index and first output byte: {in, k, packet, byte} per frame.  Lane 0 does
//                     the same look-back for the frame behind the row's last: the new packetRead, written with the new lastCounter
//                     into the other slot of the double-buffered state.  Writes the counts and d_offs[row][count].
//   fpkt_pack_kernel  grid (nframes + 1, nchan), 256 lanes.  The workgroup of a frame that emits a pending packet gathers it:
//                     g's residue (or the carried bytes), the whole data areas of the continuation frames between, its own
//                     data[0 .. pkt).  Then its own packets, one contiguous copy of data[pkt .. e), and their offset entries by
//                     rank of the start bits.  Workgroup `count` of a row gathers the packet still pending behind the last frame
//                     the same way into the other slot of the double-buffered carry (a row of no frames copies its carry over).
//                     Every copy has rs_pack_kernel's form: bytes up to the destination's 16-byte boundary, 16-byte stores built
//                     from aligned dword loads, bytes at the end.
//                     (The issue's sketch has every frame push its three pieces; here the emitting frame pulls, so that a frame
//                     needs no forward search for the frame that completes its residue.  The results are the same.)
// Bounds: a row has n = min(max(in_counts[row], 0), nframes) frames; only bytes 0 .. 1194 of frames < n are read, through aligned
// dwords that hold at least one of them.  Packets <= 397 n < out_packets(n) = 398 n, bytes <= 16392 + 1191 n per row and call: the exclusive sums stay
// below them, so every store lies in out_size(nframes) bytes / out_packets(nframes) + 1 offsets of the row.  in_f <= 16392 bounds
// the carry.
#pragma once
#include "stream_op.h"

namespace qk {

constexpr int kFpktFrame = 1195;                  // bytes read of a frame: 4 of header, 1191 of data
constexpr int kFpktHeader = 4;
constexpr int kFpktData = 1191;
constexpr int kFpktCap = 0x4008;                  // 16392: the reference's packet[]
constexpr int kFpktCont = 2047;                   // pkt of a continuation frame
constexpr int kFpktMaxWalk = kFpktData / 3;       // 397: the bound on a frame's walked packets that out_packets states (396 are reached)
constexpr int kFpktMaxRun = 13;                   // continuation frames that fit under the cap: 14 * 1191 > 16392
constexpr int kFpktBitWords = 40;                 // 1191 start bits, padded to a multiple of 16 bytes
constexpr int kFpktImgWords = (3 + kFpktFrame + 3) / 4;    // dwords of the longest image: 300
constexpr int kFpktWalkNT = 64;
constexpr int kFpktScanNT = 256;
constexpr int kFpktPackNT = 256;
constexpr int kFpktState = 2;                     // ints per row: lastCounter, packetRead

struct FpktArgs {
    const unsigned char* in;    // rows of frames, frame_stride apart
    const int* in_counts;       // [nchan] or null
    unsigned char* out;         // rows of packets back to back
    int* offs;                  // [nchan][offs_stride]: where packet k begins; [count]: the row's bytes
    const int* state;           // [nchan][kFpktState] (slot cur)
    int* state_next;
    const unsigned char* pending;    // [nchan][kFpktCap] (slot cur)
    unsigned char* pending_next;
    int4* sum;                  // [nchan][nframes]: ctr, pkt | e << 16, T, walked packets
    unsigned* bits;             // [nchan][nframes][kFpktBitWords]: bit i set: a packet begins at data[i]
    int4* pos;                  // [nchan][nframes + 1]: in, k, first packet, first byte; entry `count`: the carry's in and k
    int* counts;                // [2][nchan]: packets, bytes (the handle's)
    int* counts_out;            // the caller's, or null
    long long in_stride, out_stride, offs_stride;   // bytes, bytes, ints
    int nframes, nchan, frame_stride;
};

}  // namespace qk

namespace qh {

struct Fpkt : StreamOp {
    static constexpr OpKind kKind = OpKind::Rs;   // the Falcon tail's kind ...
    static constexpr int kSub = 1;                // ... and the table's sub-kind that tells it from the decoder (0)
    int frame_stride = 1275;
    int* d_state[2] = {nullptr, nullptr};
    unsigned char* d_pending[2] = {nullptr, nullptr};
    int cur = 0;
    int4* d_sum = nullptr;                 // scratch for calls of up to scratch_frames frames per row
    unsigned* d_bits = nullptr;
    int4* d_pos = nullptr;
    int64_t scratch_frames = 0;
    int* d_offs = nullptr;                 // the library's own offset table: [nchan][398 offs_frames + 1]
    int64_t offs_frames = 0;
    int* d_counts = nullptr;               // [2][nchan]
    int* h_count = nullptr;                // pinned: row 0's packet count of the last call (process_ex reads it)
};

}  // namespace qh
