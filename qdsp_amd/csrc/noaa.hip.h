// noaa.hip.h -- the NOAA HRPT tail batched over channel rows (gfx950): HRPTDemux (src/dsp/noaa/hrpt.h:36-78), TIPDemux
// (src/dsp/noaa/tip.h:31-124) and HIRSDemux (src/dsp/noaa/tip.h:136-238).  All three are bit-field gathers; bits are numbered MSB
// first as readBits does (src/dsp/utils/bitstream.h:4-42).  Every global load is an aligned dword or wider: a field is picked out
// of the aligned words around it, and no word is read that holds no byte of the row.
//   HrptDemux, a frame = 13863 bytes = 11090 words of 10 bits:
//   hrpt_avhrr_kernel  grid (nframes, nchan), 256 lanes.  The frame's bytes 937 .. 13737 (words 750 .. 10989) are staged in LDS from
//                      16-byte loads of the 16-byte blocks around them -- 937 > 15 and 13737 + 15 < 13863, so every block lies inside
//                      the frame -- byte-swapped on the way in, so that two LDS dwords give 64 frame bits in order.  13863 is odd: the
//                      offset of byte 937 in its block (0 .. 15) differs from frame to frame and is carried into every bit
//                      position.  Five passes, one per plane: lane t extracts pixels 8 t .. 8 t + 7 (words 750 + 5 p + c) and stores
//                      them as one 16-byte store where the plane's line is 16-byte aligned, else as eight 2-byte stores.
//   hrpt_scan_kernel   one workgroup per row: `minor` (bits 61 .. 62) of every frame, ranked by ballot: frame -> TIP slot, AIP slot
//                      or none; the three per-row counts (lines, TIP and AIP minor frames).
//   hrpt_gather_kernel grid (nframes, nchan), 192 lanes: a frame with a slot stages bytes 128 .. 778 (words 103 .. 622) the same way
//                      and lane q writes bytes 4 q .. 4 q + 3 of the five minor frames: one dword store where the row allows.
//   TipDemux: tip_kernel, grid (ceil(count / 64), nchan), 256 lanes: 64 minor frames (6656 bytes) go to LDS from aligned dword loads,
//                      the records go out as bytes up to the first 16-byte boundary, 16-byte stores, bytes at the end.
//   HirsDemux, the reference's serial loop in its closed form (include/qdsp_hip.h states it):
//   hirs_scan_kernel   one workgroup per row, two passes over the elements e[i] (bits 19 .. 24 of a packet): the first counts the
//                      flushes, so that only the lines that exist are cleared in the (line, slot) -> packet map; the second scans
//                      the flushes 256 packets a step and enters every surviving write in the map.  Writes the line count, the
//                      new state and the number of the line in progress.
//   hirs_pack_kernel   one lane per 8 slots of a (line, channel): two 16-byte loads of the map, the 13-bit fields of the packets it
//                      names (the carried partial line in line 0, 0xFFF elsewhere, where it names none), one 16-byte store where the
//                      address allows.  The line in progress goes to the other slot of the double-buffered partial line.
// Bounds: a row's count is min(max(in_counts[row], 0), count); frames, minor frames and packets below it are read, nothing else;
// TIP / AIP slots < 5 count; HIRS lines <= count + 1 (both flushes can fall on packet 0), the map has count + 2 lines.
#pragma once
#include "stream_op.h"

#include <vector>

#if defined(__HIPCC__)
#define QNOAA_HD __host__ __device__
#else
#define QNOAA_HD
#endif

namespace qk {

constexpr int kHrptFrameBytes = 13863;            // 110900 bits
constexpr int kHrptPixels = 2048, kHrptPlanes = 5;
constexpr int kHrptFirstByte = 937;               // word 750 begins at bit 7500 = 8 * 937 + 4
constexpr int kHrptImgBytes = 12801;              // bytes 937 .. 13737
constexpr int kHrptNT = 256;
constexpr int kHrptImgVec = (15 + kHrptImgBytes + 15) / 16;    // 16-byte blocks of the longest image
constexpr int kHrptMinorFrames = 5;               // per frame
constexpr int kTipFrame = 104;                    // bytes of a minor frame
constexpr int kHrptTipBytes = kHrptMinorFrames * kTipFrame;    // 520
constexpr int kHrptTipFirstByte = 128;            // word 103 begins at bit 1030 = 8 * 128 + 6
constexpr int kHrptTipImgBytes = 651;             // bytes 128 .. 778
constexpr int kHrptGatherNT = 192;
constexpr int kHrptScanNT = 256;

constexpr int kTipRecord = QDSP_HIP_TIP_RECORD_BYTES;
constexpr int kTipRun = 64;                       // minor frames per workgroup
constexpr int kTipNT = 256;

constexpr int kHirsPacket = 36;
constexpr int kHirsChannels = 20, kHirsLine = 56;
constexpr int kHirsNT = 256;
constexpr int kHirsState = 2;                     // ints per row: lastElement, newImageData

// byte j of a TIP record: HIRS[36] | SEM[2] | DCS[32] | SBUV[4] (src/dsp/noaa/tip.h:36-71, 75-76, 80-111, 115-118)
QNOAA_HD inline int tip_src(int j) {
    constexpr unsigned char t[kTipRecord] = {
        16, 17, 22, 23, 26, 27, 30, 31, 34, 35, 38, 39, 42, 43, 54, 55, 58, 59, 62, 63, 66, 67, 70, 71, 74, 75, 78, 79, 82, 83, 84, 85, 88, 89, 92, 93,
        20, 21,
        18, 19, 24, 25, 28, 29, 32, 33, 40, 41, 44, 45, 52, 53, 56, 57, 60, 61, 64, 65, 68, 69, 72, 73, 76, 77, 86, 87, 90, 91, 94, 95,
        36, 37, 80, 81};
    return t[j];
}
// the bit offset of radiance channel ch in a HIRS packet (src/dsp/noaa/tip.h:192-211)
QNOAA_HD inline int hirs_bit(int ch) {
    constexpr unsigned short t[kHirsChannels] = {26, 52, 65, 91, 221, 208, 143, 156, 273, 182, 119, 247, 78, 195, 234, 260, 39, 104, 130, 169};
    return t[ch];
}
// src/dsp/noaa/tip.h:136-138
QNOAA_HD inline unsigned hirs_unsigned(unsigned n) { return (n & 0x1000u) ? 0x1000u + (n & 0xFFFu) : 0xFFFu - (n & 0xFFFu); }

struct HrptArgs {
    const unsigned char* in;    // rows of frames
    const int* in_counts;       // [nchan] or null
    unsigned short* avhrr;      // [row][plane][frame][2048] by the two strides, or null
    unsigned char* tip;         // rows of minor frames, or null
    unsigned char* aip;
    int* slots;                 // [nchan][nframes]: rank (TIP), rank | 1 << 30 (AIP), -1 neither
    int* counts;                // [3][nchan]: lines, TIP minor frames, AIP minor frames (the handle's)
    int* tip_counts;            // the caller's, or null
    int* aip_counts;
    long long in_stride, row_stride, plane_stride, tip_stride, aip_stride;   // bytes, elements, elements, bytes, bytes
    int nframes, nchan;
};

struct TipArgs {
    const unsigned char* in;
    const int* in_counts;
    unsigned char* out;
    int* counts;                // [nchan] (the handle's)
    int* counts_out;            // the caller's, or null
    long long in_stride, out_stride;   // bytes
    int count;
};

struct HirsArgs {
    const unsigned char* in;
    const int* in_counts;
    unsigned short* out;
    const int* state;           // [nchan][kHirsState] (slot cur)
    int* state_next;
    const unsigned short* partial;   // [nchan][20][56] (slot cur)
    unsigned short* partial_next;
    int* map;                   // [nchan][count + 2][56]: the packet that writes (line, slot), -1 none
    int* meta;                  // [nchan]: lines emitted = the number of the line in progress
    int* counts;                // [nchan] (the handle's)
    int* counts_out;            // the caller's, or null
    long long in_stride, row_stride, plane_stride;   // bytes, elements, elements
    int count, packet_stride;
};

}  // namespace qk

namespace qh {

struct Hrpt : StreamOp {
    static constexpr OpKind kKind = OpKind::Hrpt;
    int* d_slots = nullptr;                // scratch for calls of up to scratch_frames frames per row
    unsigned char* d_tip = nullptr;        // the single-output entry points' TIP and AIP rows: [nchan][scratch_frames * 520]
    unsigned char* d_aip = nullptr;
    int64_t scratch_frames = 0;
    int64_t last_frames = 0;               // nframes of the last call: the row stride of d_slots
    int* d_counts = nullptr;               // [3][nchan]
};

struct Tip : StreamOp {
    static constexpr OpKind kKind = OpKind::Tip;
    int* d_counts = nullptr;
};

struct Hirs : StreamOp {
    static constexpr OpKind kKind = OpKind::Hirs;
    int packet_stride = qk::kHirsPacket;
    int* d_state[2] = {nullptr, nullptr};
    unsigned short* d_partial[2] = {nullptr, nullptr};
    int cur = 0;
    int* d_map = nullptr;                  // scratch for calls of up to scratch_count packets per row
    int64_t scratch_count = 0;
    int* d_meta = nullptr;
    int* d_counts = nullptr;
    int* h_count = nullptr;                // pinned: row 0's line count of the last process_ex call
};

}  // namespace qh
