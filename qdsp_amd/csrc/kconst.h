// kconst.h -- the kernel constants that kernel selection and filter planning read (select.cpp), in plain C++: the kernel headers
// include this file, so each constant is still defined once.
#pragma once
#include <stddef.h>

namespace qk {

constexpr int kFftN = 4096;       // fft_fir.hip.h: points per overlap-save segment

constexpr int kPfbD = 8;          // pfb_dec.hip.h: decimation = number of polyphase columns
constexpr int kPfbSeg = 4096;     // input samples per segment
constexpr int kPfbMaxQ = 136;     // taps per column the dispatch accepts (>= 377 valid outputs per 512; 1024 taps at decimation 4 need 129)

constexpr int kMfMaxKJ = 16;      // mf_dec.hip.h: K / 8: decimations up to 128
constexpr int kMfMaxQ = 32;       // taps per column: two sets of 16 rows of the A operand

constexpr int kRmNE = 12;         // rm_resamp.hip.h: samples per lane and tile held in registers: 4 G M + ext <= 768
constexpr int kRmMaxGrp = 3;      // groups of 16 blocks = 64 outputs per period: L <= 192
constexpr int kRmMaxKB = 40;      // band columns per block

inline size_t rm_lds_bytes(int ngrp, int KB, int G, int pitch, bool real = false) {
    return (size_t)((ngrp * KB * 64 + 2 * ngrp * 64 + 3) & ~3) * 4 + 4 * ((size_t)4 * G * pitch + 64) * (real ? 4 : 8);      // A operands + block tables + four waves' tiles
}

}  // namespace qk

namespace qh {

constexpr int kMaxDynLds = 64 * 1024;  // default dynamic-LDS ceiling; tiles are sized under it

}  // namespace qh
