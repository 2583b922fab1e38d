// noaa.hip -- HrptDemux, TipDemux and HirsDemux batched over channel rows (design notes: noaa.hip.h), and their C entry points.
#include "noaa.hip.h"

#include <cstring>
#include <new>

namespace qk {

namespace {

// items of row `row` in this call
__device__ __forceinline__ int row_count(const int* in_counts, int row, int count) {
    if (!in_counts) return count;
    const int c = in_counts[row];
    return c < 0 ? 0 : (c < count ? c : count);
}

// `len` bits (at most 17) from bit `bit` of the bytes at p, MSB first: out of the aligned dwords that hold the field's first and
// last byte, and no other
__device__ __forceinline__ unsigned bits_at(const unsigned char* p, int bit, int len) {
    const uintptr_t a0 = (uintptr_t)p + (uintptr_t)(bit >> 3), a1 = (uintptr_t)p + (uintptr_t)((bit + len - 1) >> 3);
    const unsigned* w = reinterpret_cast<const unsigned*>(a0 & ~(uintptr_t)3);
    const unsigned lo = w[0];
    const unsigned hi = ((a1 ^ a0) & ~(uintptr_t)3) ? w[1] : 0u;
    const unsigned be = __builtin_bswap32(__builtin_amdgcn_alignbyte(hi, lo, (unsigned)(a0 & 3)));   // bytes a0 .. a0 + 3, first byte on top
    return (be >> (32 - (bit & 7) - len)) & ((1u << len) - 1u);
}

// `len` bits from bit `bit` of an LDS image of byte-swapped dwords (dword i holds image bits 32 i .. 32 i + 31, first bit on top);
// img[i + 1] exists
__device__ __forceinline__ unsigned img_bits(const unsigned* img, int bit, int len) {
    const int i = bit >> 5;
    const unsigned long long v = ((unsigned long long)img[i] << 32) | img[i + 1];
    return (unsigned)(v >> (64 - (bit & 31) - len)) & ((1u << len) - 1u);
}

__device__ __forceinline__ void store8(unsigned short* dst, const unsigned (&px)[8]) {
    if (((uintptr_t)dst & 15) == 0) {
        *reinterpret_cast<uint4*>(dst) = make_uint4(px[0] | (px[1] << 16), px[2] | (px[3] << 16), px[4] | (px[5] << 16), px[6] | (px[7] << 16));
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) dst[k] = (unsigned short)px[k];
    }
}

__device__ __forceinline__ int hirs_elem(const unsigned char* pkt) { return (int)bits_at(pkt, 19, 6); }

}  // namespace

__global__ __launch_bounds__(kHrptNT) void hrpt_avhrr_kernel(const HrptArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned img[4 * kHrptImgVec + 4];
    const int f = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
    if (f >= row_count(a.in_counts, row, a.nframes)) return;
    // bytes 937 .. 13737 of the frame and the 16-byte blocks around them: all inside the frame
    const unsigned char* src = a.in + (long long)row * a.in_stride + (long long)f * kHrptFrameBytes + kHrptFirstByte;
    const int mis = (int)((uintptr_t)src & 15);
    const uint4* v = reinterpret_cast<const uint4*>(src - mis);
    const int nv = (mis + kHrptImgBytes + 15) >> 4;            // <= kHrptImgVec
    constexpr int kPer = (kHrptImgVec + kHrptNT - 1) / kHrptNT;
    uint4 r[kPer];
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int j = u * kHrptNT + t;
        r[u] = j < nv ? v[j] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int j = u * kHrptNT + t;
        if (j < nv)
            reinterpret_cast<uint4*>(img)[j] =
                make_uint4(__builtin_bswap32(r[u].x), __builtin_bswap32(r[u].y), __builtin_bswap32(r[u].z), __builtin_bswap32(r[u].w));
    }
    __syncthreads();
    // word 750 + 5 p + c begins at image bit 8 mis + 4 + 50 p + 10 c; the last one ends in dword <= 4 nv - 1, so img[i + 1] is in the array
    const int bit0 = 8 * mis + 4 + 400 * t;
    unsigned short* line = a.avhrr + (long long)row * a.row_stride + (long long)f * kHrptPixels + 8 * t;
#pragma unroll
    for (int c = 0; c < kHrptPlanes; c++) {
        unsigned px[8];
#pragma unroll
        for (int k = 0; k < 8; k++) px[k] = img_bits(img, bit0 + 50 * k + 10 * c, 10);
        store8(line + (long long)c * a.plane_stride, px);
    }
}

__global__ __launch_bounds__(kHrptScanNT) void hrpt_scan_kernel(const HrptArgs a) {
    __shared__ int wt[2][kHrptScanNT / 64];
    const int row = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n = row_count(a.in_counts, row, a.nframes);
    const unsigned char* in = a.in + (long long)row * a.in_stride;
    int* slots = a.slots + (long long)row * a.nframes;
    int ntip = 0, naip = 0;
    for (int base = 0; base < n; base += kHrptScanNT) {
        const int i = base + t;
        const int minor = i < n ? (int)bits_at(in + (long long)i * kHrptFrameBytes, 61, 2) : -1;
        const unsigned long long bt = __ballot(minor == 1), ba = __ballot(minor == 3);
        if (lane == 0) {
            wt[0][wv] = __popcll(bt);
            wt[1][wv] = __popcll(ba);
        }
        __syncthreads();
        int ot = 0, oa = 0, tt = 0, ta = 0;
#pragma unroll
        for (int k = 0; k < kHrptScanNT / 64; k++) {
            if (k < wv) {
                ot += wt[0][k];
                oa += wt[1][k];
            }
            tt += wt[0][k];
            ta += wt[1][k];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        if (i < n) {
            int s = -1;
            if (minor == 1) s = ntip + ot + __popcll(bt & below);
            else if (minor == 3) s = (naip + oa + __popcll(ba & below)) | (1 << 30);
            slots[i] = s;
        }
        ntip += tt;
        naip += ta;
        __syncthreads();
    }
    if (t == 0) {
        a.counts[row] = n;
        a.counts[a.nchan + row] = kHrptMinorFrames * ntip;
        a.counts[2 * a.nchan + row] = kHrptMinorFrames * naip;
        if (a.tip_counts) a.tip_counts[row] = kHrptMinorFrames * ntip;
        if (a.aip_counts) a.aip_counts[row] = kHrptMinorFrames * naip;
    }
}

__global__ __launch_bounds__(kHrptGatherNT) void hrpt_gather_kernel(const HrptArgs a) {
    constexpr int kWords = (3 + kHrptTipImgBytes + 3) / 4;     // dwords of the longest image
    static_assert(kWords <= kHrptGatherNT && kHrptTipBytes / 4 <= kHrptGatherNT, "one dword per lane");
    __shared__ unsigned img[kWords + 2];
    const int f = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
    if (f >= row_count(a.in_counts, row, a.nframes)) return;
    const int slot = a.slots[(long long)row * a.nframes + f];
    if (slot < 0) return;
    const bool aip = (slot >> 30) != 0;
    unsigned char* rows = aip ? a.aip : a.tip;
    if (!rows) return;
    unsigned char* dst = rows + (long long)row * (aip ? a.aip_stride : a.tip_stride) + (long long)(slot & 0x3fffffff) * kHrptTipBytes;
    const unsigned char* src = a.in + (long long)row * a.in_stride + (long long)f * kHrptFrameBytes + kHrptTipFirstByte;
    const int mis = (int)((uintptr_t)src & 3);
    const unsigned* w = reinterpret_cast<const unsigned*>(src - mis);
    const int nw = (mis + kHrptTipImgBytes + 3) >> 2;          // the last dword holds byte 778
    if (t < nw) img[t] = __builtin_bswap32(w[t]);
    __syncthreads();
    if (t < kHrptTipBytes / 4) {
        // byte j = (word(103 + j) >> 2) & 0xFF: the 8 bits at image bit 8 mis + 6 + 10 j
        unsigned b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) b[k] = img_bits(img, 8 * mis + 6 + 10 * (4 * t + k), 8);
        if (((uintptr_t)dst & 3) == 0) {
            reinterpret_cast<unsigned*>(dst)[t] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) dst[4 * t + k] = (unsigned char)b[k];
        }
    }
}

__global__ __launch_bounds__(kTipNT) void tip_kernel(const TipArgs a) {
    constexpr int kWords = (kTipRun * kTipFrame + 3) / 4 + 1;
    __shared__ __attribute__((aligned(16))) unsigned img[kWords];
    __shared__ unsigned char smap[(kTipRecord + 3) / 4 * 4];
    const int row = blockIdx.y, t = threadIdx.x;
    const int n = row_count(a.in_counts, row, a.count);
    if (blockIdx.x == 0 && t == 0) {
        a.counts[row] = n;
        if (a.counts_out) a.counts_out[row] = n;
    }
    const int m0 = blockIdx.x * kTipRun;
    if (m0 >= n) return;
    const int nm = n - m0 < kTipRun ? n - m0 : kTipRun;
    const unsigned char* src = a.in + (long long)row * a.in_stride + (long long)m0 * kTipFrame;
    const int mis = (int)((uintptr_t)src & 3);
    const unsigned* w = reinterpret_cast<const unsigned*>(src - mis);
    const int nw = (mis + nm * kTipFrame + 3) >> 2;            // <= kWords; the last dword holds the run's last byte
    constexpr int kPer = (kWords + kTipNT - 1) / kTipNT;
    unsigned r[kPer];
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int j = u * kTipNT + t;
        r[u] = j < nw ? w[j] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int j = u * kTipNT + t;
        if (j < nw) img[j] = r[u];
    }
    if (t < kTipRecord) smap[t] = (unsigned char)tip_src(t);
    __syncthreads();
    const unsigned char* b = reinterpret_cast<const unsigned char*>(img) + mis;
    auto rec_byte = [&](int o) -> unsigned {
        const int m = o / kTipRecord;
        return b[m * kTipFrame + smap[o - m * kTipRecord]];
    };
    unsigned char* dst = a.out + (long long)row * a.out_stride + (long long)m0 * kTipRecord;
    const int fo = nm * kTipRecord;
    int head = (int)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > fo) head = fo;
    const int nvec = (fo - head) >> 4, tail0 = head + 16 * nvec;
    if (t < head) dst[t] = (unsigned char)rec_byte(t);
    for (int v = t; v < nvec; v += kTipNT) {
        const int off = head + 16 * v;
        unsigned x[4];
#pragma unroll
        for (int q = 0; q < 4; q++)
            x[q] = rec_byte(off + 4 * q) | (rec_byte(off + 4 * q + 1) << 8) | (rec_byte(off + 4 * q + 2) << 16) | (rec_byte(off + 4 * q + 3) << 24);
        *reinterpret_cast<uint4*>(dst + off) = make_uint4(x[0], x[1], x[2], x[3]);
    }
    if (t < fo - tail0) dst[tail0 + t] = (unsigned char)rec_byte(tail0 + t);     // fewer than 16
}

__global__ __launch_bounds__(kHirsNT) void hirs_scan_kernel(const HirsArgs a) {
    __shared__ int wt[kHirsNT / 64];
    const int row = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n = row_count(a.in_counts, row, a.count);
    const unsigned char* in = a.in + (long long)row * a.in_stride;
    const long long ps = a.packet_stride;
    const int last0 = a.state[row * kHirsState], nid0 = a.state[row * kHirsState + 1];
    // the flushes of packet i < n: fb before its write, fa = (e == 55) after it; returns fb + fa
    auto flushes = [&](int i, int& e, int& fb) -> int {
        e = hirs_elem(in + i * ps);
        const int ep = i > 0 ? hirs_elem(in + (i - 1) * ps) : last0;
        const bool nid = i > 0 ? ep < 55 : nid0 != 0;
        fb = ((e < ep || e > 55) && nid) ? 1 : 0;
        return fb + (e == 55 ? 1 : 0);
    };
    // 1. the lines of the call, so that the map is cleared for lines 0 .. total only
    int mine = 0;
    for (int i = t; i < n; i += kHirsNT) {
        int e, fb;
        mine += flushes(i, e, fb);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m);
    if (lane == 0) wt[wv] = mine;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int k = 0; k < kHirsNT / 64; k++) total += wt[k];
    int* map = a.map + (long long)row * (a.count + 2) * kHirsLine;
    for (int j = t; j < (total + 1) * kHirsLine; j += kHirsNT) map[j] = -1;      // total + 1 <= n + 2 <= count + 2 lines
    __syncthreads();                                           // the clearing stores come before the entries below
    // 2. line(i) = flushes before packet i + fb(i); the write of packet i survives unless packet i + 1 repeats its element in its line
    int running = 0;
    for (int base = 0; base < n; base += kHirsNT) {
        const int i = base + t;
        int e = 64, fb = 0, c = 0;
        if (i < n) c = flushes(i, e, fb);
        int inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(inc, d);
            if (lane >= d) inc += v;
        }
        if (lane == 63) wt[wv] = inc;
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < kHirsNT / 64; k++) {
            if (k < wv) off += wt[k];
            tot += wt[k];
        }
        if (i < n && e <= 55) {
            const int line = running + off + inc - c + fb;     // <= total
            const bool dropped = i + 1 < n && e != 55 && hirs_elem(in + (i + 1) * ps) == e;
            if (!dropped) map[line * kHirsLine + e] = i;
        }
        running += tot;
        __syncthreads();
    }
    if (t == 0) {
        int* st = a.state_next + row * kHirsState;
        if (n > 0) {
            const int el = hirs_elem(in + (n - 1) * ps);
            st[0] = el;
            st[1] = el < 55 ? 1 : 0;
        } else {
            st[0] = last0;
            st[1] = nid0;
        }
        a.meta[row] = total;
        a.counts[row] = total;
        if (a.counts_out) a.counts_out[row] = total;
    }
}

__global__ __launch_bounds__(kHirsNT) void hirs_pack_kernel(const HirsArgs a) {
    constexpr int kPerLine = kHirsChannels * (kHirsLine / 8);
    const int row = blockIdx.y;
    const long long id = (long long)blockIdx.x * kHirsNT + threadIdx.x;
    const int total = a.meta[row];
    const long long line = id / kPerLine;
    if (line > total) return;                                  // line `total` is the one in progress
    const int r = (int)(id - line * kPerLine), ch = r / (kHirsLine / 8), g = r - ch * (kHirsLine / 8);
    const int* m = a.map + ((long long)row * (a.count + 2) + line) * kHirsLine + 8 * g;     // 16-byte aligned
    const int4 m0 = *reinterpret_cast<const int4*>(m), m1 = *reinterpret_cast<const int4*>(m + 4);
    const int p[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
    const unsigned char* in = a.in + (long long)row * a.in_stride;
    const unsigned short* part = a.partial + (long long)row * (kHirsChannels * kHirsLine) + ch * kHirsLine + 8 * g;
    const int bit = hirs_bit(ch);
    unsigned px[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (p[k] >= 0) px[k] = hirs_unsigned(bits_at(in + (long long)p[k] * a.packet_stride, bit, 13));
        else px[k] = line == 0 ? part[k] : 0xFFFu;
    }
    unsigned short* dst = line < total ? a.out + (long long)row * a.row_stride + (long long)ch * a.plane_stride + line * kHirsLine + 8 * g
                                       : a.partial_next + (long long)row * (kHirsChannels * kHirsLine) + ch * kHirsLine + 8 * g;
    store8(dst, px);
}

}  // namespace qk

namespace qh {

namespace {

bool spans_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}

constexpr int64_t kHrptMaxFrames = (int64_t)1 << 20;     // per row and call
constexpr int64_t kTipMaxCount = (int64_t)1 << 24;
constexpr int64_t kHirsMaxCount = (int64_t)1 << 22;
constexpr int64_t kAvhrrFrame = (int64_t)qk::kHrptPlanes * qk::kHrptPixels;      // uint16 per frame, all planes
constexpr int64_t kHirsLineAll = (int64_t)qk::kHirsChannels * qk::kHirsLine;     // uint16 per line, all channels

// ---- HrptDemux ----

void hrpt_free(Hrpt* d) {
    op_free(d, [d] { hip_free_all({d->d_slots, d->d_tip, d->d_aip, d->d_counts}); });
}

// slots and the library-owned TIP / AIP rows for calls of up to `frames` frames per row (a larger call than any before synchronises)
hipError_t hrpt_scratch(Hrpt* d, int64_t frames) {
    if (frames <= d->scratch_frames) return hipSuccess;
    hipError_t err = hipDeviceSynchronize();
    hip_free_all({d->d_slots, d->d_tip, d->d_aip});
    d->d_slots = nullptr;
    d->d_tip = d->d_aip = nullptr;
    d->scratch_frames = 0;
    const size_t n = (size_t)d->nchan * (size_t)frames;
    if (err == hipSuccess) err = hipMalloc(&d->d_slots, n * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&d->d_tip, n * qk::kHrptTipBytes);
    if (err == hipSuccess) err = hipMalloc(&d->d_aip, n * qk::kHrptTipBytes);
    if (err == hipSuccess) d->scratch_frames = frames;
    return err;
}

// strides: bytes (in, tip, aip) and uint16 elements (the two of avhrr)
int hrpt_launch_all(Hrpt* d, const void* d_in, int64_t nframes, int64_t in_stride, const int* d_in_counts, void* d_avhrr, int64_t row_stride,
                    int64_t plane_stride, void* d_tip, int64_t tip_stride, int* d_tip_counts, void* d_aip, int64_t aip_stride, int* d_aip_counts,
                    hipStream_t s) {
    if (nframes < 0 || nframes > kHrptMaxFrames || (nframes > 0 && !d_in)) return QDSP_HIP_EINVAL;
    if (in_stride < nframes * qk::kHrptFrameBytes) return QDSP_HIP_EINVAL;
    if (d_avhrr && (((uintptr_t)d_avhrr & 1) || plane_stride < nframes * qk::kHrptPixels || row_stride < 0)) return QDSP_HIP_EINVAL;
    if ((d_tip && tip_stride < nframes * qk::kHrptTipBytes) || (d_aip && aip_stride < nframes * qk::kHrptTipBytes)) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    if (nframes == 0) {
        HIPCHK(hipMemsetAsync(d->d_counts, 0, 3 * (size_t)d->nchan * sizeof(int), s));
        if (d_tip_counts) HIPCHK(hipMemsetAsync(d_tip_counts, 0, (size_t)d->nchan * sizeof(int), s));
        if (d_aip_counts) HIPCHK(hipMemsetAsync(d_aip_counts, 0, (size_t)d->nchan * sizeof(int), s));
        return 0;
    }
    const size_t in_span = (size_t)(d->nchan - 1) * in_stride + (size_t)nframes * qk::kHrptFrameBytes;
    if (d_avhrr) {
        const size_t span = ((size_t)(d->nchan - 1) * row_stride + (size_t)(qk::kHrptPlanes - 1) * plane_stride + (size_t)nframes * qk::kHrptPixels) * 2;
        if (spans_overlap(d_in, in_span, d_avhrr, span)) return QDSP_HIP_EINVAL;
    }
    if (d_tip && spans_overlap(d_in, in_span, d_tip, (size_t)(d->nchan - 1) * tip_stride + (size_t)nframes * qk::kHrptTipBytes)) return QDSP_HIP_EINVAL;
    if (d_aip && spans_overlap(d_in, in_span, d_aip, (size_t)(d->nchan - 1) * aip_stride + (size_t)nframes * qk::kHrptTipBytes)) return QDSP_HIP_EINVAL;
    if (const hipError_t err = hrpt_scratch(d, nframes)) return -(int)err;
    qk::HrptArgs a;
    a.in = static_cast<const unsigned char*>(d_in);
    a.in_counts = d_in_counts;
    a.avhrr = static_cast<unsigned short*>(d_avhrr);
    a.tip = static_cast<unsigned char*>(d_tip);
    a.aip = static_cast<unsigned char*>(d_aip);
    a.slots = d->d_slots;
    a.counts = d->d_counts;
    a.tip_counts = d_tip_counts;
    a.aip_counts = d_aip_counts;
    a.in_stride = in_stride;
    a.row_stride = row_stride;
    a.plane_stride = plane_stride;
    a.tip_stride = tip_stride;
    a.aip_stride = aip_stride;
    a.nframes = (int)nframes;
    a.nchan = d->nchan;
    const dim3 grid((unsigned)nframes, (unsigned)d->nchan);
    if (d_avhrr) {
        hipLaunchKernelGGL(qk::hrpt_avhrr_kernel, grid, dim3(qk::kHrptNT), 0, s, a);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(qk::hrpt_scan_kernel, dim3((unsigned)d->nchan), dim3(qk::kHrptScanNT), 0, s, a);
    HIPCHK(hipGetLastError());
    if (d_tip || d_aip) {
        hipLaunchKernelGGL(qk::hrpt_gather_kernel, grid, dim3(qk::kHrptGatherNT), 0, s, a);
        HIPCHK(hipGetLastError());
    }
    d->last = Launch{"hrpt_avhrr_kernel", (int)grid.x, qk::kHrptNT, (int)sizeof(unsigned) * (4 * qk::kHrptImgVec + 4)};
    d->last_frames = nframes;
    return 0;
}

// the shared host path: strides in frames, the planes nframes * 2048 apart, TIP and AIP into the library's own rows
int hrpt_launch(Hrpt* d, const void* d_in, int64_t nframes, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (nframes > 0 && !d_out) return QDSP_HIP_EINVAL;
    if (nframes > 0) {
        HIPCHK(hipSetDevice(d->device));
        if (const hipError_t err = hrpt_scratch(d, nframes)) return -(int)err;
    }
    const int64_t own = d->scratch_frames * qk::kHrptTipBytes;
    return hrpt_launch_all(d, d_in, nframes, in_stride * qk::kHrptFrameBytes, nullptr, d_out, out_stride * kAvhrrFrame, out_stride * qk::kHrptPixels,
                           d->d_tip, own, nullptr, d->d_aip, own, nullptr, s);
}

// which: 1 TIP, 2 AIP
int hrpt_own_dev(void* h, int which, void** d_rows, int64_t* stride_bytes, int** d_counts) {
    Hrpt* d = as<Hrpt>(h);
    if (!d || !d_rows || !stride_bytes || !d_counts) return QDSP_HIP_EINVAL;
    *d_rows = which == 1 ? d->d_tip : d->d_aip;
    *stride_bytes = d->scratch_frames * qk::kHrptTipBytes;
    *d_counts = d->d_counts + (size_t)which * d->nchan;
    return 0;
}

int hrpt_own_get(void* h, int which, int chan, uint8_t* out, int cap) {
    Hrpt* d = as<Hrpt>(h);
    if (!d || !chan_ok(d, chan) || cap < 0 || (cap > 0 && !out)) return QDSP_HIP_EINVAL;
    int n = 0;
    if (const int rc = sync_download(d, &n, d->d_counts + (size_t)which * d->nchan + chan, sizeof(int))) return rc;
    const int m = n < cap ? n : cap;
    const unsigned char* rows = which == 1 ? d->d_tip : d->d_aip;
    if (m > 0) HIPCHK(hipMemcpy(out, rows + (size_t)chan * d->scratch_frames * qk::kHrptTipBytes, (size_t)m * qk::kTipFrame, hipMemcpyDeviceToHost));
    return n;
}

// ---- TipDemux ----

void tip_free(Tip* d) {
    op_free(d, [d] { hip_free_all({d->d_counts}); });
}

// strides in bytes
int tip_launch_counts(Tip* d, const void* d_in, int64_t count, int64_t in_stride, const int* d_in_counts, void* d_out, int64_t out_stride,
                      int* d_counts, hipStream_t s) {
    if (count < 0 || count > kTipMaxCount || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count * qk::kTipFrame || out_stride < count * qk::kTipRecord) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    if (count == 0) {
        HIPCHK(hipMemsetAsync(d->d_counts, 0, (size_t)d->nchan * sizeof(int), s));
        if (d_counts) HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)d->nchan * sizeof(int), s));
        return 0;
    }
    const size_t in_span = (size_t)(d->nchan - 1) * in_stride + (size_t)count * qk::kTipFrame;
    const size_t out_span = (size_t)(d->nchan - 1) * out_stride + (size_t)count * qk::kTipRecord;
    if (spans_overlap(d_in, in_span, d_out, out_span)) return QDSP_HIP_EINVAL;
    qk::TipArgs a;
    a.in = static_cast<const unsigned char*>(d_in);
    a.in_counts = d_in_counts;
    a.out = static_cast<unsigned char*>(d_out);
    a.counts = d->d_counts;
    a.counts_out = d_counts;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.count = (int)count;
    const dim3 grid((unsigned)((count + qk::kTipRun - 1) / qk::kTipRun), (unsigned)d->nchan);
    hipLaunchKernelGGL(qk::tip_kernel, grid, dim3(qk::kTipNT), 0, s, a);
    HIPCHK(hipGetLastError());
    d->last = Launch{"tip_kernel", (int)grid.x, qk::kTipNT, (int)sizeof(unsigned) * ((qk::kTipRun * qk::kTipFrame + 3) / 4 + 1) + (qk::kTipRecord + 3) / 4 * 4};
    return 0;
}

// the shared host path: strides in minor frames / records
int tip_launch(Tip* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    return tip_launch_counts(d, d_in, count, in_stride * qk::kTipFrame, nullptr, d_out, out_stride * qk::kTipRecord, nullptr, s);
}

// ---- HirsDemux ----

int64_t hirs_out_count(const StreamOp*, int64_t count) { return count + 1; }

void hirs_free(Hirs* d) {
    op_free(d, [d] {
        hip_free_all({d->d_state[0], d->d_state[1], d->d_partial[0], d->d_partial[1], d->d_map, d->d_meta, d->d_counts});
        if (d->h_count) (void)hipHostFree(d->h_count);
    });
}

hipError_t hirs_scratch(Hirs* d, int64_t count) {
    if (count <= d->scratch_count) return hipSuccess;
    hipError_t err = hipDeviceSynchronize();
    if (d->d_map) (void)hipFree(d->d_map);
    d->d_map = nullptr;
    d->scratch_count = 0;
    if (err == hipSuccess) err = hipMalloc(&d->d_map, (size_t)d->nchan * (size_t)(count + 2) * qk::kHirsLine * sizeof(int));
    if (err == hipSuccess) d->scratch_count = count;
    return err;
}

// the state after create / reset, in both slots
int hirs_fill_initial(Hirs* d) {
    const std::vector<unsigned short> part((size_t)d->nchan * kHirsLineAll, 0xFFF);
    for (int s = 0; s < 2; s++) {
        HIPCHK(hipMemset(d->d_state[s], 0, (size_t)d->nchan * qk::kHirsState * sizeof(int)));
        HIPCHK(hipMemcpy(d->d_partial[s], part.data(), part.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(d->d_counts, 0, (size_t)d->nchan * sizeof(int)));
    return 0;
}

// strides: bytes (in) and uint16 elements (the two of out)
int hirs_launch_counts(Hirs* d, const void* d_in, int64_t count, int64_t in_stride, const int* d_in_counts, void* d_out, int64_t row_stride,
                       int64_t plane_stride, int* d_counts, hipStream_t s) {
    if (count < 0 || count > kHirsMaxCount || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (count > 0 && in_stride < (count - 1) * d->packet_stride + qk::kHirsPacket) return QDSP_HIP_EINVAL;
    if (plane_stride < (count + 1) * qk::kHirsLine || row_stride < 0 || ((uintptr_t)d_out & 1)) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    if (count == 0) {
        HIPCHK(hipMemsetAsync(d->d_counts, 0, (size_t)d->nchan * sizeof(int), s));
        if (d_counts) HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)d->nchan * sizeof(int), s));
        return 0;
    }
    const size_t in_span = (size_t)(d->nchan - 1) * in_stride + (size_t)(count - 1) * d->packet_stride + qk::kHirsPacket;
    const size_t out_span = ((size_t)(d->nchan - 1) * row_stride + (size_t)(qk::kHirsChannels - 1) * plane_stride + (size_t)(count + 1) * qk::kHirsLine) * 2;
    if (spans_overlap(d_in, in_span, d_out, out_span)) return QDSP_HIP_EINVAL;
    if (const hipError_t err = hirs_scratch(d, count)) return -(int)err;
    qk::HirsArgs a;
    a.in = static_cast<const unsigned char*>(d_in);
    a.in_counts = d_in_counts;
    a.out = static_cast<unsigned short*>(d_out);
    a.state = d->d_state[d->cur];
    a.state_next = d->d_state[d->cur ^ 1];
    a.partial = d->d_partial[d->cur];
    a.partial_next = d->d_partial[d->cur ^ 1];
    a.map = d->d_map;
    a.meta = d->d_meta;
    a.counts = d->d_counts;
    a.counts_out = d_counts;
    a.in_stride = in_stride;
    a.row_stride = row_stride;
    a.plane_stride = plane_stride;
    a.count = (int)count;
    a.packet_stride = d->packet_stride;
    hipLaunchKernelGGL(qk::hirs_scan_kernel, dim3((unsigned)d->nchan), dim3(qk::kHirsNT), 0, s, a);
    HIPCHK(hipGetLastError());
    const int64_t lanes = (count + 2) * qk::kHirsChannels * (qk::kHirsLine / 8);       // the lines that can end in the call, and the one in progress
    const dim3 grid((unsigned)((lanes + qk::kHirsNT - 1) / qk::kHirsNT), (unsigned)d->nchan);
    hipLaunchKernelGGL(qk::hirs_pack_kernel, grid, dim3(qk::kHirsNT), 0, s, a);
    HIPCHK(hipGetLastError());
    d->last = Launch{"hirs_pack_kernel", (int)grid.x, qk::kHirsNT, 0};
    d->cur ^= 1;
    if (d->nchan == 1) HIPCHK(hipMemcpyAsync(d->h_count, d->d_counts, sizeof(int), hipMemcpyDeviceToHost, s));   // process_ex reads it
    return 0;
}

// the shared host path: strides in packets / lines, the planes out_stride * 56 apart
int hirs_launch(Hirs* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    return hirs_launch_counts(d, d_in, count, in_stride * d->packet_stride, nullptr, d_out, out_stride * kHirsLineAll, out_stride * qk::kHirsLine,
                              nullptr, s);
}

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_hrpt_create(void** h, int device, int nchan, int max_block) {
    Hrpt* d = nullptr;
    if (const int rc = op_new<Hrpt, hrpt_launch>(&d, h, max_block <= kHrptMaxFrames, device, nchan, max_block)) return rc;
    hipError_t err = stream_op_init(d, device, nchan, max_block, (size_t)qk::kHrptFrameBytes, (size_t)kAvhrrFrame * 2);
    d->nchan = nchan;
    if (err == hipSuccess) err = hipMalloc(&d->d_counts, 3 * (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipMemset(d->d_counts, 0, 3 * (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hrpt_scratch(d, max_block > 0 ? max_block : 1);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return op_created<hrpt_free>(h, d, err);
}
int64_t qdsp_hip_hrpt_out_size(void* h, int64_t nframes) { return (as<Hrpt>(h) && nframes >= 0) ? nframes : QDSP_HIP_EINVAL; }
int qdsp_hip_hrpt_process_batch_dev(void* h, const void* d_in, int64_t nframes, int64_t in_stride_bytes, const int* d_in_counts, uint16_t* d_avhrr,
                                    int64_t row_stride, int64_t plane_stride, uint8_t* d_tip, int64_t tip_stride_bytes, int* d_tip_counts,
                                    uint8_t* d_aip, int64_t aip_stride_bytes, int* d_aip_counts, void* hip_stream) {
    Hrpt* d = as<Hrpt>(h);
    if (!d) return QDSP_HIP_EINVAL;
    return hrpt_launch_all(d, d_in, nframes, in_stride_bytes, d_in_counts, d_avhrr, row_stride, plane_stride, d_tip, tip_stride_bytes, d_tip_counts,
                           d_aip, aip_stride_bytes, d_aip_counts, static_cast<hipStream_t>(hip_stream));
}
int qdsp_hip_hrpt_process_dev(void* h, const void* d_in, int64_t nframes, void* d_avhrr, void* hip_stream) {
    return op_process_dev<Hrpt, hrpt_launch>(h, d_in, nframes, d_avhrr, hip_stream);
}
int qdsp_hip_hrpt_process_ex(void* h, const void* in, int in_link, int nframes, void* avhrr, int out_link) {
    return op_process_ex<Hrpt>(h, in, in_link, nframes, avhrr, out_link);
}
int qdsp_hip_hrpt_process(void* h, const uint8_t* in, int nframes, uint16_t* avhrr) {
    return qdsp_hip_hrpt_process_ex(h, in, QDSP_HIP_LINK_HOST, nframes, avhrr, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_hrpt_get_counts(void* h, int* counts) {
    Hrpt* d = as<Hrpt>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    return sync_download(d, counts, d->d_counts, 3 * (size_t)d->nchan * sizeof(int));
}
int qdsp_hip_hrpt_tip_dev(void* h, void** d_tip, int64_t* stride_bytes, int** d_counts) { return hrpt_own_dev(h, 1, d_tip, stride_bytes, d_counts); }
int qdsp_hip_hrpt_aip_dev(void* h, void** d_aip, int64_t* stride_bytes, int** d_counts) { return hrpt_own_dev(h, 2, d_aip, stride_bytes, d_counts); }
int qdsp_hip_hrpt_get_frame_slots(void* h, int chan, int* slots, int cap) {
    Hrpt* d = as<Hrpt>(h);
    if (!d || !chan_ok(d, chan) || cap < 0 || (cap > 0 && !slots)) return QDSP_HIP_EINVAL;
    int n = 0;
    if (const int rc = sync_download(d, &n, d->d_counts + chan, sizeof(int))) return rc;
    const int m = n < cap ? n : cap;
    if (m > 0) HIPCHK(hipMemcpy(slots, d->d_slots + (size_t)chan * d->last_frames, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
    return n;
}
int qdsp_hip_hrpt_get_tip(void* h, int chan, uint8_t* out, int cap) { return hrpt_own_get(h, 1, chan, out, cap); }
int qdsp_hip_hrpt_get_aip(void* h, int chan, uint8_t* out, int cap) { return hrpt_own_get(h, 2, chan, out, cap); }
void qdsp_hip_hrpt_destroy(void* h) { hrpt_free(as<Hrpt>(h)); }

int qdsp_hip_tip_create(void** h, int device, int nchan, int max_block) {
    Tip* d = nullptr;
    if (const int rc = op_new<Tip, tip_launch>(&d, h, max_block <= kTipMaxCount, device, nchan, max_block)) return rc;
    hipError_t err = stream_op_init(d, device, nchan, max_block, (size_t)qk::kTipFrame, (size_t)qk::kTipRecord);
    d->nchan = nchan;
    if (err == hipSuccess) err = hipMalloc(&d->d_counts, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipMemset(d->d_counts, 0, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return op_created<tip_free>(h, d, err);
}
int64_t qdsp_hip_tip_out_size(void* h, int64_t count) { return (as<Tip>(h) && count >= 0) ? count : QDSP_HIP_EINVAL; }
int qdsp_hip_tip_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride_bytes, const int* d_in_counts, void* d_out,
                                   int64_t out_stride_bytes, int* d_counts, void* hip_stream) {
    Tip* d = as<Tip>(h);
    if (!d) return QDSP_HIP_EINVAL;
    return tip_launch_counts(d, d_in, count, in_stride_bytes, d_in_counts, d_out, out_stride_bytes, d_counts, static_cast<hipStream_t>(hip_stream));
}
int qdsp_hip_tip_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<Tip, tip_launch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_tip_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<Tip>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_tip_process(void* h, const uint8_t* in, int count, uint8_t* out) {
    return qdsp_hip_tip_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_tip_get_counts(void* h, int* counts) {
    Tip* d = as<Tip>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    return sync_download(d, counts, d->d_counts, (size_t)d->nchan * sizeof(int));
}
void qdsp_hip_tip_destroy(void* h) { tip_free(as<Tip>(h)); }

int qdsp_hip_hirs_create(void** h, int device, int nchan, int max_block, int packet_stride) {
    Hirs* d = nullptr;
    const bool args_ok = packet_stride >= qk::kHirsPacket && packet_stride <= 4096 && max_block <= kHirsMaxCount;
    if (const int rc = op_new<Hirs, hirs_launch, hirs_out_count>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->packet_stride = packet_stride;
    hipError_t err = stream_op_init(d, device, nchan, max_block, (size_t)packet_stride, (size_t)kHirsLineAll * 2);
    d->nchan = nchan;
    if (err == hipSuccess && max_block > 0) {
        // the host side's staging row holds out_size(max_block) lines
        (void)hipFree(d->d_out);
        d->d_out = nullptr;
        err = hipMalloc(&d->d_out, (size_t)(max_block + 1) * kHirsLineAll * 2);
    }
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc(&d->d_state[i], (size_t)nchan * qk::kHirsState * sizeof(int));
        if (err == hipSuccess) err = hipMalloc(&d->d_partial[i], (size_t)nchan * kHirsLineAll * sizeof(unsigned short));
    }
    if (err == hipSuccess) err = hipMalloc(&d->d_meta, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&d->d_counts, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipHostMalloc(reinterpret_cast<void**>(&d->h_count), sizeof(int), hipHostMallocDefault);
    if (err == hipSuccess) err = hirs_scratch(d, max_block > 0 ? max_block : 1);
    if (err == hipSuccess) {
        *d->h_count = 0;
        const int rc = hirs_fill_initial(d);
        if (rc) err = (hipError_t)(-rc);
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return op_created<hirs_free>(h, d, err);
}
int64_t qdsp_hip_hirs_out_size(void* h, int64_t count) { return (as<Hirs>(h) && count >= 0) ? count + 1 : QDSP_HIP_EINVAL; }
int qdsp_hip_hirs_packet_stride(void* h) {
    Hirs* d = as<Hirs>(h);
    return d ? d->packet_stride : QDSP_HIP_EINVAL;
}
int qdsp_hip_hirs_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride_bytes, const int* d_in_counts, uint16_t* d_out,
                                    int64_t row_stride, int64_t plane_stride, int* d_counts, void* hip_stream) {
    Hirs* d = as<Hirs>(h);
    if (!d) return QDSP_HIP_EINVAL;
    return hirs_launch_counts(d, d_in, count, in_stride_bytes, d_in_counts, d_out, row_stride, plane_stride, d_counts, static_cast<hipStream_t>(hip_stream));
}
int qdsp_hip_hirs_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    Hirs* d = as<Hirs>(h);
    return d ? hirs_launch(d, d_in, count, count, d_out, count + 1, static_cast<hipStream_t>(hip_stream)) : QDSP_HIP_EINVAL;
}
int qdsp_hip_hirs_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    Hirs* d = as<Hirs>(h);
    // the line count is returned, so the call has to have run: an output link that hands over without waiting cannot be served
    if (!d || (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE)) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, count, out, out_link);
    if (rc < 0 || count == 0) return (int)rc;
    return *d->h_count;
}
int qdsp_hip_hirs_process(void* h, const uint8_t* in, int count, uint16_t* out) {
    return qdsp_hip_hirs_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_hirs_get_counts(void* h, int* counts) {
    Hirs* d = as<Hirs>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    return sync_download(d, counts, d->d_counts, (size_t)d->nchan * sizeof(int));
}
int qdsp_hip_hirs_get_state(void* h, int chan, int* last_element, int* new_image_data) {
    Hirs* d = as<Hirs>(h);
    if (!d || !chan_ok(d, chan) || !last_element || !new_image_data) return QDSP_HIP_EINVAL;
    int v[2];
    if (const int rc = sync_download(d, v, d->d_state[d->cur] + (size_t)chan * qk::kHirsState, sizeof(v))) return rc;
    *last_element = v[0];
    *new_image_data = v[1];
    return 0;
}
int qdsp_hip_hirs_set_state(void* h, int chan, int last_element, int new_image_data) {
    Hirs* d = as<Hirs>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    if (last_element < 0 || last_element > 63 || (new_image_data != 0 && new_image_data != 1)) return QDSP_HIP_EINVAL;
    const int v[2] = {last_element, new_image_data};
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++)
        HIPCHK(hipMemcpy(d->d_state[d->cur] + (size_t)c * qk::kHirsState, v, sizeof(v), hipMemcpyHostToDevice));
    return 0;
}
int qdsp_hip_hirs_reset(void* h) {
    Hirs* d = as<Hirs>(h);
    if (!d) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    return hirs_fill_initial(d);
}
void qdsp_hip_hirs_destroy(void* h) { hirs_free(as<Hirs>(h)); }

}  // extern "C"
