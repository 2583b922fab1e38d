// fpkt.hip -- FalconPacketSync batched over channel rows (design notes: fpkt.hip.h), and its C entry points.
#include "fpkt.hip.h"

#include <cstring>
#include <new>
#include <vector>

namespace qk {

namespace {

// frames of row `row` in this call
__device__ __forceinline__ int row_count(const int* in_counts, int row, int count) {
    if (!in_counts) return count;
    const int c = in_counts[row];
    return c < 0 ? 0 : (c < count ? c : count);
}

// n bytes from src to dst, both at any byte, by the lanes of a workgroup: bytes up to dst's 16-byte boundary, 16-byte stores built
// from the aligned dwords that hold their bytes (the fifth only where the source is misaligned), bytes at the end
__device__ __forceinline__ void copy_bytes(unsigned char* dst, const unsigned char* src, int n, int t) {
    int head = (int)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > n) head = n;
    const int nvec = (n - head) >> 4, tail0 = head + 16 * nvec;
    if (t < head) dst[t] = src[t];
    const unsigned sh = (unsigned)((uintptr_t)(src + head) & 3);
    for (int v = t; v < nvec; v += kFpktPackNT) {
        const int off = head + 16 * v;
        const unsigned* w = reinterpret_cast<const unsigned*>(src + off - sh);
        const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = sh ? w[4] : 0u;
        *reinterpret_cast<uint4*>(dst + off) =
            make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh),
                       __builtin_amdgcn_alignbyte(w4, w3, sh));
    }
    if (t < n - tail0) dst[tail0 + t] = src[tail0 + t];                     // fewer than 16
}

}  // namespace

__global__ __launch_bounds__(kFpktWalkNT) void fpkt_walk_kernel(const FpktArgs a) {
    __shared__ unsigned img[kFpktImgWords];
    const int f = blockIdx.x, row = blockIdx.y, lane = threadIdx.x;
    if (f >= row_count(a.in_counts, row, a.nframes)) return;
    const unsigned char* src = a.in + (long long)row * a.in_stride + (long long)f * a.frame_stride;
    const int mis = (int)((uintptr_t)src & 3);
    const unsigned* w = reinterpret_cast<const unsigned*>(src - mis);
    const int nw = (mis + kFpktFrame + 3) >> 2;                // <= kFpktImgWords; the last dword holds byte 1194
    constexpr int kPer = (kFpktImgWords + kFpktWalkNT - 1) / kFpktWalkNT;
    unsigned r[kPer];
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int j = u * kFpktWalkNT + lane;
        r[u] = j < nw ? w[j] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int j = u * kFpktWalkNT + lane;
        if (j < nw) img[j] = r[u];
    }
    __syncthreads();
    const unsigned char* b = reinterpret_cast<const unsigned char*>(img) + mis;
    const unsigned b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    const int pkt = __builtin_amdgcn_readfirstlane((int)(b3 | ((b2 & 7u) << 8)));
    const unsigned ctr = (b2 >> 3) | (b1 << 5) | ((b0 & 0x3fu) << 13);
    const unsigned char* data = b + kFpktHeader;
    int e = 0, tail = -1, np = 0;
    unsigned starts = 0u;                                      // lane l: bits 32 l .. 32 l + 31 of the map of packet starts
    if (pkt <= kFpktData) {
        int i = pkt;                                           // wave-uniform
        while (i < kFpktData) {
            const int left = kFpktData - i;
            if (left < 4) {
                tail = left;
                break;
            }
            const int len = __builtin_amdgcn_readfirstlane((int)((((unsigned)data[i] & 15u) << 8) | data[i + 1]) + 2);
            if (len <= 2) break;
            if (left < len) {
                tail = left;
                break;
            }
            if (lane == (i >> 5)) starts |= 1u << (i & 31);
            np++;
            i += len;
        }
        e = i;
    }
    const long long fi = (long long)row * a.nframes + f;
    if (lane == 0) a.sum[fi] = make_int4((int)ctr, pkt | (e << 16), tail, np);
    if (lane < kFpktBitWords) a.bits[fi * kFpktBitWords + lane] = starts;
}

__global__ __launch_bounds__(kFpktScanNT) void fpkt_scan_kernel(const FpktArgs a) {
    __shared__ int wt[2][kFpktScanNT / 64];
    const int row = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n = row_count(a.in_counts, row, a.nframes);
    const int4* sum = a.sum + (long long)row * a.nframes;
    int4* pos = a.pos + (long long)row * (a.nframes + 1);
    const unsigned last0 = (unsigned)a.state[row * kFpktState];
    const int read0 = a.state[row * kFpktState + 1];
    auto ctr_of = [&](int j) -> unsigned { return j < 0 ? last0 : (unsigned)sum[j].x; };
    // the pending length that reaches frame f <= n (f == n: what stays behind the row's last frame) and the continuation frames
    // k it came through; -1: nothing pending.  At most kFpktMaxRun + 1 frames back.
    auto incoming = [&](int f, int& k) -> int {
        k = 0;
        if (f < n && ctr_of(f - 1) + 1u != ctr_of(f)) return -1;
        int base = -1;
        for (int j = f - 1;; j--) {
            if (j < 0) {
                base = read0;
                break;
            }
            const int4 s = sum[j];
            const int pkt = s.y & 0xffff;
            if (pkt != kFpktCont) {
                base = pkt <= kFpktData ? s.z : -1;            // the frame's own tail; a bad pointer leaves nothing
                break;
            }
            if (ctr_of(j - 1) + 1u != (unsigned)s.x) break;    // dropped in front of this continuation frame
            if (++k > kFpktMaxRun) break;                      // past the cap whatever the base
        }
        if (base < 0) return -1;
        const int v = base + kFpktData * k;
        return v <= kFpktCap ? v : -1;
    };
    int run_pk = 0, run_by = 0;
    for (int base = 0; base < n; base += kFpktScanNT) {
        const int i = base + t;
        int in = -1, k = 0, npk = 0, nby = 0;
        if (i < n) {
            const int4 s = sum[i];
            const int pkt = s.y & 0xffff, e = s.y >> 16;
            if (pkt <= kFpktData) {
                in = incoming(i, k);
                if (in >= 0 && in + pkt > kFpktCap) in = -1;   // a completion that would pass the cap: dropped
                npk = s.w + (in >= 0 ? 1 : 0);
                nby = e - pkt + (in >= 0 ? in + pkt : 0);
            }
        }
        int ipk = npk, iby = nby;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int vp = __shfl_up(ipk, d), vb = __shfl_up(iby, d);
            if (lane >= d) {
                ipk += vp;
                iby += vb;
            }
        }
        if (lane == 63) {
            wt[0][wv] = ipk;
            wt[1][wv] = iby;
        }
        __syncthreads();
        int opk = 0, oby = 0, tpk = 0, tby = 0;
#pragma unroll
        for (int q = 0; q < kFpktScanNT / 64; q++) {
            if (q < wv) {
                opk += wt[0][q];
                oby += wt[1][q];
            }
            tpk += wt[0][q];
            tby += wt[1][q];
        }
        if (i < n) pos[i] = make_int4(in, k, run_pk + opk + ipk - npk, run_by + oby + iby - nby);
        run_pk += tpk;
        run_by += tby;
        __syncthreads();
    }
    if (t == 0) {
        int k;
        const int in = incoming(n, k);
        pos[n] = make_int4(in, k, run_pk, run_by);
        int* st = a.state_next + row * kFpktState;
        st[0] = n > 0 ? sum[n - 1].x : (int)last0;
        st[1] = in;
        a.counts[row] = run_pk;
        a.counts[a.nchan + row] = run_by;
        if (a.counts_out) a.counts_out[row] = run_pk;
        a.offs[(long long)row * a.offs_stride + run_pk] = run_by;
    }
}

__global__ __launch_bounds__(kFpktPackNT) void fpkt_pack_kernel(const FpktArgs a) {
    const int f = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
    const int n = row_count(a.in_counts, row, a.nframes);
    if (f > n) return;                                         // workgroup n gathers the carry
    const unsigned char* in = a.in + (long long)row * a.in_stride;
    const long long fs = a.frame_stride;
    const int4 p = a.pos[(long long)row * (a.nframes + 1) + f];
    int pkt = 0, e = 0;
    unsigned char* dst;
    if (f < n) {
        const int4 s = a.sum[(long long)row * a.nframes + f];
        pkt = s.y & 0xffff;
        if (pkt > kFpktData) return;                           // a continuation frame is gathered by the frame that emits it
        e = s.y >> 16;
        dst = a.out + (long long)row * a.out_stride + p.w;
    } else {
        dst = a.pending_next + (long long)row * kFpktCap;
    }
    const int inl = p.x;
    if (inl >= 0) {
        // the pending packet: g's residue or the carried bytes (g == -1), the continuation frames between, this frame's head
        const int k = p.y, g = f - 1 - k, first = inl - kFpktData * k;
        const unsigned char* s0 = g >= 0 ? in + g * fs + (kFpktFrame - first) : a.pending + (long long)row * kFpktCap;
        copy_bytes(dst, s0, first, t);
        dst += first;
        for (int j = g + 1; j < f; j++) {
            copy_bytes(dst, in + j * fs + kFpktHeader, kFpktData, t);
            dst += kFpktData;
        }
        if (f < n) {
            copy_bytes(dst, in + f * fs + kFpktHeader, pkt, t);
            dst += pkt;
        }
    }
    if (f == n) return;
    copy_bytes(dst, in + f * fs + kFpktHeader + pkt, e - pkt, t);
    int* offs = a.offs + (long long)row * a.offs_stride + p.z;
    int by = p.w;
    if (inl >= 0) {
        if (t == 0) offs[0] = by;
        offs++;
        by += inl + pkt;
    }
    if (t < 64) {
        // the frame's own packets by rank of their start bits
        unsigned m = t < kFpktBitWords ? a.bits[((long long)row * a.nframes + f) * kFpktBitWords + t] : 0u;
        const int c = __popc(m);
        int inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(inc, d);
            if (t >= d) inc += v;
        }
        int r = inc - c;
        while (m) {
            const int bit = __ffs((int)m) - 1;
            m &= m - 1u;
            offs[r++] = by + (32 * t + bit - pkt);
        }
    }
}

}  // namespace qk

namespace qh {

namespace {

bool spans_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}

constexpr int64_t kFpktMaxFrames = (int64_t)1 << 20;     // per row and call: 16392 + 1191 * 2^20 < 2^31
constexpr int64_t kFpktPerFrame = 1 + qk::kFpktMaxWalk;  // 398 packets

int64_t fpkt_bytes(int64_t nframes) { return qk::kFpktCap + (int64_t)qk::kFpktData * nframes; }
int64_t fpkt_packets(int64_t nframes) { return kFpktPerFrame * nframes; }
int64_t fpkt_out_count(const StreamOp*, int64_t nframes) { return fpkt_bytes(nframes); }

void fpkt_free(Fpkt* d) {
    op_free(d, [d] {
        hip_free_all({d->d_state[0], d->d_state[1], d->d_pending[0], d->d_pending[1], d->d_sum, d->d_bits, d->d_pos, d->d_offs, d->d_counts});
        if (d->h_count) (void)hipHostFree(d->h_count);
    });
}

// summaries, start maps and positions for calls of up to `frames` frames per row (a larger call than any before synchronises)
hipError_t fpkt_scratch(Fpkt* d, int64_t frames) {
    if (frames <= d->scratch_frames) return hipSuccess;
    hipError_t err = hipDeviceSynchronize();
    hip_free_all({d->d_sum, d->d_bits, d->d_pos});
    d->d_sum = d->d_pos = nullptr;
    d->d_bits = nullptr;
    d->scratch_frames = 0;
    const size_t n = (size_t)d->nchan * (size_t)frames;
    if (err == hipSuccess) err = hipMalloc(&d->d_sum, n * sizeof(int4));
    if (err == hipSuccess) err = hipMalloc(&d->d_bits, n * qk::kFpktBitWords * sizeof(unsigned));
    if (err == hipSuccess) err = hipMalloc(&d->d_pos, (n + (size_t)d->nchan) * sizeof(int4));
    if (err == hipSuccess) d->scratch_frames = frames;
    return err;
}

// the library's own offset table, for calls that pass none
hipError_t fpkt_own_offs(Fpkt* d, int64_t frames) {
    if (d->d_offs && frames <= d->offs_frames) return hipSuccess;
    hipError_t err = hipDeviceSynchronize();
    if (d->d_offs) (void)hipFree(d->d_offs);
    d->d_offs = nullptr;
    d->offs_frames = 0;
    if (err == hipSuccess) err = hipMalloc(&d->d_offs, (size_t)d->nchan * (size_t)(fpkt_packets(frames) + 1) * sizeof(int));
    if (err == hipSuccess) err = hipMemset(d->d_offs, 0, (size_t)d->nchan * (size_t)(fpkt_packets(frames) + 1) * sizeof(int));
    if (err == hipSuccess) d->offs_frames = frames;
    return err;
}

// the state after create / reset, in both slots
int fpkt_fill_initial(Fpkt* d) {
    std::vector<int> st((size_t)d->nchan * qk::kFpktState);
    for (int c = 0; c < d->nchan; c++) {
        st[(size_t)c * qk::kFpktState] = 0;
        st[(size_t)c * qk::kFpktState + 1] = -1;
    }
    for (int s = 0; s < 2; s++) {
        HIPCHK(hipMemcpy(d->d_state[s], st.data(), st.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(d->d_pending[s], 0, (size_t)d->nchan * qk::kFpktCap));
    }
    HIPCHK(hipMemset(d->d_counts, 0, 2 * (size_t)d->nchan * sizeof(int)));
    *d->h_count = 0;
    return 0;
}

// strides: bytes (in, out) and ints (offs)
int fpkt_launch_counts(Fpkt* d, const void* d_in, int64_t nframes, int64_t in_stride, const int* d_in_counts, void* d_out, int64_t out_stride,
                       int* d_offs, int64_t offs_stride, int* d_counts, hipStream_t s) {
    if (nframes < 0 || nframes > kFpktMaxFrames || (nframes > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (nframes > 0 && in_stride < (nframes - 1) * d->frame_stride + qk::kFpktFrame) return QDSP_HIP_EINVAL;
    if (nframes > 0 && out_stride < fpkt_bytes(nframes)) return QDSP_HIP_EINVAL;
    if (d_offs && (offs_stride < fpkt_packets(nframes) + 1 || ((uintptr_t)d_offs & 3))) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    if (nframes == 0) {
        HIPCHK(hipMemsetAsync(d->d_counts, 0, 2 * (size_t)d->nchan * sizeof(int), s));
        if (d_counts) HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)d->nchan * sizeof(int), s));
        return 0;
    }
    const size_t in_span = (size_t)(d->nchan - 1) * in_stride + (size_t)(nframes - 1) * d->frame_stride + qk::kFpktFrame;
    const size_t out_span = (size_t)(d->nchan - 1) * out_stride + (size_t)fpkt_bytes(nframes);
    if (spans_overlap(d_in, in_span, d_out, out_span)) return QDSP_HIP_EINVAL;
    if (const hipError_t err = fpkt_scratch(d, nframes)) return -(int)err;
    if (!d_offs) {
        if (const hipError_t err = fpkt_own_offs(d, nframes)) return -(int)err;
        d_offs = d->d_offs;
        offs_stride = fpkt_packets(d->offs_frames) + 1;
    }
    qk::FpktArgs a;
    a.in = static_cast<const unsigned char*>(d_in);
    a.in_counts = d_in_counts;
    a.out = static_cast<unsigned char*>(d_out);
    a.offs = d_offs;
    a.state = d->d_state[d->cur];
    a.state_next = d->d_state[d->cur ^ 1];
    a.pending = d->d_pending[d->cur];
    a.pending_next = d->d_pending[d->cur ^ 1];
    a.sum = d->d_sum;
    a.bits = d->d_bits;
    a.pos = d->d_pos;
    a.counts = d->d_counts;
    a.counts_out = d_counts;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.offs_stride = offs_stride;
    a.nframes = (int)nframes;
    a.nchan = d->nchan;
    a.frame_stride = d->frame_stride;
    const dim3 grid((unsigned)nframes, (unsigned)d->nchan), pack_grid((unsigned)nframes + 1, (unsigned)d->nchan);
    hipLaunchKernelGGL(qk::fpkt_walk_kernel, grid, dim3(qk::kFpktWalkNT), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(qk::fpkt_scan_kernel, dim3((unsigned)d->nchan), dim3(qk::kFpktScanNT), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(qk::fpkt_pack_kernel, pack_grid, dim3(qk::kFpktPackNT), 0, s, a);
    HIPCHK(hipGetLastError());
    d->last = Launch{"fpkt_pack_kernel", (int)pack_grid.x, qk::kFpktPackNT, 0};
    d->cur ^= 1;
    if (d->nchan == 1) HIPCHK(hipMemcpyAsync(d->h_count, d->d_counts, sizeof(int), hipMemcpyDeviceToHost, s));   // process_ex reads it
    return 0;
}

// the shared host path: in_stride in frames, out_stride in bytes; the offsets go to the library's table
int fpkt_launch(Fpkt* d, const void* d_in, int64_t nframes, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    return fpkt_launch_counts(d, d_in, nframes, in_stride * d->frame_stride, nullptr, d_out, out_stride, nullptr, 0, nullptr, s);
}

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_fpkt_create(void** h, int device, int nchan, int max_block, int frame_stride) {
    Fpkt* d = nullptr;
    const bool args_ok = frame_stride >= qk::kFpktFrame && frame_stride <= 4096 && max_block <= kFpktMaxFrames;
    if (const int rc = op_new<Fpkt, fpkt_launch, fpkt_out_count>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->frame_stride = frame_stride;
    hipError_t err = stream_op_init(d, device, nchan, max_block, (size_t)frame_stride, 1);
    d->nchan = nchan;
    if (err == hipSuccess && max_block > 0) {
        // the host side's staging row holds out_size(max_block) bytes
        (void)hipFree(d->d_out);
        d->d_out = nullptr;
        err = hipMalloc(&d->d_out, (size_t)fpkt_bytes(max_block));
    }
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc(&d->d_state[i], (size_t)nchan * qk::kFpktState * sizeof(int));
        if (err == hipSuccess) err = hipMalloc(&d->d_pending[i], (size_t)nchan * qk::kFpktCap);
    }
    if (err == hipSuccess) err = hipMalloc(&d->d_counts, 2 * (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipHostMalloc(reinterpret_cast<void**>(&d->h_count), sizeof(int), hipHostMallocDefault);
    if (err == hipSuccess) err = fpkt_scratch(d, max_block > 0 ? max_block : 1);
    // (the table the single-row entry points fill; a batch call that passes no table of its own makes one on its first call)
    if (err == hipSuccess && nchan == 1) err = fpkt_own_offs(d, max_block > 0 ? max_block : 1);
    if (err == hipSuccess) {
        const int rc = fpkt_fill_initial(d);
        if (rc) err = (hipError_t)(-rc);
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return op_created<fpkt_free>(h, d, err);
}
int64_t qdsp_hip_fpkt_out_size(void* h, int64_t nframes) {
    return (as<Fpkt>(h) && nframes >= 0 && nframes <= kFpktMaxFrames) ? fpkt_bytes(nframes) : QDSP_HIP_EINVAL;
}
int64_t qdsp_hip_fpkt_out_packets(void* h, int64_t nframes) {
    return (as<Fpkt>(h) && nframes >= 0 && nframes <= kFpktMaxFrames) ? fpkt_packets(nframes) : QDSP_HIP_EINVAL;
}
int qdsp_hip_fpkt_frame_stride(void* h) {
    Fpkt* d = as<Fpkt>(h);
    return d ? d->frame_stride : QDSP_HIP_EINVAL;
}
int qdsp_hip_fpkt_process_batch_dev(void* h, const void* d_in, int64_t nframes, int64_t in_stride_bytes, const int* d_in_counts, void* d_out,
                                    int64_t out_stride_bytes, int* d_offs, int64_t offs_stride, int* d_counts, void* hip_stream) {
    Fpkt* d = as<Fpkt>(h);
    if (!d) return QDSP_HIP_EINVAL;
    return fpkt_launch_counts(d, d_in, nframes, in_stride_bytes, d_in_counts, d_out, out_stride_bytes, d_offs, offs_stride, d_counts,
                              static_cast<hipStream_t>(hip_stream));
}
int qdsp_hip_fpkt_process_dev(void* h, const void* d_in, int64_t nframes, void* d_out, void* hip_stream) {
    Fpkt* d = as<Fpkt>(h);
    if (!d) return QDSP_HIP_EINVAL;
    if (nframes < 0 || nframes > kFpktMaxFrames) return QDSP_HIP_EINVAL;
    return fpkt_launch(d, d_in, nframes, nframes, d_out, fpkt_bytes(nframes), static_cast<hipStream_t>(hip_stream));
}
int qdsp_hip_fpkt_process_ex(void* h, const void* in, int in_link, int nframes, void* out, int out_link) {
    Fpkt* d = as<Fpkt>(h);
    // the packet count is returned, so the call has to have run: an output link that hands over without waiting cannot be served
    if (!d || (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE)) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, nframes, out, out_link);
    if (rc < 0 || nframes == 0) return (int)rc;
    return *d->h_count;
}
int qdsp_hip_fpkt_process(void* h, const uint8_t* in, int nframes, uint8_t* out) {
    return qdsp_hip_fpkt_process_ex(h, in, QDSP_HIP_LINK_HOST, nframes, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_fpkt_offs_dev(void* h, int** d_offs, int64_t* stride, int** d_counts) {
    Fpkt* d = as<Fpkt>(h);
    if (!d || !d_offs || !stride || !d_counts) return QDSP_HIP_EINVAL;
    *d_offs = d->d_offs;
    *stride = d->d_offs ? fpkt_packets(d->offs_frames) + 1 : 0;
    *d_counts = d->d_counts;
    return 0;
}
int qdsp_hip_fpkt_get_offsets(void* h, int chan, int* offs, int cap) {
    Fpkt* d = as<Fpkt>(h);
    if (!d || !chan_ok(d, chan) || cap < 0 || !offs) return QDSP_HIP_EINVAL;
    int n = 0;
    if (const int rc = sync_download(d, &n, d->d_counts + chan, sizeof(int))) return rc;
    if (!d->d_offs) return QDSP_HIP_EINVAL;                   // no call has used the library's table
    const int m = n < cap ? n : cap;
    HIPCHK(hipMemcpy(offs, d->d_offs + (size_t)chan * (size_t)(fpkt_packets(d->offs_frames) + 1), (size_t)(m + 1) * sizeof(int), hipMemcpyDeviceToHost));
    return n;
}
int qdsp_hip_fpkt_get_counts(void* h, int* counts) {
    Fpkt* d = as<Fpkt>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    return sync_download(d, counts, d->d_counts, 2 * (size_t)d->nchan * sizeof(int));
}
int qdsp_hip_fpkt_get_state(void* h, int chan, uint32_t* last_counter, int* packet_read, uint8_t* pending) {
    Fpkt* d = as<Fpkt>(h);
    if (!d || !chan_ok(d, chan) || !last_counter || !packet_read) return QDSP_HIP_EINVAL;
    int v[2];
    if (const int rc = sync_download(d, v, d->d_state[d->cur] + (size_t)chan * qk::kFpktState, sizeof(v))) return rc;
    *last_counter = (uint32_t)v[0];
    *packet_read = v[1];
    if (pending) HIPCHK(hipMemcpy(pending, d->d_pending[d->cur] + (size_t)chan * qk::kFpktCap, qk::kFpktCap, hipMemcpyDeviceToHost));
    return 0;
}
int qdsp_hip_fpkt_set_state(void* h, int chan, uint32_t last_counter, int packet_read, const uint8_t* pending) {
    Fpkt* d = as<Fpkt>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    if (packet_read != -1 && (packet_read < 1 || packet_read > qk::kFpktCap || !pending)) return QDSP_HIP_EINVAL;
    const int v[2] = {(int)last_counter, packet_read};
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++) {
        HIPCHK(hipMemcpy(d->d_state[d->cur] + (size_t)c * qk::kFpktState, v, sizeof(v), hipMemcpyHostToDevice));
        if (packet_read > 0) HIPCHK(hipMemcpy(d->d_pending[d->cur] + (size_t)c * qk::kFpktCap, pending, (size_t)packet_read, hipMemcpyHostToDevice));
    }
    return 0;
}
int qdsp_hip_fpkt_reset(void* h) {
    Fpkt* d = as<Fpkt>(h);
    if (!d) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    return fpkt_fill_initial(d);
}
void qdsp_hip_fpkt_destroy(void* h) { fpkt_free(as<Fpkt>(h)); }

}  // extern "C"
