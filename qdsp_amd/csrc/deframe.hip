// deframe.hip -- Threshold and Deframer batched over channel rows (design notes: deframe.hip.h), and their C entry points.
#include "deframe.hip.h"

#include <cstring>
#include <new>

namespace qk {

namespace {

// in > 0.0f on the bit pattern: positive, not zero, not NaN (independent of the denormal mode)
__device__ __forceinline__ unsigned thr_bit(float x) {
    const int b = __float_as_int(x);
    return (b > 0 && b <= 0x7f800000) ? 1u : 0u;
}

// bytes of row `row` in this call
__device__ __forceinline__ int row_count(const int* in_counts, int row, long long count) {
    if (!in_counts) return (int)count;
    const int c = in_counts[row];
    return c < 0 ? 0 : (c < count ? c : (int)count);
}

template <int KIND> __device__ __forceinline__ unsigned in_byte(const void* row, int i) {
    if constexpr (KIND == 0) return static_cast<const unsigned char*>(row)[i];
    else return thr_bit(static_cast<const float*>(row)[i]);
}

// B[j], 0 <= j < n + L: the carried tail, then the call's bytes
template <int KIND> __device__ __forceinline__ unsigned work_byte(const unsigned char* tail, const void* row, int L, int j) {
    return j < L ? tail[j] : in_byte<KIND>(row, j - L);
}

template <int KIND> __device__ __forceinline__ const void* in_row(const DeframeArgs& a, int row) {
    if constexpr (KIND == 0) return static_cast<const unsigned char*>(a.in) + (long long)row * a.in_stride;
    else return static_cast<const float*>(a.in) + (long long)row * a.in_stride;
}

}  // namespace

__global__ __launch_bounds__(kThrNT) void threshold_kernel(const ThresholdArgs a) {
    const int row = blockIdx.y, t = threadIdx.x;
    const int n = row_count(a.in_counts, row, a.count);
    const float* x = a.in + (long long)row * a.in_stride;
    unsigned char* y = a.out + (long long)row * a.out_stride;
    int head = (int)((16 - ((uintptr_t)y & 15)) & 15);
    if (head > n) head = n;
    if (blockIdx.x == 0 && t < head) y[t] = (unsigned char)thr_bit(x[t]);
    const long long i0 = head + ((long long)blockIdx.x * kThrNT + t) * kThrPer;
    if (i0 >= n) return;
    if (i0 + kThrPer <= n) {
        float v[kThrPer];
        if (((uintptr_t)(x + i0) & 15) == 0) {
            const float4* p = reinterpret_cast<const float4*>(x + i0);
#pragma unroll
            for (int j = 0; j < kThrPer / 4; j++) {
                const float4 q = p[j];
                v[4 * j] = q.x;
                v[4 * j + 1] = q.y;
                v[4 * j + 2] = q.z;
                v[4 * j + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kThrPer; j++) v[j] = x[i0 + j];
        }
        unsigned w[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            w[j] = thr_bit(v[4 * j]) | (thr_bit(v[4 * j + 1]) << 8) | (thr_bit(v[4 * j + 2]) << 16) | (thr_bit(v[4 * j + 3]) << 24);
        *reinterpret_cast<uint4*>(y + i0) = make_uint4(w[0], w[1], w[2], w[3]);      // y + head is 16-byte aligned
    } else {
        for (long long i = i0; i < n; i++) y[i] = (unsigned char)thr_bit(x[i]);
    }
}

template <int KIND> __global__ __launch_bounds__(kDfNT) void deframe_match_kernel(const DeframeArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char img[kDfTile + kDfMaxSync];
    __shared__ unsigned char sw[kDfMaxSync];
    const int row = blockIdx.y, t = threadIdx.x;
    const int n = row_count(a.in_counts, row, a.count);
    const int L = a.sync_len;
    const long long t0 = (long long)blockIdx.x * kDfTile;
    if (blockIdx.x != 0 && t0 >= n) return;
    const void* x = in_row<KIND>(a, row);
    const unsigned char* tail = a.tail + (long long)row * L;
    if (blockIdx.x == 0 && t < L) a.tail_next[(long long)row * L + t] = (unsigned char)work_byte<KIND>(tail, x, L, n + t);   // n + t - L < n
    if (t0 >= n) return;
    const long long top = (long long)n + L;                    // B has n + L bytes
    // the lane's bytes of the tile and its halo go into registers first, so that the loads are in flight together
    constexpr int kPer = (kDfTile + kDfMaxSync + kDfNT - 1) / kDfNT;
    unsigned char v[kPer];
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int j = u * kDfNT + t;
        v[u] = (j < kDfTile + L - 1 && t0 + j < top) ? (unsigned char)work_byte<KIND>(tail, x, L, (int)(t0 + j)) : 0;
    }
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int j = u * kDfNT + t;
        if (j < kDfTile + L - 1) img[j] = v[u];
    }
    if (t < L) sw[t] = a.sync[t];
    __syncthreads();
    unsigned long long* words = a.words + (long long)row * a.wstride;
    const unsigned* img32 = reinterpret_cast<const unsigned*>(img);
    unsigned long long s8 = 0ull;                              // the word's first eight bytes, and which of them exist
    for (int c = 0; c < 8 && c < L; c++) s8 |= (unsigned long long)sw[c] << (8 * c);
    const unsigned long long mask8 = L >= 8 ? ~0ull : (1ull << (8 * L)) - 1ull;
#pragma unroll
    for (int k = 0; k < kDfTile / kDfNT; k++) {
        const int p = k * kDfNT + t;
        bool m = false;
        if (t0 + p < n) {
            // the first eight bytes at once: the three aligned words around img[p], shifted into place (bytes behind the word's
            // length are masked, so what lies behind the halo does not matter: p + 11 < sizeof(img))
            const unsigned w0 = img32[p >> 2], w1 = img32[(p >> 2) + 1], w2 = img32[(p >> 2) + 2];
            const unsigned lo = __builtin_amdgcn_alignbyte(w1, w0, p & 3), hi = __builtin_amdgcn_alignbyte(w2, w1, p & 3);
            const unsigned long long v = ((unsigned long long)hi << 32) | lo;
            if (((v ^ s8) & mask8) == 0ull) {
                int c = L < 8 ? L : 8;
                while (c < L && img[p + c] == sw[c]) c++;      // p + c <= kDfTile - 1 + L - 1
                m = c == L;
            }
        }
        const unsigned long long bal = __ballot(m);
        if ((t & 63) == 0 && t0 + p < n) words[(t0 + p) >> 6] = bal;   // word < ceil(n / 64) <= wstride
    }
}

__global__ __launch_bounds__(64) void deframe_walk_kernel(const DeframeArgs a) {
    __shared__ unsigned long long w[kDfWalkWords];
    const int row = blockIdx.x, lane = threadIdx.x;
    // (every value that steers the walk is the same in all lanes: readfirstlane tells the compiler, so the loop is scalar code)
    const int n = __builtin_amdgcn_readfirstlane(row_count(a.in_counts, row, a.count));
    const int nw = (n + 63) >> 6;
    const unsigned long long* words = a.words + (long long)row * a.wstride;
    int* starts = a.starts + (long long)row * (a.cap + 1);
    int br = __builtin_amdgcn_readfirstlane(a.state[row * kDfState]), bad = __builtin_amdgcn_readfirstlane(a.state[row * kDfState + 1]);
    int after = __builtin_amdgcn_readfirstlane(a.state[row * kDfState + 2]);
    int start = br >= 0 ? -br : 0;
    int nf = 0, i = 0;
    const int flen = a.frame_len;
    // reading: the rest of the frame, or of the call, at once; a frame that ends leaves its start behind
    auto read_on = [&]() {
        const int step = flen - br < n - i ? flen - br : n - i;
        i += step;
        br += step;
        if (br == flen) {
            if (lane == 0 && nf < a.cap) starts[nf] = start;
            nf++;
            br = -1;
            after = 1;
        }
    };
    while (i < n) {
        if (br >= 0) {                                         // reading needs no match bits
            read_on();
            continue;
        }
        const int w0 = (i >> 6) / kDfWalkWords * kDfWalkWords;
        const int cw = nw - w0 < kDfWalkWords ? nw - w0 : kDfWalkWords;
        for (int j0 = 0; j0 < cw; j0 += 64 * kDfWalkBatch) {       // kDfWalkBatch loads per lane in flight together
            unsigned long long r[kDfWalkBatch];
#pragma unroll
            for (int u = 0; u < kDfWalkBatch; u++) {
                const int j = j0 + u * 64 + lane;
                r[u] = j < cw ? words[w0 + j] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < kDfWalkBatch; u++) {
                const int j = j0 + u * 64 + lane;
                if (j < cw) w[j] = r[u];
            }
        }
        __syncthreads();
        const int cend = (w0 + cw) * 64 < n ? (w0 + cw) * 64 : n;
        while (i < cend) {
            if (br >= 0) {
                read_on();
                continue;
            }
            if (after) {
                after = 0;
                const bool m = __builtin_amdgcn_readfirstlane((int)((w[(i >> 6) - w0] >> (i & 63)) & 1));
                if (m) {
                    bad = 0;
                    br = 0;
                    start = i;
                } else if (bad < 5) {
                    bad++;
                    br = 0;
                    start = i;
                }
                continue;
            }
            // searching: 64 words per step
            const int wi = (i >> 6) - w0 + lane;
            unsigned long long mw = wi < cw ? w[wi] : 0ull;
            if (lane == 0) mw &= ~0ull << (i & 63);
            const unsigned long long bal = __ballot(mw != 0ull);
            if (bal) {
                const int fl = __ffsll((long long)bal) - 1;
                const unsigned lo = __shfl((unsigned)mw, fl), hi = __shfl((unsigned)(mw >> 32), fl);
                const unsigned long long hit = ((unsigned long long)hi << 32) | lo;
                i = __builtin_amdgcn_readfirstlane((((i >> 6) + fl) << 6) + __ffsll((long long)hit) - 1);   // a set bit lies below n: < cend
                bad = 0;
                br = 0;
                start = i;
            } else {
                const int nx = ((i >> 6) + 64) << 6;
                i = nx < cend ? nx : cend;
            }
        }
        __syncthreads();                                       // the next chunk overwrites w
    }
    if (lane == 0) {
        int* st = a.state_next + row * kDfState;
        st[0] = br;
        st[1] = bad;
        st[2] = after;
        st[3] = 0;
        int* me = a.meta + row * kDfMeta;
        me[0] = nf < a.cap ? nf : a.cap;
        me[1] = br > 0 ? 1 : 0;
        me[2] = start;
        me[3] = br > 0 ? br : 0;
        a.counts[row] = nf < a.cap ? nf : a.cap;
    }
}

template <int KIND> __global__ __launch_bounds__(kDfNT) void deframe_pack_kernel(const DeframeArgs a) {
    const int row = blockIdx.y;
    const long long t = (long long)blockIdx.x * kDfNT + threadIdx.x;
    const int fb = a.frame_bytes;
    const long long m = t / fb;
    const int b = (int)(t - m * fb);
    const int* me = a.meta + row * kDfMeta;
    const int nf = me[0];
    int s, bits;
    unsigned char* dst;
    if (m < nf) {
        s = a.starts[(long long)row * (a.cap + 1) + m];
        bits = a.frame_len;
        dst = a.out + (long long)row * a.out_stride + m * fb + b;          // m < cap: inside out_stride
    } else if (m == nf && me[1]) {
        s = me[2];
        bits = me[3];
        if (8 * b >= bits) return;
        dst = a.carry_next + (long long)row * fb + b;
    } else {
        return;
    }
    const int n = row_count(a.in_counts, row, a.count);
    const int L = a.sync_len;
    const void* x = in_row<KIND>(a, row);
    const unsigned char* tail = a.tail + (long long)row * L;
    unsigned v = 0;
    if (s < 0 && 8 * b < -s) v = a.carry[(long long)row * fb + b];         // the bits of earlier calls
#pragma unroll
    for (int kk = 0; kk < 8; kk++) {
        const int k = 8 * b + kk;
        const long long j = (long long)s + k;
        if (k < bits && j >= 0 && j < n) v |= (work_byte<KIND>(tail, x, L, (int)j) << (7 - kk)) & 0xffu;
    }
    *dst = (unsigned char)v;
}

}  // namespace qk

namespace qh {

namespace {

bool spans_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}

constexpr int64_t kMaxCount = (int64_t)1 << 30;     // positions of a call are ints

// ---- Threshold ----

int thr_launch_counts(Threshold* d, const void* d_in, int64_t count, int64_t in_stride, const int* d_in_counts, void* d_out,
                      int64_t out_stride, hipStream_t s) {
    if (count < 0 || count > kMaxCount || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < count || ((uintptr_t)d_in & 3)) return QDSP_HIP_EINVAL;
    if (count == 0) return 0;
    const size_t in_span = ((size_t)(d->nchan - 1) * in_stride + count) * sizeof(float), out_span = (size_t)(d->nchan - 1) * out_stride + count;
    if (spans_overlap(d_in, in_span, d_out, out_span)) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    qk::ThresholdArgs a;
    a.in = static_cast<const float*>(d_in);
    a.out = static_cast<unsigned char*>(d_out);
    a.in_counts = d_in_counts;
    a.count = count;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    const int64_t groups = (count + qk::kThrPer - 1) / qk::kThrPer;
    const dim3 grid((unsigned)((groups + qk::kThrNT - 1) / qk::kThrNT), (unsigned)d->nchan), block(qk::kThrNT);
    hipLaunchKernelGGL(qk::threshold_kernel, grid, block, 0, s, a);
    HIPCHK(hipGetLastError());
    d->last = Launch{"threshold_kernel", (int)grid.x, qk::kThrNT, 0};
    return 0;
}

int thr_launch(Threshold* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    return thr_launch_counts(d, d_in, count, in_stride, nullptr, d_out, out_stride, s);
}

void thr_free(Threshold* d) {
    op_free(d, [] {});
}

// ---- Deframer ----

int64_t df_out_size(const Deframer* d, int64_t count) { return count <= 0 ? 0 : (count + d->frame_len - 1) / d->frame_len; }
int64_t df_out_count(const StreamOp* op, int64_t count) {
    const Deframer* d = static_cast<const Deframer*>(op);
    return df_out_size(d, count) * d->frame_bytes;
}

void df_free(Deframer* d) {
    op_free(d, [d] {
        hip_free_all({d->d_sync, d->d_tail[0], d->d_tail[1], d->d_carry[0], d->d_carry[1], d->d_state[0], d->d_state[1], d->d_words, d->d_starts,
                      d->d_meta, d->d_counts});
        if (d->h_count) (void)hipHostFree(d->h_count);
    });
}

// the match words and frame starts of calls of up to `count` bytes per row (a larger call than any before synchronises the device)
hipError_t df_scratch(Deframer* d, int64_t count) {
    if (count <= d->scratch_count) return hipSuccess;
    hipError_t err = hipDeviceSynchronize();
    if (d->d_words) (void)hipFree(d->d_words);
    if (d->d_starts) (void)hipFree(d->d_starts);
    d->d_words = nullptr;
    d->d_starts = nullptr;
    d->scratch_count = 0;
    const size_t wstride = (size_t)((count + 63) / 64), cap = (size_t)df_out_size(d, count);
    if (err == hipSuccess) err = hipMalloc(&d->d_words, (size_t)d->nchan * wstride * sizeof(unsigned long long));
    if (err == hipSuccess) err = hipMalloc(&d->d_starts, (size_t)d->nchan * (cap + 1) * sizeof(int));
    if (err == hipSuccess) d->scratch_count = count;
    return err;
}

// the state after create / reset, in both slots
int df_fill_initial(Deframer* d) {
    std::vector<int> st((size_t)d->nchan * qk::kDfState, 0);
    for (int c = 0; c < d->nchan; c++) {
        st[(size_t)c * qk::kDfState] = -1;
        st[(size_t)c * qk::kDfState + 1] = 5;
    }
    for (int s = 0; s < 2; s++) {
        HIPCHK(hipMemcpy(d->d_state[s], st.data(), st.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(d->d_tail[s], 0, (size_t)d->nchan * d->sync_len));
        HIPCHK(hipMemset(d->d_carry[s], 0, (size_t)d->nchan * d->frame_bytes));
    }
    HIPCHK(hipMemset(d->d_counts, 0, (size_t)d->nchan * sizeof(int)));
    return 0;
}

int df_launch_counts(Deframer* d, const void* d_in, int64_t count, int64_t in_stride, const int* d_in_counts, void* d_out,
                     int64_t out_stride, hipStream_t s) {
    if (count < 0 || count > kMaxCount || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    const int64_t cap = df_out_size(d, count);
    if (in_stride < count || out_stride < cap * d->frame_bytes) return QDSP_HIP_EINVAL;
    if (d->kind && ((uintptr_t)d_in & 3)) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    if (count == 0) {
        HIPCHK(hipMemsetAsync(d->d_counts, 0, (size_t)d->nchan * sizeof(int), s));
        return 0;
    }
    const size_t es = d->kind ? sizeof(float) : 1;
    const size_t in_span = ((size_t)(d->nchan - 1) * in_stride + count) * es;
    const size_t out_span = (size_t)(d->nchan - 1) * out_stride + (size_t)cap * d->frame_bytes;
    if (spans_overlap(d_in, in_span, d_out, out_span)) return QDSP_HIP_EINVAL;
    if (const hipError_t err = df_scratch(d, count)) return -(int)err;
    qk::DeframeArgs a;
    a.in = d_in;
    a.in_counts = d_in_counts;
    a.out = static_cast<unsigned char*>(d_out);
    a.sync = d->d_sync;
    a.tail = d->d_tail[d->cur];
    a.tail_next = d->d_tail[d->cur ^ 1];
    a.carry = d->d_carry[d->cur];
    a.carry_next = d->d_carry[d->cur ^ 1];
    a.state = d->d_state[d->cur];
    a.state_next = d->d_state[d->cur ^ 1];
    a.words = d->d_words;
    a.starts = d->d_starts;
    a.meta = d->d_meta;
    a.counts = d->d_counts;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.wstride = (count + 63) / 64;
    a.count = (int)count;
    a.cap = (int)cap;
    a.frame_len = d->frame_len;
    a.frame_bytes = d->frame_bytes;
    a.sync_len = d->sync_len;
    a.nchan = d->nchan;
    const dim3 block(qk::kDfNT);
    const dim3 mgrid((unsigned)((count + qk::kDfTile - 1) / qk::kDfTile), (unsigned)d->nchan);
    if (d->kind) hipLaunchKernelGGL(qk::deframe_match_kernel<1>, mgrid, block, 0, s, a);
    else hipLaunchKernelGGL(qk::deframe_match_kernel<0>, mgrid, block, 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(qk::deframe_walk_kernel, dim3((unsigned)d->nchan), dim3(64), 0, s, a);
    HIPCHK(hipGetLastError());
    const int64_t bytes = (cap + 1) * d->frame_bytes;          // the frames that end in the call, and the one in progress
    const dim3 pgrid((unsigned)((bytes + qk::kDfNT - 1) / qk::kDfNT), (unsigned)d->nchan);
    if (d->kind) hipLaunchKernelGGL(qk::deframe_pack_kernel<1>, pgrid, block, 0, s, a);
    else hipLaunchKernelGGL(qk::deframe_pack_kernel<0>, pgrid, block, 0, s, a);
    HIPCHK(hipGetLastError());
    d->last = Launch{"deframe_match_kernel", (int)mgrid.x, qk::kDfNT, qk::kDfTile + 2 * qk::kDfMaxSync};
    d->cur ^= 1;
    if (d->nchan == 1) HIPCHK(hipMemcpyAsync(d->h_count, d->d_counts, sizeof(int), hipMemcpyDeviceToHost, s));   // process_ex reads it
    return 0;
}

int df_launch(Deframer* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    return df_launch_counts(d, d_in, count, in_stride, nullptr, d_out, out_stride, s);
}

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_threshold_create(void** h, int device, int nchan, int max_block) {
    Threshold* d = nullptr;
    if (const int rc = op_new<Threshold, thr_launch>(&d, h, true, device, nchan, max_block)) return rc;
    return op_created<thr_free>(h, d, stream_op_init(d, device, nchan, max_block, sizeof(float), 1));
}
int qdsp_hip_threshold_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, const int* d_in_counts, void* d_out,
                                         int64_t out_stride, void* hip_stream) {
    Threshold* d = as<Threshold>(h);
    return d ? thr_launch_counts(d, d_in, count, in_stride, d_in_counts, d_out, out_stride, static_cast<hipStream_t>(hip_stream)) : QDSP_HIP_EINVAL;
}
int qdsp_hip_threshold_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<Threshold, thr_launch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_threshold_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<Threshold>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_threshold_process(void* h, const float* in, int count, uint8_t* out) {
    return qdsp_hip_threshold_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
void qdsp_hip_threshold_destroy(void* h) { thr_free(as<Threshold>(h)); }
int qdsp_hip_threshold_span(void) { return qk::kThrNT * qk::kThrPer; }

int qdsp_hip_deframer_create(void** h, int device, int kind, int nchan, int max_block, int frame_len, const uint8_t* sync, int sync_len) {
    Deframer* d = nullptr;
    const bool args_ok = (kind == 0 || kind == 1) && frame_len >= 1 && frame_len <= (1 << 20) && sync && sync_len >= 1 && sync_len <= qk::kDfMaxSync;
    if (const int rc = op_new<Deframer, df_launch, df_out_count>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->kind = kind;
    d->frame_len = frame_len;
    d->frame_bytes = (frame_len + 7) / 8;
    d->sync_len = sync_len;
    d->sync.assign(sync, sync + sync_len);
    hipError_t err = stream_op_init(d, device, nchan, max_block, kind ? sizeof(float) : 1, 1);
    d->nchan = nchan;
    if (err == hipSuccess && max_block > 0) {
        // the host side's staging row holds out_size(max_block) frames, not max_block bytes
        (void)hipFree(d->d_out);
        d->d_out = nullptr;
        err = hipMalloc(&d->d_out, (size_t)df_out_count(d, max_block));
    }
    if (err == hipSuccess) err = hipMalloc(&d->d_sync, (size_t)sync_len);
    if (err == hipSuccess) err = hipMemcpy(d->d_sync, sync, (size_t)sync_len, hipMemcpyHostToDevice);
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc(&d->d_tail[i], (size_t)nchan * sync_len);
        if (err == hipSuccess) err = hipMalloc(&d->d_carry[i], (size_t)nchan * d->frame_bytes);
        if (err == hipSuccess) err = hipMalloc(&d->d_state[i], (size_t)nchan * qk::kDfState * sizeof(int));
    }
    if (err == hipSuccess) err = hipMalloc(&d->d_meta, (size_t)nchan * qk::kDfMeta * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&d->d_counts, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipHostMalloc(reinterpret_cast<void**>(&d->h_count), sizeof(int), hipHostMallocDefault);
    if (err == hipSuccess) err = df_scratch(d, max_block > 0 ? max_block : 1);
    if (err == hipSuccess) {
        *d->h_count = 0;
        const int rc = df_fill_initial(d);
        if (rc) err = (hipError_t)(-rc);
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return op_created<df_free>(h, d, err);
}
int qdsp_hip_deframer_set_sync(void* h, const uint8_t* sync, int sync_len) {
    Deframer* d = as<Deframer>(h);
    if (!d || !sync || sync_len != d->sync_len) return QDSP_HIP_EINVAL;
    if (const int rc = sync_upload(d, d->d_sync, sync, (size_t)sync_len)) return rc;
    d->sync.assign(sync, sync + sync_len);
    return 0;
}
int qdsp_hip_deframer_get_state(void* h, int chan, int* bits_read, int* bad, int* after) {
    Deframer* d = as<Deframer>(h);
    if (!d || !chan_ok(d, chan) || !bits_read || !bad || !after) return QDSP_HIP_EINVAL;
    int v[3];
    if (const int rc = sync_download(d, v, d->d_state[d->cur] + (size_t)chan * qk::kDfState, sizeof(v))) return rc;
    *bits_read = v[0];
    *bad = v[1];
    *after = v[2];
    return 0;
}
int qdsp_hip_deframer_set_state(void* h, int chan, int bits_read, int bad, int after) {
    Deframer* d = as<Deframer>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    if (bits_read < -1 || bits_read >= d->frame_len || bad < 0 || bad > 5 || (after != 0 && after != 1)) return QDSP_HIP_EINVAL;
    if (bits_read >= 0 && after) return QDSP_HIP_EINVAL;      // `after` is only ever set between two frames
    const int v[3] = {bits_read, bad, after};
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++)
        HIPCHK(hipMemcpy(d->d_state[d->cur] + (size_t)c * qk::kDfState, v, sizeof(v), hipMemcpyHostToDevice));
    return 0;
}
int64_t qdsp_hip_deframer_out_size(void* h, int64_t count) {
    Deframer* d = as<Deframer>(h);
    return (d && count >= 0) ? df_out_size(d, count) : QDSP_HIP_EINVAL;
}
int qdsp_hip_deframer_frame_bytes(void* h) {
    Deframer* d = as<Deframer>(h);
    return d ? d->frame_bytes : QDSP_HIP_EINVAL;
}
int qdsp_hip_deframer_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, const int* d_in_counts, void* d_out,
                                        int64_t out_stride_bytes, int* d_counts, void* hip_stream) {
    Deframer* d = as<Deframer>(h);
    if (!d) return QDSP_HIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (const int rc = df_launch_counts(d, d_in, count, in_stride, d_in_counts, d_out, out_stride_bytes, s)) return rc;
    if (d_counts) HIPCHK(hipMemcpyAsync(d_counts, d->d_counts, (size_t)d->nchan * sizeof(int), hipMemcpyDeviceToDevice, s));
    return 0;
}
int qdsp_hip_deframer_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    Deframer* d = as<Deframer>(h);
    return d ? df_launch(d, d_in, count, count, d_out, df_out_count(d, count), static_cast<hipStream_t>(hip_stream)) : QDSP_HIP_EINVAL;
}
int qdsp_hip_deframer_get_counts(void* h, int* counts) {
    Deframer* d = as<Deframer>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    return sync_download(d, counts, d->d_counts, (size_t)d->nchan * sizeof(int));
}
int qdsp_hip_deframer_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    Deframer* d = as<Deframer>(h);
    // the frame count is returned, so the call has to have run: an output link that hands over without waiting cannot be served
    if (!d || (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE)) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, count, out, out_link);
    if (rc < 0 || count == 0) return (int)rc;
    return *d->h_count;
}
int qdsp_hip_deframer_process(void* h, const void* in, int count, uint8_t* out) {
    return qdsp_hip_deframer_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_deframer_reset(void* h) {
    Deframer* d = as<Deframer>(h);
    if (!d) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    return df_fill_initial(d);
}
void qdsp_hip_deframer_destroy(void* h) { df_free(as<Deframer>(h)); }
int qdsp_hip_deframer_tile(void) { return qk::kDfTile; }
int qdsp_hip_deframer_pack_span(void) { return qk::kDfNT * 8; }

}  // extern "C"
