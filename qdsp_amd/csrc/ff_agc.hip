// ff_agc.hip -- FeedForwardAGC (design notes: ff_agc.hip.h) and its C entry points.
// Compiled with the library's default flags: no fast-math, correctly rounded f32 division.  The reference's fastAmplitude is
// restated below under `#pragma clang fp contract(off)`.
#include "ff_agc.hip.h"

namespace qk {

namespace {
// sample i of [history | in] of one row, NC floats
template <int NC> __device__ __forceinline__ void row_sample(const FfAgcArgs& a, const float* hist, const float* in, long long i, float (&v)[NC]) {
    const float* p = i < a.fill ? hist + i * NC : in + (i - a.fill) * NC;
#pragma unroll
    for (int e = 0; e < NC; e++) v[e] = p[e];
}

// what the window maximum is taken of: fabsf of the float / of re; a NaN as +0.0f (it never passes `val > level`)
__device__ __forceinline__ float level_arg(float v) {
    const float r = fabsf(v);
    return r >= 0.0f ? r : 0.0f;
}

// the level of one output from the maximum of r over its window
template <int KIND> __device__ __forceinline__ float level_of(float r) {
#pragma clang fp contract(off)
    float val = r;
    if constexpr (KIND == kFfAgcComplex) {
        const float t = 0.4f * r;   // fastAmplitude (types.h:58-63): im_abs + 0.4f * re_abs, both fabsf(re)
        val = r + t;
    }
    float level = 1e-4f;
    if (val > level) level = val;
    return level;
}

__device__ __forceinline__ float max2(float a, float b) { return b > a ? b : a; }   // (no NaN in LDS)
__device__ __forceinline__ float4 max4(float4 a, float4 b) { return make_float4(max2(a.x, b.x), max2(a.y, b.y), max2(a.z, b.z), max2(a.w, b.w)); }
}  // namespace

template <int KIND> __global__ __launch_bounds__(kDemodNT) void ff_agc_kernel(const FfAgcArgs a) {
    constexpr int NC = KIND == kFfAgcComplex ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int c = blockIdx.y, t = threadIdx.x;
    const float* __restrict__ in = a.in + (long long)c * a.in_stride * NC;
    const float* __restrict__ hist = a.hist + (long long)c * a.hstride * NC;
    const long long total = (long long)a.fill + a.count;   // samples of [history | in]

    if ((int)blockIdx.x == a.tiles) {   // the next history: samples nout .. nout + fill_next - 1
        float* __restrict__ hn = a.hist_next + (long long)c * a.hstride * NC;
        for (int j = t; j < a.fill_next; j += kDemodNT) {
            float v[NC];
            row_sample<NC>(a, hist, in, a.nout + j, v);
#pragma unroll
            for (int e = 0; e < NC; e++) hn[j * NC + e] = v[e];
        }
        return;
    }

    const int L4 = a.L >> 2, L = L4 << 2, nst = kFfAgcTile + a.W - 1;
    const long long b = (long long)blockIdx.x * kFfAgcTile;
    float4* lds4 = reinterpret_cast<float4*>(lds);
    int src4 = 0, dst4 = L4;   // the two arrays, as offsets into lds4[]
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    // stage: float j of the first array = r of sample b + j; +0.0f past the end of the row (under outputs that are not stored)
    float x[kDemodSpl][NC];
#pragma unroll
    for (int it = 0; it < kDemodSpl; it++) {
        const long long i = b + it * kDemodNT + t;
#pragma unroll
        for (int e = 0; e < NC; e++) x[it][e] = 0.0f;
        if (i < total) row_sample<NC>(a, hist, in, i, x[it]);
        lds[it * kDemodNT + t] = level_arg(x[it][0]);
    }
    for (int j = kFfAgcTile + t; j < L; j += kDemodNT) {
        const long long i = b + j;
        float v[NC] = {};
        if (j < nst && i < total) row_sample<NC>(a, hist, in, i, v);
        lds[j] = level_arg(v[0]);
    }
    __syncthreads();

    // maxima by doubling; a partner past the array is +0.0f (no r is below it)
    int j0 = 0;
    if (a.k >= 2) {   // M_2 from r
        for (int q = t; q < L4; q += kDemodNT) {
            const float4 u = lds4[src4 + q];
            const float4 v = q + 1 < L4 ? lds4[src4 + q + 1] : zero4;
            const float uzw = max2(u.z, u.w), vxy = max2(v.x, v.y), m12 = max2(u.y, uzw), m3x = max2(u.w, v.x);
            lds4[dst4 + q] = make_float4(max2(u.x, m12), max2(m12, v.x), max2(uzw, vxy), max2(m3x, max2(v.y, v.z)));
        }
        j0 = 2;
    } else if (a.k == 1) {
        for (int p = t; p < L; p += kDemodNT) lds[L + p] = max2(lds[p], p + 1 < L ? lds[p + 1] : 0.0f);
        j0 = 1;
    }
    if (j0) {
        __syncthreads();
        src4 ^= L4; dst4 ^= L4;   // (one is 0, the other L4)
    }
    for (int j = j0; j < a.k; j++) {
        const int off4 = 1 << (j - 2);
        for (int q = t; q < L4; q += kDemodNT) {
            const float4 u = lds4[src4 + q];
            const float4 v = q + off4 < L4 ? lds4[src4 + q + off4] : zero4;
            lds4[dst4 + q] = max4(u, v);
        }
        __syncthreads();
        src4 ^= L4; dst4 ^= L4;
    }
    const int src = src4 << 2, dst = dst4 << 2;
    // the offset combine: the window of output p is [p, p + 2^k) and [p + W - 2^k, p + W)
    const int d = a.W - (1 << a.k);
#pragma unroll
    for (int it = 0; it < kDemodSpl; it++) {
        const int p = it * kDemodNT + t;   // (p + d <= kFfAgcTile - 1 + W - 1 < L)
        lds[dst + p] = level_of<KIND>(max2(lds[src + p], lds[src + p + d]));
    }
    __syncthreads();

    const long long left = a.nout - b;
    const int nv = left < kFfAgcTile ? (int)left : kFfAgcTile;   // outputs of this tile
    float* __restrict__ out = a.out + ((long long)c * a.out_stride + b) * NC;
    float y[kDemodSpl][NC];
#pragma unroll
    for (int it = 0; it < kDemodSpl; it++) {
        const float level = lds[dst + it * kDemodNT + t];
#pragma unroll
        for (int e = 0; e < NC; e++) y[it][e] = x[it][e] / level;
    }
    if (!a.vec) {
#pragma unroll
        for (int it = 0; it < kDemodSpl; it++) {
            const int p = it * kDemodNT + t;
            if (p < nv) {
#pragma unroll
                for (int e = 0; e < NC; e++) out[p * NC + e] = y[it][e];
            }
        }
        return;
    }
    // 16-byte stores: the tile's quotients laid out in LDS as they lie in the row (kFfAgcTile * NC <= 2 * L floats)
    __syncthreads();   // (every lane has read its levels)
#pragma unroll
    for (int it = 0; it < kDemodSpl; it++) {
#pragma unroll
        for (int e = 0; e < NC; e++) lds[(it * kDemodNT + t) * NC + e] = y[it][e];
    }
    __syncthreads();
    const int nf = nv * NC;   // floats to store
#pragma unroll
    for (int it = 0; it < kDemodSpl * NC / 4; it++) {
        const int f = (it * kDemodNT + t) * 4;
        if (f + 4 <= nf) {
            *reinterpret_cast<float4*>(out + f) = lds4[it * kDemodNT + t];
        } else {
            for (int e = f; e < nf; e++) out[e] = lds[e];
        }
    }
}

}  // namespace qk

namespace qh {

namespace {
int comps(const FfAgc* d) { return d->kind == qk::kFfAgcComplex ? 2 : 1; }
int hstride(const FfAgc* d) { return d->window > 1 ? d->window - 1 : 1; }
size_t hist_bytes(const FfAgc* d) { return (size_t)d->nchan * hstride(d) * comps(d) * sizeof(float); }
int64_t out_count(const StreamOp* op, int64_t count) {   // (StreamOp::out_count)
    const FfAgc* d = static_cast<const FfAgc*>(op);
    const int64_t n = (int64_t)d->fill + count - (d->window - 1);
    return n > 0 ? n : 0;
}

void ffagc_free(FfAgc* d) {
    op_free(d, [d] { hip_free_all({d->d_hist[0], d->d_hist[1]}); });
}

int64_t ffagc_launch(FfAgc* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s);

int ffagc_new(void** h, int device, int kind, int nchan, int max_block, int window) {
    FfAgc* d = nullptr;
    const bool args_ok = (kind == QDSP_HIP_FFAGC_REAL || kind == QDSP_HIP_FFAGC_COMPLEX) && window >= 1 && window <= qk::kFfAgcMaxWindow;
    if (const int rc = op_new<FfAgc, ffagc_launch, out_count>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->kind = kind;
    d->window = window;
    hipError_t err = stream_op_init(d, device, nchan, max_block, comps(d) * sizeof(float), comps(d) * sizeof(float));
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc(&d->d_hist[i], hist_bytes(d));
        if (err == hipSuccess) err = hipMemset(d->d_hist[i], 0, hist_bytes(d));
    }
    return op_created<ffagc_free>(h, d, err);
}

// d_in: nchan rows of `count` samples, in_stride apart; d_out: nchan rows of the call's outputs, out_stride apart.  Returns the
// number of outputs per row (>= 0) or an error.
int64_t ffagc_launch(FfAgc* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (count < 0 || (count > 0 && !d_in)) return QDSP_HIP_EINVAL;
    const int64_t nout = out_count(d, count);
    if (nout > 0 && !d_out) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < nout) return QDSP_HIP_EINVAL;
    const int nc = comps(d);
    const size_t es = (size_t)nc * sizeof(float);
    const uintptr_t amask = (uintptr_t)(es - 1);
    if (((uintptr_t)d_in & amask) || ((uintptr_t)d_out & amask)) return QDSP_HIP_EINVAL;
    if (count == 0) return 0;
    if (nout > 0) {   // (an output depends on the W - 1 inputs after its own: no overlap at all)
        const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + ((uintptr_t)(d->nchan - 1) * in_stride + count) * es;
        const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + ((uintptr_t)(d->nchan - 1) * out_stride + nout) * es;
        if (i0 < o1 && o0 < i1) return QDSP_HIP_EINVAL;
    }
    const long long tiles = (nout + qk::kFfAgcTile - 1) / qk::kFfAgcTile;
    if (tiles >= 0x7fffffffLL) return QDSP_HIP_ESIZE;
    HIPCHK(hipSetDevice(d->device));
    qk::FfAgcArgs a;
    a.in = static_cast<const float*>(d_in);
    a.out = static_cast<float*>(d_out);
    a.hist = d->d_hist[d->cur];
    a.hist_next = d->d_hist[d->cur ^ 1];
    a.count = count;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.nout = nout;
    a.W = d->window;
    a.k = 0;
    while ((2 << a.k) <= a.W) a.k++;
    a.fill = d->fill;
    a.fill_next = (int)((int64_t)d->fill + count - nout);
    a.hstride = hstride(d);
    a.tiles = (int)tiles;
    a.L = qk::ff_agc_L(a.W);
    const int per16 = 4 / nc;   // samples per 16 bytes
    a.vec = ((uintptr_t)d_out & 15) == 0 && (d->nchan == 1 || out_stride % per16 == 0);   // (one row: its stride places nothing)
    const int gx = (int)tiles + (a.fill_next > 0 ? 1 : 0);
    const int lds = tiles > 0 ? qk::ff_agc_lds(a.W) : 0;
    if (gx > 0) {
        const dim3 grid((unsigned)gx, (unsigned)d->nchan);
        if (nc == 2) hipLaunchKernelGGL((qk::ff_agc_kernel<qk::kFfAgcComplex>), grid, dim3(qk::kDemodNT), lds, s, a);
        else hipLaunchKernelGGL((qk::ff_agc_kernel<qk::kFfAgcReal>), grid, dim3(qk::kDemodNT), lds, s, a);
        HIPCHK(hipGetLastError());
        d->last = Launch{"ff_agc_kernel", gx, qk::kDemodNT, lds};
        d->cur ^= 1;
    }
    d->fill = a.fill_next;
    return nout;
}

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_ffagc_create(void** h, int device, int kind, int nchan, int max_block, int window) {
    return ffagc_new(h, device, kind, nchan, max_block, window);
}
int qdsp_hip_ffagc_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<FfAgc>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_ffagc_process(void* h, const float* in, int count, float* out) {
    return qdsp_hip_ffagc_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int64_t qdsp_hip_ffagc_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    FfAgc* d = as<FfAgc>(h);
    if (!d) return QDSP_HIP_EINVAL;
    return ffagc_launch(d, d_in, count, count, d_out, out_count(d, count), static_cast<hipStream_t>(hip_stream));
}
int64_t qdsp_hip_ffagc_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                         void* hip_stream) {
    FfAgc* d = as<FfAgc>(h);
    return d ? ffagc_launch(d, d_in, count, in_stride, d_out, out_stride, static_cast<hipStream_t>(hip_stream)) : QDSP_HIP_EINVAL;
}
int64_t qdsp_hip_ffagc_out_size(void* h, int64_t count) {
    FfAgc* d = as<FfAgc>(h);
    return (d && count >= 0) ? out_count(d, count) : QDSP_HIP_EINVAL;
}
int qdsp_hip_ffagc_window(void* h) {
    FfAgc* d = as<FfAgc>(h);
    return d ? d->window : QDSP_HIP_EINVAL;
}
int qdsp_hip_ffagc_fill(void* h) {
    FfAgc* d = as<FfAgc>(h);
    return d ? d->fill : QDSP_HIP_EINVAL;
}
int qdsp_hip_ffagc_get_history(void* h, int chan, float* hist) {
    FfAgc* d = as<FfAgc>(h);
    if (!d || chan < 0 || chan >= d->nchan || !hist) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t es = (size_t)comps(d) * sizeof(float);
    if (d->fill > 0)
        HIPCHK(hipMemcpy(hist, d->d_hist[d->cur] + (size_t)chan * hstride(d) * comps(d), (size_t)d->fill * es, hipMemcpyDeviceToHost));
    return 0;
}
int qdsp_hip_ffagc_set_history(void* h, int chan, const float* hist, int fill) {
    FfAgc* d = as<FfAgc>(h);
    if (!d || chan < -1 || chan >= d->nchan || fill < 0 || fill > d->window - 1 || (fill > 0 && !hist)) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t es = (size_t)comps(d) * sizeof(float);
    const int c0 = chan < 0 ? 0 : chan, c1 = chan < 0 ? d->nchan : chan + 1;
    for (int c = c0; c < c1 && fill > 0; c++)
        HIPCHK(hipMemcpy(d->d_hist[d->cur] + (size_t)c * hstride(d) * comps(d), hist, (size_t)fill * es, hipMemcpyHostToDevice));
    d->fill = fill;
    return 0;
}
int qdsp_hip_ffagc_reset(void* h) {
    FfAgc* d = as<FfAgc>(h);
    if (!d) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++) HIPCHK(hipMemset(d->d_hist[i], 0, hist_bytes(d)));
    d->fill = 0;
    return 0;
}
void qdsp_hip_ffagc_destroy(void* h) { ffagc_free(as<FfAgc>(h)); }

}  // extern "C"
