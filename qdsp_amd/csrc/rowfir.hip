// rowfir.hip -- RowFir and DelayImag (design notes: rowfir.hip.h) and their C entry points.
// Compiled with the demodulators' flags: no fast-math; the filter is an explicit chain of fmaf in tap order.
#include "rowfir.hip.h"

#include <string.h>

namespace qk {

// 1: the re and im of a complex sample as one two-wide fma (v_pk_fma_f32); 0: two v_fmac_f32.  The same bits either way; measured
// in EXPERIMENTS.md ("PSKDemod / MSKDemod")
#ifndef QDSP_ROWFIR_PK
#define QDSP_ROWFIR_PK 1
#endif
namespace {
typedef float v2f __attribute__((ext_vector_type(2)));
// acc = fma(h, x, acc) on the NC components of one sample, each fused and rounded on its own
template <int NC> __device__ __forceinline__ void fma_sample(float h, const float* x, float* acc) {
    if constexpr (NC == 2 && QDSP_ROWFIR_PK) {
        const v2f a = __builtin_elementwise_fma((v2f){h, h}, (v2f){x[0], x[1]}, (v2f){acc[0], acc[1]});
        acc[0] = a.x;
        acc[1] = a.y;
    } else {
#pragma unroll
        for (int e = 0; e < NC; e++) acc[e] = __builtin_fmaf(h, x[e], acc[e]);
    }
}
}  // namespace

// grid (tiles, nchan); LDS sample j of a workgroup = the sample at call position tile start - (T - 1) + j.
template <int NC>
__global__ __launch_bounds__(kDemodNT) void row_fir_kernel(const RowFirArgs a) {
    __shared__ __attribute__((aligned(16))) float s[kRowFirLds * NC];
    const int c = blockIdx.y, t = threadIdx.x;
    const int T = a.T, H = T - 1;
    const long long b = (long long)blockIdx.x * kRowFirTile;
    const float* __restrict__ x = a.in + (long long)c * a.in_stride * NC;
    const float* __restrict__ hist = a.hist + (long long)c * H * NC;
    const int nstage = kRowFirTile + H;
    for (int j = t; j < nstage; j += kDemodNT) {
        const long long pos = b - H + j;
        const float* p = nullptr;              // (past the end of the call: zeros under outputs that are not stored)
        if (pos < 0) p = hist + (H + pos) * NC;
        else if (pos < a.count) p = x + pos * NC;
        if constexpr (NC == 2) {
            reinterpret_cast<float2*>(s)[j] = p ? *reinterpret_cast<const float2*>(p) : make_float2(0.0f, 0.0f);
        } else {
            s[j] = p ? *p : 0.0f;
        }
    }
    __syncthreads();

    // outputs o0 .. o0 + 7 of the tile: output r at tap k reads sample o0 + k + r; w[] is a ring of 12 samples over o0 + k ..
    const int o0 = t * kDemodSpl;
    const float* __restrict__ taps = a.taps + (long long)c * T;
    const float4* s4 = reinterpret_cast<const float4*>(s);
    float acc[kDemodSpl * NC];
#pragma unroll
    for (int r = 0; r < kDemodSpl * NC; r++) acc[r] = 0.0f;
    float w[kRowFirGroup * NC];
#pragma unroll
    for (int i = 0; i < 2 * NC; i++) {
        const float4 v = s4[((o0 * NC) >> 2) + i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    int k0 = 0;
    // (the read-ahead of the last group reaches sample o0 + k0 + 19 <= T + 2047: inside the array (kRowFirLds) but, for the last
    // lane, one sample past the staged ones -- read uninitialised and never used in an FMA)
    for (; k0 + kRowFirGroup <= T; k0 += kRowFirGroup) {
#pragma unroll
        for (int u = 0; u < 3; u++) {
#pragma unroll
            for (int i = 0; i < NC; i++) {
                const float4 nx = s4[(((o0 + k0 + 4 * u + 8) * NC) >> 2) + i];
                const float f[4] = {nx.x, nx.y, nx.z, nx.w};
#pragma unroll
                for (int q = 0; q < 4; q++) w[((8 + 4 * u + (4 * i + q) / NC) % kRowFirGroup) * NC + (4 * i + q) % NC] = f[q];
            }
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const float h = taps[k0 + 4 * u + kk];
#pragma unroll
                for (int r = 0; r < kDemodSpl; r++) fma_sample<NC>(h, &w[((4 * u + kk + r) % kRowFirGroup) * NC], &acc[r * NC]);
            }
        }
    }
    for (int k = k0; k < T; k++) {             // the last T % 12 taps: the same chain, one LDS sample per FMA
        const float h = taps[k];
#pragma unroll
        for (int r = 0; r < kDemodSpl; r++) fma_sample<NC>(h, &s[(o0 + k + r) * NC], &acc[r * NC]);
    }

    const long long rem = a.count - (b + o0);
    const int n = rem < 0 ? 0 : (rem < kDemodSpl ? (int)rem : kDemodSpl);
    store_lane<NC>(a.out + (long long)c * a.out_stride * NC, b + o0, n, a.vec, acc);

    // the next history = positions count - H .. count - 1: a sample of this call by the tile that holds it, a sample of the old
    // history (count < H) by the last tile, which has staged all of them
    float* __restrict__ hist_next = a.hist_next + (long long)c * H * NC;
    const bool last = (int)blockIdx.x == a.tiles - 1;
    for (int j = t; j < nstage; j += kDemodNT) {
        const long long pos = b - H + j;
        const long long q = pos - (a.count - H);
        const bool own = pos >= 0 ? pos >= b : last;
        if (q >= 0 && pos < a.count && own) {
#pragma unroll
            for (int e = 0; e < NC; e++) hist_next[q * NC + e] = s[j * NC + e];
        }
    }
}

// grid (tiles, nchan); a lane moves kDemodSpl consecutive samples
__global__ __launch_bounds__(kDemodNT) void delay_imag_kernel(const DelayImagArgs a) {
    const int c = blockIdx.y;
    const long long i0 = ((long long)blockIdx.x * kDemodNT + threadIdx.x) * kDemodSpl;
    if (i0 >= a.count) return;
    const uint2* __restrict__ in = a.in + (long long)c * a.in_stride;
    uint2* __restrict__ out = a.out + (long long)c * a.out_stride;
    unsigned prev = i0 > 0 ? in[i0 - 1].y : a.last[c];
    const long long rem = a.count - i0;
    const int n = rem < kDemodSpl ? (int)rem : kDemodSpl;
    for (int j = 0; j < n; j++) {
        const uint2 v = in[i0 + j];
        out[i0 + j] = make_uint2(v.x, prev);
        prev = v.y;
    }
    if (i0 + n == a.count) a.last_next[c] = prev;
}

}  // namespace qk

namespace qh {

namespace {

size_t sample_bytes(const RowFir* d) { return d->kind ? sizeof(float2) : sizeof(float); }
size_t hist_bytes(const RowFir* d, int ntaps) { return (size_t)d->nchan * (size_t)(ntaps > 1 ? ntaps - 1 : 1) * sample_bytes(d); }

void rowfir_free(RowFir* d) {
    op_free(d, [d] { hip_free_all({d->d_taps, d->d_hist[0], d->d_hist[1]}); });
}

// `taps`: [nchan][ntaps].  New tap and history buffers when the count changes, the newest min(old, new) - 1 samples of every row
// kept at the end of its new history (qdsp_hip_fir_cf32_set_taps' rule); the device is idle.  On failure the handle is unchanged.
hipError_t install_taps(RowFir* d, const std::vector<float>& taps, int ntaps) {
    if (ntaps == d->ntaps) {
        const hipError_t err = hipMemcpy(d->d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice);
        if (err == hipSuccess) d->taps = taps;
        return err;
    }
    const int nc = d->kind ? 2 : 1;
    const int oldH = d->ntaps > 0 ? d->ntaps - 1 : 0, newH = ntaps - 1;
    const int keep = oldH < newH ? oldH : newH;
    std::vector<float> nh((size_t)d->nchan * (size_t)(newH > 0 ? newH : 1) * nc, 0.0f);
    hipError_t err = hipSuccess;
    if (keep > 0) {
        std::vector<float> oh((size_t)d->nchan * oldH * nc);
        err = hipMemcpy(oh.data(), d->d_hist[d->cur], oh.size() * sizeof(float), hipMemcpyDeviceToHost);
        if (err != hipSuccess) return err;
        for (int c = 0; c < d->nchan; c++)
            memcpy(&nh[((size_t)c * newH + (newH - keep)) * nc], &oh[((size_t)c * oldH + (oldH - keep)) * nc], (size_t)keep * nc * sizeof(float));
    }
    float* fresh[3] = {nullptr, nullptr, nullptr};   // the taps and both history slots before the old ones go
    err = hipMalloc(&fresh[0], taps.size() * sizeof(float));
    for (int i = 1; i < 3 && err == hipSuccess; i++) err = hipMalloc(&fresh[i], nh.size() * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(fresh[0], taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(fresh[1], nh.data(), nh.size() * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemset(fresh[2], 0, nh.size() * sizeof(float));
    if (err != hipSuccess) {
        for (float* p : fresh)
            if (p) (void)hipFree(p);
        return err;
    }
    for (void* p : {(void*)d->d_taps, (void*)d->d_hist[0], (void*)d->d_hist[1]})
        if (p) (void)hipFree(p);
    d->d_taps = fresh[0];
    d->d_hist[0] = fresh[1];
    d->d_hist[1] = fresh[2];
    d->cur = 0;
    d->ntaps = ntaps;
    d->taps = taps;
    return hipSuccess;
}

// d_in / d_out: nchan rows of `count` samples, in_stride / out_stride samples apart
int rowfir_launch(RowFir* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (count < 0 || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < count) return QDSP_HIP_EINVAL;
    const uintptr_t es = sample_bytes(d);
    if (((uintptr_t)d_in & (es - 1)) || ((uintptr_t)d_out & (es - 1))) return QDSP_HIP_EINVAL;
    if (count == 0) return 0;
    {   // (a tile reads its neighbours' inputs: no overlap at all)
        const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + ((uintptr_t)(d->nchan - 1) * in_stride + count) * es;
        const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + ((uintptr_t)(d->nchan - 1) * out_stride + count) * es;
        if (i0 < o1 && o0 < i1) return QDSP_HIP_EINVAL;
    }
    const long long tiles = (count + qk::kRowFirTile - 1) / qk::kRowFirTile;
    if (tiles > 0x7fffffffLL) return QDSP_HIP_ESIZE;
    HIPCHK(hipSetDevice(d->device));
    qk::RowFirArgs a;
    a.in = static_cast<const float*>(d_in);
    a.out = static_cast<float*>(d_out);
    a.taps = d->d_taps;
    a.hist = d->d_hist[d->cur];
    a.hist_next = d->d_hist[d->cur ^ 1];
    a.count = count;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.T = d->ntaps;
    a.tiles = (int)tiles;
    a.vec = ((uintptr_t)d_out & 15) == 0 && ((out_stride * (int64_t)es) & 15) == 0;
    const dim3 grid((unsigned)tiles, (unsigned)d->nchan);
    if (d->kind) hipLaunchKernelGGL(qk::row_fir_kernel<2>, grid, dim3(qk::kDemodNT), 0, s, a);
    else hipLaunchKernelGGL(qk::row_fir_kernel<1>, grid, dim3(qk::kDemodNT), 0, s, a);
    HIPCHK(hipGetLastError());
    d->cur ^= 1;
    d->last = Launch{"row_fir_kernel", (int)tiles, qk::kDemodNT, (int)(qk::kRowFirLds * es)};
    return 0;
}

void delay_free(DelayImagOp* d) {
    op_free(d, [d] { hip_free_all({d->d_last[0], d->d_last[1]}); });
}

int delay_launch(DelayImagOp* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (count < 0 || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < count) return QDSP_HIP_EINVAL;
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return QDSP_HIP_EINVAL;
    if (count == 0) return 0;
    {   // (a lane reads the sample before its own, which another lane may already have replaced: no overlap at all)
        const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + ((uintptr_t)(d->nchan - 1) * in_stride + count) * 8;
        const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + ((uintptr_t)(d->nchan - 1) * out_stride + count) * 8;
        if (i0 < o1 && o0 < i1) return QDSP_HIP_EINVAL;
    }
    const long long tiles = (count + qk::kRowFirTile - 1) / qk::kRowFirTile;
    if (tiles > 0x7fffffffLL) return QDSP_HIP_ESIZE;
    HIPCHK(hipSetDevice(d->device));
    qk::DelayImagArgs a;
    a.in = static_cast<const uint2*>(d_in);
    a.out = static_cast<uint2*>(d_out);
    a.last = d->d_last[d->cur];
    a.last_next = d->d_last[d->cur ^ 1];
    a.count = count;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    hipLaunchKernelGGL(qk::delay_imag_kernel, dim3((unsigned)tiles, (unsigned)d->nchan), dim3(qk::kDemodNT), 0, s, a);
    HIPCHK(hipGetLastError());
    d->cur ^= 1;
    d->last = Launch{"delay_imag_kernel", (int)tiles, qk::kDemodNT, 0};
    return 0;
}

bool taps_ok(const float* taps, int ntaps) { return taps && ntaps >= 1 && ntaps <= qk::kRowFirMaxTaps; }

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_rowfir_tile(void) { return qk::kRowFirTile; }
int qdsp_hip_rowfir_tap_group(void) { return qk::kRowFirGroup; }

int qdsp_hip_rowfir_create(void** h, int device, int kind, int nchan, const float* taps, int ntaps, int max_block) {
    RowFir* d = nullptr;
    const bool args_ok = (kind == 0 || kind == 1) && taps_ok(taps, ntaps);
    if (const int rc = op_new<RowFir, rowfir_launch>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->kind = kind;
    hipError_t err = stream_op_init(d, device, nchan, max_block, sample_bytes(d), sample_bytes(d));
    d->nchan = nchan;
    if (err == hipSuccess) {
        std::vector<float> all((size_t)nchan * ntaps);
        for (int c = 0; c < nchan; c++) memcpy(&all[(size_t)c * ntaps], taps, (size_t)ntaps * sizeof(float));
        err = install_taps(d, all, ntaps);
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return op_created<rowfir_free>(h, d, err);
}
int qdsp_hip_rowfir_set_taps(void* h, int chan, const float* taps, int ntaps) {
    RowFir* d = as<RowFir>(h);
    if (!d || !taps_ok(taps, ntaps) || (chan != -1 && (!chan_ok(d, chan) || ntaps != d->ntaps))) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<float> all;
    if (chan == -1) {
        all.resize((size_t)d->nchan * ntaps);
        for (int c = 0; c < d->nchan; c++) memcpy(&all[(size_t)c * ntaps], taps, (size_t)ntaps * sizeof(float));
    } else {
        all = d->taps;
        memcpy(&all[(size_t)chan * ntaps], taps, (size_t)ntaps * sizeof(float));
    }
    HIPCHK(install_taps(d, all, ntaps));
    return 0;
}
int qdsp_hip_rowfir_ntaps(void* h) {
    RowFir* d = as<RowFir>(h);
    return d ? d->ntaps : QDSP_HIP_EINVAL;
}
int qdsp_hip_rowfir_get_history(void* h, int chan, float* hist) {
    RowFir* d = as<RowFir>(h);
    if (!d || !chan_ok(d, chan) || !hist) return QDSP_HIP_EINVAL;
    const size_t row = (size_t)(d->ntaps - 1) * sample_bytes(d);
    if (row == 0) return 0;
    return sync_download(d, hist, reinterpret_cast<char*>(d->d_hist[d->cur]) + (size_t)chan * row, row);
}
int qdsp_hip_rowfir_set_history(void* h, int chan, const float* hist) {
    RowFir* d = as<RowFir>(h);
    if (!d || !chan_ok(d, chan) || !hist) return QDSP_HIP_EINVAL;
    const size_t row = (size_t)(d->ntaps - 1) * sample_bytes(d);
    if (row == 0) return 0;
    return sync_upload(d, reinterpret_cast<char*>(d->d_hist[d->cur]) + (size_t)chan * row, hist, row);
}
int qdsp_hip_rowfir_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<RowFir>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_rowfir_process(void* h, const float* in, int count, float* out) {
    return qdsp_hip_rowfir_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_rowfir_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<RowFir, rowfir_launch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_rowfir_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                      void* hip_stream) {
    return op_process_batch_dev<RowFir, rowfir_launch>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_rowfir_reset(void* h) {
    RowFir* d = as<RowFir>(h);
    if (!d) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++) HIPCHK(hipMemset(d->d_hist[i], 0, hist_bytes(d, d->ntaps)));
    return 0;
}
void qdsp_hip_rowfir_destroy(void* h) { rowfir_free(as<RowFir>(h)); }

int qdsp_hip_delay_imag_create(void** h, int device, int nchan, int max_block) {
    DelayImagOp* d = nullptr;
    if (const int rc = op_new<DelayImagOp, delay_launch>(&d, h, true, device, nchan, max_block)) return rc;
    hipError_t err = stream_op_init(d, device, nchan, max_block, sizeof(float2), sizeof(float2));
    d->nchan = nchan;
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc(&d->d_last[i], (size_t)nchan * sizeof(unsigned));
        if (err == hipSuccess) err = hipMemset(d->d_last[i], 0, (size_t)nchan * sizeof(unsigned));
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return op_created<delay_free>(h, d, err);
}
int qdsp_hip_delay_imag_get_state(void* h, int chan, float* last_im) {
    DelayImagOp* d = as<DelayImagOp>(h);
    if (!d || !chan_ok(d, chan) || !last_im) return QDSP_HIP_EINVAL;
    return sync_download(d, last_im, d->d_last[d->cur] + chan, sizeof(float));
}
int qdsp_hip_delay_imag_set_state(void* h, int chan, float last_im) {
    DelayImagOp* d = as<DelayImagOp>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    unsigned bits;
    memcpy(&bits, &last_im, sizeof(bits));
    const std::vector<unsigned> w((size_t)chan_count(d, chan), bits);
    return sync_upload(d, d->d_last[d->cur] + chan_first(chan), w.data(), w.size() * sizeof(unsigned));
}
int qdsp_hip_delay_imag_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<DelayImagOp>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_delay_imag_process(void* h, const float* in_iq, int count, float* out_iq) {
    return qdsp_hip_delay_imag_process_ex(h, in_iq, QDSP_HIP_LINK_HOST, count, out_iq, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_delay_imag_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<DelayImagOp, delay_launch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_delay_imag_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                          void* hip_stream) {
    return op_process_batch_dev<DelayImagOp, delay_launch>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_delay_imag_reset(void* h) {
    DelayImagOp* d = as<DelayImagOp>(h);
    if (!d) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++) HIPCHK(hipMemset(d->d_last[i], 0, (size_t)d->nchan * sizeof(unsigned)));
    return 0;
}
void qdsp_hip_delay_imag_destroy(void* h) { delay_free(as<DelayImagOp>(h)); }

}  // extern "C"
