// deemp.hip -- BFMDeemp as a batched FP64 prefix scan (design notes: deemp.hip.h) and its C entry points.
#include "deemp.hip.h"
#include "scan.hip.h"

namespace qk {

namespace {
// y -> A y + B[c]; both components of a stereo_t share the coefficient, hence one A
template <int NC> struct Aff {
    double A;
    double B[NC];
    static __device__ __forceinline__ Aff identity() {
        Aff r;
        r.A = 1.0;
#pragma unroll
        for (int c = 0; c < NC; c++) r.B[c] = 0.0;
        return r;
    }
};

// `later` after `earlier`
template <int NC> __device__ __forceinline__ Aff<NC> compose(const Aff<NC>& later, const Aff<NC>& earlier) {
    Aff<NC> r;
    r.A = later.A * earlier.A;
#pragma unroll
    for (int c = 0; c < NC; c++) r.B[c] = fma(later.A, earlier.B[c], later.B[c]);
    return r;
}

template <int NC> __device__ __forceinline__ Aff<NC> shfl_up(const Aff<NC>& v, int d) {
    Aff<NC> r;
    r.A = __shfl_up(v.A, d);
#pragma unroll
    for (int c = 0; c < NC; c++) r.B[c] = __shfl_up(v.B[c], d);
    return r;
}

// the lane's n samples as one map
template <int NC> __device__ __forceinline__ Aff<NC> fold_lane(const float (&x)[kDemodSpl * NC], int n, double a, double b) {
    Aff<NC> p = Aff<NC>::identity();
#pragma unroll
    for (int j = 0; j < kDemodSpl; j++) {
        if (j < n) {
#pragma unroll
            for (int c = 0; c < NC; c++) p.B[c] = fma(b, p.B[c], a * (double)x[j * NC + c]);
            p.A *= b;
        }
    }
    return p;
}

// chunk g of row c: the carried state moved over the chunks before it, then tile by tile
template <int NC> __device__ __forceinline__ void scan_chunk(const DeempArgs& a) {
    __shared__ Aff<NC> wt[kDemodNT / 64];
    const int c = blockIdx.y, g = blockIdx.x;
    const float alpha = a.alpha[c];
    const double al = (double)alpha, b = (double)(1.0f - alpha);
    double carry[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) {
        const double s = a.state[c * NC + k];
        carry[k] = isfinite(s) ? s : 0.0;
    }
    const double* part = a.part + (long long)c * a.G * (1 + NC);
    for (int k = 0; k < g; k++) {
#pragma unroll
        for (int m = 0; m < NC; m++) carry[m] = fma(part[k * (1 + NC)], carry[m], part[k * (1 + NC) + 1 + m]);
    }
    const float* in = a.in + (long long)c * a.in_stride * NC;
    float* out = a.out + (long long)c * a.out_stride * NC;
    const long long tiles = scan_tiles_of(a.count);
    const long long t0 = (long long)g * a.T;
    const long long t1 = t0 + a.T < tiles ? t0 + a.T : tiles;
    for (long long t = t0; t < t1; t++) {
        const long long i0 = (t * kDemodNT + threadIdx.x) * kDemodSpl;
        float x[kDemodSpl * NC];
        const int n = load_lane<NC>(in, i0, a.count, a.vec, x);
        Aff<NC> ex;
        const Aff<NC> tot = tile_scan(fold_lane<NC>(x, n, al, b), wt, &ex);
        double y[NC];
#pragma unroll
        for (int m = 0; m < NC; m++) y[m] = fma(ex.A, carry[m], ex.B[m]);
        float o[kDemodSpl * NC];
#pragma unroll
        for (int j = 0; j < kDemodSpl; j++) {
#pragma unroll
            for (int m = 0; m < NC; m++) {
                if (j < n) y[m] = fma(b, y[m], al * (double)x[j * NC + m]);
                o[j * NC + m] = (float)y[m];
            }
        }
        store_lane<NC>(out, i0, n, a.vec, o);
        if (n > 0 && i0 + n == a.count) {
#pragma unroll
            for (int m = 0; m < NC; m++) a.state_next[c * NC + m] = y[m];
        }
#pragma unroll
        for (int m = 0; m < NC; m++) carry[m] = fma(tot.A, carry[m], tot.B[m]);
    }
}
}  // namespace

template <int NC> __global__ __launch_bounds__(kDemodNT) void deemp_row_kernel(const DeempArgs a) { scan_chunk<NC>(a); }
template <int NC> __global__ __launch_bounds__(kDemodNT) void deemp_scan_kernel(const DeempArgs a) { scan_chunk<NC>(a); }

// pass 1; grid (G - 1, nchan): every tile of these chunks is full
template <int NC> __global__ __launch_bounds__(kDemodNT) void deemp_partial_kernel(const DeempArgs a) {
    __shared__ Aff<NC> wt[kDemodNT / 64];
    const int c = blockIdx.y, g = blockIdx.x;
    const float alpha = a.alpha[c];
    const double al = (double)alpha, b = (double)(1.0f - alpha);
    const float* in = a.in + (long long)c * a.in_stride * NC;
    Aff<NC> acc = Aff<NC>::identity();
    const long long t0 = (long long)g * a.T;
    for (long long t = t0; t < t0 + a.T; t++) {
        const long long i0 = (t * kDemodNT + threadIdx.x) * kDemodSpl;
        float x[kDemodSpl * NC];
        const int n = load_lane<NC>(in, i0, a.count, a.vec, x);
        Aff<NC> ex;
        acc = compose(tile_scan(fold_lane<NC>(x, n, al, b), wt, &ex), acc);
    }
    if (threadIdx.x == 0) {
        double* p = a.part + ((long long)c * a.G + g) * (1 + NC);
        p[0] = acc.A;
#pragma unroll
        for (int m = 0; m < NC; m++) p[1 + m] = acc.B[m];
    }
}

}  // namespace qk

namespace qh {

namespace {
int comps(const Deemp* d) { return d->kind == QDSP_HIP_DEEMP_STEREO ? 2 : 1; }

void deemp_free(Deemp* d) {
    op_free(d, [d] { hip_free_all({d->d_state[0], d->d_state[1], d->d_alpha, d->d_part}); });
}

// d_in / d_out: nchan rows of `count` samples, in_stride / out_stride samples apart
int deemp_launch(Deemp* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (count < 0 || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < count) return QDSP_HIP_EINVAL;
    const int nc = comps(d);
    const uintptr_t amask = (uintptr_t)(nc * sizeof(float) - 1);
    if (((uintptr_t)d_in & amask) || ((uintptr_t)d_out & amask)) return QDSP_HIP_EINVAL;
    if (d_in == d_out && in_stride != out_stride) return QDSP_HIP_EINVAL;   // in place: the same rows exactly
    if (count == 0) return 0;
    HIPCHK(hipSetDevice(d->device));
    const size_t es = (size_t)nc * sizeof(float);
    if (d->bypass) {
        if (d_in != d_out)
            HIPCHK(hipMemcpy2DAsync(d_out, (size_t)out_stride * es, d_in, (size_t)in_stride * es, (size_t)count * es, (size_t)d->nchan,
                                    hipMemcpyDeviceToDevice, s));
        d->last = Launch{"bypass", 0, 0, 0};
        return 0;
    }
    const long long tiles = qk::scan_tiles_of(count);
    qk::DeempArgs a;
    a.in = static_cast<const float*>(d_in);
    a.out = static_cast<float*>(d_out);
    a.alpha = d->d_alpha;
    a.state = d->d_state[d->cur];
    a.state_next = d->d_state[d->cur ^ 1];
    a.part = d->d_part;
    a.count = count;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    const int per16 = 4 / nc;   // samples per 16 bytes
    a.vec = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0 && in_stride % per16 == 0 && out_stride % per16 == 0;
    const int lds = (int)((qk::kDemodNT / 64) * (1 + nc) * sizeof(double));
    qk::scan_chunks(tiles, qk::kDeempRowTiles, &a.T, &a.G);
    if (a.G == 1) {
        const dim3 grid(1, (unsigned)d->nchan);
        if (nc == 2) hipLaunchKernelGGL((qk::deemp_row_kernel<2>), grid, dim3(qk::kDemodNT), 0, s, a);
        else hipLaunchKernelGGL((qk::deemp_row_kernel<1>), grid, dim3(qk::kDemodNT), 0, s, a);
        HIPCHK(hipGetLastError());
        d->last = Launch{"deemp_row_kernel", 1, qk::kDemodNT, lds};
    } else {
        const dim3 g1((unsigned)(a.G - 1), (unsigned)d->nchan), g2((unsigned)a.G, (unsigned)d->nchan);
        if (nc == 2) {
            hipLaunchKernelGGL((qk::deemp_partial_kernel<2>), g1, dim3(qk::kDemodNT), 0, s, a);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL((qk::deemp_scan_kernel<2>), g2, dim3(qk::kDemodNT), 0, s, a);
        } else {
            hipLaunchKernelGGL((qk::deemp_partial_kernel<1>), g1, dim3(qk::kDemodNT), 0, s, a);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL((qk::deemp_scan_kernel<1>), g2, dim3(qk::kDemodNT), 0, s, a);
        }
        HIPCHK(hipGetLastError());
        d->last = Launch{"deemp_scan_kernel", a.G, qk::kDemodNT, lds};
    }
    d->cur ^= 1;
    return 0;
}

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_deemp_create(void** h, int device, int kind, int nchan, int max_block) {
    Deemp* d = nullptr;
    const bool args_ok = kind == QDSP_HIP_DEEMP_MONO || kind == QDSP_HIP_DEEMP_STEREO;
    if (const int rc = op_new<Deemp, deemp_launch>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->kind = kind;
    d->alpha.assign(nchan, 1.0f);   // sample_rate 1, tau 0 until set: y = x
    const int nc = comps(d);
    hipError_t err = stream_op_init(d, device, nchan, max_block, nc * sizeof(float), nc * sizeof(float));
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc(&d->d_state[i], (size_t)nchan * nc * sizeof(double));
        if (err == hipSuccess) err = hipMemset(d->d_state[i], 0, (size_t)nchan * nc * sizeof(double));
    }
    if (err == hipSuccess) err = hipMalloc(&d->d_alpha, (size_t)nchan * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(d->d_alpha, d->alpha.data(), (size_t)nchan * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc(&d->d_part, (size_t)nchan * qk::kAmMaxParts * (1 + nc) * sizeof(double));
    return op_created<deemp_free>(h, d, err);
}
int qdsp_hip_deemp_set(void* h, int chan, float sample_rate, float tau) {
    Deemp* d = as<Deemp>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    if (!std::isfinite(sample_rate) || sample_rate <= 0.0f || !std::isfinite(tau) || tau < 0.0f) return QDSP_HIP_EINVAL;
    // BFMDeemp::init / setSampleRate / setTau (filter.h:102-103), in float
    const float dt = 1.0f / sample_rate;
    const float alpha = dt / (tau + dt);
    if (!std::isfinite(alpha) || alpha <= 0.0f) return QDSP_HIP_EINVAL;
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++) d->alpha[c] = alpha;
    return sync_upload(d, d->d_alpha, d->alpha.data(), (size_t)d->nchan * sizeof(float));
}
int qdsp_hip_deemp_set_bypass(void* h, int on) {
    Deemp* d = as<Deemp>(h);
    if (!d) return QDSP_HIP_EINVAL;
    d->bypass = on != 0;
    return 0;
}
int qdsp_hip_deemp_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<Deemp>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_deemp_process(void* h, const float* in, int count, float* out) {
    return qdsp_hip_deemp_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_deemp_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<Deemp, deemp_launch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_deemp_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                     void* hip_stream) {
    return op_process_batch_dev<Deemp, deemp_launch>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_deemp_get_state(void* h, int chan, float* l, float* r) {
    Deemp* d = as<Deemp>(h);
    if (!d || !chan_ok(d, chan) || !l || (comps(d) == 2 && !r)) return QDSP_HIP_EINVAL;
    double v[2] = {0.0, 0.0};
    const int nc = comps(d);
    if (const int rc = sync_download(d, v, d->d_state[d->cur] + (size_t)chan * nc, (size_t)nc * sizeof(double))) return rc;
    *l = (float)v[0];
    if (r) *r = (float)v[nc - 1];
    return 0;
}
int qdsp_hip_deemp_set_state(void* h, int chan, float l, float r) {
    Deemp* d = as<Deemp>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    const int nc = comps(d), n = chan_count(d, chan);
    std::vector<double> v((size_t)n * nc);
    for (int i = 0; i < n; i++) {
        v[(size_t)i * nc] = (double)l;
        if (nc == 2) v[(size_t)i * nc + 1] = (double)r;
    }
    return sync_upload(d, d->d_state[d->cur] + (size_t)chan_first(chan) * nc, v.data(), v.size() * sizeof(double));
}
int qdsp_hip_deemp_get_alpha(void* h, int chan, float* alpha) {
    Deemp* d = as<Deemp>(h);
    if (!d || !chan_ok(d, chan) || !alpha) return QDSP_HIP_EINVAL;
    *alpha = d->alpha[chan];
    return 0;
}
int qdsp_hip_deemp_reset(void* h) {
    Deemp* d = as<Deemp>(h);
    if (!d) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++) HIPCHK(hipMemset(d->d_state[i], 0, (size_t)d->nchan * comps(d) * sizeof(double)));
    return 0;
}
void qdsp_hip_deemp_destroy(void* h) { deemp_free(as<Deemp>(h)); }

}  // extern "C"
