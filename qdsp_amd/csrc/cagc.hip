// cagc.hip -- ComplexAGC as a batched FP64 clamped prefix scan, its serial path for rows out of the scan's domain (design notes:
// cagc.hip.h) and its C entry points.
#include "cagc.hip.h"
#include "scan.hip.h"

#include <cfloat>

namespace qk {

namespace {
// g -> min(a g + b, c)
struct Clamp {
    double a, b, c;
    static __device__ __forceinline__ Clamp identity() { return Clamp{1.0, 0.0, DBL_MAX}; }
};

// `later` after `earlier`
__device__ __forceinline__ Clamp compose(const Clamp& later, const Clamp& earlier) {
    Clamp r;
    r.a = later.a * earlier.a;
    r.b = fma(later.a, earlier.b, later.b);
    r.c = fmin(fma(later.a, earlier.c, later.b), later.c);
    return r;
}

__device__ __forceinline__ double apply(const Clamp& m, double g) { return fmin(fma(m.a, g, m.b), m.c); }

__device__ __forceinline__ Clamp shfl_up(const Clamp& v, int d) {
    return Clamp{__shfl_up(v.a, d), __shfl_up(v.b, d), __shfl_up(v.c, d)};
}

// a row's parameters, widened, and whether they and the carried gain are in the scan's domain
struct RowPar {
    double r, b, c, g0;
    bool ok;
};

__device__ __forceinline__ RowPar row_par(const CagcArgs& a, int ch) {
    const float sp = a.par[3 * ch], mg = a.par[3 * ch + 1], rt = a.par[3 * ch + 2];
    RowPar p;
    p.r = (double)rt;
    p.b = (double)sp * (double)rt;          // exact
    p.c = fmin((double)mg, DBL_MAX);
    p.g0 = a.state[ch];
    p.ok = isfinite(p.g0) && p.g0 >= 0.0 && p.b >= 0.0 && isfinite(p.b) && p.c >= 0.0 && p.r >= 0.0;
    return p;
}

// a_j of the lane's n samples; *bad is set if one of them is out of the domain (NaN and Inf samples fail a >= 0 too)
__device__ __forceinline__ void lane_coeffs(const float (&x)[kDemodSpl * 2], int n, double r, double (&aj)[kDemodSpl], bool* bad) {
#pragma unroll
    for (int j = 0; j < kDemodSpl; j++) {
        const double re = (double)x[2 * j], im = (double)x[2 * j + 1];
        const double a = fma(-r, sqrt(fma(re, re, im * im)), 1.0);
        aj[j] = a;
        if (j < n && !(a >= 0.0)) *bad = true;
    }
}

// the lane's n samples as one map
__device__ __forceinline__ Clamp fold_lane(const double (&aj)[kDemodSpl], int n, double b, double c) {
    Clamp p = Clamp::identity();
#pragma unroll
    for (int j = 0; j < kDemodSpl; j++) {
        if (j < n) {
            p.c = fmin(fma(aj[j], p.c, b), c);
            p.b = fma(aj[j], p.b, b);
            p.a *= aj[j];
        }
    }
    return p;
}

// whether pass 1 found the row out of the domain: the flags of all G chunks (every lane of the workgroup gets the answer)
__device__ __forceinline__ bool row_failed(const CagcArgs& a, int ch, bool bad) {
    const double* part = a.part + (long long)ch * a.G * kCagcPart;
    for (int k = threadIdx.x; k < a.G; k += blockDim.x) bad |= part[k * kCagcPart + 3] != 0.0;
    return __syncthreads_or(bad) != 0;
}

// chunk g of row ch (known to be in the domain): the carried gain moved over the chunks before it, then tile by tile
__device__ __forceinline__ void scan_chunk(const CagcArgs& a, const RowPar& p, Clamp* wt) {
    const int ch = blockIdx.y, g = blockIdx.x;
    double carry = p.g0;
    const double* part = a.part + (long long)ch * a.G * kCagcPart;
    for (int k = 0; k < g; k++) carry = fmin(fma(part[k * kCagcPart], carry, part[k * kCagcPart + 1]), part[k * kCagcPart + 2]);
    const float* in = a.in + (long long)ch * a.in_stride * 2;
    float* out = a.out + (long long)ch * a.out_stride * 2;
    const long long tiles = scan_tiles_of(a.count);
    const long long t0 = (long long)g * a.T;
    const long long t1 = t0 + a.T < tiles ? t0 + a.T : tiles;
    for (long long t = t0; t < t1; t++) {
        const long long i0 = (t * kDemodNT + threadIdx.x) * kDemodSpl;
        float x[kDemodSpl * 2];
        const int n = load_lane<2>(in, i0, a.count, a.vec, x);
        double aj[kDemodSpl];
        bool bad = false;
        lane_coeffs(x, n, p.r, aj, &bad);
        Clamp ex;
        const Clamp tot = tile_scan(fold_lane(aj, n, p.b, p.c), wt, &ex);
        double gain = apply(ex, carry);
        float o[kDemodSpl * 2];
#pragma unroll
        for (int j = 0; j < kDemodSpl; j++) {
            o[2 * j] = (float)((double)x[2 * j] * gain);
            o[2 * j + 1] = (float)((double)x[2 * j + 1] * gain);
            if (j < n) gain = fmin(fma(aj[j], gain, p.b), p.c);
        }
        store_lane<2>(out, i0, n, a.vec, o);
        if (n > 0 && i0 + n == a.count) a.state_next[ch] = gain;
        carry = apply(tot, carry);
    }
}
}  // namespace

// grid (1, nchan): a sweep that only checks the domain (the row may be its own output: nothing is stored before the whole row is
// known to be in the domain), then the scan
__global__ __launch_bounds__(kDemodNT) void cagc_row_kernel(const CagcArgs a) {
    __shared__ Clamp wt[kDemodNT / 64];
    const int ch = blockIdx.y;
    const RowPar p = row_par(a, ch);
    const float* in = a.in + (long long)ch * a.in_stride * 2;
    bool bad = !p.ok;
    const long long tiles = scan_tiles_of(a.count);
    for (long long t = 0; t < tiles; t++) {
        const long long i0 = (t * kDemodNT + threadIdx.x) * kDemodSpl;
        float x[kDemodSpl * 2];
        const int n = load_lane<2>(in, i0, a.count, a.vec, x);
        double aj[kDemodSpl];
        lane_coeffs(x, n, p.r, aj, &bad);
    }
    const bool failed = __syncthreads_or(bad) != 0;
    if (threadIdx.x == 0) a.part[(long long)ch * kCagcPart + 3] = failed ? 1.0 : 0.0;   // (G == 1) for cagc_serial_kernel
    if (failed) return;
    scan_chunk(a, p, wt);
}

// pass 1; grid (G, nchan).  The last chunk's triple is not used (nothing follows it) but its samples are checked like the others.
__global__ __launch_bounds__(kDemodNT) void cagc_partial_kernel(const CagcArgs a) {
    __shared__ Clamp wt[kDemodNT / 64];
    const int ch = blockIdx.y, g = blockIdx.x;
    const RowPar p = row_par(a, ch);
    const float* in = a.in + (long long)ch * a.in_stride * 2;
    Clamp acc = Clamp::identity();
    bool bad = !p.ok;
    const long long tiles = scan_tiles_of(a.count);
    const long long t0 = (long long)g * a.T;
    const long long t1 = t0 + a.T < tiles ? t0 + a.T : tiles;
    for (long long t = t0; t < t1; t++) {
        const long long i0 = (t * kDemodNT + threadIdx.x) * kDemodSpl;
        float x[kDemodSpl * 2];
        const int n = load_lane<2>(in, i0, a.count, a.vec, x);
        double aj[kDemodSpl];
        lane_coeffs(x, n, p.r, aj, &bad);
        Clamp ex;
        acc = compose(tile_scan(fold_lane(aj, n, p.b, p.c), wt, &ex), acc);
    }
    const bool failed = __syncthreads_or(bad) != 0;
    if (threadIdx.x == 0) {
        double* q = a.part + ((long long)ch * a.G + g) * kCagcPart;
        q[0] = acc.a;
        q[1] = acc.b;
        q[2] = acc.c;
        q[3] = failed ? 1.0 : 0.0;
    }
}

// pass 2; grid (G, nchan)
__global__ __launch_bounds__(kDemodNT) void cagc_scan_kernel(const CagcArgs a) {
    __shared__ Clamp wt[kDemodNT / 64];
    const RowPar p = row_par(a, blockIdx.y);
    if (row_failed(a, blockIdx.y, !p.ok)) return;
    scan_chunk(a, p, wt);
}

// The reference's loop for the rows the scan left alone; grid nchan, one wave each.  64 samples are loaded at once, every lane
// runs the same recurrence over them (a sample reaches all lanes by a cross-lane read) and keeps its own output, 64 are stored.
__global__ __launch_bounds__(64) void cagc_serial_kernel(const CagcArgs a) {
#pragma clang fp contract(off)
    const int ch = blockIdx.x, lane = threadIdx.x;
    const RowPar p = row_par(a, ch);
    if (!row_failed(a, ch, !p.ok)) return;
    const float sp = a.par[3 * ch], mg = a.par[3 * ch + 1], rt = a.par[3 * ch + 2];
    const float2* in = reinterpret_cast<const float2*>(a.in + (long long)ch * a.in_stride * 2);
    float2* out = reinterpret_cast<float2*>(a.out + (long long)ch * a.out_stride * 2);
    float g = (float)p.g0;
    for (long long i0 = 0; i0 < a.count; i0 += 64) {
        const long long i = i0 + lane;
        const float2 v = i < a.count ? in[i] : make_float2(0.0f, 0.0f);
        const int n = a.count - i0 < 64 ? (int)(a.count - i0) : 64;
        float2 o = v;
        for (int j = 0; j < n; j++) {
            const float re = __shfl(v.x, j), im = __shfl(v.y, j);
            const float yr = re * g, yi = im * g;
            if (lane == j) o = make_float2(yr, yi);
            const float amp = sqrtf(yr * yr + yi * yi);
            g = g + (sp - amp) * rt;
            g = g > mg ? mg : g;
        }
        if (i < a.count) out[i] = o;
    }
    if (lane == 0) a.state_next[ch] = (double)g;
}

}  // namespace qk

namespace qh {

namespace {

void cagc_free(Cagc* d) {
    op_free(d, [d] { hip_free_all({d->d_state[0], d->d_state[1], d->d_par, d->d_part}); });
}

int cagc_fill_state(Cagc* d, int chan, double gain, bool both) {
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    const std::vector<double> v((size_t)chan_count(d, chan), gain);
    for (int s = 0; s < 2; s++)
        if (both || s == d->cur)
            HIPCHK(hipMemcpy(d->d_state[s] + chan_first(chan), v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

// d_in / d_out: nchan rows of `count` complex samples, in_stride / out_stride samples apart
int cagc_launch(Cagc* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (count < 0 || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < count) return QDSP_HIP_EINVAL;
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return QDSP_HIP_EINVAL;
    if (d_in == d_out && in_stride != out_stride) return QDSP_HIP_EINVAL;   // in place: the same rows exactly
    if (count == 0) return 0;
    HIPCHK(hipSetDevice(d->device));
    const long long tiles = qk::scan_tiles_of(count);
    qk::CagcArgs a;
    a.in = static_cast<const float*>(d_in);
    a.out = static_cast<float*>(d_out);
    a.par = d->d_par;
    a.state = d->d_state[d->cur];
    a.state_next = d->d_state[d->cur ^ 1];
    a.part = d->d_part;
    a.count = count;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.vec = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0 && in_stride % 2 == 0 && out_stride % 2 == 0;
    const int lds = (int)((qk::kDemodNT / 64) * 3 * sizeof(double));
    qk::scan_chunks(tiles, qk::kCagcRowTiles, &a.T, &a.G);
    if (a.G == 1) {
        hipLaunchKernelGGL(qk::cagc_row_kernel, dim3(1, (unsigned)d->nchan), dim3(qk::kDemodNT), 0, s, a);
        HIPCHK(hipGetLastError());
        d->last = Launch{"cagc_row_kernel", 1, qk::kDemodNT, lds};
    } else {
        const dim3 grid((unsigned)a.G, (unsigned)d->nchan);
        hipLaunchKernelGGL(qk::cagc_partial_kernel, grid, dim3(qk::kDemodNT), 0, s, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(qk::cagc_scan_kernel, grid, dim3(qk::kDemodNT), 0, s, a);
        HIPCHK(hipGetLastError());
        d->last = Launch{"cagc_scan_kernel", a.G, qk::kDemodNT, lds};
    }
    hipLaunchKernelGGL(qk::cagc_serial_kernel, dim3((unsigned)d->nchan), dim3(64), 0, s, a);
    HIPCHK(hipGetLastError());
    d->cur ^= 1;
    return 0;
}

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_cagc_create(void** h, int device, int nchan, int max_block) {
    Cagc* d = nullptr;
    if (const int rc = op_new<Cagc, cagc_launch>(&d, h, true, device, nchan, max_block)) return rc;
    d->par.resize((size_t)nchan * 3);
    for (int c = 0; c < nchan; c++) {   // the reference's defaults (processing.h:291-294)
        d->par[3 * c] = 1.0f;
        d->par[3 * c + 1] = 10e4f;
        d->par[3 * c + 2] = 10e-4f;
    }
    hipError_t err = stream_op_init(d, device, nchan, max_block, sizeof(float2), sizeof(float2));
    const std::vector<double> ones((size_t)nchan, 1.0);
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc(&d->d_state[i], (size_t)nchan * sizeof(double));
        if (err == hipSuccess) err = hipMemcpy(d->d_state[i], ones.data(), (size_t)nchan * sizeof(double), hipMemcpyHostToDevice);
    }
    if (err == hipSuccess) err = hipMalloc(&d->d_par, d->par.size() * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(d->d_par, d->par.data(), d->par.size() * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc(&d->d_part, (size_t)nchan * qk::kAmMaxParts * qk::kCagcPart * sizeof(double));
    return op_created<cagc_free>(h, d, err);
}
int qdsp_hip_cagc_set(void* h, int chan, float set_point, float max_gain, float rate) {
    Cagc* d = as<Cagc>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    if (std::isnan(set_point) || std::isnan(max_gain) || std::isnan(rate)) return QDSP_HIP_EINVAL;
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++) {
        d->par[3 * c] = set_point;
        d->par[3 * c + 1] = max_gain;
        d->par[3 * c + 2] = rate;
    }
    return sync_upload(d, d->d_par, d->par.data(), d->par.size() * sizeof(float));
}
int qdsp_hip_cagc_get_gain(void* h, int chan, double* gain) {
    Cagc* d = as<Cagc>(h);
    if (!d || !chan_ok(d, chan) || !gain) return QDSP_HIP_EINVAL;
    return sync_download(d, gain, d->d_state[d->cur] + chan, sizeof(double));
}
int qdsp_hip_cagc_set_gain(void* h, int chan, double gain) {
    Cagc* d = as<Cagc>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    return cagc_fill_state(d, chan, gain, false);
}
int qdsp_hip_cagc_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<Cagc>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_cagc_process(void* h, const float* in, int count, float* out) {
    return qdsp_hip_cagc_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_cagc_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<Cagc, cagc_launch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_cagc_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                    void* hip_stream) {
    return op_process_batch_dev<Cagc, cagc_launch>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_cagc_reset(void* h) {
    Cagc* d = as<Cagc>(h);
    return d ? cagc_fill_state(d, -1, 1.0, true) : QDSP_HIP_EINVAL;
}
void qdsp_hip_cagc_destroy(void* h) { cagc_free(as<Cagc>(h)); }

}  // extern "C"
