// costas.hip -- CostasLoop<2 / 4 / 8> batched with one row per lane (design notes: costas.hip.h) and its C entry points.
#include "costas.hip.h"

#include <cmath>
#include <limits>

namespace qk {

namespace {
constexpr double kCostasWrap = (double)(2.0f * 3.1415926535f);   // the reference's 2.0f * FL_M_PI, a float
constexpr double kCostasK = 0.41421353816986083984375;           // (float)(sqrtf(2.0) - 1), exactly

struct Vco {
    double re, im;   // cos(-phase), sin(-phase)
};

// |p| <= kCostasWrap.  p = k pi / 2 + r, |k| <= 4, |r| <= pi / 4 (+ 3e-16: pi / 2 is taken as one double); Taylor to r^11 and
// r^12 by Estrin's scheme, five dependent operations behind r; truncation < 7e-12.
__device__ __forceinline__ Vco vco_of(double p) {
    const double k = __builtin_rint(p * 0.63661977236758134);
    const double r = fma(-k, 1.5707963267948966, p);
    const double z = r * r, z2 = z * z, z4 = z2 * z2, rz = r * z;
    const double sp = fma(z4, -2.5052108385441719e-08, fma(z2, fma(z, 2.7557319223985891e-06, -1.9841269841269841e-04),
                                                           fma(z, 8.3333333333333333e-03, -1.6666666666666667e-01)));
    const double cp = fma(z4, fma(z, 2.0876756987868099e-09, -2.7557319223985891e-07),
                          fma(z2, fma(z, 2.4801587301587302e-05, -1.3888888888888889e-03), fma(z, 4.1666666666666667e-02, -0.5)));
    const double sn = fma(rz, sp, r), cs = fma(z, cp, 1.0);
    const int q = (int)k;
    const double s = (q & 1) ? cs : sn, c = (q & 1) ? sn : cs;
    return Vco{((q + 1) & 2) ? -c : c, (q & 2) ? s : -s};
}

template <int ORDER> __device__ __forceinline__ double costas_error(double re, double im) {
    if constexpr (ORDER == 2) {
        return re * im;
    } else {
        const double a = re > 0.0 ? im : -im;   // DSP_STEP(re) * im
        const double b = im > 0.0 ? re : -re;   // DSP_STEP(im) * re
        if constexpr (ORDER == 4) return a - b;
        return fabs(re) >= fabs(im) ? a - b * kCostasK : a * kCostasK - b;
    }
}

// The three staging steps of a round, for a wave of R <= 16 rows that takes S = 1 << SH segments of 64 samples from each (R S <= 64):
// instruction k serves segment k % S of row k / S.  SH is a template parameter so that the LDS offsets are immediates.
// (The row stride passes through an empty asm statement: the row offsets are then formed where they are used, round by round;
// hoisted out of the round loop, as loop invariants, they would take 128 scalar registers for each side and spill.)
__device__ __forceinline__ long long per_round(long long v) {
    asm volatile("" : "+s"(v));
    return v;
}
__device__ __forceinline__ int per_round(int v) {   // (likewise the 64 lane masks of `row < R`)
    asm volatile("" : "+s"(v));
    return v;
}

// round c into registers; samples past the row's end read as 0
template <int SH> __device__ __forceinline__ void costas_load(const CostasArgs& a, int row0, int R, long long c, float2 (&pre)[kCostasSlots]) {
    constexpr int S = 1 << SH;
    R = per_round(R);
    const long long stride = per_round(a.in_stride);
    const long long i0 = c * (64 * S) + threadIdx.x;
    const float2* p = a.in + (long long)row0 * stride + i0;
#pragma unroll
    for (int k = 0; k < kCostasSlots; k++) {
        const int row = k >> SH, seg = k & (S - 1);
        if (row < R) pre[k] = i0 + seg * 64 < a.count ? p[row * stride + seg * 64] : make_float2(0.0f, 0.0f);
    }
}

// registers -> image
template <int SH> __device__ __forceinline__ void costas_stage(float2* img, int R, const float2 (&pre)[kCostasSlots]) {
    constexpr int S = 1 << SH, pitch = 64 * S + 1;
    R = per_round(R);
#pragma unroll
    for (int k = 0; k < kCostasSlots; k++)
        if ((k >> SH) < R) img[(k >> SH) * pitch + (k & (S - 1)) * 64 + threadIdx.x] = pre[k];
}

// image -> the first n samples of round c of every row.  The LDS reads of 16 instructions are issued together and waited for once:
// read and stored one by one, each store would wait out its own read's latency.
template <int SH> __device__ __forceinline__ void costas_store(const CostasArgs& a, const float2* img, int row0, int R, long long c, int n) {
    constexpr int S = 1 << SH, pitch = 64 * S + 1;
    const long long stride = per_round(a.out_stride);
    R = per_round(R);
    float2* q = a.out + (long long)row0 * stride + c * (64 * S) + threadIdx.x;
#pragma unroll
    for (int k0 = 0; k0 < kCostasSlots; k0 += 16) {
        if ((k0 >> SH) < R) {
            float2 t[16];
#pragma unroll
            for (int j = 0; j < 16; j++) t[j] = img[((k0 + j) >> SH) * pitch + ((k0 + j) & (S - 1)) * 64 + threadIdx.x];   // (inside the image for any row)
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int row = (k0 + j) >> SH, seg = (k0 + j) & (S - 1);
                if (row < R && seg * 64 + (int)threadIdx.x < n) q[row * stride + seg * 64] = t[j];
            }
        }
    }
}

template <int N> struct Shift {
    static constexpr int value = N;
};

// f(Shift<sh>{})
template <class F> __device__ __forceinline__ void by_shift(int sh, F f) {
    switch (sh) {
        case 2: f(Shift<2>{}); break;
        case 3: f(Shift<3>{}); break;
        case 4: f(Shift<4>{}); break;
        case 5: f(Shift<5>{}); break;
        default: f(Shift<6>{}); break;
    }
}
}  // namespace

template <int ORDER> __global__ __launch_bounds__(kCostasLanes) void costas_kernel(const CostasArgs a) {
    __shared__ float2 img[kCostasImg];
    const int lane = threadIdx.x;
    const int row0 = blockIdx.x * kCostasRows;
    const int R = a.nchan - row0 < kCostasRows ? a.nchan - row0 : kCostasRows;
    int sh = 2;
    while ((R << (sh + 1)) <= kCostasSlots) sh++;
    const int L = 64 << sh, pitch = L + 1;      // R * pitch <= kCostasImg
    const long long rounds = (a.count + L - 1) / L;

    double freq = 0.0, phase = 0.0, alpha = 0.0, beta = 0.0;
    if (lane < R) {
        const int ch = row0 + lane;
        alpha = (double)a.par[2 * ch];
        beta = (double)a.par[2 * ch + 1];
        freq = a.state[2 * ch];
        phase = a.state[2 * ch + 1];
        if (!isfinite(freq)) freq = 0.0;
        if (!isfinite(phase)) phase = 0.0;
    }
    Vco v = vco_of(phase);
    bool bad = false;
    const float qnan = __builtin_nanf("");

    float2 pre[kCostasSlots];
    by_shift(sh, [&](auto s) { costas_load<decltype(s)::value>(a, row0, R, 0, pre); });
    for (long long c = 0; c < rounds; c++) {
        by_shift(sh, [&](auto s) {
            costas_stage<decltype(s)::value>(img, R, pre);
            if (c + 1 < rounds) costas_load<decltype(s)::value>(a, row0, R, c + 1, pre);   // in flight during the walk
        });
        __syncthreads();
        const long long left = a.count - c * L;
        const int n = left < L ? (int)left : L;
        if (lane < R) {
            float2* p = img + lane * pitch;
            float2 xn = p[0];
            for (int s = 0; s < n; s++) {
                const float2 x = xn;
                xn = p[s + 1];                             // (slot L of the row is its padding)
                const double xr = (double)x.x, xi = (double)x.y;
                const double ore = fma(-v.im, xi, v.re * xr);
                const double oim = fma(v.re, xi, v.im * xr);
                p[s] = bad ? make_float2(qnan, qnan) : make_float2((float)ore, (float)oim);
                double e = costas_error<ORDER>(ore, oim);
                bad |= e != e;
                e = fmin(fmax(e, -1.0), 1.0);
                freq = fmin(fmax(fma(beta, e, freq), -1.0), 1.0);
                phase += fma(alpha, e, freq);
                phase = phase > kCostasWrap ? phase - kCostasWrap : (phase < -kCostasWrap ? phase + kCostasWrap : phase);
                v = vco_of(phase);
            }
        }
        __syncthreads();
        by_shift(sh, [&](auto s) { costas_store<decltype(s)::value>(a, img, row0, R, c, n); });
        __syncthreads();
    }
    if (lane < R) {
        const double dnan = __builtin_nan("");
        a.state_next[2 * (row0 + lane)] = bad ? dnan : freq;
        a.state_next[2 * (row0 + lane) + 1] = bad ? dnan : phase;
    }
}

}  // namespace qk

namespace qh {

namespace {

// pll.h:20-23: the damping factor and the coefficients are floats, the denominator is summed in double and rounded to float
bool costas_gains(float bw, float* alpha, float* beta) {
#pragma clang fp contract(off)
    if (!(bw >= 0.0f) || !std::isfinite(bw)) return false;
    const float damp = sqrtf(2.0f) / 2.0f;
    const float den = (1.0 + 2.0 * damp * bw + bw * bw);
    *alpha = (4 * damp * bw) / den;
    *beta = (4 * bw * bw) / den;
    return std::isfinite(*alpha) && std::isfinite(*beta);   // (bw * bw overflows float from 1.9e19 on)
}

void costas_free(Costas* d) {
    op_free(d, [d] { hip_free_all({d->d_state[0], d->d_state[1], d->d_par}); });
}

int costas_fill_state(Costas* d, int chan, double freq, double phase, bool both) {
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    const int c0 = chan_first(chan), n = chan_count(d, chan);
    std::vector<double> v((size_t)n * 2);
    for (int c = 0; c < n; c++) {
        v[2 * c] = freq;
        v[2 * c + 1] = phase;
    }
    for (int s = 0; s < 2; s++)
        if (both || s == d->cur) HIPCHK(hipMemcpy(d->d_state[s] + 2 * c0, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

// d_in / d_out: nchan rows of `count` complex samples, in_stride / out_stride samples apart
int costas_launch(Costas* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (count < 0 || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < count) return QDSP_HIP_EINVAL;
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return QDSP_HIP_EINVAL;
    if (d_in == d_out && in_stride != out_stride) return QDSP_HIP_EINVAL;   // in place: the same rows exactly
    if (count == 0) return 0;
    HIPCHK(hipSetDevice(d->device));
    qk::CostasArgs a;
    a.in = static_cast<const float2*>(d_in);
    a.out = static_cast<float2*>(d_out);
    a.par = d->d_par;
    a.state = d->d_state[d->cur];
    a.state_next = d->d_state[d->cur ^ 1];
    a.count = count;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.nchan = d->nchan;
    const dim3 grid((unsigned)((d->nchan + qk::kCostasRows - 1) / qk::kCostasRows)), block(qk::kCostasLanes);
    if (d->order == 2) hipLaunchKernelGGL(qk::costas_kernel<2>, grid, block, 0, s, a);
    else if (d->order == 4) hipLaunchKernelGGL(qk::costas_kernel<4>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(qk::costas_kernel<8>, grid, block, 0, s, a);
    HIPCHK(hipGetLastError());
    d->last = Launch{"costas_kernel", (int)grid.x, qk::kCostasLanes, (int)(qk::kCostasImg * sizeof(float2))};
    d->cur ^= 1;
    return 0;
}

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_costas_create(void** h, int device, int order, int nchan, int max_block) {
    Costas* d = nullptr;
    if (const int rc = op_new<Costas, costas_launch>(&d, h, order == 2 || order == 4 || order == 8, device, nchan, max_block)) return rc;
    d->order = order;
    d->par.resize((size_t)nchan * 2);
    for (int c = 0; c < nchan; c++) (void)costas_gains(1.0f, &d->par[2 * c], &d->par[2 * c + 1]);   // _loopBandwidth = 1.0f (pll.h:107)
    hipError_t err = stream_op_init(d, device, nchan, max_block, sizeof(float2), sizeof(float2));
    const size_t st_b = (size_t)nchan * 2 * sizeof(double);
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc(&d->d_state[i], st_b);
        if (err == hipSuccess) err = hipMemset(d->d_state[i], 0, st_b);
    }
    if (err == hipSuccess) err = hipMalloc(&d->d_par, d->par.size() * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(d->d_par, d->par.data(), d->par.size() * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return op_created<costas_free>(h, d, err);
}
int qdsp_hip_costas_set_bandwidth(void* h, int chan, float bw) {
    Costas* d = as<Costas>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    float alpha = 0.0f, beta = 0.0f;
    if (!costas_gains(bw, &alpha, &beta)) return QDSP_HIP_EINVAL;
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++) {
        d->par[2 * c] = alpha;
        d->par[2 * c + 1] = beta;
    }
    return sync_upload(d, d->d_par, d->par.data(), d->par.size() * sizeof(float));
}
int qdsp_hip_costas_get_gains(void* h, int chan, float* alpha, float* beta) {
    Costas* d = as<Costas>(h);
    if (!d || !chan_ok(d, chan) || !alpha || !beta) return QDSP_HIP_EINVAL;
    *alpha = d->par[2 * chan];
    *beta = d->par[2 * chan + 1];
    return 0;
}
int qdsp_hip_costas_get_state(void* h, int chan, double* freq, double* phase) {
    Costas* d = as<Costas>(h);
    if (!d || !chan_ok(d, chan) || !freq || !phase) return QDSP_HIP_EINVAL;
    double v[2];
    if (const int rc = sync_download(d, v, d->d_state[d->cur] + 2 * chan, sizeof(v))) return rc;
    *freq = v[0];
    *phase = v[1];
    return 0;
}
int qdsp_hip_costas_set_state(void* h, int chan, double freq, double phase) {
    Costas* d = as<Costas>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    if (std::isfinite(phase) && std::fabs(phase) > (double)(2.0f * 3.1415926535f)) return QDSP_HIP_EINVAL;   // the loop keeps it inside
    return costas_fill_state(d, chan, freq, phase, false);
}
int qdsp_hip_costas_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<Costas>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_costas_process(void* h, const float* in, int count, float* out) {
    return qdsp_hip_costas_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_costas_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<Costas, costas_launch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_costas_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                      void* hip_stream) {
    return op_process_batch_dev<Costas, costas_launch>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_costas_reset(void* h) {
    Costas* d = as<Costas>(h);
    return d ? costas_fill_state(d, -1, 0.0, 0.0, true) : QDSP_HIP_EINVAL;
}
void qdsp_hip_costas_destroy(void* h) { costas_free(as<Costas>(h)); }

}  // extern "C"
