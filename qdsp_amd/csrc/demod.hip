// demod.hip -- FM / FM stereo / AM / SSB demodulators (design notes: demod.hip.h) and their C entry points.
// Compiled with the library's default flags: no fast-math, correctly rounded f32 division and square root.  The
// reference's arithmetic is restated below under `#pragma clang fp contract(off)`, so products are rounded before they
// are added, as the x86 build of the reference rounds them.
#include "demod.hip.h"

namespace qk {

namespace {
constexpr float kPi = 3.1415926535f;   // FL_M_PI (src/dsp/types.h:4), also the literal of the wrap (demodulator.h:89-90)

// fast_arctan2 (demodulator.h:14-30) without branches: the same predicates pick the same operands
__device__ __forceinline__ float fast_arctan2(float y, float x) {
#pragma clang fp contract(off)
    constexpr float c1 = kPi / 4.0f;            // FAST_ATAN2_COEF1
    constexpr float c2 = 3.0f * kPi / 4.0f;     // FAST_ATAN2_COEF2 (3.0f * FL_M_PI / 4.0f after macro expansion)
    const float ay = fabsf(y);
    const bool right = x >= 0.0f;               // true for -0, false for NaN
    const float num = right ? x - ay : x + ay;
    const float den = right ? x + ay : ay - x;
    const float angle = (right ? c1 : c2) - c1 * (num / den);
    const float s = y < 0.0f ? -angle : angle;
    return (x == 0.0f && y == 0.0f) ? 0.0f : s;
}

// one output of FloatFMDemod::run (demodulator.h:88-91)
__device__ __forceinline__ float fm_out(float cp, float prev, float speed) {
#pragma clang fp contract(off)
    const float d = cp - prev;
    const float w = d > kPi ? d - 2 * kPi : (d <= -kPi ? d + 2 * kPi : d);
    return w / speed;
}

// the up to kDemodSpl samples at in[i0..): 16-byte loads when the row is aligned and the lane's samples are all there
template <class F> __device__ __forceinline__ int for_samples(const float2* __restrict__ in, long long i0, long long count, int vec, F f) {
    const long long rem = count - i0;
    const int n = rem < kDemodSpl ? (int)rem : kDemodSpl;
    if (vec && n == kDemodSpl) {
        const float4* p = reinterpret_cast<const float4*>(in + i0);
        float4 v[kDemodSpl / 2];
#pragma unroll
        for (int j = 0; j < kDemodSpl / 2; j++) v[j] = p[j];
#pragma unroll
        for (int j = 0; j < kDemodSpl / 2; j++) {
            f(2 * j, make_float2(v[j].x, v[j].y));
            f(2 * j + 1, make_float2(v[j].z, v[j].w));
        }
    } else {
#pragma unroll
        for (int j = 0; j < kDemodSpl; j++)
            if (j < n) f(j, in[i0 + j]);
    }
    return n;
}
}  // namespace

// FloatFMDemod / FMDemod::run.  Lane: kDemodSpl consecutive samples of row blockIdx.y; the phase of the sample before
// them is computed once more (or, for the row's first sample, read from the carried state).
template <bool STEREO> __global__ __launch_bounds__(kDemodNT) void fm_demod_kernel(const FmArgs a) {
    const int c = blockIdx.y;
    const long long i0 = ((long long)blockIdx.x * kDemodNT + threadIdx.x) * kDemodSpl;
    if (i0 >= a.count) return;
    const float2* __restrict__ in = a.in + (long long)c * a.in_stride;
    const float speed = a.speed[c];
    float prev;
    if (i0 == 0) {
        prev = a.phase[c];
    } else {
        const float2 v = in[i0 - 1];
        prev = fast_arctan2(v.y, v.x);
    }
    float cp[kDemodSpl];
#pragma unroll
    for (int j = 0; j < kDemodSpl; j++) cp[j] = 0.0f;
    const int n = for_samples(in, i0, a.count, a.vec, [&](int j, float2 v) { cp[j] = fast_arctan2(v.y, v.x); });
    float o[kDemodSpl];
    float last = prev;
#pragma unroll
    for (int j = 0; j < kDemodSpl; j++) {
        o[j] = fm_out(cp[j], prev, speed);
        prev = cp[j];
        if (j < n) last = cp[j];
    }
    if (STEREO) {
        float2* __restrict__ out = static_cast<float2*>(a.out) + (long long)c * a.out_stride + i0;
        if (a.vec && n == kDemodSpl) {
            float4* q = reinterpret_cast<float4*>(out);
#pragma unroll
            for (int j = 0; j < kDemodSpl / 2; j++) q[j] = make_float4(o[2 * j], o[2 * j], o[2 * j + 1], o[2 * j + 1]);
        } else {
#pragma unroll
            for (int j = 0; j < kDemodSpl; j++)
                if (j < n) out[j] = make_float2(o[j], o[j]);
        }
    } else {
        float* __restrict__ out = static_cast<float*>(a.out) + (long long)c * a.out_stride + i0;
        if (a.vec && n == kDemodSpl) {
            float4* q = reinterpret_cast<float4*>(out);
#pragma unroll
            for (int j = 0; j < kDemodSpl / 4; j++) q[j] = make_float4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < kDemodSpl; j++)
                if (j < n) out[j] = o[j];
        }
    }
    if (i0 + n == a.count) a.phase_next[c] = last;
}

// AMDemod, pass 1: FP64 sum of |x| per workgroup; grid (G, nchan), lanes stride over the row
__global__ __launch_bounds__(kDemodNT) void am_partial_kernel(const AmArgs a) {
    __shared__ double red[kDemodNT];
    const int c = blockIdx.y;
    const float2* __restrict__ in = a.in + (long long)c * a.in_stride;
    const long long step = (long long)a.G * kDemodNT * kDemodSpl;
    double s = 0.0;
    for (long long i0 = ((long long)blockIdx.x * kDemodNT + threadIdx.x) * kDemodSpl; i0 < a.count; i0 += step) {
        float m[kDemodSpl];
        const int n = for_samples(in, i0, a.count, a.vec, [&](int j, float2 v) { m[j] = am_mag(v); });
#pragma unroll
        for (int j = 0; j < kDemodSpl; j++)
            if (j < n) s += (double)m[j];
    }
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) a.part[(long long)c * a.G + blockIdx.x] = t;
}

// AMDemod, pass 2: every workgroup reduces its channel's G partials (same order in all of them), then out = |x| - avg
__global__ __launch_bounds__(kDemodNT) void am_sub_kernel(const AmArgs a) {
    __shared__ double red[kDemodNT];
    const int c = blockIdx.y;
    const double* __restrict__ part = a.part + (long long)c * a.G;
    double s = 0.0;
    for (int k = threadIdx.x; k < a.G; k += kDemodNT) s += part[k];
    const float avg = (float)(block_sum(s, red) / (double)a.count);
    const float2* __restrict__ in = a.in + (long long)c * a.in_stride;
    float* __restrict__ out = a.out + (long long)c * a.out_stride;
    const long long step = (long long)a.G * kDemodNT * kDemodSpl;
    for (long long i0 = ((long long)blockIdx.x * kDemodNT + threadIdx.x) * kDemodSpl; i0 < a.count; i0 += step) {
        float m[kDemodSpl];
        const int n = for_samples(in, i0, a.count, a.vec, [&](int j, float2 v) { m[j] = am_mag(v) - avg; });
        if (a.vec && n == kDemodSpl) {
            float4* q = reinterpret_cast<float4*>(out + i0);
            q[0] = make_float4(m[0], m[1], m[2], m[3]);
            q[1] = make_float4(m[4], m[5], m[6], m[7]);
        } else {
#pragma unroll
            for (int j = 0; j < kDemodSpl; j++)
                if (j < n) out[i0 + j] = m[j];
        }
    }
}

// SSBDemod::run: xlate_kernel's loop (same geometry, same phasor recursion: bit-identical to its real part), storing
// only re(x * phase_n).  vec: in 16-byte and out 8-byte aligned.
template <int NT> __global__ __launch_bounds__(NT) void ssb_demod_kernel(const XlateArgs a, float* __restrict__ out) {
    const long long npairs = (a.count + 1) >> 1;
    const long long stride = (long long)gridDim.x * NT;
    long long p = (long long)blockIdx.x * NT + threadIdx.x;
    if (p >= npairs) return;
    double2 ph = phasor_fx(a.phase0 + (unsigned long long)(2 * p) * a.dphase);
    for (; p < npairs; p += stride) {
        const long long g = 2 * p;
        const double2 ph1 = cmul(ph, a.rot_one);
        if (g + 1 < a.count) {
            float2 x0, x1;
            if (a.vec) {
                const float4 v = reinterpret_cast<const float4*>(a.in)[p];
                x0 = make_float2(v.x, v.y);
                x1 = make_float2(v.z, v.w);
            } else {
                x0 = a.in[g];
                x1 = a.in[g + 1];
            }
            const float y0 = rotate(x0, ph, g, a.gm1).x, y1 = rotate(x1, ph1, g + 1, a.gm1).x;
            if (a.vec) {
                reinterpret_cast<float2*>(out)[p] = make_float2(y0, y1);
            } else {
                out[g] = y0;
                out[g + 1] = y1;
            }
        } else {
            out[g] = rotate(a.in[g], ph, g, a.gm1).x;
        }
        ph = cmul(ph, a.rot_stride);
    }
}

}  // namespace qk

namespace qh {

namespace {
int out_floats(const Demod* d) { return d->kind == QDSP_HIP_DEMOD_FM_STEREO ? 2 : 1; }
bool is_fm(const Demod* d) { return d->kind == QDSP_HIP_DEMOD_FM || d->kind == QDSP_HIP_DEMOD_FM_STEREO; }

template <bool SSB> Demod* as_kind(void* h) {
    Demod* d = as<Demod>(h);
    return (d && (d->kind == kDemodSsb) == SSB) ? d : nullptr;
}
constexpr auto as_plain = as_kind<false>, as_ssb = as_kind<true>;

void demod_free(Demod* d) {
    op_free(d, [d] {
        hip_free_all({d->d_phase[0], d->d_phase[1], d->d_speed, d->d_part});
        if (d->nco) destroy(d->nco);
    });
}

int demod_launch(Demod* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s);

int demod_new(void** h, int device, int kind, int nchan, int max_block) {
    Demod* d = nullptr;
    if (const int rc = op_new<Demod, demod_launch>(&d, h, kind >= 0 && kind <= kDemodSsb, device, nchan, max_block)) return rc;
    d->kind = kind;
    // phasorSpeed of sampleRate == deviation until set_fm: out = phase step / (2 pi)
    d->rate.assign(nchan, 1.0f);
    d->dev.assign(nchan, 1.0f);
    d->speed.assign(nchan, (2 * 3.1415926535f) / (1.0f / 1.0f));
    hipError_t err = stream_op_init(d, device, nchan, max_block, sizeof(float2), out_floats(d) * sizeof(float));
    if (is_fm(d)) {
        for (int i = 0; i < 2 && err == hipSuccess; i++) {
            err = hipMalloc(&d->d_phase[i], (size_t)nchan * sizeof(float));
            if (err == hipSuccess) err = hipMemset(d->d_phase[i], 0, (size_t)nchan * sizeof(float));
        }
        if (err == hipSuccess) err = hipMalloc(&d->d_speed, (size_t)nchan * sizeof(float));
        if (err == hipSuccess) err = hipMemcpy(d->d_speed, d->speed.data(), (size_t)nchan * sizeof(float), hipMemcpyHostToDevice);
    }
    if (err == hipSuccess && kind == QDSP_HIP_DEMOD_AM) err = hipMalloc(&d->d_part, (size_t)nchan * qk::kAmMaxParts * sizeof(double));
    return op_created<demod_free>(h, d, err);
}

// d_in: nchan rows of `count` complex samples, in_stride apart; d_out: nchan rows of `count` outputs, out_stride apart
int demod_launch(Demod* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (count < 0 || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < count) return QDSP_HIP_EINVAL;
    const int of = out_floats(d);
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & (uintptr_t)(of * sizeof(float) - 1))) return QDSP_HIP_EINVAL;
    if (count == 0) return 0;
    HIPCHK(hipSetDevice(d->device));
    const long long per_wg = (long long)qk::kDemodNT * qk::kDemodSpl;
    const long long tiles = (count + per_wg - 1) / per_wg;
    if (tiles > 0x7fffffffLL) return QDSP_HIP_ESIZE;
    const bool aligned = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0 && (in_stride & 1) == 0;
    if (is_fm(d)) {
        qk::FmArgs a;
        a.in = static_cast<const float2*>(d_in);
        a.out = d_out;
        a.phase = d->d_phase[d->cur];
        a.phase_next = d->d_phase[d->cur ^ 1];
        a.speed = d->d_speed;
        a.count = count;
        a.in_stride = in_stride;
        a.out_stride = out_stride;
        a.vec = aligned && out_stride % (4 / of) == 0;
        const dim3 grid((unsigned)tiles, (unsigned)d->nchan);
        if (of == 2) hipLaunchKernelGGL((qk::fm_demod_kernel<true>), grid, dim3(qk::kDemodNT), 0, s, a);
        else hipLaunchKernelGGL((qk::fm_demod_kernel<false>), grid, dim3(qk::kDemodNT), 0, s, a);
        HIPCHK(hipGetLastError());
        d->cur ^= 1;
        d->last = Launch{"fm_demod_kernel", (int)tiles, qk::kDemodNT, 0};
        return 0;
    }
    if (d->kind == QDSP_HIP_DEMOD_AM) {
        qk::AmArgs a;
        a.in = static_cast<const float2*>(d_in);
        a.out = static_cast<float*>(d_out);
        a.part = d->d_part;
        a.count = count;
        a.in_stride = in_stride;
        a.out_stride = out_stride;
        a.G = (int)(tiles < qk::kAmMaxParts ? tiles : qk::kAmMaxParts);
        a.vec = aligned && out_stride % 4 == 0;
        const dim3 grid((unsigned)a.G, (unsigned)d->nchan);
        hipLaunchKernelGGL(qk::am_partial_kernel, grid, dim3(qk::kDemodNT), 0, s, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(qk::am_sub_kernel, grid, dim3(qk::kDemodNT), 0, s, a);
        HIPCHK(hipGetLastError());
        d->last = Launch{"am_sub_kernel", a.G, qk::kDemodNT, (int)(qk::kDemodNT * sizeof(double))};
        return 0;
    }
    // SSB: the launch geometry of launch_xlate_inc (qdsp_hip.hip), which the phasor recursion depends on
    Engine* e = d->nco;
    apply_pending_inc(e);
    constexpr int NT = 256;
    qk::XlateArgs a;
    a.in = static_cast<const float2*>(d_in);
    a.out = nullptr;
    a.count = count;
    a.phase0 = e->phase;
    a.dphase = e->dphase;
    const long long npairs = (count + 1) / 2;
    long long grid = (npairs + NT - 1) / NT;
    { const long long cap = 256LL * 1024; if (grid > cap) grid = cap; }
    unit_of_fx_c(e->dphase, 1.0L, &a.rot_one.x, &a.rot_one.y);
    unit_of_fx_c(e->dphase, (long double)(2 * grid * NT), &a.rot_stride.x, &a.rot_stride.y);
    a.vec = ((uintptr_t)d_in & 15) == 0 && ((uintptr_t)d_out & 7) == 0;
    a.gm1 = e->volk_gain ? e->gm1 : 0.0f;
    hipLaunchKernelGGL((qk::ssb_demod_kernel<NT>), dim3((unsigned)grid), dim3(NT), 0, s, a, static_cast<float*>(d_out));
    HIPCHK(hipGetLastError());
    e->phase += (unsigned long long)count * e->dphase;
    d->last = Launch{"ssb_demod_kernel", (int)grid, NT, 0};
    return 0;
}

}  // namespace

// fm_demod_kernel with float rows out, for a caller that keeps its own phase slots (stereo_fm.hip): the launch alone
void launch_fm_mono(const qk::FmArgs& a, int tiles, int nchan, hipStream_t s) {
    hipLaunchKernelGGL((qk::fm_demod_kernel<false>), dim3((unsigned)tiles, (unsigned)nchan), dim3(qk::kDemodNT), 0, s, a);
}

}  // namespace qh

using namespace qh;

extern "C" {

// ---- FloatFMDemod / FMDemod / AMDemod ------------------------------------------------------------
int qdsp_hip_demod_create(void** h, int device, int kind, int nchan, int max_block) {
    if (kind == kDemodSsb) return QDSP_HIP_EINVAL;
    return demod_new(h, device, kind, nchan, max_block);
}
int qdsp_hip_demod_set_fm(void* h, int chan, float sample_rate, float deviation) {
    Demod* d = as_plain(h);
    if (!d || !is_fm(d) || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    // FloatFMDemod::init / setSampleRate / setDeviation (demodulator.h:42,62,72), in float
    const float speed = (2 * 3.1415926535f) / (sample_rate / deviation);
    if (!std::isfinite(sample_rate) || !std::isfinite(deviation) || !std::isfinite(speed) || speed == 0.0f) return QDSP_HIP_EINVAL;
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++) {
        d->rate[c] = sample_rate;
        d->dev[c] = deviation;
        d->speed[c] = speed;
    }
    return sync_upload(d, d->d_speed, d->speed.data(), (size_t)d->nchan * sizeof(float));
}
int qdsp_hip_demod_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<Demod, as_plain>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_demod_process(void* h, const float* in_iq, int count, void* out) {
    return qdsp_hip_demod_process_ex(h, in_iq, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_demod_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<Demod, demod_launch, as_plain>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_demod_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                     void* hip_stream) {
    return op_process_batch_dev<Demod, demod_launch, as_plain>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_demod_get_phase(void* h, int chan, float* phase) {
    Demod* d = as_plain(h);
    if (!d || !is_fm(d) || !chan_ok(d, chan) || !phase) return QDSP_HIP_EINVAL;
    return sync_download(d, phase, d->d_phase[d->cur] + chan, sizeof(float));
}
int qdsp_hip_demod_set_phase(void* h, int chan, float phase) {
    Demod* d = as_plain(h);
    if (!d || !is_fm(d) || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    const std::vector<float> v((size_t)chan_count(d, chan), phase);
    return sync_upload(d, d->d_phase[d->cur] + chan_first(chan), v.data(), v.size() * sizeof(float));
}
int qdsp_hip_demod_reset(void* h) {
    Demod* d = as_plain(h);
    if (!d) return QDSP_HIP_EINVAL;
    if (!is_fm(d)) return 0;   // (AM keeps no state between calls)
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++) HIPCHK(hipMemset(d->d_phase[i], 0, (size_t)d->nchan * sizeof(float)));
    return 0;
}
void qdsp_hip_demod_destroy(void* h) { demod_free(as_plain(h)); }

// ---- SSBDemod: the xlate_cf32 NCO, real part out --------------------------------------------------
int qdsp_hip_ssb_cf32_create(void** h, int device, float phase_inc_re, float phase_inc_im, int max_block) {
    if (phase_inc_re == 0.0f && phase_inc_im == 0.0f) return QDSP_HIP_EINVAL;
    int rc = demod_new(h, device, kDemodSsb, 1, max_block);
    if (rc) return rc;
    Demod* d = static_cast<Demod*>(*h);
    void* e = nullptr;
    rc = create(&e, KIND_XLATE, device, 2, true, false, 0);
    if (rc) {
        demod_free(d);
        *h = nullptr;
        return rc;
    }
    d->nco = static_cast<Engine*>(e);
    set_inc_now(d->nco, phase_inc_re, phase_inc_im);
    return 0;
}
int qdsp_hip_ssb_cf32_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<Demod, as_ssb>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_ssb_cf32_process(void* h, const float* in_iq, int count, float* out) {
    return qdsp_hip_ssb_cf32_process_ex(h, in_iq, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_ssb_cf32_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<Demod, demod_launch, as_ssb>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_ssb_cf32_set_phase_inc(void* h, float re, float im) {
    Demod* d = as_ssb(h);
    if (!d || (re == 0.0f && im == 0.0f)) return QDSP_HIP_EINVAL;
    set_inc(d->nco, re, im);
    return 0;
}
int qdsp_hip_ssb_cf32_get_phase(void* h, float* re, float* im) {
    Demod* d = as_ssb(h);
    return d ? get_phase(d->nco, re, im) : QDSP_HIP_EINVAL;
}
int qdsp_hip_ssb_cf32_set_phase(void* h, float re, float im) {
    Demod* d = as_ssb(h);
    return d ? set_phase(d->nco, re, im) : QDSP_HIP_EINVAL;
}
int qdsp_hip_ssb_cf32_advance(void* h, int64_t n) {
    Demod* d = as_ssb(h);
    if (!d) return QDSP_HIP_EINVAL;
    apply_pending_inc(d->nco);
    d->nco->phase += (unsigned long long)n * d->nco->dphase;
    return 0;
}
int qdsp_hip_ssb_cf32_set_volk_gain(void* h, int on) {
    Demod* d = as_ssb(h);
    if (!d) return QDSP_HIP_EINVAL;
    d->nco->volk_gain = on != 0;
    return 0;
}
void qdsp_hip_ssb_cf32_destroy(void* h) { demod_free(as_ssb(h)); }

}  // extern "C"
