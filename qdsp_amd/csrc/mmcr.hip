// mmcr.hip -- MMClockRecovery<float | complex_t> batched with one row per lane (design notes: mmcr.hip.h), its interpolator table
// and its C entry points.
#include "mmcr.hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

// the reference's float expressions, operation by operation: nothing in this file is contracted into an FMA by the compiler
#pragma clang fp contract(off)

namespace qk {

namespace {

// (as in costas.hip: values that would otherwise be hoisted out of the round loop and held in 2 x 32 scalar registers)
__device__ __forceinline__ long long per_round(long long v) {
    asm volatile("" : "+s"(v));
    return v;
}
__device__ __forceinline__ int per_round(int v) {
    asm volatile("" : "+s"(v));
    return v;
}

template <class T> __device__ __forceinline__ T mm_zero() {
    if constexpr (std::is_same_v<T, float>) return 0.0f;
    else return make_float2(0.0f, 0.0f);
}

// The staging steps of a round, for a wave of R <= 16 rows that takes S = 1 << SH segments of 64 samples from each (R S <= 32):
// instruction k serves segment k % S of row k / S.
// round c into registers; samples past the row's end read as 0
template <class T, int SH> __device__ __forceinline__ void mm_load(const MmcrArgs& a, int row0, int R, long long c, T (&pre)[kMmcrSlots]) {
    constexpr int S = 1 << SH;
    R = per_round(R);
    const long long stride = per_round(a.in_stride);
    const long long i0 = c * (64 * S) + threadIdx.x;
    const T* p = static_cast<const T*>(a.in) + (long long)row0 * stride + i0;
#pragma unroll
    for (int k = 0; k < kMmcrSlots; k++) {
        const int row = k >> SH, seg = k & (S - 1);
        if (row < R) pre[k] = i0 + seg * 64 < a.count ? p[row * stride + seg * 64] : mm_zero<T>();
    }
}

// registers -> input image, behind each row's halo
template <class T, int SH> __device__ __forceinline__ void mm_stage(T* img, int R, const T (&pre)[kMmcrSlots]) {
    constexpr int S = 1 << SH, pitch = 64 * S + kMmcrHalo;
    R = per_round(R);
#pragma unroll
    for (int k = 0; k < kMmcrSlots; k++)
        if ((k >> SH) < R) img[(k >> SH) * pitch + kMmcrHalo + (k & (S - 1)) * 64 + threadIdx.x] = pre[k];
}

template <int N> struct Shift {
    static constexpr int value = N;
};

// f(Shift<sh>{})
template <class F> __device__ __forceinline__ void by_shift(int sh, F f) {
    switch (sh) {
        case 1: f(Shift<1>{}); break;
        case 2: f(Shift<2>{}); break;
        case 3: f(Shift<3>{}); break;
        case 4: f(Shift<4>{}); break;
        default: f(Shift<5>{}); break;
    }
}

__device__ __forceinline__ float dsp_step(float v) { return v > 0.0f ? 1.0f : -1.0f; }   // DSP_STEP (utils/macros.h)

// sum_k x[k] t[k]: exact products, added in tap order in FP64 (fma with an exact product rounds as the sum does), rounded once
__device__ __forceinline__ float mm_dot(const float (&x)[kMmcrTaps], const float (&t)[kMmcrTaps]) {
    double acc = (double)x[0] * (double)t[0];
#pragma unroll
    for (int k = 1; k < kMmcrTaps; k++) acc = fma((double)x[k], (double)t[k], acc);
    return (float)acc;
}

}  // namespace

template <class T> __global__ __launch_bounds__(kMmcrLanes) void mm_clock_kernel(const MmcrArgs a) {
    constexpr bool kCplx = !std::is_same_v<T, float>;
    __shared__ T img[kMmcrImgIn];
    __shared__ T oimg[kMmcrImgOut];
    __shared__ float4 tab[kMmcrTable / 4];
    __shared__ int meta[2 * kMmcrRows];          // per row: symbols of this round, symbols before it
    const int lane = threadIdx.x;
    const int row0 = blockIdx.x * kMmcrRows;
    const int R = a.nchan - row0 < kMmcrRows ? a.nchan - row0 : kMmcrRows;
    int sh = 1;
    while ((R << (sh + 1)) <= kMmcrSlots) sh++;
    const int L = 64 << sh, pitch = L + kMmcrHalo, opitch = L + 1;   // R * pitch <= kMmcrImgIn, R * opitch <= kMmcrImgOut
    const long long rounds = (a.count + L - 1) / L;

    for (int i = lane; i < kMmcrTable / 4; i += kMmcrLanes) tab[i] = reinterpret_cast<const float4*>(a.taps)[i];

    float mu = 0.5f, dyn = 1.0f, g_omega = 0.0f, g_mu = 0.0f, o_min = 1.0f, o_max = 1.0f;
    float det[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // float rows: lastOutput; complex rows: p0, p1, c0, c1
    T tail[kMmcrHalo];
    int next = 0, total = 0;
    bool bad = false;
    if (lane < R) {
        const float* st = a.state + (long long)(row0 + lane) * kMmcrState;
        const float* pr = a.par + (long long)(row0 + lane) * kMmcrPar;
        g_omega = pr[0];
        g_mu = pr[1];
        o_min = pr[2];
        o_max = pr[3];
        mu = st[0];
        dyn = st[1];
        next = __float_as_int(st[2]);
        bad = !(mu >= 0.0f && mu < 1.0f) || next < 0;      // a stopped row carries a NaN
#pragma unroll
        for (int j = 0; j < (kCplx ? 8 : 1); j++) det[j] = st[kMmcrStDet + j];
#pragma unroll
        for (int j = 0; j < kMmcrHalo; j++) {
            if constexpr (kCplx) tail[j] = make_float2(st[kMmcrStHist + 2 * j], st[kMmcrStHist + 2 * j + 1]);
            else tail[j] = st[kMmcrStHist + j];
            img[lane * pitch + j] = tail[j];
        }
    }

    T pre[kMmcrSlots];
    by_shift(sh, [&](auto s) { mm_load<T, decltype(s)::value>(a, row0, R, 0, pre); });
    for (long long c = 0; c < rounds; c++) {
        by_shift(sh, [&](auto s) {
            mm_stage<T, decltype(s)::value>(img, R, pre);
            if (c + 1 < rounds) mm_load<T, decltype(s)::value>(a, row0, R, c + 1, pre);   // in flight during the walk
        });
        __syncthreads();
        const long long left = a.count - c * L;
        const int n = left < L ? (int)left : L;
        if (lane < R) {
            const T* p = img + lane * pitch;
            T* q = oimg + lane * opitch;
            int m = 0;
            while (!bad && next < n) {               // 0 <= next: the window is p[next .. next + 7], inside the row's pitch
                int idx = (int)roundf(mu * 128.0f);
                idx = idx < 0 ? 0 : (idx > kMmcrSteps ? kMmcrSteps : idx);
                const float4 t0 = tab[2 * idx], t1 = tab[2 * idx + 1];
                const float t[kMmcrTaps] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
                float e;
                if constexpr (kCplx) {
                    float xr[kMmcrTaps], xi[kMmcrTaps];
#pragma unroll
                    for (int k = 0; k < kMmcrTaps; k++) {
                        const float2 v = p[next + k];
                        xr[k] = v.x;
                        xi[k] = v.y;
                    }
                    const float yr = mm_dot(xr, t), yi = mm_dot(xi, t);
                    if (total + m < a.cap) q[m++] = make_float2(yr, yi);
                    // p2 = p1; p1 = p0; c2 = c1; c1 = c0; p0 = y; c0 = DSP_STEP_CPLX(p0);
                    // e = ((p0 - p2) * c1.conj() - (c0 - c2) * p1.conj()).re, with complex_t's operators
                    const float p2r = det[2], p2i = det[3], c2r = det[6], c2i = det[7];
                    const float p1r = det[0], p1i = det[1], c1r = det[4], c1i = det[5];
                    const float c0r = dsp_step(yr), c0i = dsp_step(yi);
                    const float ur = yr - p2r, ui = yi - p2i, vr = c0r - c2r, vi = c0i - c2i;
                    const float ea = (ur * c1r) - (ui * -c1i);
                    const float eb = (vr * p1r) - (vi * -p1i);
                    e = ea - eb;
                    det[2] = p1r;
                    det[3] = p1i;
                    det[6] = c1r;
                    det[7] = c1i;
                    det[0] = yr;
                    det[1] = yi;
                    det[4] = c0r;
                    det[5] = c0i;
                } else {
                    float x[kMmcrTaps];
#pragma unroll
                    for (int k = 0; k < kMmcrTaps; k++) x[k] = p[next + k];
                    const float y = mm_dot(x, t);
                    if (total + m < a.cap) q[m++] = y;
                    e = (dsp_step(det[0]) * y) - (det[0] * dsp_step(y));
                    det[0] = y;
                }
                bad = e != e;
                e = fminf(fmaxf(e, -1.0f), 1.0f);
                dyn = fminf(fmaxf(dyn + (g_omega * e), o_min), o_max);
                mu = mu + dyn + (g_mu * e);
                const float step = floorf(mu);
                const int istep = (int)step;
                next += istep < 1 ? 1 : istep;
                mu -= step;
            }
            next -= n;                               // (a stopped row's is never read again)
            if (bad) next = 0;
            meta[lane] = m;
            meta[kMmcrRows + lane] = total;
            total += m;
            // the row's last 7 samples, those of earlier rounds included, become the next round's halo
#pragma unroll
            for (int j = 0; j < kMmcrHalo; j++) tail[j] = p[n + j];
#pragma unroll
            for (int j = 0; j < kMmcrHalo; j++) img[lane * pitch + j] = tail[j];
        }
        __syncthreads();
        {
            const long long stride = per_round(a.out_stride);
            T* o = static_cast<T*>(a.out) + (long long)row0 * stride;
            for (int r = 0; r < R; r++) {
                const int m = meta[r], base = meta[kMmcrRows + r];      // base + m <= cap <= out_stride
                for (int j = lane; j < m; j += kMmcrLanes) o[r * stride + base + j] = oimg[r * opitch + j];
            }
        }
        // (the next round's stage writes behind the halos, its walk writes oimg and meta: the barrier after that stage orders both)
    }
    if (lane < R) {
        float* st = a.state_next + (long long)(row0 + lane) * kMmcrState;
        st[0] = bad ? __builtin_nanf("") : mu;
        st[1] = dyn;
        st[2] = __int_as_float(next);
        st[3] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; j++) st[kMmcrStDet + j] = det[j];
#pragma unroll
        for (int j = 0; j < kMmcrHalo; j++) {
            if constexpr (kCplx) {
                st[kMmcrStHist + 2 * j] = tail[j].x;
                st[kMmcrStHist + 2 * j + 1] = tail[j].y;
            } else {
                st[kMmcrStHist + j] = tail[j];
            }
        }
        a.counts[row0 + lane] = total;
    }
}

}  // namespace qk

namespace qh {

namespace {

constexpr double kPi = 3.14159265358979323846;

double mm_sinc(double x) { return x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x); }

// The 8-tap MMSE interpolator for a band of +-0.25 cycles per sample: row m (mu = m / 128) solves R h = p with
// R[k][l] = sinc((k - l) / 2), p[k] = sinc((3 + mu - k) / 2).  Solved in FP64 (elimination with partial pivoting); an entry below
// 1e-9 in magnitude is 0, every other is rounded to six significant decimal digits and then to float.
void mmse_table(float* out) {
    for (int m = 0; m <= qk::kMmcrSteps; m++) {
        const double mu = (double)m / qk::kMmcrSteps;
        double A[8][9];
        for (int k = 0; k < 8; k++) {
            for (int l = 0; l < 8; l++) A[k][l] = mm_sinc(0.5 * (k - l));
            A[k][8] = mm_sinc(0.5 * (3.0 + mu - k));
        }
        for (int c = 0; c < 8; c++) {
            int piv = c;
            for (int r = c + 1; r < 8; r++)
                if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
            for (int l = 0; l < 9; l++) std::swap(A[c][l], A[piv][l]);
            for (int r = c + 1; r < 8; r++) {
                const double f = A[r][c] / A[c][c];
                for (int l = c; l < 9; l++) A[r][l] -= f * A[c][l];
            }
        }
        double h[8];
        for (int k = 7; k >= 0; k--) {
            double s = A[k][8];
            for (int l = k + 1; l < 8; l++) s -= A[k][l] * h[l];
            h[k] = s / A[k][k];
        }
        for (int k = 0; k < 8; k++) {
            char buf[32];
            snprintf(buf, sizeof(buf), "%.5e", std::fabs(h[k]) < 1e-9 ? 0.0 : h[k]);
            out[m * 8 + k] = (float)strtod(buf, nullptr);
        }
    }
}

// The parameter rule (include/qdsp_hip.h); the limits as clock_recovery.h:83-84 forms them
bool mmcr_limits(float omega, float g_omega, float g_mu, float rel, float* o_min, float* o_max, float* min_step) {
    if (!std::isfinite(omega) || !std::isfinite(g_omega) || !std::isfinite(g_mu) || !std::isfinite(rel)) return false;
    if (!(omega > 0.0f) || !(rel >= 0.0f) || !(rel < 1.0f)) return false;
    *o_min = omega - (omega * rel);
    *o_max = omega + (omega * rel);
    *min_step = *o_min - std::fabs(g_mu);
    const float top = *o_max + std::fabs(g_mu);
    return std::isfinite(*o_max) && *min_step >= 1.0f && top < 1048576.0f;
}

void mmcr_free(Mmcr* d) {
    op_free(d, [d] {
        hip_free_all({d->d_state[0], d->d_state[1], d->d_par, d->d_taps, d->d_counts});
        if (d->h_count) (void)hipHostFree(d->h_count);
    });
}

void mmcr_min_step(Mmcr* d) {
    float lo = d->par[2] - std::fabs(d->par[1]);
    for (int c = 1; c < d->nchan; c++) lo = std::fmin(lo, d->par[4 * c + 2] - std::fabs(d->par[4 * c + 1]));
    d->min_step = (int64_t)std::floor(lo);
}

int64_t mmcr_out_size(const Mmcr* d, int64_t count) { return count <= 0 ? 0 : (count + d->min_step - 1) / d->min_step; }

// rows c0 .. c0 + n - 1 of the current slot, or of both: the state after create / reset
int mmcr_fill_initial(Mmcr* d, int c0, int n, bool both) {
    std::vector<float> v((size_t)n * qk::kMmcrState, 0.0f);
    for (int c = 0; c < n; c++) {
        v[(size_t)c * qk::kMmcrState] = 0.5f;
        v[(size_t)c * qk::kMmcrState + 1] = d->omega[c0 + c];
    }
    for (int s = 0; s < 2; s++)
        if (both || s == d->cur)
            HIPCHK(hipMemcpy(d->d_state[s] + (size_t)c0 * qk::kMmcrState, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// new parameters for `chan` (-1: all); `which`: 0 omega (and dynOmega, as setOmega does), 1 the gains, 2 the limit
int mmcr_set(Mmcr* d, int chan, int which, float a, float b) {
    if (chan != -1 && !chan_ok(d, chan)) return QDSP_HIP_EINVAL;
    const int c0 = chan_first(chan), n = chan_count(d, chan);
    std::vector<float> par = d->par, omega = d->omega, rel = d->rel;
    for (int c = c0; c < c0 + n; c++) {
        if (which == 0) omega[c] = a;
        if (which == 1) {
            par[4 * c] = a;
            par[4 * c + 1] = b;
        }
        if (which == 2) rel[c] = a;
        float lo = 0.0f;
        if (!mmcr_limits(omega[c], par[4 * c], par[4 * c + 1], rel[c], &par[4 * c + 2], &par[4 * c + 3], &lo)) return QDSP_HIP_EINVAL;
    }
    if (const int rc = sync_upload(d, d->d_par, par.data(), par.size() * sizeof(float))) return rc;
    d->par = par;
    d->omega = omega;
    d->rel = rel;
    mmcr_min_step(d);
    if (which == 0) {
        std::vector<float> st((size_t)n * qk::kMmcrState);
        float* p = d->d_state[d->cur] + (size_t)c0 * qk::kMmcrState;
        HIPCHK(hipMemcpy(st.data(), p, st.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int c = 0; c < n; c++) st[(size_t)c * qk::kMmcrState + 1] = a;
        HIPCHK(hipMemcpy(p, st.data(), st.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}

// d_in: nchan rows of `count` samples, in_stride apart; d_out: rows of at least out_size(count) slots, out_stride apart; the
// per-row symbol counts go to d->d_counts.  Returns 0: the count of a call is only known once it has run.
int mmcr_launch(Mmcr* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    const int64_t cap = mmcr_out_size(d, count);
    if (count < 0 || count > (int64_t)1 << 40 || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < cap || cap > INT32_MAX) return QDSP_HIP_EINVAL;
    const uintptr_t mask = d->kind ? 7 : 3;
    if (((uintptr_t)d_in & mask) || ((uintptr_t)d_out & mask)) return QDSP_HIP_EINVAL;
    if (count > 0 && d_in == d_out) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    if (count == 0) {
        HIPCHK(hipMemsetAsync(d->d_counts, 0, (size_t)d->nchan * sizeof(int), s));
        return 0;
    }
    qk::MmcrArgs a;
    a.in = d_in;
    a.out = d_out;
    a.taps = d->d_taps;
    a.par = d->d_par;
    a.state = d->d_state[d->cur];
    a.state_next = d->d_state[d->cur ^ 1];
    a.counts = d->d_counts;
    a.count = count;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.cap = (int)cap;
    a.nchan = d->nchan;
    const dim3 grid((unsigned)((d->nchan + qk::kMmcrRows - 1) / qk::kMmcrRows)), block(qk::kMmcrLanes);
    if (d->kind) hipLaunchKernelGGL(qk::mm_clock_kernel<float2>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(qk::mm_clock_kernel<float>, grid, block, 0, s, a);
    HIPCHK(hipGetLastError());
    const int lds = (int)((qk::kMmcrImgIn + qk::kMmcrImgOut) * (d->kind ? sizeof(float2) : sizeof(float)) + qk::kMmcrTable * sizeof(float) +
                          2 * qk::kMmcrRows * sizeof(int));
    d->last = Launch{"mm_clock_kernel", (int)grid.x, qk::kMmcrLanes, lds};
    d->cur ^= 1;
    if (d->nchan == 1) HIPCHK(hipMemcpyAsync(d->h_count, d->d_counts, sizeof(int), hipMemcpyDeviceToHost, s));   // process_ex reads it
    return 0;
}

int64_t mmcr_out_count(const StreamOp* op, int64_t count) { return mmcr_out_size(static_cast<const Mmcr*>(op), count); }

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_mmcr_create(void** h, int device, int kind, int nchan, int max_block, float omega, float gain_omega, float mu_gain,
                         float rel_limit) {
    float o_min = 0.0f, o_max = 0.0f, lo = 0.0f;
    const bool args_ok = (kind == 0 || kind == 1) && mmcr_limits(omega, gain_omega, mu_gain, rel_limit, &o_min, &o_max, &lo);
    Mmcr* d = nullptr;
    if (const int rc = op_new<Mmcr, mmcr_launch, mmcr_out_count>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->kind = kind;
    d->omega.assign((size_t)nchan, omega);
    d->rel.assign((size_t)nchan, rel_limit);
    d->par.resize((size_t)nchan * qk::kMmcrPar);
    for (int c = 0; c < nchan; c++) {
        d->par[4 * c] = gain_omega;
        d->par[4 * c + 1] = mu_gain;
        d->par[4 * c + 2] = o_min;
        d->par[4 * c + 3] = o_max;
    }
    d->taps.resize(qk::kMmcrTable);
    mmse_table(d->taps.data());
    const size_t es = kind ? sizeof(float2) : sizeof(float);
    hipError_t err = stream_op_init(d, device, nchan, max_block, es, es);
    d->nchan = nchan;
    mmcr_min_step(d);
    const size_t st_b = (size_t)nchan * qk::kMmcrState * sizeof(float);
    for (int i = 0; i < 2 && err == hipSuccess; i++) err = hipMalloc(&d->d_state[i], st_b);
    if (err == hipSuccess) err = hipMalloc(&d->d_par, d->par.size() * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(d->d_par, d->par.data(), d->par.size() * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc(&d->d_taps, qk::kMmcrTable * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(d->d_taps, d->taps.data(), qk::kMmcrTable * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc(&d->d_counts, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipMemset(d->d_counts, 0, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipHostMalloc(reinterpret_cast<void**>(&d->h_count), sizeof(int), hipHostMallocDefault);
    if (err == hipSuccess) {
        *d->h_count = 0;
        const int rc = mmcr_fill_initial(d, 0, nchan, true);
        if (rc) err = (hipError_t)(-rc);
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return op_created<mmcr_free>(h, d, err);
}
int qdsp_hip_mmcr_set_omega(void* h, int chan, float omega) {
    Mmcr* d = as<Mmcr>(h);
    return d ? mmcr_set(d, chan, 0, omega, 0.0f) : QDSP_HIP_EINVAL;
}
int qdsp_hip_mmcr_set_gains(void* h, int chan, float gain_omega, float mu_gain) {
    Mmcr* d = as<Mmcr>(h);
    return d ? mmcr_set(d, chan, 1, gain_omega, mu_gain) : QDSP_HIP_EINVAL;
}
int qdsp_hip_mmcr_set_limit(void* h, int chan, float rel_limit) {
    Mmcr* d = as<Mmcr>(h);
    return d ? mmcr_set(d, chan, 2, rel_limit, 0.0f) : QDSP_HIP_EINVAL;
}
int qdsp_hip_mmcr_get_state(void* h, int chan, float* mu, float* dyn_omega, int* next) {
    Mmcr* d = as<Mmcr>(h);
    if (!d || !chan_ok(d, chan) || !mu || !dyn_omega || !next) return QDSP_HIP_EINVAL;
    float v[3];
    if (const int rc = sync_download(d, v, d->d_state[d->cur] + (size_t)chan * qk::kMmcrState, sizeof(v))) return rc;
    *mu = v[0];
    *dyn_omega = v[1];
    memcpy(next, &v[2], sizeof(int));
    return 0;
}
int qdsp_hip_mmcr_set_state(void* h, int chan, float mu, float dyn_omega, int next) {
    Mmcr* d = as<Mmcr>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    if (!(mu >= 0.0f && mu < 1.0f) || !std::isfinite(dyn_omega) || next < 0 || next > (1 << 21)) return QDSP_HIP_EINVAL;
    float v[3] = {mu, dyn_omega, 0.0f};
    memcpy(&v[2], &next, sizeof(int));
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++)
        HIPCHK(hipMemcpy(d->d_state[d->cur] + (size_t)c * qk::kMmcrState, v, sizeof(v), hipMemcpyHostToDevice));
    return 0;
}
int64_t qdsp_hip_mmcr_out_size(void* h, int64_t count) {
    Mmcr* d = as<Mmcr>(h);
    return (d && count >= 0) ? mmcr_out_size(d, count) : QDSP_HIP_EINVAL;
}
int qdsp_hip_mmcr_get_interp_taps(void* h, float* taps) {
    Mmcr* d = as<Mmcr>(h);
    if (!d || !taps) return QDSP_HIP_EINVAL;
    memcpy(taps, d->taps.data(), qk::kMmcrTable * sizeof(float));
    return 0;
}
int qdsp_hip_mmcr_set_interp_taps(void* h, const float* taps) {
    Mmcr* d = as<Mmcr>(h);
    if (!d || !taps) return QDSP_HIP_EINVAL;
    for (int i = 0; i < qk::kMmcrTable; i++)
        if (!std::isfinite(taps[i])) return QDSP_HIP_EINVAL;
    if (const int rc = sync_upload(d, d->d_taps, taps, qk::kMmcrTable * sizeof(float))) return rc;
    memcpy(d->taps.data(), taps, qk::kMmcrTable * sizeof(float));
    return 0;
}
int qdsp_hip_mmcr_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                    int* d_counts, void* hip_stream) {
    Mmcr* d = as<Mmcr>(h);
    if (!d) return QDSP_HIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (const int rc = mmcr_launch(d, d_in, count, in_stride, d_out, out_stride, s)) return rc;
    if (d_counts) HIPCHK(hipMemcpyAsync(d_counts, d->d_counts, (size_t)d->nchan * sizeof(int), hipMemcpyDeviceToDevice, s));
    return 0;
}
int qdsp_hip_mmcr_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    Mmcr* d = as<Mmcr>(h);
    return d ? mmcr_launch(d, d_in, count, count, d_out, mmcr_out_size(d, count), static_cast<hipStream_t>(hip_stream)) : QDSP_HIP_EINVAL;
}
int qdsp_hip_mmcr_get_counts(void* h, int* counts) {
    Mmcr* d = as<Mmcr>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    return sync_download(d, counts, d->d_counts, (size_t)d->nchan * sizeof(int));
}
int qdsp_hip_mmcr_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    Mmcr* d = as<Mmcr>(h);
    // the count is returned, so the call has to have run: an output link that hands over without waiting cannot be served
    if (!d || (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE)) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, count, out, out_link);
    if (rc < 0 || count == 0) return (int)rc;
    return *d->h_count;
}
int qdsp_hip_mmcr_process(void* h, const float* in, int count, float* out) {
    return qdsp_hip_mmcr_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_mmcr_reset(void* h) {
    Mmcr* d = as<Mmcr>(h);
    if (!d) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(d->d_counts, 0, (size_t)d->nchan * sizeof(int)));
    return mmcr_fill_initial(d, 0, d->nchan, true);
}
void qdsp_hip_mmcr_destroy(void* h) { mmcr_free(as<Mmcr>(h)); }

}  // extern "C"
