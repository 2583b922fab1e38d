// stereo_fm.hip -- StereoFMDemod (design notes: stereo_fm.hip.h) and its C entry points.
// Compiled with the demodulators' flags: no fast-math, correctly rounded f32 division.  The reference's element-wise lines are
// restated under `#pragma clang fp contract(off)`; the pilot filter is an explicit chain of fmaf in tap order.
#include "stereo_fm.hip.h"

namespace qk {

// The pilot filter.  grid (tiles, nchan); LDS float j of a workgroup = the sample at call position tile start - (T - 1) + j.
__global__ __launch_bounds__(kDemodNT) void pilot_fir_kernel(const PilotArgs a) {
    __shared__ __attribute__((aligned(16))) float s[kPilotLds];
    __shared__ float red[kDemodNT];
    const int c = blockIdx.y, t = threadIdx.x;
    const int T = a.T, H = T - 1;
    const long long b = (long long)blockIdx.x * kPilotTile;
    const float* __restrict__ m = a.m + (long long)c * a.sstride;
    const float* __restrict__ hist = a.hist + (long long)c * H;
    const int nstage = kPilotTile + H;
    for (int j = t; j < nstage; j += kDemodNT) {
        const long long pos = b - H + j;
        float v = 0.0f;                        // (past the end of the call: under outputs that are not stored)
        if (pos < 0) v = hist[H + pos];
        else if (pos < a.count) v = m[pos];
        s[j] = v;
    }
    __syncthreads();

    // outputs o0 .. o0 + 7 of the tile: output r at tap k reads s[o0 + k + r]; w[] is a ring of 12 over s[o0 + k ..]
    const int o0 = t * kDemodSpl;
    const float* __restrict__ taps = a.taps;
    const float4* s4 = reinterpret_cast<const float4*>(s);
    float acc[kDemodSpl];
#pragma unroll
    for (int r = 0; r < kDemodSpl; r++) acc[r] = 0.0f;
    float w[12];
    {
        const float4 v0 = s4[o0 >> 2], v1 = s4[(o0 >> 2) + 1];
        w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w;
        w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
    }
    int k0 = 0;
    // (the read-ahead of the last group reaches s[o0 + k0 + 19] <= s[T + 2047]: inside the array (kPilotLds) but, for the last lane,
    // one float past the staged ones -- read uninitialised and never used in an FMA)
    for (; k0 + 12 <= T; k0 += 12) {
#pragma unroll
        for (int u = 0; u < 3; u++) {
            const float4 nx = s4[(o0 + k0 + 4 * u + 8) >> 2];
            w[(8 + 4 * u) % 12] = nx.x;
            w[(9 + 4 * u) % 12] = nx.y;
            w[(10 + 4 * u) % 12] = nx.z;
            w[(11 + 4 * u) % 12] = nx.w;
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const float h = taps[k0 + 4 * u + kk];
#pragma unroll
                for (int r = 0; r < kDemodSpl; r++) acc[r] = __builtin_fmaf(h, w[(4 * u + kk + r) % 12], acc[r]);
            }
        }
    }
    for (int k = k0; k < T; k++) {             // the last T % 12 taps: the same chain, one LDS float per FMA
        const float h = taps[k];
#pragma unroll
        for (int r = 0; r < kDemodSpl; r++) acc[r] = __builtin_fmaf(h, s[o0 + k + r], acc[r]);
    }

    const long long rem = a.count - (b + o0);
    const int n = rem < 0 ? 0 : (rem < kDemodSpl ? (int)rem : kDemodSpl);
    store_lane<1>(a.f + (long long)c * a.sstride, b + o0, n, 1, acc);
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < kDemodSpl; r++)
        if (r < n && acc[r] > mx) mx = acc[r];
    const float top = block_max(mx, red);
    if (t == 0) a.part[(long long)c * a.tiles + blockIdx.x] = (double)top;

    // the next history = positions count - H .. count - 1: a sample of this call by the tile that holds it, a sample of the old
    // history (count < H) by the last tile, which has staged all of them
    float* __restrict__ hist_next = a.hist_next + (long long)c * H;
    const bool last = (int)blockIdx.x == a.tiles - 1;
    for (int j = t; j < nstage; j += kDemodNT) {
        const long long pos = b - H + j;
        const long long q = pos - (a.count - H);
        const bool own = pos >= 0 ? pos >= b : last;
        if (q >= 0 && pos < a.count && own) hist_next[q] = s[j];
    }
}

namespace {
// run()'s VOLK lines (demodulator.h:263-268) on the AGC's output p = f * (1.0f / level) (processing.h:129)
__device__ __forceinline__ void mix_one(float m, float f, float scalar, float& l, float& r) {
#pragma clang fp contract(off)
    const float p = f * scalar;
    const float d = p * p;
    const float sd = m * d;
    l = m + sd;
    r = m - sd;
}
}  // namespace

// AGC's level of the call and the matrix.  grid (tiles, nchan)
__global__ __launch_bounds__(kDemodNT) void stereo_mix_kernel(const MixArgs a) {
    __shared__ float red[kDemodNT];
    const int c = blockIdx.y, t = threadIdx.x;
    const double* __restrict__ part = a.part + (long long)c * a.tiles;
    float acc = -INFINITY;
    for (int k = t; k < a.tiles; k += kDemodNT) {
        const float v = (float)part[k];
        if (v > acc) acc = v;
    }
    const float level = agc_level(a.level[c], a.cfr[c], a.count, block_max(acc, red));
    if (blockIdx.x == 0 && t == 0) a.level_next[c] = level;
    const float scalar = 1.0f / level;
    const long long i0 = ((long long)blockIdx.x * kDemodNT + t) * kDemodSpl;
    if (i0 >= a.count) return;
    float m[kDemodSpl], f[kDemodSpl], y[2 * kDemodSpl];
    const int n = load_lane<1>(a.m + (long long)c * a.sstride, i0, a.count, 1, m);
    load_lane<1>(a.f + (long long)c * a.sstride, i0, a.count, 1, f);
#pragma unroll
    for (int j = 0; j < kDemodSpl; j++) mix_one(m[j], f[j], scalar, y[2 * j], y[2 * j + 1]);
    store_lane<2>(a.out + (long long)c * a.out_stride * 2, i0, n, a.vec, y);
}

}  // namespace qk

namespace qh {

namespace {
size_t hist_floats(const StereoFm* d) { return (size_t)d->nchan * (size_t)(d->ntaps > 1 ? d->ntaps - 1 : 1); }

void free_scratch(StereoFm* d) {
    for (void* p : {(void*)d->d_m, (void*)d->d_f, (void*)d->d_part})
        if (p) (void)hipFree(p);
    d->d_m = d->d_f = nullptr;
    d->d_part = nullptr;
    d->scratch_cap = 0;
}

void sfm_free(StereoFm* d) {
    op_free(d, [d] {
        free_scratch(d);
        hip_free_all({d->d_phase[0], d->d_phase[1], d->d_hist[0], d->d_hist[1], d->d_level[0], d->d_level[1], d->d_speed, d->d_cfr, d->d_taps});
    });
}

// rows of `cap` samples (a multiple of 4) for m and f, one partial per tile
hipError_t alloc_scratch(StereoFm* d, long long cap) {
    const long long tiles = (cap + qk::kPilotTile - 1) / qk::kPilotTile;
    hipError_t err = hipMalloc(&d->d_m, (size_t)d->nchan * (size_t)cap * sizeof(float));
    if (err == hipSuccess) err = hipMalloc(&d->d_f, (size_t)d->nchan * (size_t)cap * sizeof(float));
    if (err == hipSuccess) err = hipMalloc(&d->d_part, (size_t)d->nchan * (size_t)tiles * sizeof(double));
    if (err == hipSuccess) d->scratch_cap = cap;
    else free_scratch(d);
    return err;
}

// the taps and a zero history of their length, in both slots; the device is idle.  On failure the handle keeps its old taps and
// history slots (their contents zeroed if the length did not change).
hipError_t load_taps(StereoFm* d, const float* taps, int ntaps) {
    float* fresh[2] = {d->d_hist[0], d->d_hist[1]};
    const size_t floats = (size_t)d->nchan * (size_t)(ntaps > 1 ? ntaps - 1 : 1);
    if (ntaps != d->ntaps) {   // both new slots before the old ones go
        fresh[0] = fresh[1] = nullptr;
        for (int i = 0; i < 2; i++) {
            const hipError_t err = hipMalloc(&fresh[i], floats * sizeof(float));
            if (err != hipSuccess) {
                if (fresh[0]) (void)hipFree(fresh[0]);
                return err;
            }
        }
    }
    hipError_t err = hipSuccess;
    for (int i = 0; i < 2 && err == hipSuccess; i++) err = hipMemset(fresh[i], 0, floats * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(d->d_taps, taps, (size_t)ntaps * sizeof(float), hipMemcpyHostToDevice);
    if (fresh[0] != d->d_hist[0]) {
        if (err != hipSuccess) {
            for (int i = 0; i < 2; i++) (void)hipFree(fresh[i]);
            return err;
        }
        for (int i = 0; i < 2; i++) {
            if (d->d_hist[i]) (void)hipFree(d->d_hist[i]);
            d->d_hist[i] = fresh[i];
        }
    }
    if (err == hipSuccess) d->ntaps = ntaps;
    return err;
}

int sfm_launch(StereoFm* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s);

int sfm_new(void** h, int device, int nchan, const float* taps, int ntaps, int max_block) {
    StereoFm* d = nullptr;
    const bool args_ok = taps && ntaps >= 1 && ntaps <= qk::kPilotMaxTaps;
    if (const int rc = op_new<StereoFm, sfm_launch>(&d, h, args_ok, device, nchan, max_block)) return rc;
    // sampleRate == deviation == 1 until set_fm
    d->speed.assign(nchan, (2 * 3.1415926535f) / (1.0f / 1.0f));
    d->cfr.assign(nchan, 20.0f / 1.0f);
    const size_t per_chan = (size_t)nchan * sizeof(float);
    hipError_t err = stream_op_init(d, device, nchan, max_block, sizeof(float2), sizeof(float2));
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc(&d->d_phase[i], per_chan);
        if (err == hipSuccess) err = hipMemset(d->d_phase[i], 0, per_chan);
        if (err == hipSuccess) err = hipMalloc(&d->d_level[i], per_chan);
        if (err == hipSuccess) err = hipMemset(d->d_level[i], 0, per_chan);
    }
    if (err == hipSuccess) err = hipMalloc(&d->d_speed, per_chan);
    if (err == hipSuccess) err = hipMemcpy(d->d_speed, d->speed.data(), per_chan, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc(&d->d_cfr, per_chan);
    if (err == hipSuccess) err = hipMemcpy(d->d_cfr, d->cfr.data(), per_chan, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc(&d->d_taps, (size_t)qk::kPilotMaxTaps * sizeof(float));
    if (err == hipSuccess) err = load_taps(d, taps, ntaps);
    if (err == hipSuccess && max_block > 0) err = alloc_scratch(d, ((long long)max_block + 3) & ~3LL);
    return op_created<sfm_free>(h, d, err);
}

// d_in: nchan rows of `count` complex samples, in_stride apart; d_out: nchan rows of `count` stereo_t, out_stride apart
int sfm_launch(StereoFm* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (count < 0 || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < count) return QDSP_HIP_EINVAL;
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return QDSP_HIP_EINVAL;
    if (count == 0) return 0;
    {   // (both sides are 8 bytes per sample; the output of a sample depends on its neighbours: no overlap at all)
        const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + ((uintptr_t)(d->nchan - 1) * in_stride + count) * 8;
        const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + ((uintptr_t)(d->nchan - 1) * out_stride + count) * 8;
        if (i0 < o1 && o0 < i1) return QDSP_HIP_EINVAL;
    }
    const long long tiles = (count + qk::kPilotTile - 1) / qk::kPilotTile;
    if (tiles > 0x7fffffffLL) return QDSP_HIP_ESIZE;
    HIPCHK(hipSetDevice(d->device));
    const long long sstride = ((long long)count + 3) & ~3LL;
    if (sstride > d->scratch_cap) {   // a larger call than any before: the scratch rows grow (nothing of ours is in flight after the wait)
        HIPCHK(hipDeviceSynchronize());
        free_scratch(d);
        HIPCHK(alloc_scratch(d, sstride));
    }
    qk::FmArgs fa;
    fa.in = static_cast<const float2*>(d_in);
    fa.out = d->d_m;
    fa.phase = d->d_phase[d->cur];
    fa.phase_next = d->d_phase[d->cur ^ 1];
    fa.speed = d->d_speed;
    fa.count = count;
    fa.in_stride = in_stride;
    fa.out_stride = sstride;
    fa.vec = ((uintptr_t)d_in & 15) == 0 && (in_stride & 1) == 0;   // (the scratch rows are 16-byte aligned)
    launch_fm_mono(fa, (int)tiles, d->nchan, s);
    HIPCHK(hipGetLastError());
    const dim3 grid((unsigned)tiles, (unsigned)d->nchan);
    qk::PilotArgs pa;
    pa.m = d->d_m;
    pa.f = d->d_f;
    pa.taps = d->d_taps;
    pa.hist = d->d_hist[d->cur];
    pa.hist_next = d->d_hist[d->cur ^ 1];
    pa.part = d->d_part;
    pa.count = count;
    pa.sstride = sstride;
    pa.T = d->ntaps;
    pa.tiles = (int)tiles;
    hipLaunchKernelGGL(qk::pilot_fir_kernel, grid, dim3(qk::kDemodNT), 0, s, pa);
    HIPCHK(hipGetLastError());
    qk::MixArgs ma;
    ma.m = d->d_m;
    ma.f = d->d_f;
    ma.out = static_cast<float*>(d_out);
    ma.cfr = d->d_cfr;
    ma.level = d->d_level[d->cur];
    ma.level_next = d->d_level[d->cur ^ 1];
    ma.part = d->d_part;
    ma.count = count;
    ma.sstride = sstride;
    ma.out_stride = out_stride;
    ma.tiles = (int)tiles;
    ma.vec = ((uintptr_t)d_out & 15) == 0 && (out_stride & 1) == 0;
    hipLaunchKernelGGL(qk::stereo_mix_kernel, grid, dim3(qk::kDemodNT), 0, s, ma);
    HIPCHK(hipGetLastError());
    d->cur ^= 1;
    d->last_count = count;
    d->last_sstride = sstride;
    d->last = Launch{"stereo_mix_kernel", (int)tiles, qk::kDemodNT, (int)(qk::kDemodNT * sizeof(float))};
    return 0;
}

// one float of channel `chan` of a double-buffered state (slot cur), after everything queued has run
int get_word(StereoFm* d, float* const* slots, int chan, float* v) { return sync_download(d, v, slots[d->cur] + chan, sizeof(float)); }
int set_word(StereoFm* d, float* const* slots, int chan, float v) {
    const std::vector<float> w((size_t)chan_count(d, chan), v);
    return sync_upload(d, slots[d->cur] + chan_first(chan), w.data(), w.size() * sizeof(float));
}
}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_stereo_fm_create(void** h, int device, int nchan, const float* pilot_taps, int ntaps, int max_block) {
    return sfm_new(h, device, nchan, pilot_taps, ntaps, max_block);
}
int qdsp_hip_stereo_fm_set_fm(void* h, int chan, float sample_rate, float deviation) {
    StereoFm* d = as<StereoFm>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    // FloatFMDemod::init (demodulator.h:42) and AGC::init's _CorrectedFallRate with fallRate 20 (demodulator.h:219, processing.h:93)
    const float speed = (2 * 3.1415926535f) / (sample_rate / deviation);
    const float cfr = 20.0f / sample_rate;
    if (!std::isfinite(sample_rate) || sample_rate <= 0.0f || !std::isfinite(deviation) || !std::isfinite(speed) || speed == 0.0f)
        return QDSP_HIP_EINVAL;
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++) {
        d->speed[c] = speed;
        d->cfr[c] = cfr;
    }
    if (const int rc = sync_upload(d, d->d_speed, d->speed.data(), (size_t)d->nchan * sizeof(float))) return rc;
    HIPCHK(hipMemcpy(d->d_cfr, d->cfr.data(), (size_t)d->nchan * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
int qdsp_hip_stereo_fm_set_pilot_taps(void* h, const float* taps, int ntaps) {
    StereoFm* d = as<StereoFm>(h);
    if (!d || !taps || ntaps < 1 || ntaps > qk::kPilotMaxTaps) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(load_taps(d, taps, ntaps));
    return 0;
}
int qdsp_hip_stereo_fm_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<StereoFm>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_stereo_fm_process(void* h, const float* in_iq, int count, float* out_lr) {
    return qdsp_hip_stereo_fm_process_ex(h, in_iq, QDSP_HIP_LINK_HOST, count, out_lr, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_stereo_fm_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<StereoFm, sfm_launch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_stereo_fm_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                         void* hip_stream) {
    return op_process_batch_dev<StereoFm, sfm_launch>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_stereo_fm_get_phase(void* h, int chan, float* phase) {
    StereoFm* d = as<StereoFm>(h);
    if (!d || !chan_ok(d, chan) || !phase) return QDSP_HIP_EINVAL;
    return get_word(d, d->d_phase, chan, phase);
}
int qdsp_hip_stereo_fm_set_phase(void* h, int chan, float phase) {
    StereoFm* d = as<StereoFm>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    return set_word(d, d->d_phase, chan, phase);
}
int qdsp_hip_stereo_fm_get_level(void* h, int chan, float* level) {
    StereoFm* d = as<StereoFm>(h);
    if (!d || !chan_ok(d, chan) || !level) return QDSP_HIP_EINVAL;
    return get_word(d, d->d_level, chan, level);
}
int qdsp_hip_stereo_fm_set_level(void* h, int chan, float level) {
    StereoFm* d = as<StereoFm>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    return set_word(d, d->d_level, chan, level);
}
int qdsp_hip_stereo_fm_pilot_dev(void* h, void** d_pilot, int64_t* stride) {
    StereoFm* d = as<StereoFm>(h);
    if (!d || !d_pilot || !stride) return QDSP_HIP_EINVAL;
    *d_pilot = d->last_count > 0 ? d->d_f : nullptr;
    *stride = d->last_sstride;
    return 0;
}
int qdsp_hip_stereo_fm_reset(void* h) {
    StereoFm* d = as<StereoFm>(h);
    if (!d) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++) {
        HIPCHK(hipMemset(d->d_phase[i], 0, (size_t)d->nchan * sizeof(float)));
        HIPCHK(hipMemset(d->d_level[i], 0, (size_t)d->nchan * sizeof(float)));
        HIPCHK(hipMemset(d->d_hist[i], 0, hist_floats(d) * sizeof(float)));
    }
    return 0;
}
void qdsp_hip_stereo_fm_destroy(void* h) { sfm_free(as<StereoFm>(h)); }

}  // extern "C"
