// level.hip -- Squelch and AGC (design notes: level.hip.h) and their C entry points.
// Compiled with the library's default flags: no fast-math, correctly rounded f32 division.  The reference's arithmetic is
// restated below under `#pragma clang fp contract(off)`.
#include "level.hip.h"

namespace qk {

namespace {
template <int KIND> struct Red { using type = double; };    // Squelch: FP64 sum of |x|
template <> struct Red<kLevelAgc> { using type = float; };  // AGC: maximum of x

// the n samples a lane holds, folded into its accumulator: sum of |x| (Squelch) / maximum (AGC: `if (x > level) level = x`)
template <int KIND, int NC> __device__ __forceinline__ void fold_lane(const float (&x)[kDemodSpl * NC], int n, typename Red<KIND>::type& acc) {
#pragma unroll
    for (int j = 0; j < kDemodSpl; j++) {
        if (j < n) {
            if constexpr (KIND == kLevelSquelch) acc += (double)am_mag(make_float2(x[2 * j], x[2 * j + 1]));
            else if (x[j] > acc) acc = x[j];
        }
    }
}

// Squelch::run's test (processing.h:467-469) on the FP64 sum
__device__ __forceinline__ bool squelch_open(double sum, long long count, float level) {
#pragma clang fp contract(off)
    const float mean = (float)(sum / (double)count);
    return 10.0f * log10f(mean) >= level;
}

// The call's scalar of channel c from the workgroup's reduced value: Squelch 1.0f (open) or 0.0f, AGC 1.0f / level.  Every lane
// computes it; `first` (one workgroup per channel) has lane 0 write the next state.
template <int KIND> __device__ __forceinline__ float call_scalar(const LevelArgs& a, int c, typename Red<KIND>::type r, bool first) {
    if constexpr (KIND == kLevelSquelch) {
        const bool open = squelch_open(r, a.count, a.param[c]);
        if (first && threadIdx.x == 0) static_cast<int*>(a.state_next)[c] = open ? 1 : 0;
        return open ? 1.0f : 0.0f;
    } else {
        const float level = agc_level(static_cast<const float*>(a.state)[c], a.param[c], a.count, r);
        if (first && threadIdx.x == 0) static_cast<float*>(a.state_next)[c] = level;
        return 1.0f / level;   // volk_32f_s32f_multiply_32f's scalar (processing.h:129)
    }
}

// Squelch: the samples as they are (memcpy) or +0.0f (memset); AGC: one rounded product per sample
template <int KIND, int NC> __device__ __forceinline__ void apply_lane(float (&x)[kDemodSpl * NC], float s) {
#pragma unroll
    for (int j = 0; j < kDemodSpl * NC; j++) {
        if constexpr (KIND == kLevelSquelch) x[j] = s != 0.0f ? x[j] : 0.0f;
        else x[j] = x[j] * s;
    }
}

template <int KIND> __device__ __forceinline__ typename Red<KIND>::type red_start() {
    if constexpr (KIND == kLevelSquelch) return 0.0;
    else return -INFINITY;
}

template <int KIND> __device__ __forceinline__ typename Red<KIND>::type block_reduce(typename Red<KIND>::type v, typename Red<KIND>::type* red) {
    if constexpr (KIND == kLevelSquelch) return block_sum(v, red);
    else return block_max(v, red);
}
}  // namespace

// short rows, one launch; grid (1, nchan).  a.tiles <= kLevelRowTiles is uniform, so x[][] stays in registers.
template <int KIND> __global__ __launch_bounds__(kDemodNT) void level_row_kernel(const LevelArgs a) {
    constexpr int NC = KIND == kLevelSquelch ? 2 : 1;
    using R = typename Red<KIND>::type;
    __shared__ R red[kDemodNT];
    const int c = blockIdx.y;
    const float* in = a.in + (long long)c * a.in_stride * NC;
    float* out = a.out + (long long)c * a.out_stride * NC;
    float x[kLevelRowTiles][kDemodSpl * NC];
    int n[kLevelRowTiles];
#pragma unroll
    for (int t = 0; t < kLevelRowTiles; t++) {
        n[t] = 0;
        if (t < a.tiles) n[t] = load_lane<NC>(in, ((long long)t * kDemodNT + threadIdx.x) * kDemodSpl, a.count, a.vec, x[t]);
    }
    R acc = red_start<KIND>();
#pragma unroll
    for (int t = 0; t < kLevelRowTiles; t++)
        if (t < a.tiles) fold_lane<KIND, NC>(x[t], n[t], acc);
    const float s = call_scalar<KIND>(a, c, block_reduce<KIND>(acc, red), true);
#pragma unroll
    for (int t = 0; t < kLevelRowTiles; t++) {
        if (t < a.tiles) {
            apply_lane<KIND, NC>(x[t], s);
            store_lane<NC>(out, ((long long)t * kDemodNT + threadIdx.x) * kDemodSpl, n[t], a.vec, x[t]);
        }
    }
}

// long rows, pass 1; grid (G, nchan), lanes stride over the row
template <int KIND> __global__ __launch_bounds__(kDemodNT) void level_partial_kernel(const LevelArgs a) {
    constexpr int NC = KIND == kLevelSquelch ? 2 : 1;
    using R = typename Red<KIND>::type;
    __shared__ R red[kDemodNT];
    const int c = blockIdx.y;
    const float* in = a.in + (long long)c * a.in_stride * NC;
    const long long step = (long long)a.G * kDemodNT * kDemodSpl;
    R acc = red_start<KIND>();
    for (long long i0 = ((long long)blockIdx.x * kDemodNT + threadIdx.x) * kDemodSpl; i0 < a.count; i0 += step) {
        float x[kDemodSpl * NC];
        const int n = load_lane<NC>(in, i0, a.count, a.vec, x);
        fold_lane<KIND, NC>(x, n, acc);
    }
    const R r = block_reduce<KIND>(acc, red);
    if (threadIdx.x == 0) a.part[(long long)c * a.G + blockIdx.x] = (double)r;
}

// long rows, pass 2; grid (G, nchan): every workgroup folds its channel's G partials (same order in all of them)
template <int KIND> __global__ __launch_bounds__(kDemodNT) void level_apply_kernel(const LevelArgs a) {
    constexpr int NC = KIND == kLevelSquelch ? 2 : 1;
    using R = typename Red<KIND>::type;
    __shared__ R red[kDemodNT];
    const int c = blockIdx.y;
    const double* __restrict__ part = a.part + (long long)c * a.G;
    R acc = red_start<KIND>();
    for (int k = threadIdx.x; k < a.G; k += kDemodNT) {
        if constexpr (KIND == kLevelSquelch) acc += part[k];
        else if ((float)part[k] > acc) acc = (float)part[k];
    }
    const float s = call_scalar<KIND>(a, c, block_reduce<KIND>(acc, red), blockIdx.x == 0);
    const float* in = a.in + (long long)c * a.in_stride * NC;
    float* out = a.out + (long long)c * a.out_stride * NC;
    const long long step = (long long)a.G * kDemodNT * kDemodSpl;
    for (long long i0 = ((long long)blockIdx.x * kDemodNT + threadIdx.x) * kDemodSpl; i0 < a.count; i0 += step) {
        float x[kDemodSpl * NC];
        int n;
        if (KIND == kLevelSquelch && s == 0.0f) {   // a closed row is not read again
            const long long rem = a.count - i0;
            n = rem < kDemodSpl ? (int)rem : kDemodSpl;
#pragma unroll
            for (int j = 0; j < kDemodSpl * NC; j++) x[j] = 0.0f;
        } else {
            n = load_lane<NC>(in, i0, a.count, a.vec, x);
            apply_lane<KIND, NC>(x, s);
        }
        store_lane<NC>(out, i0, n, a.vec, x);
    }
}

}  // namespace qk

namespace qh {

namespace {
int comps(const Level* d) { return d->kind == qk::kLevelSquelch ? 2 : 1; }
template <int KIND> Level* as_kind(void* h) {
    Level* d = as<Level>(h);
    return (d && d->kind == KIND) ? d : nullptr;
}
constexpr auto as_squelch = as_kind<qk::kLevelSquelch>, as_agc = as_kind<qk::kLevelAgc>;

void level_free(Level* d) {
    op_free(d, [d] { hip_free_all({d->d_state[0], d->d_state[1], d->d_param, d->d_part}); });
}

int level_launch(Level* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s);

int level_new(void** h, int device, int kind, int nchan, int max_block, float param0) {
    Level* d = nullptr;
    if (const int rc = op_new<Level, level_launch>(&d, h, true, device, nchan, max_block)) return rc;
    d->kind = kind;
    d->param.assign(nchan, param0);
    d->fall.assign(nchan, 0.0f);
    d->rate.assign(nchan, 1.0f);
    hipError_t err = stream_op_init(d, device, nchan, max_block, comps(d) * sizeof(float), comps(d) * sizeof(float));
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc(&d->d_state[i], (size_t)nchan * 4);
        if (err == hipSuccess) err = hipMemset(d->d_state[i], 0, (size_t)nchan * 4);   // level 0.0f / closed
    }
    if (err == hipSuccess) err = hipMalloc(&d->d_param, (size_t)nchan * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(d->d_param, d->param.data(), (size_t)nchan * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc(&d->d_part, (size_t)nchan * qk::kAmMaxParts * sizeof(double));
    return op_created<level_free>(h, d, err);
}

int push_param(Level* d, int chan, float v) {
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++) d->param[c] = v;
    return sync_upload(d, d->d_param, d->param.data(), (size_t)d->nchan * sizeof(float));
}

template <int KIND> void launch_kind(const qk::LevelArgs& a, bool row, int nchan, hipStream_t s) {
    if (row) {
        hipLaunchKernelGGL((qk::level_row_kernel<KIND>), dim3(1, (unsigned)nchan), dim3(qk::kDemodNT), 0, s, a);
    } else {
        const dim3 grid((unsigned)a.G, (unsigned)nchan);
        hipLaunchKernelGGL((qk::level_partial_kernel<KIND>), grid, dim3(qk::kDemodNT), 0, s, a);
        hipLaunchKernelGGL((qk::level_apply_kernel<KIND>), grid, dim3(qk::kDemodNT), 0, s, a);
    }
}

// d_in / d_out: nchan rows of `count` samples, in_stride / out_stride samples apart
int level_launch(Level* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (count < 0 || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count || out_stride < count) return QDSP_HIP_EINVAL;
    const int nc = comps(d);
    const size_t es = (size_t)nc * sizeof(float);
    const uintptr_t amask = (uintptr_t)(es - 1);
    if (((uintptr_t)d_in & amask) || ((uintptr_t)d_out & amask)) return QDSP_HIP_EINVAL;
    if (count == 0) return 0;
    if (!(d_in == d_out && in_stride == out_stride)) {   // in place is the same rows exactly; nothing else may overlap
        const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + ((uintptr_t)(d->nchan - 1) * in_stride + count) * es;
        const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + ((uintptr_t)(d->nchan - 1) * out_stride + count) * es;
        if (i0 < o1 && o0 < i1) return QDSP_HIP_EINVAL;
    }
    HIPCHK(hipSetDevice(d->device));
    const long long per_wg = (long long)qk::kDemodNT * qk::kDemodSpl;
    const long long tiles = (count + per_wg - 1) / per_wg;
    if (tiles > 0x7fffffffLL) return QDSP_HIP_ESIZE;
    qk::LevelArgs a;
    a.in = static_cast<const float*>(d_in);
    a.out = static_cast<float*>(d_out);
    a.param = d->d_param;
    a.state = d->d_state[d->cur];
    a.state_next = d->d_state[d->cur ^ 1];
    a.part = d->d_part;
    a.count = count;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.tiles = (int)tiles;
    a.G = (int)(tiles < qk::kAmMaxParts ? tiles : qk::kAmMaxParts);
    const int per16 = 4 / nc;   // samples per 16 bytes
    a.vec = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0 && in_stride % per16 == 0 && out_stride % per16 == 0;
    int row_tiles = qk::knob(qk::K_LEVEL_ROW_TILES, qk::kLevelRowTiles);   // (0: always the two-pass form)
    if (row_tiles > qk::kLevelRowTiles) row_tiles = qk::kLevelRowTiles;    // the registers of level_row_kernel
    const bool row = tiles <= row_tiles;
    if (nc == 2) launch_kind<qk::kLevelSquelch>(a, row, d->nchan, s);
    else launch_kind<qk::kLevelAgc>(a, row, d->nchan, s);
    HIPCHK(hipGetLastError());
    const int lds = (int)(qk::kDemodNT * (nc == 2 ? sizeof(double) : sizeof(float)));
    d->last = row ? Launch{"level_row_kernel", 1, qk::kDemodNT, lds} : Launch{"level_apply_kernel", a.G, qk::kDemodNT, lds};
    d->cur ^= 1;
    return 0;
}

// one 4-byte state word of channel `chan` (slot cur), after everything queued has run
int get_state(Level* d, int chan, void* v) { return sync_download(d, v, static_cast<char*>(d->d_state[d->cur]) + (size_t)chan * 4, 4); }

int level_reset(Level* d) {
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++) HIPCHK(hipMemset(d->d_state[i], 0, (size_t)d->nchan * 4));
    return 0;
}
}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

// ---- Squelch ------------------------------------------------------------------------------------
int qdsp_hip_squelch_create(void** h, int device, int nchan, int max_block) {
    return level_new(h, device, qk::kLevelSquelch, nchan, max_block, -50.0f);   // _level (processing.h:486)
}
int qdsp_hip_squelch_set_level(void* h, int chan, float level) {
    Level* d = as_squelch(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    return push_param(d, chan, level);
}
int qdsp_hip_squelch_get_open(void* h, int chan, int* open) {
    Level* d = as_squelch(h);
    if (!d || !chan_ok(d, chan) || !open) return QDSP_HIP_EINVAL;
    return get_state(d, chan, open);
}
int qdsp_hip_squelch_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<Level, as_squelch>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_squelch_process(void* h, const float* in_iq, int count, float* out_iq) {
    return qdsp_hip_squelch_process_ex(h, in_iq, QDSP_HIP_LINK_HOST, count, out_iq, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_squelch_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<Level, level_launch, as_squelch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_squelch_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                       void* hip_stream) {
    return op_process_batch_dev<Level, level_launch, as_squelch>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_squelch_reset(void* h) {
    Level* d = as_squelch(h);
    return d ? level_reset(d) : QDSP_HIP_EINVAL;
}
void qdsp_hip_squelch_destroy(void* h) { level_free(as_squelch(h)); }

// ---- AGC ----------------------------------------------------------------------------------------
int qdsp_hip_agc_create(void** h, int device, int nchan, int max_block) {
    return level_new(h, device, qk::kLevelAgc, nchan, max_block, 0.0f);   // fall_rate 0 / sample_rate 1
}
int qdsp_hip_agc_set(void* h, int chan, float fall_rate, float sample_rate) {
    Level* d = as_agc(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    if (!std::isfinite(sample_rate) || sample_rate <= 0.0f || !std::isfinite(fall_rate)) return QDSP_HIP_EINVAL;
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++) {
        d->fall[c] = fall_rate;
        d->rate[c] = sample_rate;
    }
    return push_param(d, chan, fall_rate / sample_rate);   // _CorrectedFallRate (processing.h:93), in float
}
int qdsp_hip_agc_get_level(void* h, int chan, float* level) {
    Level* d = as_agc(h);
    if (!d || !chan_ok(d, chan) || !level) return QDSP_HIP_EINVAL;
    return get_state(d, chan, level);
}
int qdsp_hip_agc_set_level(void* h, int chan, float level) {
    Level* d = as_agc(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    const std::vector<float> v((size_t)chan_count(d, chan), level);
    return sync_upload(d, static_cast<float*>(d->d_state[d->cur]) + chan_first(chan), v.data(), v.size() * sizeof(float));
}
int qdsp_hip_agc_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<Level, as_agc>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_agc_process(void* h, const float* in, int count, float* out) {
    return qdsp_hip_agc_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_agc_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<Level, level_launch, as_agc>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_agc_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                   void* hip_stream) {
    return op_process_batch_dev<Level, level_launch, as_agc>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_agc_reset(void* h) {
    Level* d = as_agc(h);
    return d ? level_reset(d) : QDSP_HIP_EINVAL;
}
void qdsp_hip_agc_destroy(void* h) { level_free(as_agc(h)); }

}  // extern "C"
