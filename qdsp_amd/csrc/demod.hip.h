// demod.hip.h -- the demodulators of src/dsp/demodulator.h that are data-parallel (gfx950):
//   fm_demod_kernel       FloatFMDemod / FMDemod (demodulator.h:33-187): fast_arctan2 of every sample, the difference to the
//                         previous sample's phase wrapped once by +-2 pi, divided by phasorSpeed.  Bit-identical to the reference
//                         loop, call boundaries included: the last sample's phase is carried on the device.
//   am_partial_kernel     AMDemod (demodulator.h:353-372): |x| (VOLK's generic magnitude, separately rounded) summed in FP64,
//   am_sub_kernel         one partial per workgroup; then every workgroup reduces its channel's partials in the same fixed
//                         order, avg = (float)(sum / count), and stores |x| - avg.  Deterministic; no atomics, no grid barrier.
//   ssb_demod_kernel      SSBDemod (demodulator.h:467-476): xlate_kernel's NCO, only the real part stored.
// Every kernel takes `nchan` channel-major rows (grid.y = channel) with strides in samples: the layout
// qdsp_hip_chan_cf32_process_dev writes.  The host side (handles, C entry points) is demod.hip.
#pragma once
#include "engine.hip.h"

namespace qk {

constexpr int kDemodNT = 256;     // lanes per workgroup
constexpr int kDemodSpl = 8;      // consecutive samples per lane (four 16-byte loads)
constexpr int kAmMaxParts = 1024; // workgroups (= FP64 partials) per channel of the AM passes

struct FmArgs {
    const float2* in;
    void* out;                  // float, or float2 {l, r} (STEREO)
    const float* phase;         // [nchan] phase carried from the previous call (slot cur)
    float* phase_next;          // [nchan] this call's last phase (slot cur ^ 1)
    const float* speed;         // [nchan] phasorSpeed
    long long count, in_stride, out_stride;
    int vec;                    // 1: every row 16-byte aligned
};

struct AmArgs {
    const float2* in;
    float* out;
    double* part;               // [nchan][G]
    long long count, in_stride, out_stride;
    int G;                      // workgroups per channel
    int vec;
};

// ---- device helpers shared by demod.hip, deemp.hip and level.hip ----
// volk_32fc_magnitude_32f, generic kernel: sqrtf(re*re + im*im), each operation rounded
__device__ __forceinline__ float am_mag(float2 v) {
#pragma clang fp contract(off)
    return sqrtf(v.x * v.x + v.y * v.y);
}

// a workgroup's sum of one double per lane, always added in the same tree order
__device__ __forceinline__ double block_sum(double s, double* red) {
    const int t = threadIdx.x;
    red[t] = s;
    __syncthreads();
#pragma unroll
    for (int w = kDemodNT / 2; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    return red[0];
}

// the up to kDemodSpl samples at row[i0..) (NC floats each): 16-byte loads when the row is aligned and the lane's samples are all there
template <int NC> __device__ __forceinline__ int load_lane(const float* row, long long i0, long long count, int vec, float (&x)[kDemodSpl * NC]) {
    const long long rem = count - i0;
    const int n = rem < 0 ? 0 : (rem < kDemodSpl ? (int)rem : kDemodSpl);
    if (vec && n == kDemodSpl) {
        const float4* p = reinterpret_cast<const float4*>(row + i0 * NC);
#pragma unroll
        for (int j = 0; j < kDemodSpl * NC / 4; j++) {
            const float4 v = p[j];
            x[4 * j] = v.x;
            x[4 * j + 1] = v.y;
            x[4 * j + 2] = v.z;
            x[4 * j + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kDemodSpl * NC; j++) x[j] = (j < n * NC) ? row[i0 * NC + j] : 0.0f;
    }
    return n;
}

template <int NC> __device__ __forceinline__ void store_lane(float* row, long long i0, int n, int vec, const float (&y)[kDemodSpl * NC]) {
    if (vec && n == kDemodSpl) {
        float4* q = reinterpret_cast<float4*>(row + i0 * NC);
#pragma unroll
        for (int j = 0; j < kDemodSpl * NC / 4; j++) q[j] = make_float4(y[4 * j], y[4 * j + 1], y[4 * j + 2], y[4 * j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < kDemodSpl * NC; j++)
            if (j < n * NC) row[i0 * NC + j] = y[j];
    }
}

}  // namespace qk

namespace qh {

// the demodulator handle (FM, FM stereo, AM, and SSB around an xlator engine); misc_ops.hip's harness helpers take it as the
// StreamOp it begins with (stream_op.h)
constexpr int kDemodSsb = 3;                   // (QDSP_HIP_DEMOD_FM / _FM_STEREO / _AM are 0..2)
struct Demod : StreamOp {
    static constexpr OpKind kKind = OpKind::Demod;
    int kind = 0;
    // FM: carried phase, double-buffered (lanes of one launch read slot cur, the last sample's lane writes cur ^ 1)
    float* d_phase[2] = {nullptr, nullptr};
    int cur = 0;
    float* d_speed = nullptr;
    std::vector<float> rate, dev, speed;
    // AM: FP64 partials
    double* d_part = nullptr;
    // SSB: the NCO state of an xlate_cf32 engine (never launched through the engine itself)
    Engine* nco = nullptr;
};
void launch_fm_mono(const qk::FmArgs& a, int tiles, int nchan, hipStream_t s);

}  // namespace qh
