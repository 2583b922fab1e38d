// TEST-ONLY stand-in for qdsp_amd/csrc/mmcr.hip on the fake synchronous HIP runtime (fake_hip_runtime.cpp), so that clock_check --
// dsp/clock_recovery.h over the real qdsp_amd/csrc/stream_op.cpp -- runs under -fsanitize=address,undefined without a GPU
// (tests/test_mmcr_cpu.py).  Same C entry points and the same handle plumbing as the library's (the out_count hook, the count read
// after the shared path has waited, the refused output links); the "kernel" emits every floor(omega)-th sample of the stream,
// whatever the call cuts.  "Device" memory is host memory here.
#include "../../qdsp_amd/csrc/stream_op.h"

#include <math.h>
#include <string.h>

using namespace qh;

namespace {

struct FakeMmcr : StreamOp {
    static constexpr OpKind kKind = OpKind::Mmcr;
    int kind = 0;
    float omega = 2.0f, gain_omega = 0.0f, mu_gain = 0.0f, rel = 0.0f;
    int64_t next = 0;          // samples from the start of the next call to the next symbol
    int last_count = 0;
    float taps[1032] = {};
};

bool rule(float omega, float gain_omega, float mu_gain, float rel) {
    if (!isfinite(omega) || !isfinite(gain_omega) || !isfinite(mu_gain) || !isfinite(rel)) return false;
    if (!(omega > 0.0f) || !(rel >= 0.0f) || !(rel < 1.0f)) return false;
    const float lo = omega - (omega * rel), hi = omega + (omega * rel);
    return lo - fabsf(mu_gain) >= 1.0f && hi + fabsf(mu_gain) < 1048576.0f;
}

int64_t step_of(const FakeMmcr* d) { return (int64_t)floorf(d->omega); }
int64_t min_step_of(const FakeMmcr* d) { return (int64_t)floorf((d->omega - (d->omega * d->rel)) - fabsf(d->mu_gain)); }
int64_t out_size_of(const FakeMmcr* d, int64_t count) { return count <= 0 ? 0 : (count + min_step_of(d) - 1) / min_step_of(d); }
int64_t out_count(const StreamOp* op, int64_t count) { return out_size_of(static_cast<const FakeMmcr*>(op), count); }

int64_t fake_launch(FakeMmcr* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t) {
    if (count < 0 || in_stride < count || out_stride < out_size_of(d, count) || (count > 0 && (!d_in || !d_out || d_in == d_out))) return QDSP_HIP_EINVAL;
    const size_t es = d->in_es;
    int n = 0;
    int64_t i = d->next;
    for (; i < count; i += step_of(d)) {
        if (n >= out_stride) return QDSP_HIP_EINVAL;
        memcpy(static_cast<char*>(d_out) + (size_t)n * es, static_cast<const char*>(d_in) + (size_t)i * es, es);
        n++;
    }
    d->next = i - count;
    d->last_count = n;
    return 0;
}

void drop(FakeMmcr* d) {
    op_free(d, [] {});
}

int set(FakeMmcr* d, int chan, float omega, float gain_omega, float mu_gain, float rel) {
    if (!d || (chan != -1 && chan != 0) || !rule(omega, gain_omega, mu_gain, rel)) return QDSP_HIP_EINVAL;
    d->omega = omega;
    d->gain_omega = gain_omega;
    d->mu_gain = mu_gain;
    d->rel = rel;
    return 0;
}

}  // namespace

extern "C" {

int qdsp_hip_mmcr_create(void** h, int device, int kind, int nchan, int max_block, float omega, float gain_omega, float mu_gain,
                         float rel_limit) {
    FakeMmcr* d = nullptr;
    const bool args_ok = (kind == 0 || kind == 1) && nchan == 1 && rule(omega, gain_omega, mu_gain, rel_limit);
    if (const int rc = op_new<FakeMmcr, fake_launch, out_count>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->kind = kind;
    (void)set(d, 0, omega, gain_omega, mu_gain, rel_limit);
    const size_t es = kind ? 8 : 4;
    return op_created<drop>(h, d, stream_op_init(d, device, nchan, max_block, es, es));
}
int qdsp_hip_mmcr_set_omega(void* h, int chan, float omega) {
    FakeMmcr* d = as<FakeMmcr>(h);
    return d ? set(d, chan, omega, d->gain_omega, d->mu_gain, d->rel) : QDSP_HIP_EINVAL;
}
int qdsp_hip_mmcr_set_gains(void* h, int chan, float gain_omega, float mu_gain) {
    FakeMmcr* d = as<FakeMmcr>(h);
    return d ? set(d, chan, d->omega, gain_omega, mu_gain, d->rel) : QDSP_HIP_EINVAL;
}
int qdsp_hip_mmcr_set_limit(void* h, int chan, float rel_limit) {
    FakeMmcr* d = as<FakeMmcr>(h);
    return d ? set(d, chan, d->omega, d->gain_omega, d->mu_gain, rel_limit) : QDSP_HIP_EINVAL;
}
int qdsp_hip_mmcr_get_state(void* h, int chan, float* mu, float* dyn_omega, int* next) {
    FakeMmcr* d = as<FakeMmcr>(h);
    if (!d || chan != 0 || !mu || !dyn_omega || !next) return QDSP_HIP_EINVAL;
    *mu = 0.5f;
    *dyn_omega = d->omega;
    *next = (int)d->next;
    return 0;
}
int qdsp_hip_mmcr_set_state(void* h, int chan, float mu, float dyn_omega, int next) {
    FakeMmcr* d = as<FakeMmcr>(h);
    if (!d || (chan != -1 && chan != 0) || !(mu >= 0.0f && mu < 1.0f) || !isfinite(dyn_omega) || next < 0) return QDSP_HIP_EINVAL;
    d->next = next;
    return 0;
}
int64_t qdsp_hip_mmcr_out_size(void* h, int64_t count) {
    FakeMmcr* d = as<FakeMmcr>(h);
    return (d && count >= 0) ? out_size_of(d, count) : QDSP_HIP_EINVAL;
}
int qdsp_hip_mmcr_get_interp_taps(void* h, float* taps) {
    FakeMmcr* d = as<FakeMmcr>(h);
    if (!d || !taps) return QDSP_HIP_EINVAL;
    memcpy(taps, d->taps, sizeof(d->taps));
    return 0;
}
int qdsp_hip_mmcr_set_interp_taps(void* h, const float* taps) {
    FakeMmcr* d = as<FakeMmcr>(h);
    if (!d || !taps) return QDSP_HIP_EINVAL;
    memcpy(d->taps, taps, sizeof(d->taps));
    return 0;
}
int qdsp_hip_mmcr_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                    int* d_counts, void* hip_stream) {
    FakeMmcr* d = as<FakeMmcr>(h);
    if (!d) return QDSP_HIP_EINVAL;
    const int rc = (int)fake_launch(d, d_in, count, in_stride, d_out, out_stride, static_cast<hipStream_t>(hip_stream));
    if (rc == 0 && d_counts) d_counts[0] = d->last_count;
    return rc;
}
int qdsp_hip_mmcr_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    FakeMmcr* d = as<FakeMmcr>(h);
    return d ? qdsp_hip_mmcr_process_batch_dev(h, d_in, count, count, d_out, out_size_of(d, count), nullptr, hip_stream) : QDSP_HIP_EINVAL;
}
int qdsp_hip_mmcr_get_counts(void* h, int* counts) {
    FakeMmcr* d = as<FakeMmcr>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    counts[0] = d->last_count;
    return 0;
}
int qdsp_hip_mmcr_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    FakeMmcr* d = as<FakeMmcr>(h);
    if (!d || (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE)) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, count, out, out_link);
    if (rc < 0 || count == 0) return (int)rc;
    return d->last_count;
}
int qdsp_hip_mmcr_process(void* h, const float* in, int count, float* out) {
    return qdsp_hip_mmcr_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_mmcr_reset(void* h) {
    FakeMmcr* d = as<FakeMmcr>(h);
    if (!d) return QDSP_HIP_EINVAL;
    d->next = 0;
    d->last_count = 0;
    return 0;
}
void qdsp_hip_mmcr_destroy(void* h) { drop(as<FakeMmcr>(h)); }

}  // extern "C"
