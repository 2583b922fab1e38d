// TEST-ONLY stand-in for qdsp_amd/csrc/rowfir.hip on the fake synchronous HIP runtime (fake_hip_runtime.cpp), so that psk_check --
// dsp/psk_demod.h over the real qdsp_amd/csrc/psk_chain.cpp and stream_op.cpp -- runs under -fsanitize=address,undefined without a GPU
// (tests/test_psk_cpu.py).  The rowfir / delay_imag entry points with the library's handle plumbing and plain loops for kernels
// (the k-ordered fmaf chain; the one-sample delay of the imaginary part); the batch entry points, resets and the two runtime calls
// that the chain needs and the older fakes (fake_qdsp_hip.cpp, fake_mmcr.cpp, fake_hip_runtime.cpp: unchanged) lack.  "Device"
// memory is host memory here.
#include "../../qdsp_amd/csrc/stream_op.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace qh;

namespace {

struct FakeRowFir : StreamOp {
    static constexpr OpKind kKind = OpKind::RowFir;
    int nc = 1;                         // floats per sample
    int ntaps = 0;
    std::vector<float> taps;            // [nchan][ntaps]
    std::vector<float> hist;            // [nchan][ntaps - 1] samples
};

struct FakeDelay : StreamOp {
    static constexpr OpKind kKind = OpKind::DelayImag;
    std::vector<float> last;            // [nchan]
};

bool spans_overlap(const void* a, int64_t a_stride, const void* b, int64_t b_stride, int nchan, int64_t count, size_t es) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + ((uintptr_t)(nchan - 1) * a_stride + count) * es;
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + ((uintptr_t)(nchan - 1) * b_stride + count) * es;
    return a0 < b1 && b0 < a1;
}

int64_t fir_launch(FakeRowFir* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t) {
    if (count < 0 || in_stride < count || out_stride < count || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (count == 0) return 0;
    const int nc = d->nc, T = d->ntaps, H = T - 1;
    if (spans_overlap(d_in, in_stride, d_out, out_stride, d->nchan, count, nc * sizeof(float))) return QDSP_HIP_EINVAL;
    std::vector<float> x((size_t)(H + count) * nc);
    for (int c = 0; c < d->nchan; c++) {
        const float* in = static_cast<const float*>(d_in) + (size_t)c * in_stride * nc;
        float* out = static_cast<float*>(d_out) + (size_t)c * out_stride * nc;
        if (H) memcpy(x.data(), &d->hist[(size_t)c * H * nc], (size_t)H * nc * sizeof(float));
        memcpy(x.data() + (size_t)H * nc, in, (size_t)count * nc * sizeof(float));
        for (int64_t i = 0; i < count; i++)
            for (int e = 0; e < nc; e++) {
                float acc = 0.0f;
                for (int k = 0; k < T; k++) acc = fmaf(d->taps[(size_t)c * T + k], x[(size_t)(i + k) * nc + e], acc);
                out[(size_t)i * nc + e] = acc;
            }
        if (H) memcpy(&d->hist[(size_t)c * H * nc], x.data() + (size_t)count * nc, (size_t)H * nc * sizeof(float));
    }
    return 0;
}

int64_t delay_launch(FakeDelay* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t) {
    if (count < 0 || in_stride < count || out_stride < count || (count > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (count == 0) return 0;
    if (spans_overlap(d_in, in_stride, d_out, out_stride, d->nchan, count, 2 * sizeof(float))) return QDSP_HIP_EINVAL;
    for (int c = 0; c < d->nchan; c++) {
        const float* in = static_cast<const float*>(d_in) + (size_t)c * in_stride * 2;
        float* out = static_cast<float*>(d_out) + (size_t)c * out_stride * 2;
        for (int64_t i = 0; i < count; i++) {
            out[2 * i] = in[2 * i];
            out[2 * i + 1] = d->last[c];
            d->last[c] = in[2 * i + 1];
        }
    }
    return 0;
}

// (the history keeps its newest samples across a change of the count, as qdsp_hip_fir_cf32_set_taps keeps them)
void install(FakeRowFir* d, const std::vector<float>& taps, int ntaps) {
    if (ntaps != d->ntaps) {
        const int oldH = d->ntaps > 0 ? d->ntaps - 1 : 0, newH = ntaps - 1, keep = oldH < newH ? oldH : newH;
        std::vector<float> nh((size_t)d->nchan * newH * d->nc, 0.0f);
        for (int c = 0; c < d->nchan && keep > 0; c++)
            memcpy(&nh[((size_t)c * newH + (newH - keep)) * d->nc], &d->hist[((size_t)c * oldH + (oldH - keep)) * d->nc], (size_t)keep * d->nc * sizeof(float));
        d->hist.swap(nh);
        d->ntaps = ntaps;
    }
    d->taps = taps;
}

template <class T> void drop(T* d) {
    op_free(d, [] {});
}

}  // namespace

extern "C" {

// ---- the HIP runtime calls psk_chain.cpp makes that fake_hip_runtime.cpp lacks ----
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) {
    *p = calloc(1, n ? n : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) {
    free(p);
    return hipSuccess;
}

// ---- the batch entry points and resets of the stages fake_qdsp_hip.cpp stands in for (its handles are its own: one channel, which
// is what a block graph runs; the operators there copy) ----
int qdsp_hip_cagc_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t, void* d_out, int64_t, void*) {
    return qdsp_hip_cagc_process_ex(h, d_in, QDSP_HIP_LINK_DEVICE, (int)count, d_out, QDSP_HIP_LINK_DEVICE);
}
int qdsp_hip_cagc_reset(void* h) { return qdsp_hip_cagc_process_ex(h, nullptr, QDSP_HIP_LINK_DEVICE, 0, nullptr, QDSP_HIP_LINK_DEVICE); }
int qdsp_hip_costas_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t, void* d_out, int64_t, void*) {
    if (d_in == d_out) count = 0;   // in place: the copy is the identity (and memcpy may not be given one buffer twice)
    return qdsp_hip_costas_process_ex(h, d_in, QDSP_HIP_LINK_DEVICE, (int)count, d_out, QDSP_HIP_LINK_DEVICE);
}
int qdsp_hip_costas_reset(void* h) { return qdsp_hip_costas_process_ex(h, nullptr, QDSP_HIP_LINK_DEVICE, 0, nullptr, QDSP_HIP_LINK_DEVICE); }
int qdsp_hip_demod_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t, void* d_out, int64_t, void*) {
    return qdsp_hip_demod_process_ex(h, d_in, QDSP_HIP_LINK_DEVICE, (int)count, d_out, QDSP_HIP_LINK_DEVICE);
}
int qdsp_hip_demod_reset(void* h) { return qdsp_hip_demod_process_ex(h, nullptr, QDSP_HIP_LINK_DEVICE, 0, nullptr, QDSP_HIP_LINK_DEVICE); }

// ---- RowFir ----
int qdsp_hip_rowfir_tile(void) { return 2048; }
int qdsp_hip_rowfir_tap_group(void) { return 12; }
int qdsp_hip_rowfir_create(void** h, int device, int kind, int nchan, const float* taps, int ntaps, int max_block) {
    FakeRowFir* d = nullptr;
    const bool args_ok = (kind == 0 || kind == 1) && taps && ntaps >= 1 && ntaps <= 4096;
    if (const int rc = op_new<FakeRowFir, fir_launch>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->nc = kind ? 2 : 1;
    const hipError_t err = stream_op_init(d, device, nchan, max_block, d->nc * sizeof(float), d->nc * sizeof(float));
    if (err == hipSuccess) {
        std::vector<float> all((size_t)nchan * ntaps);
        for (int c = 0; c < nchan; c++) memcpy(&all[(size_t)c * ntaps], taps, (size_t)ntaps * sizeof(float));
        install(d, all, ntaps);
    }
    return op_created<drop<FakeRowFir>>(h, d, err);
}
int qdsp_hip_rowfir_set_taps(void* h, int chan, const float* taps, int ntaps) {
    FakeRowFir* d = as<FakeRowFir>(h);
    if (!d || !taps || ntaps < 1 || ntaps > 4096 || (chan != -1 && (!chan_ok(d, chan) || ntaps != d->ntaps))) return QDSP_HIP_EINVAL;
    std::vector<float> all = d->taps;
    if (chan == -1) all.resize((size_t)d->nchan * ntaps);
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++) memcpy(&all[(size_t)c * ntaps], taps, (size_t)ntaps * sizeof(float));
    install(d, all, ntaps);
    return 0;
}
int qdsp_hip_rowfir_ntaps(void* h) {
    FakeRowFir* d = as<FakeRowFir>(h);
    return d ? d->ntaps : QDSP_HIP_EINVAL;
}
int qdsp_hip_rowfir_get_history(void* h, int chan, float* hist) {
    FakeRowFir* d = as<FakeRowFir>(h);
    if (!d || !chan_ok(d, chan) || !hist) return QDSP_HIP_EINVAL;
    const size_t row = (size_t)(d->ntaps - 1) * d->nc;
    if (row) memcpy(hist, &d->hist[chan * row], row * sizeof(float));
    return 0;
}
int qdsp_hip_rowfir_set_history(void* h, int chan, const float* hist) {
    FakeRowFir* d = as<FakeRowFir>(h);
    if (!d || !chan_ok(d, chan) || !hist) return QDSP_HIP_EINVAL;
    const size_t row = (size_t)(d->ntaps - 1) * d->nc;
    if (row) memcpy(&d->hist[chan * row], hist, row * sizeof(float));
    return 0;
}
int qdsp_hip_rowfir_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<FakeRowFir>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_rowfir_process(void* h, const float* in, int count, float* out) {
    return qdsp_hip_rowfir_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_rowfir_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                      void* hip_stream) {
    return op_process_batch_dev<FakeRowFir, fir_launch>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_rowfir_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<FakeRowFir, fir_launch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_rowfir_reset(void* h) {
    FakeRowFir* d = as<FakeRowFir>(h);
    if (!d) return QDSP_HIP_EINVAL;
    d->hist.assign(d->hist.size(), 0.0f);
    return 0;
}
void qdsp_hip_rowfir_destroy(void* h) { drop(as<FakeRowFir>(h)); }

// ---- DelayImag ----
int qdsp_hip_delay_imag_create(void** h, int device, int nchan, int max_block) {
    FakeDelay* d = nullptr;
    if (const int rc = op_new<FakeDelay, delay_launch>(&d, h, true, device, nchan, max_block)) return rc;
    d->last.assign((size_t)nchan, 0.0f);
    return op_created<drop<FakeDelay>>(h, d, stream_op_init(d, device, nchan, max_block, 2 * sizeof(float), 2 * sizeof(float)));
}
int qdsp_hip_delay_imag_get_state(void* h, int chan, float* last_im) {
    FakeDelay* d = as<FakeDelay>(h);
    if (!d || !chan_ok(d, chan) || !last_im) return QDSP_HIP_EINVAL;
    *last_im = d->last[chan];
    return 0;
}
int qdsp_hip_delay_imag_set_state(void* h, int chan, float last_im) {
    FakeDelay* d = as<FakeDelay>(h);
    if (!d || (chan != -1 && !chan_ok(d, chan))) return QDSP_HIP_EINVAL;
    for (int c = chan_first(chan), c1 = c + chan_count(d, chan); c < c1; c++) d->last[c] = last_im;
    return 0;
}
int qdsp_hip_delay_imag_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<FakeDelay>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_delay_imag_process(void* h, const float* in_iq, int count, float* out_iq) {
    return qdsp_hip_delay_imag_process_ex(h, in_iq, QDSP_HIP_LINK_HOST, count, out_iq, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_delay_imag_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                          void* hip_stream) {
    return op_process_batch_dev<FakeDelay, delay_launch>(h, d_in, count, in_stride, d_out, out_stride, hip_stream);
}
int qdsp_hip_delay_imag_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_dev<FakeDelay, delay_launch>(h, d_in, count, d_out, hip_stream);
}
int qdsp_hip_delay_imag_reset(void* h) {
    FakeDelay* d = as<FakeDelay>(h);
    if (!d) return QDSP_HIP_EINVAL;
    d->last.assign(d->last.size(), 0.0f);
    return 0;
}
void qdsp_hip_delay_imag_destroy(void* h) { drop(as<FakeDelay>(h)); }

}  // extern "C"
