// psk_chain.cpp -- PSKDemod<ORDER, OFFSET> and MSKDemod (src/dsp/demodulator.h:499-682) as one handle over nchan channel rows.
// Host code only, no kernels: a chain is a StreamOp that owns one handle of each stage, created through the public C ABI
// (include/qdsp_hip.h), and calls their *_process_batch_dev on the call's stream, one after the other:
//   PSK   cagc (set point 1, max gain 65535) -> rowfir kind 1 (the RRC taps) -> costas, in place -> [delay_imag] -> mmcr kind 1
//   MSK   demod QDSP_HIP_DEMOD_FM -> mmcr kind 0
// Every intermediate stays in two library-owned scratch row sets ([nchan][sstride] samples, rows 16-byte aligned), ping-ponged
// between the stages:  in -> A (cagc) -> B (rowfir; costas in place) -> [A (delay_imag)] -> out (mmcr).  They grow to the largest
// call seen as StereoFm's do: wait for the device, then reallocate.  The stage handles are made with max_block 1: they never see a
// host pointer.  The symbol counts go to the chain's own device array and, for one channel, on to pinned memory, which
// process_ex reads once the shared host path has waited.
#include "stream_op.h"

namespace qh {

namespace {

constexpr int kMaxStages = 5;

struct Chain : StreamOp {
    static constexpr OpKind kKind = OpKind::Chain;
    bool msk = false;
    bool offset = false;
    void* stage[kMaxStages] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // PSK: agc, rrc, costas, delay, clock; MSK: fm, clock
    void* d_rows[2] = {nullptr, nullptr};          // scratch row sets A and B
    long long scratch_cap = 0;                     // samples per row
    long long last_count = 0, last_sstride = 0;
    int* d_counts = nullptr;                       // [nchan] symbols of the last call
    int* h_count = nullptr;                        // pinned: row 0's count of the last process_ex call
};

Chain* as_chain(void* h, bool msk) {
    Chain* d = as<Chain>(h);
    return (d && d->msk == msk) ? d : nullptr;
}

void* clock_of(const Chain* d) { return d->stage[d->msk ? QDSP_HIP_MSK_CLOCK : QDSP_HIP_PSK_CLOCK]; }
size_t scratch_es(const Chain* d) { return d->msk ? sizeof(float) : 2 * sizeof(float); }

void free_scratch(Chain* d) {
    for (void*& p : d->d_rows) {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    d->scratch_cap = 0;
}

hipError_t alloc_scratch(Chain* d, long long cap) {
    const int sets = d->msk ? 1 : 2;
    hipError_t err = hipSuccess;
    for (int i = 0; i < sets && err == hipSuccess; i++) err = hipMalloc(&d->d_rows[i], (size_t)d->nchan * (size_t)cap * scratch_es(d));
    if (err == hipSuccess) d->scratch_cap = cap;
    else free_scratch(d);
    return err;
}

void chain_free(Chain* d) {
    op_free(d, [d] {
        if (d->msk) {
            qdsp_hip_demod_destroy(d->stage[QDSP_HIP_MSK_FM]);
            qdsp_hip_mmcr_destroy(d->stage[QDSP_HIP_MSK_CLOCK]);
        } else {
            qdsp_hip_cagc_destroy(d->stage[QDSP_HIP_PSK_AGC]);
            qdsp_hip_rowfir_destroy(d->stage[QDSP_HIP_PSK_RRC]);
            qdsp_hip_costas_destroy(d->stage[QDSP_HIP_PSK_COSTAS]);
            qdsp_hip_delay_imag_destroy(d->stage[QDSP_HIP_PSK_DELAY]);
            qdsp_hip_mmcr_destroy(d->stage[QDSP_HIP_PSK_CLOCK]);
        }
        free_scratch(d);
        if (d->d_counts) (void)hipFree(d->d_counts);
        if (d->h_count) (void)hipHostFree(d->h_count);
    });
}

int64_t chain_out_size(const Chain* d, int64_t count) { return qdsp_hip_mmcr_out_size(clock_of(d), count); }
int64_t chain_out_count(const StreamOp* op, int64_t count) { return chain_out_size(static_cast<const Chain*>(op), count); }

// d_in: nchan rows of `count` complex samples, in_stride apart; d_out: rows of at least out_size(count) symbols, out_stride apart
int chain_launch(Chain* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    if (count < 0 || (count > 0 && (!d_in || !d_out)) || in_stride < count) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    void* clock = clock_of(d);
    if (count == 0) {   // no stage's state moves; the clock stage clears the counts
        if (const int rc = qdsp_hip_mmcr_process_batch_dev(clock, nullptr, 0, 0, nullptr, 0, d->d_counts, s)) return rc;
        return 0;
    }
    const long long sstride = ((long long)count + 3) & ~3LL;
    if (sstride > d->scratch_cap) {   // a larger call than any before: the scratch rows grow (nothing of ours is in flight after the wait)
        HIPCHK(hipDeviceSynchronize());
        free_scratch(d);
        HIPCHK(alloc_scratch(d, sstride));
    }
    void *A = d->d_rows[0], *B = d->d_rows[1];
    const void* sym_in = A;
    int rc = 0;
    if (d->msk) {
        rc = qdsp_hip_demod_process_batch_dev(d->stage[QDSP_HIP_MSK_FM], d_in, count, in_stride, A, sstride, s);
    } else {
        rc = qdsp_hip_cagc_process_batch_dev(d->stage[QDSP_HIP_PSK_AGC], d_in, count, in_stride, A, sstride, s);
        if (!rc) rc = qdsp_hip_rowfir_process_batch_dev(d->stage[QDSP_HIP_PSK_RRC], A, count, sstride, B, sstride, s);
        if (!rc) rc = qdsp_hip_costas_process_batch_dev(d->stage[QDSP_HIP_PSK_COSTAS], B, count, sstride, B, sstride, s);
        sym_in = B;
        if (!rc && d->offset) {
            rc = qdsp_hip_delay_imag_process_batch_dev(d->stage[QDSP_HIP_PSK_DELAY], B, count, sstride, A, sstride, s);
            sym_in = A;
        }
    }
    if (!rc) rc = qdsp_hip_mmcr_process_batch_dev(clock, sym_in, count, sstride, d_out, out_stride, d->d_counts, s);
    // (a stage that refuses after an earlier one has run leaves the chain's stages out of step: reset it.  The arguments are
    // checked above and the clock stage's own -- out_stride, alignment of d_out -- cannot be known before it is asked.)
    if (rc) return rc;
    if (d->nchan == 1) HIPCHK(hipMemcpyAsync(d->h_count, d->d_counts, sizeof(int), hipMemcpyDeviceToHost, s));   // process_ex reads it
    d->last_count = count;
    d->last_sstride = sstride;
    if (const StreamOp* c = as_stream_op(clock)) d->last = c->last;   // qdsp_hip_last_kernel: the clock stage's launch
    return 0;
}

// the head of both creates; the stages follow
int chain_new(Chain** out, void** h, bool args_ok, int device, int nchan, int max_block, bool msk, bool offset) {
    Chain* d = nullptr;
    if (const int rc = op_new<Chain, chain_launch, chain_out_count>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->msk = msk;
    d->offset = offset;
    const size_t out_es = msk ? sizeof(float) : 2 * sizeof(float);
    hipError_t err = stream_op_init(d, device, nchan, max_block, 2 * sizeof(float), out_es);
    d->nchan = nchan;
    if (err == hipSuccess) err = hipMalloc(&d->d_counts, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipMemset(d->d_counts, 0, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipHostMalloc(reinterpret_cast<void**>(&d->h_count), sizeof(int), hipHostMallocDefault);
    if (err != hipSuccess) {
        chain_free(d);
        return -(int)err;
    }
    *d->h_count = 0;
    *out = d;
    return 0;
}

// after the stages: the scratch rows of a handle with a host path.  Whatever fails, nothing stays allocated.
int chain_finish(Chain* d, int rc, void** h) {
    if (!rc && d->max_block > 0) {
        const hipError_t err = alloc_scratch(d, ((long long)d->max_block + 3) & ~3LL);
        if (err != hipSuccess) rc = -(int)err;
    }
    return op_created<chain_free>(h, d, rc);
}

int chain_stage(Chain* d, int which, void** stage) {
    const int n = d->msk ? 2 : kMaxStages;
    if (!stage || which < 0 || which >= n || !d->stage[which]) return QDSP_HIP_EINVAL;
    *stage = d->stage[which];
    return 0;
}

int chain_tap(Chain* d, int which, void** d_rows, int64_t* stride) {
    if (!d_rows || !stride) return QDSP_HIP_EINVAL;
    int set = -1;
    if (d->msk) {
        if (which != QDSP_HIP_MSK_FM) return QDSP_HIP_EINVAL;
        set = 0;
    } else {
        switch (which) {
            case QDSP_HIP_PSK_AGC: set = d->offset ? -1 : 0; break;   // (an offset chain's delay stage has reused these rows)
            case QDSP_HIP_PSK_RRC: set = -1; break;                   // (the Costas loop has run over them in place)
            case QDSP_HIP_PSK_COSTAS: set = 1; break;
            case QDSP_HIP_PSK_DELAY:
                if (!d->offset) return QDSP_HIP_EINVAL;
                set = 0;
                break;
            default: return QDSP_HIP_EINVAL;
        }
    }
    *d_rows = (set >= 0 && d->last_count > 0) ? d->d_rows[set] : nullptr;
    *stride = d->last_sstride;
    return 0;
}

int chain_process_ex(Chain* d, const void* in, int in_link, int count, void* out, int out_link) {
    // the count is returned, so the call has to have run: an output link that hands over without waiting cannot be served
    if (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, count, out, out_link);
    if (rc < 0 || count == 0) return (int)rc;
    return *d->h_count;
}

int chain_batch(Chain* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, int* d_counts, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = chain_launch(d, d_in, count, in_stride, d_out, out_stride, s)) return rc;
    if (d_counts) HIPCHK(hipMemcpyAsync(d_counts, d->d_counts, (size_t)d->nchan * sizeof(int), hipMemcpyDeviceToDevice, s));
    return 0;
}

int chain_reset(Chain* d) {
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    int rc = 0;
    if (d->msk) {
        rc = qdsp_hip_demod_reset(d->stage[QDSP_HIP_MSK_FM]);
    } else {
        rc = qdsp_hip_cagc_reset(d->stage[QDSP_HIP_PSK_AGC]);
        if (!rc) rc = qdsp_hip_rowfir_reset(d->stage[QDSP_HIP_PSK_RRC]);
        if (!rc) rc = qdsp_hip_costas_reset(d->stage[QDSP_HIP_PSK_COSTAS]);
        if (!rc && d->offset) rc = qdsp_hip_delay_imag_reset(d->stage[QDSP_HIP_PSK_DELAY]);
    }
    if (!rc) rc = qdsp_hip_mmcr_reset(clock_of(d));
    if (!rc) HIPCHK(hipMemset(d->d_counts, 0, (size_t)d->nchan * sizeof(int)));
    return rc;
}

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_psk_create(void** h, int device, int order, int offset, int nchan, int max_block, const float* rrc_taps, int ntaps,
                        float agc_rate, float costas_bw, float omega, float gain_omega, float mu_gain, float rel_limit) {
    const bool args_ok = (order == 2 || order == 4 || order == 8) && (offset == 0 || offset == 1) && rrc_taps;
    Chain* d = nullptr;
    if (const int rc = chain_new(&d, h, args_ok, device, nchan, max_block, false, offset != 0)) return rc;
    int rc = qdsp_hip_cagc_create(&d->stage[QDSP_HIP_PSK_AGC], device, nchan, 1);
    if (!rc) rc = qdsp_hip_cagc_set(d->stage[QDSP_HIP_PSK_AGC], -1, 1.0f, 65535, agc_rate);   // PSKDemod::init
    if (!rc) rc = qdsp_hip_rowfir_create(&d->stage[QDSP_HIP_PSK_RRC], device, 1, nchan, rrc_taps, ntaps, 1);
    if (!rc) rc = qdsp_hip_costas_create(&d->stage[QDSP_HIP_PSK_COSTAS], device, order, nchan, 1);
    if (!rc) rc = qdsp_hip_costas_set_bandwidth(d->stage[QDSP_HIP_PSK_COSTAS], -1, costas_bw);
    if (!rc && offset) rc = qdsp_hip_delay_imag_create(&d->stage[QDSP_HIP_PSK_DELAY], device, nchan, 1);
    if (!rc) rc = qdsp_hip_mmcr_create(&d->stage[QDSP_HIP_PSK_CLOCK], device, 1, nchan, 1, omega, gain_omega, mu_gain, rel_limit);
    return chain_finish(d, rc, h);
}
int qdsp_hip_msk_create(void** h, int device, int nchan, int max_block, float sample_rate, float deviation, float omega,
                        float gain_omega, float mu_gain, float rel_limit) {
    Chain* d = nullptr;
    if (const int rc = chain_new(&d, h, true, device, nchan, max_block, true, false)) return rc;
    int rc = qdsp_hip_demod_create(&d->stage[QDSP_HIP_MSK_FM], device, QDSP_HIP_DEMOD_FM, nchan, 1);
    if (!rc) rc = qdsp_hip_demod_set_fm(d->stage[QDSP_HIP_MSK_FM], -1, sample_rate, deviation);
    if (!rc) rc = qdsp_hip_mmcr_create(&d->stage[QDSP_HIP_MSK_CLOCK], device, 0, nchan, 1, omega, gain_omega, mu_gain, rel_limit);
    return chain_finish(d, rc, h);
}

#define QDSP_CHAIN_ENTRY_POINTS(name, is_msk)                                                                                       \
    int qdsp_hip_##name##_stage(void* h, int which, void** stage) {                                                                 \
        Chain* d = as_chain(h, is_msk);                                                                                             \
        return d ? chain_stage(d, which, stage) : QDSP_HIP_EINVAL;                                                                  \
    }                                                                                                                               \
    int qdsp_hip_##name##_tap_dev(void* h, int which, void** d_rows, int64_t* stride) {                                             \
        Chain* d = as_chain(h, is_msk);                                                                                             \
        return d ? chain_tap(d, which, d_rows, stride) : QDSP_HIP_EINVAL;                                                           \
    }                                                                                                                               \
    int64_t qdsp_hip_##name##_out_size(void* h, int64_t count) {                                                                    \
        Chain* d = as_chain(h, is_msk);                                                                                             \
        return (d && count >= 0) ? chain_out_size(d, count) : QDSP_HIP_EINVAL;                                                      \
    }                                                                                                                               \
    int qdsp_hip_##name##_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {                    \
        Chain* d = as_chain(h, is_msk);                                                                                             \
        return d ? chain_process_ex(d, in, in_link, count, out, out_link) : QDSP_HIP_EINVAL;                                        \
    }                                                                                                                               \
    int qdsp_hip_##name##_process(void* h, const float* in_iq, int count, float* out) {                                             \
        return qdsp_hip_##name##_process_ex(h, in_iq, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);                          \
    }                                                                                                                               \
    int qdsp_hip_##name##_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {                    \
        Chain* d = as_chain(h, is_msk);                                                                                             \
        return d ? chain_batch(d, d_in, count, count, d_out, chain_out_size(d, count), nullptr, hip_stream) : QDSP_HIP_EINVAL;      \
    }                                                                                                                               \
    int qdsp_hip_##name##_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out,               \
                                            int64_t out_stride, int* d_counts, void* hip_stream) {                                  \
        Chain* d = as_chain(h, is_msk);                                                                                             \
        return d ? chain_batch(d, d_in, count, in_stride, d_out, out_stride, d_counts, hip_stream) : QDSP_HIP_EINVAL;               \
    }                                                                                                                               \
    int qdsp_hip_##name##_get_counts(void* h, int* counts) {                                                                        \
        Chain* d = as_chain(h, is_msk);                                                                                             \
        return (d && counts) ? sync_download(d, counts, d->d_counts, (size_t)d->nchan * sizeof(int)) : QDSP_HIP_EINVAL;             \
    }                                                                                                                               \
    int qdsp_hip_##name##_reset(void* h) {                                                                                          \
        Chain* d = as_chain(h, is_msk);                                                                                             \
        return d ? chain_reset(d) : QDSP_HIP_EINVAL;                                                                                \
    }                                                                                                                               \
    void qdsp_hip_##name##_destroy(void* h) { chain_free(as_chain(h, is_msk)); }

QDSP_CHAIN_ENTRY_POINTS(psk, false)
QDSP_CHAIN_ENTRY_POINTS(msk, true)

}  // extern "C"
