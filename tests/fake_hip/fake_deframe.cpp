// TEST-ONLY stand-in for qdsp_amd/csrc/deframe.hip on the fake synchronous HIP runtime (fake_hip_runtime.cpp), so that frame_check --
// dsp/deframing.h and dsp::Threshold over the real qdsp_amd/csrc/stream_op.cpp -- runs under -fsanitize=address,undefined without a
// GPU (tests/test_deframer_cpu.py).  Same C entry points and the same handle plumbing as the library's (the out_count hook, the count
// read after the shared path has waited, the refused output links); the "kernels" are the reference's plain loops: one compare per
// float, and the per-bit state machine over a work buffer of the last sync_len bytes and the call's.  One channel.  "Device" memory
// is host memory here.
#include "../../qdsp_amd/csrc/stream_op.h"

#include <string.h>

#include <new>
#include <vector>

using namespace qh;

namespace {

struct FakeThreshold : StreamOp {
    static constexpr OpKind kKind = OpKind::Threshold;
};

int64_t thr_launch(FakeThreshold* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t) {
    if (count < 0 || in_stride < count || out_stride < count || (count > 0 && (!d_in || !d_out || d_in == d_out))) return QDSP_HIP_EINVAL;
    const float* x = static_cast<const float*>(d_in);
    uint8_t* y = static_cast<uint8_t*>(d_out);
    for (int64_t i = 0; i < count; i++) y[i] = x[i] > 0.0f;
    return 0;
}

struct FakeDeframer : StreamOp {
    static constexpr OpKind kKind = OpKind::Deframer;
    int kind = 0, frame_len = 1, frame_bytes = 1;
    std::vector<uint8_t> sync, tail, cur;
    int bits_read = -1, bad = 5;
    bool after = false;
    int last_count = 0;
};
template <class T> void drop(T* d) {
    op_free(d, [] {});
}

int64_t out_size_of(const FakeDeframer* d, int64_t count) { return count <= 0 ? 0 : (count + d->frame_len - 1) / d->frame_len; }
int64_t out_count(const StreamOp* op, int64_t count) {
    const FakeDeframer* d = static_cast<const FakeDeframer*>(op);
    return out_size_of(d, count) * d->frame_bytes;
}

int64_t df_launch(FakeDeframer* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t) {
    if (count < 0 || in_stride < count || out_stride < out_count(d, count) || (count > 0 && (!d_in || !d_out || d_in == d_out))) return QDSP_HIP_EINVAL;
    const size_t L = d->sync.size();
    std::vector<uint8_t> buf(d->tail);
    buf.resize(L + (size_t)count);
    for (int64_t i = 0; i < count; i++)
        buf[L + (size_t)i] = d->kind ? (uint8_t)(static_cast<const float*>(d_in)[i] > 0.0f) : static_cast<const uint8_t*>(d_in)[i];
    uint8_t* out = static_cast<uint8_t*>(d_out);
    int nf = 0;
    for (int64_t i = 0; i < count;) {
        if (d->bits_read >= 0) {
            if (d->bits_read % 8 == 0) d->cur[(size_t)d->bits_read / 8] = 0;
            d->cur[(size_t)d->bits_read / 8] |= (uint8_t)((unsigned)buf[(size_t)i] << (7 - d->bits_read % 8));
            i++;
            d->bits_read++;
            if (d->bits_read >= d->frame_len) {
                if ((int64_t)(nf + 1) * d->frame_bytes > out_stride) return QDSP_HIP_EINVAL;
                memcpy(out + (size_t)nf * d->frame_bytes, d->cur.data(), (size_t)d->frame_bytes);
                nf++;
                d->bits_read = -1;
                d->after = true;
            }
            continue;
        } else if (memcmp(buf.data() + i, d->sync.data(), L) == 0) {
            d->bits_read = 0;
            d->bad = 0;
            d->after = false;
            continue;
        } else if (d->after) {
            d->after = false;
            if (d->bad < 5) {
                d->bad++;
                d->bits_read = 0;
                continue;
            }
        } else {
            i++;
        }
        d->after = false;
    }
    d->tail.assign(buf.begin() + count, buf.end());
    d->last_count = nf;
    return 0;
}

void df_reset(FakeDeframer* d) {
    d->tail.assign(d->sync.size(), 0);
    d->cur.assign((size_t)d->frame_bytes, 0);
    d->bits_read = -1;
    d->bad = 5;
    d->after = false;
    d->last_count = 0;
}

}  // namespace

extern "C" {

int qdsp_hip_threshold_create(void** h, int device, int nchan, int max_block) {
    FakeThreshold* d = nullptr;
    if (const int rc = op_new<FakeThreshold, thr_launch>(&d, h, nchan == 1, device, nchan, max_block)) return rc;
    return op_created<drop<FakeThreshold>>(h, d, stream_op_init(d, device, nchan, max_block, sizeof(float), 1));
}
int qdsp_hip_threshold_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<FakeThreshold>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_threshold_process(void* h, const float* in, int count, uint8_t* out) {
    return qdsp_hip_threshold_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_threshold_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, const int* d_in_counts, void* d_out,
                                         int64_t out_stride, void* hip_stream) {
    FakeThreshold* d = as<FakeThreshold>(h);
    if (!d) return QDSP_HIP_EINVAL;
    const int64_t n = d_in_counts ? (d_in_counts[0] < 0 ? 0 : (d_in_counts[0] < count ? d_in_counts[0] : count)) : count;
    if (in_stride < count || out_stride < count) return QDSP_HIP_EINVAL;
    return (int)thr_launch(d, d_in, n, in_stride, d_out, out_stride, static_cast<hipStream_t>(hip_stream));
}
int qdsp_hip_threshold_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return qdsp_hip_threshold_process_batch_dev(h, d_in, count, count, nullptr, d_out, count, hip_stream);
}
void qdsp_hip_threshold_destroy(void* h) { drop(as<FakeThreshold>(h)); }
int qdsp_hip_threshold_span(void) { return 4096; }

int qdsp_hip_deframer_create(void** h, int device, int kind, int nchan, int max_block, int frame_len, const uint8_t* sync, int sync_len) {
    FakeDeframer* d = nullptr;
    const bool args_ok = (kind == 0 || kind == 1) && nchan == 1 && frame_len >= 1 && frame_len <= (1 << 20) && sync && sync_len >= 1 && sync_len <= 256;
    if (const int rc = op_new<FakeDeframer, df_launch, out_count>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->kind = kind;
    d->frame_len = frame_len;
    d->frame_bytes = (frame_len + 7) / 8;
    d->sync.assign(sync, sync + sync_len);
    df_reset(d);
    hipError_t err = stream_op_init(d, device, nchan, max_block, kind ? sizeof(float) : 1, 1);
    if (err == hipSuccess && max_block > 0) {
        (void)hipFree(d->d_out);
        d->d_out = nullptr;
        err = hipMalloc(&d->d_out, (size_t)out_count(d, max_block));
    }
    return op_created<drop<FakeDeframer>>(h, d, err);
}
int qdsp_hip_deframer_set_sync(void* h, const uint8_t* sync, int sync_len) {
    FakeDeframer* d = as<FakeDeframer>(h);
    if (!d || !sync || sync_len != (int)d->sync.size()) return QDSP_HIP_EINVAL;
    d->sync.assign(sync, sync + sync_len);
    return 0;
}
int qdsp_hip_deframer_get_state(void* h, int chan, int* bits_read, int* bad, int* after) {
    FakeDeframer* d = as<FakeDeframer>(h);
    if (!d || chan != 0 || !bits_read || !bad || !after) return QDSP_HIP_EINVAL;
    *bits_read = d->bits_read;
    *bad = d->bad;
    *after = d->after && d->bits_read < 0;
    return 0;
}
int qdsp_hip_deframer_set_state(void* h, int chan, int bits_read, int bad, int after) {
    FakeDeframer* d = as<FakeDeframer>(h);
    if (!d || (chan != -1 && chan != 0) || bits_read < -1 || bits_read >= d->frame_len || bad < 0 || bad > 5 || (after != 0 && after != 1) ||
        (bits_read >= 0 && after))
        return QDSP_HIP_EINVAL;
    d->bits_read = bits_read;
    d->bad = bad;
    d->after = after != 0;
    return 0;
}
int64_t qdsp_hip_deframer_out_size(void* h, int64_t count) {
    FakeDeframer* d = as<FakeDeframer>(h);
    return (d && count >= 0) ? out_size_of(d, count) : QDSP_HIP_EINVAL;
}
int qdsp_hip_deframer_frame_bytes(void* h) {
    FakeDeframer* d = as<FakeDeframer>(h);
    return d ? d->frame_bytes : QDSP_HIP_EINVAL;
}
int qdsp_hip_deframer_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, const int* d_in_counts, void* d_out,
                                        int64_t out_stride_bytes, int* d_counts, void* hip_stream) {
    FakeDeframer* d = as<FakeDeframer>(h);
    if (!d || count < 0 || in_stride < count || out_stride_bytes < out_count(d, count)) return QDSP_HIP_EINVAL;
    const int64_t n = d_in_counts ? (d_in_counts[0] < 0 ? 0 : (d_in_counts[0] < count ? d_in_counts[0] : count)) : count;
    d->last_count = 0;
    const int rc = n > 0 ? (int)df_launch(d, d_in, n, in_stride, d_out, out_stride_bytes, static_cast<hipStream_t>(hip_stream)) : 0;
    if (rc == 0 && d_counts) d_counts[0] = d->last_count;
    return rc;
}
int qdsp_hip_deframer_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    FakeDeframer* d = as<FakeDeframer>(h);
    return d ? qdsp_hip_deframer_process_batch_dev(h, d_in, count, count, nullptr, d_out, out_count(d, count), nullptr, hip_stream) : QDSP_HIP_EINVAL;
}
int qdsp_hip_deframer_get_counts(void* h, int* counts) {
    FakeDeframer* d = as<FakeDeframer>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    counts[0] = d->last_count;
    return 0;
}
int qdsp_hip_deframer_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    FakeDeframer* d = as<FakeDeframer>(h);
    if (!d || (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE)) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, count, out, out_link);
    if (rc < 0 || count == 0) return (int)rc;
    return d->last_count;
}
int qdsp_hip_deframer_process(void* h, const void* in, int count, uint8_t* out) {
    return qdsp_hip_deframer_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_deframer_reset(void* h) {
    FakeDeframer* d = as<FakeDeframer>(h);
    if (!d) return QDSP_HIP_EINVAL;
    df_reset(d);
    return 0;
}
void qdsp_hip_deframer_destroy(void* h) { drop(as<FakeDeframer>(h)); }
int qdsp_hip_deframer_tile(void) { return 1024; }
int qdsp_hip_deframer_pack_span(void) { return 2048; }

}  // extern "C"
