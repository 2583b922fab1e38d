// TEST-ONLY stand-in for qdsp_amd/csrc/noaa.hip on the fake synchronous HIP runtime (fake_hip_runtime.cpp), so that noaa_check --
// dsp/noaa/hrpt.h and dsp/noaa/tip.h over the real qdsp_amd/csrc/stream_op.cpp -- runs under -fsanitize=address,undefined without a
// GPU (tests/test_noaa_cpu.py).  Same C entry points and handle plumbing as the library's, the tables of qdsp_amd/csrc/noaa.hip.h;
// the "kernels" are plain loops, bit by bit, serial, in the order include/qdsp_hip.h states the three blocks.  One channel.
// "Device" memory is host memory here.
#include "../../qdsp_amd/csrc/noaa.hip.h"

#include <string.h>

#include <new>
#include <vector>

using namespace qh;

namespace {

unsigned bits(const uint8_t* p, int bit, int len) {
    unsigned v = 0;
    for (int k = 0; k < len; k++) v = (v << 1) | ((p[(bit + k) >> 3] >> (7 - ((bit + k) & 7))) & 1u);
    return v;
}
int clamp_count(const int* d_in_counts, int64_t count) {
    if (!d_in_counts) return (int)count;
    return d_in_counts[0] < 0 ? 0 : (d_in_counts[0] < count ? d_in_counts[0] : (int)count);
}

struct FakeHrpt : StreamOp {
    static constexpr OpKind kKind = OpKind::Hrpt;
    std::vector<uint8_t> tip, aip;      // the single-output entry points' rows
    std::vector<int> slots;             // per frame of the last call
    int counts[3] = {0, 0, 0};
};
struct FakeTip : StreamOp {
    static constexpr OpKind kKind = OpKind::Tip;
    int count = 0;
};
struct FakeHirs : StreamOp {
    static constexpr OpKind kKind = OpKind::Hirs;
    int packet_stride = qk::kHirsPacket;
    int last_element = 0, new_image_data = 0, lines = 0;
    uint16_t part[qk::kHirsChannels][qk::kHirsLine];
};
template <class T> void drop(T* d) {
    op_free(d, [] {});
}

int hrpt_all(FakeHrpt* d, const void* d_in, int64_t nframes, int64_t in_stride, int n, uint16_t* av, int64_t plane_stride, uint8_t* tip,
             int64_t tip_stride, uint8_t* aip, int64_t aip_stride) {
    if (nframes < 0 || (nframes > 0 && !d_in) || in_stride < nframes * qk::kHrptFrameBytes) return QDSP_HIP_EINVAL;
    if (av && plane_stride < nframes * qk::kHrptPixels) return QDSP_HIP_EINVAL;
    if ((tip && tip_stride < nframes * qk::kHrptTipBytes) || (aip && aip_stride < nframes * qk::kHrptTipBytes)) return QDSP_HIP_EINVAL;
    const uint8_t* in = static_cast<const uint8_t*>(d_in);
    int nt = 0, na = 0;
    d->slots.assign((size_t)n, -1);
    for (int f = 0; f < n; f++) {
        const uint8_t* fr = in + (size_t)f * qk::kHrptFrameBytes;
        const unsigned minor = bits(fr, 61, 2);
        if (minor == 1 || minor == 3) {
            d->slots[(size_t)f] = minor == 1 ? nt : (na | (1 << 30));
            uint8_t* dst = minor == 1 ? tip : aip;
            int& k = minor == 1 ? nt : na;
            if (dst)
                for (int j = 0; j < qk::kHrptTipBytes; j++) dst[(size_t)k * qk::kHrptTipBytes + j] = (uint8_t)((bits(fr, 10 * (103 + j), 10) >> 2) & 0xFF);
            k++;
        }
        if (av)
            for (int p = 0; p < qk::kHrptPixels; p++)
                for (int c = 0; c < qk::kHrptPlanes; c++) av[(size_t)c * plane_stride + (size_t)f * qk::kHrptPixels + p] = (uint16_t)bits(fr, 10 * (750 + 5 * p + c), 10);
    }
    d->counts[0] = n;
    d->counts[1] = qk::kHrptMinorFrames * nt;
    d->counts[2] = qk::kHrptMinorFrames * na;
    return 0;
}
int64_t hrpt_launch(FakeHrpt* d, const void* d_in, int64_t nframes, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t) {
    if (nframes > 0 && !d_out) return QDSP_HIP_EINVAL;
    if (nframes < 0) return QDSP_HIP_EINVAL;
    if (d->tip.size() < (size_t)nframes * qk::kHrptTipBytes) {
        d->tip.resize((size_t)nframes * qk::kHrptTipBytes);
        d->aip.resize((size_t)nframes * qk::kHrptTipBytes);
    }
    return hrpt_all(d, d_in, nframes, in_stride * qk::kHrptFrameBytes, (int)nframes, static_cast<uint16_t*>(d_out), out_stride * qk::kHrptPixels,
                    d->tip.data(), (int64_t)d->tip.size(), d->aip.data(), (int64_t)d->aip.size());
}

int tip_all(FakeTip* d, const void* d_in, int64_t count, int64_t in_stride, int n, void* d_out, int64_t out_stride) {
    if (count < 0 || (count > 0 && (!d_in || !d_out || d_in == d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < count * qk::kTipFrame || out_stride < count * qk::kTipRecord) return QDSP_HIP_EINVAL;
    const uint8_t* in = static_cast<const uint8_t*>(d_in);
    uint8_t* out = static_cast<uint8_t*>(d_out);
    for (int m = 0; m < n; m++)
        for (int j = 0; j < qk::kTipRecord; j++) out[(size_t)m * qk::kTipRecord + j] = in[(size_t)m * qk::kTipFrame + qk::tip_src(j)];
    d->count = n;
    return 0;
}
int64_t tip_launch(FakeTip* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t) {
    return tip_all(d, d_in, count, in_stride * qk::kTipFrame, (int)count, d_out, out_stride * qk::kTipRecord);
}

void hirs_clear(FakeHirs* d) {
    for (auto& ch : d->part)
        for (uint16_t& v : ch) v = 0xFFF;
}
int hirs_all(FakeHirs* d, const void* d_in, int64_t count, int64_t in_stride, int n, uint16_t* out, int64_t plane_stride) {
    if (count < 0 || (count > 0 && (!d_in || !out))) return QDSP_HIP_EINVAL;
    if (count > 0 && in_stride < (count - 1) * d->packet_stride + qk::kHirsPacket) return QDSP_HIP_EINVAL;
    if (plane_stride < (count + 1) * qk::kHirsLine) return QDSP_HIP_EINVAL;
    const uint8_t* in = static_cast<const uint8_t*>(d_in);
    int lines = 0;
    auto emit = [&] {
        for (int ch = 0; ch < qk::kHirsChannels; ch++) memcpy(out + (size_t)ch * plane_stride + (size_t)lines * qk::kHirsLine, d->part[ch], sizeof(d->part[ch]));
        lines++;
        hirs_clear(d);
    };
    for (int i = 0; i < n; i++) {
        const uint8_t* pk = in + (size_t)i * d->packet_stride;
        const int e = (int)bits(pk, 19, 6);
        if ((e < d->last_element || e > 55) && d->new_image_data) {
            d->new_image_data = 0;
            emit();
        }
        d->last_element = e;
        if (e <= 55) {
            d->new_image_data = 1;
            for (int ch = 0; ch < qk::kHirsChannels; ch++) d->part[ch][e] = (uint16_t)qk::hirs_unsigned(bits(pk, qk::hirs_bit(ch), 13));
        }
        if (e == 55) {
            d->new_image_data = 0;
            emit();
        }
    }
    d->lines = lines;
    return 0;
}
int64_t hirs_launch(FakeHirs* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t) {
    return hirs_all(d, d_in, count, in_stride * d->packet_stride, (int)count, static_cast<uint16_t*>(d_out), out_stride * qk::kHirsLine);
}
int64_t hirs_out_count(const StreamOp*, int64_t count) { return count + 1; }

template <class T, auto L, int64_t (*OC)(const StreamOp*, int64_t) = nullptr>
int create(T** out, void** h, bool ok, int device, int nchan, int max_block, size_t in_es, size_t out_es, int64_t out_slots) {
    T* d = nullptr;
    if (const int rc = op_new<T, L, OC>(&d, h, ok && nchan == 1, device, nchan, max_block)) return rc;
    int rc = -(int)stream_op_init(d, device, nchan, max_block, in_es, out_es);
    if (!rc && max_block > 0 && out_slots != max_block) {
        (void)hipFree(d->d_out);
        d->d_out = nullptr;
        rc = -(int)hipMalloc(&d->d_out, (size_t)out_slots * out_es);
    }
    *out = rc ? nullptr : d;
    return op_created<drop<T>>(h, d, rc);
}

}  // namespace

extern "C" {

int qdsp_hip_hrpt_create(void** h, int device, int nchan, int max_block) {
    FakeHrpt* d;
    return create<FakeHrpt, hrpt_launch>(&d, h, true, device, nchan, max_block, qk::kHrptFrameBytes, (size_t)qk::kHrptPlanes * qk::kHrptPixels * 2, max_block);
}
int64_t qdsp_hip_hrpt_out_size(void* h, int64_t n) { return (as<FakeHrpt>(h) && n >= 0) ? n : QDSP_HIP_EINVAL; }
int qdsp_hip_hrpt_process_batch_dev(void* h, const void* d_in, int64_t nframes, int64_t in_stride_bytes, const int* d_in_counts, uint16_t* d_avhrr,
                                    int64_t, int64_t plane_stride, uint8_t* d_tip, int64_t tip_stride_bytes, int* d_tip_counts, uint8_t* d_aip,
                                    int64_t aip_stride_bytes, int* d_aip_counts, void*) {
    FakeHrpt* d = as<FakeHrpt>(h);
    if (!d) return QDSP_HIP_EINVAL;
    const int rc = hrpt_all(d, d_in, nframes, in_stride_bytes, clamp_count(d_in_counts, nframes), d_avhrr, plane_stride, d_tip, tip_stride_bytes, d_aip,
                            aip_stride_bytes);
    if (rc == 0 && d_tip_counts) d_tip_counts[0] = d->counts[1];
    if (rc == 0 && d_aip_counts) d_aip_counts[0] = d->counts[2];
    return rc;
}
int qdsp_hip_hrpt_process_dev(void* h, const void* d_in, int64_t nframes, void* d_avhrr, void* s) {
    FakeHrpt* d = as<FakeHrpt>(h);
    return d ? (int)hrpt_launch(d, d_in, nframes, nframes, d_avhrr, nframes, static_cast<hipStream_t>(s)) : QDSP_HIP_EINVAL;
}
int qdsp_hip_hrpt_process_ex(void* h, const void* in, int in_link, int nframes, void* avhrr, int out_link) {
    return op_process_ex<FakeHrpt>(h, in, in_link, nframes, avhrr, out_link);
}
int qdsp_hip_hrpt_process(void* h, const uint8_t* in, int nframes, uint16_t* avhrr) {
    return qdsp_hip_hrpt_process_ex(h, in, QDSP_HIP_LINK_HOST, nframes, avhrr, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_hrpt_get_counts(void* h, int* counts) {
    FakeHrpt* d = as<FakeHrpt>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    memcpy(counts, d->counts, sizeof(d->counts));
    return 0;
}
static int own_dev(void* h, int which, void** rows, int64_t* stride, int** counts) {
    FakeHrpt* d = as<FakeHrpt>(h);
    if (!d || !rows || !stride || !counts) return QDSP_HIP_EINVAL;
    *rows = which == 1 ? d->tip.data() : d->aip.data();
    *stride = (int64_t)d->tip.size();
    *counts = d->counts + which;
    return 0;
}
static int own_get(void* h, int which, int chan, uint8_t* out, int cap) {
    FakeHrpt* d = as<FakeHrpt>(h);
    if (!d || chan != 0 || cap < 0 || (cap > 0 && !out)) return QDSP_HIP_EINVAL;
    const int n = d->counts[which], m = n < cap ? n : cap;
    if (m > 0) memcpy(out, which == 1 ? d->tip.data() : d->aip.data(), (size_t)m * qk::kTipFrame);
    return n;
}
int qdsp_hip_hrpt_tip_dev(void* h, void** p, int64_t* s, int** c) { return own_dev(h, 1, p, s, c); }
int qdsp_hip_hrpt_aip_dev(void* h, void** p, int64_t* s, int** c) { return own_dev(h, 2, p, s, c); }
int qdsp_hip_hrpt_get_frame_slots(void* h, int chan, int* slots, int cap) {
    FakeHrpt* d = as<FakeHrpt>(h);
    if (!d || chan != 0 || cap < 0 || (cap > 0 && !slots)) return QDSP_HIP_EINVAL;
    const int n = d->counts[0], m = n < cap ? n : cap;
    if (m > 0) memcpy(slots, d->slots.data(), (size_t)m * sizeof(int));
    return n;
}
int qdsp_hip_hrpt_get_tip(void* h, int chan, uint8_t* out, int cap) { return own_get(h, 1, chan, out, cap); }
int qdsp_hip_hrpt_get_aip(void* h, int chan, uint8_t* out, int cap) { return own_get(h, 2, chan, out, cap); }
void qdsp_hip_hrpt_destroy(void* h) { drop(as<FakeHrpt>(h)); }

int qdsp_hip_tip_create(void** h, int device, int nchan, int max_block) {
    FakeTip* d;
    return create<FakeTip, tip_launch>(&d, h, true, device, nchan, max_block, qk::kTipFrame, qk::kTipRecord, max_block);
}
int64_t qdsp_hip_tip_out_size(void* h, int64_t n) { return (as<FakeTip>(h) && n >= 0) ? n : QDSP_HIP_EINVAL; }
int qdsp_hip_tip_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride_bytes, const int* d_in_counts, void* d_out,
                                   int64_t out_stride_bytes, int* d_counts, void*) {
    FakeTip* d = as<FakeTip>(h);
    if (!d) return QDSP_HIP_EINVAL;
    const int rc = tip_all(d, d_in, count, in_stride_bytes, clamp_count(d_in_counts, count), d_out, out_stride_bytes);
    if (rc == 0 && d_counts) d_counts[0] = d->count;
    return rc;
}
int qdsp_hip_tip_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* s) {
    return op_process_dev<FakeTip, tip_launch>(h, d_in, count, d_out, s);
}
int qdsp_hip_tip_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    return op_process_ex<FakeTip>(h, in, in_link, count, out, out_link);
}
int qdsp_hip_tip_process(void* h, const uint8_t* in, int count, uint8_t* out) {
    return qdsp_hip_tip_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_tip_get_counts(void* h, int* counts) {
    FakeTip* d = as<FakeTip>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    counts[0] = d->count;
    return 0;
}
void qdsp_hip_tip_destroy(void* h) { drop(as<FakeTip>(h)); }

int qdsp_hip_hirs_create(void** h, int device, int nchan, int max_block, int packet_stride) {
    FakeHirs* d = nullptr;
    const bool ok = packet_stride >= qk::kHirsPacket && packet_stride <= 4096;
    const int rc = create<FakeHirs, hirs_launch, hirs_out_count>(&d, h, ok, device, nchan, max_block, (size_t)(ok ? packet_stride : 0),
                                                                 (size_t)qk::kHirsChannels * qk::kHirsLine * 2, (int64_t)max_block + 1);
    if (d) {
        d->packet_stride = packet_stride;
        hirs_clear(d);
    }
    return rc;
}
int64_t qdsp_hip_hirs_out_size(void* h, int64_t n) { return (as<FakeHirs>(h) && n >= 0) ? n + 1 : QDSP_HIP_EINVAL; }
int qdsp_hip_hirs_packet_stride(void* h) {
    FakeHirs* d = as<FakeHirs>(h);
    return d ? d->packet_stride : QDSP_HIP_EINVAL;
}
int qdsp_hip_hirs_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride_bytes, const int* d_in_counts, uint16_t* d_out,
                                    int64_t, int64_t plane_stride, int* d_counts, void*) {
    FakeHirs* d = as<FakeHirs>(h);
    if (!d) return QDSP_HIP_EINVAL;
    const int rc = hirs_all(d, d_in, count, in_stride_bytes, clamp_count(d_in_counts, count), d_out, plane_stride);
    if (rc == 0 && d_counts) d_counts[0] = d->lines;
    return rc;
}
int qdsp_hip_hirs_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* s) {
    FakeHirs* d = as<FakeHirs>(h);
    return d ? (int)hirs_launch(d, d_in, count, count, d_out, count + 1, static_cast<hipStream_t>(s)) : QDSP_HIP_EINVAL;
}
int qdsp_hip_hirs_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    FakeHirs* d = as<FakeHirs>(h);
    if (!d || (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE)) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, count, out, out_link);
    if (rc < 0 || count == 0) return (int)rc;
    return d->lines;
}
int qdsp_hip_hirs_process(void* h, const uint8_t* in, int count, uint16_t* out) {
    return qdsp_hip_hirs_process_ex(h, in, QDSP_HIP_LINK_HOST, count, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_hirs_get_counts(void* h, int* counts) {
    FakeHirs* d = as<FakeHirs>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    counts[0] = d->lines;
    return 0;
}
int qdsp_hip_hirs_get_state(void* h, int chan, int* last_element, int* new_image_data) {
    FakeHirs* d = as<FakeHirs>(h);
    if (!d || chan != 0 || !last_element || !new_image_data) return QDSP_HIP_EINVAL;
    *last_element = d->last_element;
    *new_image_data = d->new_image_data;
    return 0;
}
int qdsp_hip_hirs_set_state(void* h, int chan, int last_element, int new_image_data) {
    FakeHirs* d = as<FakeHirs>(h);
    if (!d || chan < -1 || chan > 0 || last_element < 0 || last_element > 63 || (new_image_data != 0 && new_image_data != 1)) return QDSP_HIP_EINVAL;
    d->last_element = last_element;
    d->new_image_data = new_image_data;
    return 0;
}
int qdsp_hip_hirs_reset(void* h) {
    FakeHirs* d = as<FakeHirs>(h);
    if (!d) return QDSP_HIP_EINVAL;
    d->last_element = d->new_image_data = d->lines = 0;
    hirs_clear(d);
    return 0;
}
void qdsp_hip_hirs_destroy(void* h) { drop(as<FakeHirs>(h)); }

}  // extern "C"
