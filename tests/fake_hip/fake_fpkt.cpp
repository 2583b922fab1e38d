// TEST-ONLY stand-in for qdsp_amd/csrc/fpkt.hip on the fake synchronous HIP runtime (fake_hip_runtime.cpp), so that packet_check --
// dsp/falcon_packet.h over the real qdsp_amd/csrc/stream_op.cpp -- runs under -fsanitize=address,undefined without a GPU
// (tests/test_fpkt_cpu.py).  Same C entry points and handle plumbing as the library's, the table's sub-kind included; the "kernel"
// is the serial loop, frame by frame, in the order include/qdsp_hip.h states it, with its two departures.  One channel.  "Device"
// memory is host memory here.
#include "../../qdsp_amd/csrc/stream_op.h"

#include <string.h>

#include <new>
#include <vector>

using namespace qh;

namespace {

constexpr int kData = 1191, kFrame = QDSP_HIP_FPKT_FRAME_BYTES, kCap = QDSP_HIP_FPKT_MAX_PACKET, kPerFrame = 1 + kData / 3;

struct FakeFpkt : StreamOp {
    static constexpr OpKind kKind = OpKind::Rs;
    static constexpr int kSub = 1;
    int frame_stride = 1275;
    uint32_t last_counter = 0;
    int packet_read = -1;
    uint8_t packet[kCap] = {};
    std::vector<int> offs;             // of the last call: count + 1 entries
};
void drop(FakeFpkt* d) {
    op_free(d, [] {});
}

int64_t out_count(const StreamOp*, int64_t nframes) { return kCap + (int64_t)kData * nframes; }

void emit(FakeFpkt* d, uint8_t* out, const uint8_t* src, int len) {
    memcpy(out + d->offs.back(), src, (size_t)len);
    d->offs.push_back(d->offs.back() + len);
}

void run_frame(FakeFpkt* d, const uint8_t* buf, uint8_t* out) {
    const int pkt = buf[3] | ((buf[2] & 7) << 8);
    const uint32_t ctr = (uint32_t)(buf[2] >> 3) | ((uint32_t)buf[1] << 5) | ((uint32_t)(buf[0] & 0x3f) << 13);
    const uint8_t* data = buf + 4;
    if (d->last_counter + 1u != ctr) d->packet_read = -1;
    d->last_counter = ctr;
    if (pkt == 2047) {
        if (d->packet_read >= 0) {
            if (d->packet_read + kData > kCap) {
                d->packet_read = -1;                           // departure: overflow
            } else {
                memcpy(d->packet + d->packet_read, data, kData);
                d->packet_read += kData;
            }
        }
        return;
    }
    if (pkt > kData) {                                         // departure: bad pointer
        d->packet_read = -1;
        return;
    }
    if (d->packet_read >= 0) {
        if (d->packet_read + pkt <= kCap) {
            memcpy(d->packet + d->packet_read, data, (size_t)pkt);
            emit(d, out, d->packet, d->packet_read + pkt);
        }
        d->packet_read = -1;
    }
    for (int i = pkt; i < kData;) {
        if (kData - i < 4) {
            d->packet_read = kData - i;
            memcpy(d->packet, data + i, (size_t)d->packet_read);
            break;
        }
        const int len = (((data[i] & 15) << 8) | data[i + 1]) + 2;
        if (len <= 2) break;
        if (kData - i < len) {
            d->packet_read = kData - i;
            memcpy(d->packet, data + i, (size_t)d->packet_read);
            break;
        }
        emit(d, out, data + i, len);
        i += len;
    }
}

// in_stride in frames, out_stride in bytes
int64_t launch(FakeFpkt* d, const void* d_in, int64_t nframes, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t) {
    if (nframes < 0 || (nframes > 0 && (!d_in || !d_out || d_in == d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < nframes || out_stride < out_count(d, nframes)) return QDSP_HIP_EINVAL;
    d->offs.assign(1, 0);
    for (int64_t f = 0; f < nframes; f++) run_frame(d, static_cast<const uint8_t*>(d_in) + f * d->frame_stride, static_cast<uint8_t*>(d_out));
    return 0;
}

}  // namespace

extern "C" {

int qdsp_hip_fpkt_create(void** h, int device, int nchan, int max_block, int frame_stride) {
    FakeFpkt* d = nullptr;
    const bool args_ok = nchan == 1 && frame_stride >= kFrame && frame_stride <= 4096;
    if (const int rc = op_new<FakeFpkt, launch, out_count>(&d, h, args_ok, device, nchan, max_block)) return rc;
    d->frame_stride = frame_stride;
    d->offs.assign(1, 0);
    hipError_t err = stream_op_init(d, device, nchan, max_block, (size_t)frame_stride, 1);
    if (err == hipSuccess && max_block > 0) {
        (void)hipFree(d->d_out);
        d->d_out = nullptr;
        err = hipMalloc(&d->d_out, (size_t)out_count(d, max_block));
    }
    return op_created<drop>(h, d, err);
}
int64_t qdsp_hip_fpkt_out_size(void* h, int64_t nframes) { return (as<FakeFpkt>(h) && nframes >= 0) ? out_count(nullptr, nframes) : QDSP_HIP_EINVAL; }
int64_t qdsp_hip_fpkt_out_packets(void* h, int64_t nframes) { return (as<FakeFpkt>(h) && nframes >= 0) ? kPerFrame * nframes : QDSP_HIP_EINVAL; }
int qdsp_hip_fpkt_frame_stride(void* h) {
    FakeFpkt* d = as<FakeFpkt>(h);
    return d ? d->frame_stride : QDSP_HIP_EINVAL;
}
int qdsp_hip_fpkt_process_ex(void* h, const void* in, int in_link, int nframes, void* out, int out_link) {
    FakeFpkt* d = as<FakeFpkt>(h);
    if (!d || (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE)) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, nframes, out, out_link);
    if (rc < 0 || nframes == 0) return (int)rc;
    return (int)d->offs.size() - 1;
}
int qdsp_hip_fpkt_process(void* h, const uint8_t* in, int nframes, uint8_t* out) {
    return qdsp_hip_fpkt_process_ex(h, in, QDSP_HIP_LINK_HOST, nframes, out, QDSP_HIP_LINK_HOST);
}
int qdsp_hip_fpkt_get_offsets(void* h, int chan, int* offs, int cap) {
    FakeFpkt* d = as<FakeFpkt>(h);
    if (!d || chan != 0 || cap < 0 || !offs) return QDSP_HIP_EINVAL;
    const int n = (int)d->offs.size() - 1, m = n < cap ? n : cap;
    memcpy(offs, d->offs.data(), (size_t)(m + 1) * sizeof(int));
    return n;
}
int qdsp_hip_fpkt_get_state(void* h, int chan, uint32_t* last_counter, int* packet_read, uint8_t* pending) {
    FakeFpkt* d = as<FakeFpkt>(h);
    if (!d || chan != 0 || !last_counter || !packet_read) return QDSP_HIP_EINVAL;
    *last_counter = d->last_counter;
    *packet_read = d->packet_read;
    if (pending) memcpy(pending, d->packet, kCap);
    return 0;
}
int qdsp_hip_fpkt_reset(void* h) {
    FakeFpkt* d = as<FakeFpkt>(h);
    if (!d) return QDSP_HIP_EINVAL;
    d->last_counter = 0;
    d->packet_read = -1;
    return 0;
}
void qdsp_hip_fpkt_destroy(void* h) { drop(as<FakeFpkt>(h)); }

}  // extern "C"
