// dsp/falcon_packet.h -- dsp::FalconPacketSync, HIP-backed.
//
// Drop-in for src/dsp/falcon_packet.h: both constructors, init(), run() and `out`.  The header parse, the counter check, the walk
// over the packet headers and the pending packet run on the device (qdsp_hip_fpkt_create with a frame stride of 1275: fpkt_walk_kernel,
// fpkt_scan_kernel, fpkt_pack_kernel); lastCounter, packetRead and the pending bytes stay in the handle.  A read of `count` bytes
// holds count / 1275 whole frames -- the reference's case is exactly one; bytes behind the last whole frame are dropped -- and every
// packet goes out with an out.swap(len) of its own, as in the reference.  The packets of one input block come back from the library
// in one piece with their offsets, so the output link is the host buffer.  Two departures from the reference, both where it leaves
// its buffers (include/qdsp_hip.h states them): a pending packet that would pass 16392 bytes and a first-header pointer of
// 1192 .. 2046 drop the pending packet.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "block.h"
#include "hip_block.h"

namespace dsp {

class FalconPacketSync : public detail::hip_block<uint8_t, uint8_t> {
    using hb = detail::hip_block<uint8_t, uint8_t>;

public:
    static constexpr int frameIn = 255 * 5;

    FalconPacketSync() : hb(qdsp_hip_fpkt_process_ex, qdsp_hip_fpkt_destroy, "FalconPacketSync::run", true) {}

    FalconPacketSync(stream<uint8_t>* in) : FalconPacketSync() { init(in); }

    ~FalconPacketSync() { hb::halt(); }     // (the worker reads `bytes` and `offs`)

    void init(stream<uint8_t>* in) {
        const int maxFrames = STREAM_BUFFER_SIZE / frameIn + 1;
        int rc = qdsp_hip_fpkt_create(&handle, detail::hipDeviceForBlocks(), 1, maxFrames, frameIn);
        if (rc == 0) {
            const int64_t nb = qdsp_hip_fpkt_out_size(handle, maxFrames), np = qdsp_hip_fpkt_out_packets(handle, maxFrames);
            if (nb < 0 || np < 0) {
                rc = (int)(nb < 0 ? nb : np);
            } else {
                bytes.resize((size_t)nb);
                offs.resize((size_t)np + 1);
            }
        }
        hb::attach(in, rc, "FalconPacketSync::init");
    }

    int run() override {
        const int count = hb::take();
        if (count < 0) { return -1; }
        stream<uint8_t>* in = this->_in;
        const void* src = in->readOnDevice ? static_cast<const void*>(in->devReadBuf) : static_cast<const void*>(in->readBuf);
        const int nframes = count / frameIn;
        int npk = qdsp_hip_fpkt_process_ex(handle, src, in->linkIn(), nframes, bytes.data(), QDSP_HIP_LINK_HOST);
        in->flush();
        if (npk > 0) { npk = qdsp_hip_fpkt_get_offsets(handle, 0, offs.data(), npk); }
        if (npk < 0) { return detail::hipBlockFail("FalconPacketSync::run", npk); }
        for (int k = 0; k < npk; k++) {
            const int len = offs[(size_t)k + 1] - offs[(size_t)k];
            memcpy(out.writeBuf, bytes.data() + offs[(size_t)k], (size_t)len);
            out.markWritten(QDSP_HIP_LINK_HOST);
            if (!out.swap(len)) { return -1; }
        }
        return count;
    }

private:
    std::vector<uint8_t> bytes;     // the packets of one input block, back to back
    std::vector<int> offs;          // where each begins; [count]: their bytes
};

}  // namespace dsp
