// dsp/falcon_fec.h -- dsp::FalconRS, HIP-backed.
//
// Drop-in for src/dsp/falcon_fec.h: both constructors, init(), run() and `out`.  De-interleaving through the dual-basis table, the
// five RS(255, 239) decodes, re-interleaving and de-randomising run on the device (qdsp_hip_falcon_rs_create: rs_decode_kernel); the
// three tables are computed by the library, not stored here.  A read of `count` bytes holds count / 1279 whole frames -- the
// reference's case is exactly one; bytes behind the last whole frame are dropped -- and every good frame goes out with an
// out.swap(1275) of its own, as in the reference; a frame with a codeword that does not decode is dropped.  The frames of one
// input block come back from the library in one piece, so the output link is the host buffer.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "block.h"
#include "hip_block.h"

namespace dsp {

class FalconRS : public detail::hip_block<uint8_t, uint8_t> {
    using hb = detail::hip_block<uint8_t, uint8_t>;

public:
    static constexpr int frameIn = 4 + 255 * 5, frameOut = 255 * 5;

    FalconRS() : hb(qdsp_hip_rs_process_ex, qdsp_hip_rs_destroy, "FalconRS::run", true) {}

    FalconRS(stream<uint8_t>* in) : FalconRS() { init(in); }

    ~FalconRS() { hb::halt(); }     // (the worker reads `frames`)

    void init(stream<uint8_t>* in) {
        const int maxFrames = STREAM_BUFFER_SIZE / frameIn + 1;
        const int rc = qdsp_hip_falcon_rs_create(&handle, detail::hipDeviceForBlocks(), 1, maxFrames);
        if (rc == 0) { frames.resize((size_t)maxFrames * (size_t)frameOut); }
        hb::attach(in, rc, "FalconRS::init");
    }

    int run() override {
        const int count = hb::take();
        if (count < 0) { return -1; }
        stream<uint8_t>* in = this->_in;
        const void* src = in->readOnDevice ? static_cast<const void*>(in->devReadBuf) : static_cast<const void*>(in->readBuf);
        const int good = qdsp_hip_rs_process_ex(handle, src, in->linkIn(), count / frameIn, frames.data(), QDSP_HIP_LINK_HOST);
        in->flush();
        if (good < 0) { return detail::hipBlockFail("FalconRS::run", good); }
        for (int f = 0; f < good; f++) {
            memcpy(out.writeBuf, frames.data() + (size_t)f * (size_t)frameOut, (size_t)frameOut);
            out.markWritten(QDSP_HIP_LINK_HOST);
            if (!out.swap(frameOut)) { return -1; }
        }
        return count;
    }

private:
    std::vector<uint8_t> frames;     // the good frames of one input block
};

}  // namespace dsp
