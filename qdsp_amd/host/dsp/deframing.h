// dsp/deframing.h -- dsp::Deframer, HIP-backed.
//
// Drop-in for src/dsp/deframing.h: both constructors, init(), run() and `out`.  The search for the sync word, the state machine
// (bitsRead, badFrameCount, nextBitIsStartOfFrame), the last syncLen symbols and the frame in progress live on the device
// (qdsp_hip_deframer_*); the input block arrives from a HIP-backed neighbour (Threshold, say) in device memory.  As in the
// reference every frame goes out with an out.swap() of its own, ceil(frameLen / 8) bytes; the frames of one input block come back
// from the library in one piece, so the output link is the host buffer.  Departures: any block size is served, and
// the frames are a function of the concatenated input, whatever the block sizes.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "block.h"
#include "hip_block.h"

namespace dsp {

class Deframer : public detail::hip_block<uint8_t, uint8_t> {
    using hb = detail::hip_block<uint8_t, uint8_t>;

public:
    Deframer() : hb(qdsp_hip_deframer_process_ex, qdsp_hip_deframer_destroy, "Deframer::run", true) {}

    Deframer(stream<uint8_t>* in, int frameLen, uint8_t* syncWord, int syncLen) : Deframer() { init(in, frameLen, syncWord, syncLen); }

    ~Deframer() { hb::halt(); }     // (the worker reads `frames`)

    void init(stream<uint8_t>* in, int frameLen, uint8_t* syncWord, int syncLen) {
        int rc = qdsp_hip_deframer_create(&handle, detail::hipDeviceForBlocks(), 0, 1, STREAM_BUFFER_SIZE, frameLen, syncWord, syncLen);
        if (rc == 0) {
            frameBytes = qdsp_hip_deframer_frame_bytes(handle);
            frames.resize((size_t)qdsp_hip_deframer_out_size(handle, STREAM_BUFFER_SIZE) * (size_t)frameBytes);
        }
        hb::attach(in, rc, "Deframer::init");
    }

    int run() override {
        const int count = hb::take();
        if (count < 0) { return -1; }
        stream<uint8_t>* in = this->_in;
        const void* src = in->readOnDevice ? static_cast<const void*>(in->devReadBuf) : static_cast<const void*>(in->readBuf);
        const int nf = qdsp_hip_deframer_process_ex(handle, src, in->linkIn(), count, frames.data(), QDSP_HIP_LINK_HOST);
        in->flush();
        if (nf < 0) { return detail::hipBlockFail("Deframer::run", nf); }
        for (int f = 0; f < nf; f++) {
            memcpy(out.writeBuf, frames.data() + (size_t)f * (size_t)frameBytes, (size_t)frameBytes);
            out.markWritten(QDSP_HIP_LINK_HOST);
            if (!out.swap(frameBytes)) { return -1; }
        }
        return count;
    }

private:
    int frameBytes = 0;
    std::vector<uint8_t> frames;     // the frames of one input block
};

}  // namespace dsp
