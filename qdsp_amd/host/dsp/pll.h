// dsp/pll.h -- dsp::CostasLoop<ORDER> (ORDER 2, 4 or 8), HIP-backed.
//
// Drop-in for src/dsp/pll.h: both constructors, init(), setInput(), setLoopBandwidth(), run() and `out`.  The loop's frequency
// and phase live on the device in FP64 (qdsp_hip_costas_*); alpha and beta are formed from the bandwidth by the library with the
// reference's formula.  A setter acts from the next run().  Two departures: a bandwidth that is negative or not
// finite is refused (the block reports the error and keeps the previous bandwidth), and a frequency or phase that a NaN sample has
// turned into NaN reads as 0 at the next run() where the reference's loop stays NaN for ever.
#pragma once
#include <cmath>

#include "block.h"
#include "filter.h"

namespace dsp {

template <int ORDER>
class CostasLoop : public generic_block<CostasLoop<ORDER>> {
    static_assert(ORDER == 2 || ORDER == 4 || ORDER == 8, "CostasLoop: ORDER 2, 4 or 8 (as in the reference)");
    using base = generic_block<CostasLoop<ORDER>>;

public:
    CostasLoop() {}

    CostasLoop(stream<complex_t>* in, float loopBandwidth) { init(in, loopBandwidth); }

    ~CostasLoop() {
        const bool live = base::running;
        base::stop();
        if (live && _in) { _in->releaseConsumer(); }
        if (handle) { qdsp_hip_costas_destroy(handle); }
    }

    void init(stream<complex_t>* in, float loopBandwidth) {
        _in = in;
        _loopBandwidth = loopBandwidth;
        int rc = qdsp_hip_costas_create(&handle, detail::hipDeviceForBlocks(), ORDER, 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_costas_set_bandwidth(handle, 0, _loopBandwidth); }
        if (rc != 0) {
            if (handle) { qdsp_hip_costas_destroy(handle); }
            handle = nullptr;
            detail::hipBlockFail("CostasLoop::init", rc);
        }
        base::registerInput(_in);
        base::registerOutput(&out);
        _in->claimConsumer(handle != nullptr, true);
    }

    void setInput(stream<complex_t>* in) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        base::unregisterInput(_in);
        _in->releaseConsumer();
        _in = in;
        _in->claimConsumer(handle != nullptr, true);
        base::registerInput(_in);
        base::tempStart();
    }

    void setLoopBandwidth(float loopBandwidth) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        if (handle) {
            const int rc = qdsp_hip_costas_set_bandwidth(handle, 0, loopBandwidth);
            if (rc == 0) { _loopBandwidth = loopBandwidth; }
            else { detail::hipBlockFail("CostasLoop::setLoopBandwidth", rc); }
        }
        base::tempStart();
    }

    int run() override {
        const int count = _in->read();
        if (count < 0) { return -1; }
        if (!handle) { return -1; }
        const bool inDev = _in->readOnDevice;
        const bool outDev = out.consumerTakesDevice && out.ensureDevice(detail::hipDeviceForBlocks());
        const void* src = inDev ? static_cast<const void*>(_in->devReadBuf) : static_cast<const void*>(_in->readBuf);
        void* dst = outDev ? static_cast<void*>(out.devWriteBuf) : static_cast<void*>(out.writeBuf);
        void* evt = nullptr;
        const int outLink = outDev ? out.linkOut(true) : done.arm(handle, evt);
        const int rc = qdsp_hip_costas_process_ex(handle, src, _in->linkIn(), count, dst, outLink);
        _in->flush();
        if (rc != 0) { return detail::hipBlockFail("CostasLoop::run", rc); }
        out.markWritten(outLink, evt);
        if (!out.swap(count)) { return -1; }
        return count;
    }

    stream<complex_t> out;

private:
    float _loopBandwidth = 1.0f;
    stream<complex_t>* _in = nullptr;
    void* handle = nullptr;
    detail::done_events done;
};

}  // namespace dsp
