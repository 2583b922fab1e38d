// dsp/deemp.h -- BFMDeemp, HIP-backed.
//
// Drop-in for BFMDeemp of src/dsp/filter.h:90-173: same constructors, init(), setInput(), setSampleRate(), setTau(), public
// `bypass` and `out`.  run() is one call into libqdsp_hip (qdsp_hip_deemp_process_ex) between `_in->read()` and `out.swap()`
// with the device links of the demodulator blocks, so FMDemod -> BFMDeemp hands its stereo_t blocks over in device memory.
// The filter runs as an FP64 prefix scan (include/qdsp_hip.h): within half an ulp of the exact recurrence rather than the
// bits of the reference's float loop; the carried output lives on the device.  alpha = dt / (tau + dt) is computed by the
// library in float, as init() computes it.
// The block has a header of its own (the reference keeps it in filter.h): graph_check includes filter.h and is also linked
// against a stand-in library without the de-emphasis entry points.
#pragma once
#include "block.h"
#include "filter.h"

namespace dsp {

class BFMDeemp : public generic_block<BFMDeemp> {
    using base = generic_block<BFMDeemp>;

public:
    BFMDeemp() {}

    BFMDeemp(stream<stereo_t>* in, float sampleRate, float tau) { init(in, sampleRate, tau); }

    ~BFMDeemp() {
        const bool live = base::running;
        base::stop();
        if (live && _in) { _in->releaseConsumer(); }
        if (handle) { qdsp_hip_deemp_destroy(handle); }
    }

    void init(stream<stereo_t>* in, float sampleRate, float tau) {
        _in = in;
        _sampleRate = sampleRate;
        _tau = tau;
        int rc = qdsp_hip_deemp_create(&handle, detail::hipDeviceForBlocks(), QDSP_HIP_DEEMP_STEREO, 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_deemp_set(handle, 0, _sampleRate, _tau); }
        if (rc != 0) { handle = nullptr; detail::hipBlockFail("BFMDeemp::init", rc); }
        base::registerInput(_in);
        base::registerOutput(&out);
        _in->claimConsumer(handle != nullptr, true);
    }

    void setInput(stream<stereo_t>* in) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        base::unregisterInput(_in);
        _in->releaseConsumer();
        _in = in;
        _in->claimConsumer(handle != nullptr, true);
        base::registerInput(_in);
        base::tempStart();
    }

    void setSampleRate(float sampleRate) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        _sampleRate = sampleRate;
        push();
        base::tempStart();
    }

    void setTau(float tau) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        _tau = tau;
        push();
        base::tempStart();
    }

    int run() override {
        const int count = _in->read();
        if (count < 0) { return -1; }
        if (!handle) { return -1; }
        const bool by = bypass;
        if (by != bypassSet) {
            qdsp_hip_deemp_set_bypass(handle, by ? 1 : 0);
            bypassSet = by;
        }
        const bool inDev = _in->readOnDevice;
        const bool outDev = out.consumerTakesDevice && out.ensureDevice(detail::hipDeviceForBlocks());
        const void* src = inDev ? static_cast<const void*>(_in->devReadBuf) : static_cast<const void*>(_in->readBuf);
        void* dst = outDev ? static_cast<void*>(out.devWriteBuf) : static_cast<void*>(out.writeBuf);
        void* evt = nullptr;
        const int outLink = outDev ? out.linkOut(true) : done.arm(handle, evt);
        const int rc = qdsp_hip_deemp_process_ex(handle, src, _in->linkIn(), count, dst, outLink);
        _in->flush();
        if (rc != 0) { return detail::hipBlockFail("BFMDeemp::run", rc); }
        out.markWritten(outLink, evt);
        if (!out.swap(count)) { return -1; }
        return count;
    }

    bool bypass = false;

    stream<stereo_t> out;

private:
    void push() {
        if (!handle) { return; }
        const int rc = qdsp_hip_deemp_set(handle, 0, _sampleRate, _tau);
        if (rc != 0) { detail::hipBlockFail("BFMDeemp::setTau", rc); }
    }

    bool bypassSet = false;
    float _tau = 0.0f;
    float _sampleRate = 1.0f;
    stream<stereo_t>* _in = nullptr;
    void* handle = nullptr;
    detail::done_events done;
};

}  // namespace dsp
