// dsp/deemp.h -- BFMDeemp, HIP-backed.
//
// Drop-in for BFMDeemp of src/dsp/filter.h:90-173: same constructors, init(), setInput(), setSampleRate(), setTau(), public
// `bypass` and `out`.  run() is one call into libqdsp_hip (qdsp_hip_deemp_process_ex) between `_in->read()` and `out.swap()`
// with the device links of every detail::hip_block (hip_block.h), so FMDemod -> BFMDeemp hands its stereo_t blocks over in device memory.
// The filter runs as an FP64 prefix scan (include/qdsp_hip.h): within half an ulp of the exact recurrence rather than the
// bits of the reference's float loop; the carried output lives on the device.  alpha = dt / (tau + dt) is computed by the
// library in float, as init() computes it.
// The block has a header of its own (the reference keeps it in filter.h), so that a program built against filter.h alone needs no
// qdsp_hip_deemp_* symbol.
#pragma once
#include "block.h"
#include "filter.h"

namespace dsp {

class BFMDeemp : public detail::hip_block<stereo_t, stereo_t> {
    using hb = detail::hip_block<stereo_t, stereo_t>;

public:
    BFMDeemp() : hb(qdsp_hip_deemp_process_ex, qdsp_hip_deemp_destroy, "BFMDeemp::run") {}

    BFMDeemp(stream<stereo_t>* in, float sampleRate, float tau) : BFMDeemp() { init(in, sampleRate, tau); }

    ~BFMDeemp() { halt(); }      // the worker is in this class's run() and reads `bypass`

    void init(stream<stereo_t>* in, float sampleRate, float tau) {
        _sampleRate = sampleRate;
        _tau = tau;
        int rc = qdsp_hip_deemp_create(&handle, detail::hipDeviceForBlocks(), QDSP_HIP_DEEMP_STEREO, 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_deemp_set(handle, 0, _sampleRate, _tau); }
        hb::attach(in, rc, "BFMDeemp::init");
    }

    void setSampleRate(float sampleRate) { paused([&] { _sampleRate = sampleRate; push(); }); }

    void setTau(float tau) { paused([&] { _tau = tau; push(); }); }

    int run() override {
        const int count = take();
        if (count < 0) { return -1; }
        const bool by = bypass;
        if (by != bypassSet) {
            qdsp_hip_deemp_set_bypass(handle, by ? 1 : 0);
            bypassSet = by;
        }
        return finish(count);
    }

    bool bypass = false;

private:
    void push() {
        if (!handle) { return; }
        const int rc = qdsp_hip_deemp_set(handle, 0, _sampleRate, _tau);
        if (rc != 0) { detail::hipBlockFail("BFMDeemp::setTau", rc); }
    }

    bool bypassSet = false;
    float _tau = 0.0f;
    float _sampleRate = 1.0f;
};

}  // namespace dsp
