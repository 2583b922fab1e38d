// dsp/stereo_demod.h -- StereoFMDemod, HIP-backed.
//
// Drop-in for src/dsp/demodulator.h:189-330: both constructors, init(), setInput(), setSampleRate() / getSampleRate(),
// setDeviation() / getDeviation(), start() / stop() and the public `out`.  The reference builds the block from five inner blocks
// (FloatFMDemod -> Splitter -> FIR<float> with BlackmanBandpassWindow(1000, 1000, 19000, sampleRate) -> AGC(20, sampleRate), and
// three VOLK lines in its own run()); none of them holds a loop that carries a value across samples but the FM phase, so here it
// is ONE block with ONE library handle: run() is one qdsp_hip_stereo_fm_process_ex call between `_in->read()` and `out.swap()`,
// with the device links of the other demodulators (dsp/demodulator.h).  The FM phase, the pilot filter's history and the AGC
// level live on the device.  The taps come from this mirror's BlackmanBandpassWindow (dsp/window.h: the reference's, bit for
// bit); setSampleRate() regenerates them, which also zeroes the filter history (include/qdsp_hip.h; the reference's
// updateWindow keeps the old samples).  As in the reference the filter's delay is not compensated.
// Kept apart from dsp/demodulator.h so that a program built against that header alone needs no qdsp_hip_stereo_fm_* symbol.
#pragma once
#include <vector>

#include "demodulator.h"
#include "window.h"

namespace dsp {

class StereoFMDemod : public detail::demod_base<stereo_t> {
    using db = detail::demod_base<stereo_t>;

public:
    StereoFMDemod() : db(qdsp_hip_stereo_fm_process_ex, qdsp_hip_stereo_fm_destroy, "StereoFMDemod") {}
    StereoFMDemod(stream<complex_t>* in, float sampleRate, float deviation) : StereoFMDemod() { init(in, sampleRate, deviation); }

    void init(stream<complex_t>* in, float sampleRate, float deviation) {
        _sampleRate = sampleRate;
        _deviation = deviation;
        win.init(1000, 1000, 19000, sampleRate);
        makeTaps();
        int rc = qdsp_hip_stereo_fm_create(&handle, detail::hipDeviceForBlocks(), 1, taps.data(), (int)taps.size(), STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_stereo_fm_set_fm(handle, 0, _sampleRate, _deviation); }
        db::attach(in, rc);
    }

    void setSampleRate(float sampleRate) {
        paused([&] {
            _sampleRate = sampleRate;
            win.setSampleRate(_sampleRate);
            makeTaps();
            if (!handle) { return; }
            int rc = qdsp_hip_stereo_fm_set_fm(handle, 0, _sampleRate, _deviation);
            if (rc == 0) { rc = qdsp_hip_stereo_fm_set_pilot_taps(handle, taps.data(), (int)taps.size()); }
            if (rc != 0) { detail::hipBlockFail("StereoFMDemod::setSampleRate", rc); }
        });
    }

    float getSampleRate() { return _sampleRate; }

    void setDeviation(float deviation) {
        paused([&] {
            _deviation = deviation;
            if (!handle) { return; }
            const int rc = qdsp_hip_stereo_fm_set_fm(handle, 0, _sampleRate, _deviation);
            if (rc != 0) { detail::hipBlockFail("StereoFMDemod::setDeviation", rc); }
        });
    }

    float getDeviation() { return _deviation; }

    int getPilotTapCount() { return (int)taps.size(); }

private:
    // FIR<float>::init (filter.h): tapCount = window->getTapCount(), createTaps(taps, tapCount) with factor 1
    void makeTaps() {
        taps.assign((size_t)win.getTapCount(), 0.0f);
        win.createTaps(taps.data(), (int)taps.size());
    }

    float _sampleRate = 1.0f, _deviation = 1.0f;
    filter_window::BlackmanBandpassWindow win;
    std::vector<float> taps;
};

}  // namespace dsp
