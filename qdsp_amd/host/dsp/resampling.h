// dsp/resampling.h -- dsp::PolyphaseResampler<T>, HIP-backed.
//
// Drop-in for src/dsp/resampling.h:9-189: rational interp/decim resampler (a decimator when
// interp == 1).  Rate handling follows the reference: interp = outSR/gcd, decim = inSR/gcd
// on the int-cast rates (resampling.h:28-30), taps designed by the window with gain
// `interp` (resampling.h:34), phase split and per-block phase restart inside the library
// (qdsp_hip_decim_*).  T = complex_t, stereo_t (same kernels: a float pair with real taps)
// or float.  setInput(), run(), the public `stream<T> out` and the destructor are those of
// detail::hip_block (hip_block.h).
#pragma once
#include <numeric>
#include <type_traits>
#include <vector>

#include "block.h"
#include "filter.h"
#include "window.h"

namespace dsp {

template <class T>
class PolyphaseResampler : public detail::hip_block<T, T> {
    using hb = detail::hip_block<T, T>;
    static constexpr bool kPair = std::is_same<T, complex_t>::value || std::is_same<T, stereo_t>::value;
    static_assert(kPair || std::is_same<T, float>::value, "PolyphaseResampler<T>: T is complex_t, stereo_t or float");

public:
    // (process_ex returns the output count; run() publishes that many and returns the input count)
    PolyphaseResampler() : hb(kPair ? qdsp_hip_decim_cf32_process_ex : qdsp_hip_decim_f32_process_ex,
                              kPair ? qdsp_hip_decim_cf32_destroy : qdsp_hip_decim_f32_destroy, "PolyphaseResampler::run", true) {}
    PolyphaseResampler(stream<T>* in, dsp::filter_window::generic_window* window, float inSampleRate, float outSampleRate) : PolyphaseResampler() {
        init(in, window, inSampleRate, outSampleRate);
    }

    void init(stream<T>* in, dsp::filter_window::generic_window* window, float inSampleRate, float outSampleRate) {
        _window = window;
        _inSampleRate = inSampleRate;
        _outSampleRate = outSampleRate;
        updateRatio();
        designTaps();
        const int dev = detail::hipDeviceForBlocks();
        const int rc = kPair ? qdsp_hip_decim_cf32_create(&this->handle, dev, taps.data(), (int)taps.size(), _interp, _decim, STREAM_BUFFER_SIZE)
                             : qdsp_hip_decim_f32_create(&this->handle, dev, taps.data(), (int)taps.size(), _interp, _decim, STREAM_BUFFER_SIZE);
        hb::attach(in, rc, "PolyphaseResampler::init");
    }

    // The reference re-splits the EXISTING taps for the new ratio without redesigning them
    // (resampling.h:53-73); so does this.
    void setInSampleRate(float inSampleRate) {
        hb::paused([&] {
            _inSampleRate = inSampleRate;
            updateRatio();
            reconfigure();
        });
    }

    void setOutSampleRate(float outSampleRate) {
        hb::paused([&] {
            _outSampleRate = outSampleRate;
            updateRatio();
            reconfigure();
        });
    }

    int getInterpolation() { return _interp; }
    int getDecimation() { return _decim; }

    void updateWindow(dsp::filter_window::generic_window* window) {
        hb::paused([&] {
            _window = window;
            designTaps();
            reconfigure();
        });
    }

    int calcOutSize(int in) override { return (in * _interp) / _decim; }

private:
    void updateRatio() {
        const int g = std::gcd((int)_inSampleRate, (int)_outSampleRate);
        _interp = _outSampleRate / g;
        _decim = _inSampleRate / g;
    }

    void designTaps() {
        const int n = _window->getTapCount();
        taps.assign(n > 0 ? (size_t)n + 1 : 1, 0.0f);
        _window->createTaps(taps.data(), n, _interp);
        taps.resize(n > 0 ? n : 0);
    }

    void reconfigure() {
        if (!this->handle) { return; }
        const int rc = kPair ? qdsp_hip_decim_cf32_configure(this->handle, taps.data(), (int)taps.size(), _interp, _decim)
                             : qdsp_hip_decim_f32_configure(this->handle, taps.data(), (int)taps.size(), _interp, _decim);
        if (rc != 0) { detail::hipBlockFail("PolyphaseResampler::reconfigure", rc); }
    }

    dsp::filter_window::generic_window* _window = nullptr;
    int _interp = 1, _decim = 1;
    float _inSampleRate = 1.0f, _outSampleRate = 1.0f;
    std::vector<float> taps;
};

}  // namespace dsp
