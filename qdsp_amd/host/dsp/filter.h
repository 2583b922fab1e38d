// dsp/filter.h -- dsp::FIR<T>, HIP-backed.
//
// Drop-in for the reference block (src/dsp/filter.h:9-88): same constructors, init(),
// setInput(), updateWindow(), run() and public `out`.  What run() does between
// `_in->read()` and `out.swap()` -- the per-sample VOLK dot products over a history-prefixed
// buffer (filter.h:55-71) -- is one call into libqdsp_hip (qdsp_hip_fir_{cf32,f32}_process):
// the block's history lives on the GPU, the stream buffers are pinned so the call DMAs
// straight from readBuf and into writeBuf.  T = complex_t or float.  setInput(), run(), the
// public `stream<T> out` and the destructor are those of detail::hip_block (hip_block.h).
#pragma once
#include <type_traits>
#include <vector>

#include "block.h"
#include "hip_block.h"
#include "window.h"

namespace dsp {

template <class T>
class FIR : public detail::hip_block<T, T> {
    static_assert(std::is_same<T, complex_t>::value || std::is_same<T, float>::value, "FIR<T>: T is complex_t or float");
    using hb = detail::hip_block<T, T>;
    static constexpr bool kComplex = std::is_same<T, complex_t>::value;

public:
    FIR() : hb(kComplex ? qdsp_hip_fir_cf32_process_ex : qdsp_hip_fir_f32_process_ex,
               kComplex ? qdsp_hip_fir_cf32_destroy : qdsp_hip_fir_f32_destroy, "FIR::run") {}
    FIR(stream<T>* in, dsp::filter_window::generic_window* window) : FIR() { init(in, window); }

    void init(stream<T>* in, dsp::filter_window::generic_window* window) {
        loadTaps(window);
        const int dev = detail::hipDeviceForBlocks();
        const int rc = kComplex ? qdsp_hip_fir_cf32_create(&this->handle, dev, taps.data(), (int)taps.size(), STREAM_BUFFER_SIZE)
                                : qdsp_hip_fir_f32_create(&this->handle, dev, taps.data(), (int)taps.size(), STREAM_BUFFER_SIZE);
        hb::attach(in, rc, "FIR::init");
    }

    // As in the reference, the caller stops the block around this (filter.h:43-49 takes no lock).
    void updateWindow(dsp::filter_window::generic_window* window) {
        loadTaps(window);
        if (!this->handle) { return; }
        const int rc = kComplex ? qdsp_hip_fir_cf32_set_taps(this->handle, taps.data(), (int)taps.size())
                                : qdsp_hip_fir_f32_set_taps(this->handle, taps.data(), (int)taps.size());
        if (rc != 0) { detail::hipBlockFail("FIR::updateWindow", rc); }
    }

private:
    void loadTaps(dsp::filter_window::generic_window* window) {
        _window = window;
        const int n = window->getTapCount();
        taps.assign(n > 0 ? (size_t)n + 1 : 1, 0.0f);  // +1: RRCTaps may write taps[n] for even n
        window->createTaps(taps.data(), n);
        taps.resize(n > 0 ? n : 0);
    }

    dsp::filter_window::generic_window* _window = nullptr;
    std::vector<float> taps;
};

}  // namespace dsp
