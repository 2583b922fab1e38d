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
class CostasLoop : public detail::hip_block<complex_t, complex_t> {
    static_assert(ORDER == 2 || ORDER == 4 || ORDER == 8, "CostasLoop: ORDER 2, 4 or 8 (as in the reference)");
    using hb = detail::hip_block<complex_t, complex_t>;

public:
    CostasLoop() : hb(qdsp_hip_costas_process_ex, qdsp_hip_costas_destroy, "CostasLoop::run") {}

    CostasLoop(stream<complex_t>* in, float loopBandwidth) : CostasLoop() { init(in, loopBandwidth); }

    void init(stream<complex_t>* in, float loopBandwidth) {
        _loopBandwidth = loopBandwidth;
        int rc = qdsp_hip_costas_create(&handle, detail::hipDeviceForBlocks(), ORDER, 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_costas_set_bandwidth(handle, 0, _loopBandwidth); }
        if (rc != 0 && handle) {     // a refused bandwidth after a successful create
            qdsp_hip_costas_destroy(handle);
            handle = nullptr;
        }
        hb::attach(in, rc, "CostasLoop::init");
    }

    void setLoopBandwidth(float loopBandwidth) {
        paused([&] {
            if (!handle) { return; }
            const int rc = qdsp_hip_costas_set_bandwidth(handle, 0, loopBandwidth);
            if (rc == 0) { _loopBandwidth = loopBandwidth; }
            else { detail::hipBlockFail("CostasLoop::setLoopBandwidth", rc); }
        });
    }

private:
    float _loopBandwidth = 1.0f;
};

}  // namespace dsp
