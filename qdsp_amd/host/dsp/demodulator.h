// dsp/demodulator.h -- FloatFMDemod, FMDemod, AMDemod, SSBDemod, HIP-backed.
//
// Drop-in for the data-parallel blocks of src/dsp/demodulator.h (:33-187, :332-497): same constructors, init(), setInput(),
// setters / getters and public `out`.  run() is one call into libqdsp_hip between `_in->read()` and `out.swap()`, with the
// device links of detail::hip_block (hip_block.h), the base of every block here: a HIP-backed producer hands its block over in
// device memory.
//   FloatFMDemod / FMDemod  qdsp_hip_demod_* (FM / FM_STEREO): bit-identical to the reference loop; the carried phase lives
//                           on the device.  phasorSpeed is computed by the library from (sampleRate, deviation) exactly as
//                           init() computes it.
//   AMDemod                 qdsp_hip_demod_* (AM): |x| minus the mean of the call, the mean summed in FP64
//   SSBDemod                qdsp_hip_ssb_cf32_*: the xlator's NCO with the reference's phaseDelta, real part out
// StereoFMDemod is in dsp/stereo_demod.h: the reference's block has no PLL -- FloatFMDemod, a FIR<float> on the 19 kHz pilot, AGC
// and three element-wise lines -- and is one handle here (qdsp_hip_stereo_fm_*).  MSKDemod and PSKDemod are in dsp/psk_demod.h, one
// chain handle each; their parts as blocks of their own: ComplexAGC (dsp/processing.h), FIR (dsp/filter.h), CostasLoop (dsp/pll.h),
// DelayImag (dsp/psk_demod.h), MMClockRecovery (dsp/clock_recovery.h).
#pragma once
#include <cmath>

#include "block.h"
#include "filter.h"

namespace dsp {

namespace detail {
// complex_t in, OUT out (float or stereo_t); a failing run() is reported under the bare class name
template <class OUT> using demod_base = hip_block<complex_t, OUT>;

// FloatFMDemod and FMDemod differ only in the output type (FMDemod: l == r, demodulator.h:169-170)
template <class OUT>
class fm_demod : public demod_base<OUT> {
    using db = demod_base<OUT>;
    static constexpr int kKind = std::is_same<OUT, stereo_t>::value ? QDSP_HIP_DEMOD_FM_STEREO : QDSP_HIP_DEMOD_FM;

public:
    fm_demod() : db(qdsp_hip_demod_process_ex, qdsp_hip_demod_destroy, "FMDemod") {}

    void init(stream<complex_t>* in, float sampleRate, float deviation) {
        _sampleRate = sampleRate;
        _deviation = deviation;
        int rc = qdsp_hip_demod_create(&this->handle, hipDeviceForBlocks(), kKind, 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_demod_set_fm(this->handle, 0, _sampleRate, _deviation); }
        db::attach(in, rc);
    }

    void setSampleRate(float sampleRate) { db::paused([&] { _sampleRate = sampleRate; push(); }); }
    float getSampleRate() { return _sampleRate; }

    void setDeviation(float deviation) { db::paused([&] { _deviation = deviation; push(); }); }
    float getDeviation() { return _deviation; }

private:
    // phasorSpeed = (2 * FL_M_PI) / (_sampleRate / _deviation), computed by the library in float as init() does
    void push() {
        if (!this->handle) { return; }
        const int rc = qdsp_hip_demod_set_fm(this->handle, 0, _sampleRate, _deviation);
        if (rc != 0) { hipBlockFail("FMDemod::setDeviation", rc); }
    }

    float _sampleRate = 1.0f, _deviation = 1.0f;
};
}  // namespace detail

class FloatFMDemod : public detail::fm_demod<float> {
public:
    FloatFMDemod() {}
    FloatFMDemod(stream<complex_t>* in, float sampleRate, float deviation) { init(in, sampleRate, deviation); }
};

class FMDemod : public detail::fm_demod<stereo_t> {
public:
    FMDemod() {}
    FMDemod(stream<complex_t>* in, float sampleRate, float deviation) { init(in, sampleRate, deviation); }
};

class AMDemod : public detail::demod_base<float> {
    using db = detail::demod_base<float>;

public:
    AMDemod() : db(qdsp_hip_demod_process_ex, qdsp_hip_demod_destroy, "AMDemod") {}
    AMDemod(stream<complex_t>* in) : AMDemod() { init(in); }

    void init(stream<complex_t>* in) {
        const int rc = qdsp_hip_demod_create(&handle, detail::hipDeviceForBlocks(), QDSP_HIP_DEMOD_AM, 1, STREAM_BUFFER_SIZE);
        db::attach(in, rc);
    }
};

class SSBDemod : public detail::demod_base<float> {
    using db = detail::demod_base<float>;

public:
    SSBDemod() : db(qdsp_hip_ssb_cf32_process_ex, qdsp_hip_ssb_cf32_destroy, "SSBDemod") {}
    SSBDemod(stream<complex_t>* in, float sampleRate, float bandWidth, int mode) : SSBDemod() { init(in, sampleRate, bandWidth, mode); }

    enum {
        MODE_USB,
        MODE_LSB,
        MODE_DSB
    };

    void init(stream<complex_t>* in, float sampleRate, float bandWidth, int mode) {
        _sampleRate = sampleRate;
        _bandWidth = bandWidth;
        _mode = mode;
        computeDelta();
        const int rc = qdsp_hip_ssb_cf32_create(&handle, detail::hipDeviceForBlocks(), deltaRe, deltaIm, STREAM_BUFFER_SIZE);
        db::attach(in, rc);
    }

    // (as in the reference, no restart: the NCO takes the new increment between two run() calls)
    void setSampleRate(float sampleRate) {
        _sampleRate = sampleRate;
        pushDelta();
    }
    void setBandWidth(float bandWidth) {
        _bandWidth = bandWidth;
        pushDelta();
    }
    void setMode(int mode) {
        _mode = mode;
        pushDelta();
    }

private:
    // phaseDelta of SSBDemod::init (demodulator.h:408-419): the float cos / sin of +-(bandWidth / sampleRate) * FL_M_PI
    void computeDelta() {
        switch (_mode) {
        case MODE_USB:
            deltaRe = std::cos((_bandWidth / _sampleRate) * FL_M_PI);
            deltaIm = std::sin((_bandWidth / _sampleRate) * FL_M_PI);
            break;
        case MODE_LSB:
            deltaRe = std::cos(-(_bandWidth / _sampleRate) * FL_M_PI);
            deltaIm = std::sin(-(_bandWidth / _sampleRate) * FL_M_PI);
            break;
        case MODE_DSB:
            deltaRe = 1.0f;
            deltaIm = 0.0f;
            break;
        }
    }
    void pushDelta() {
        computeDelta();
        if (handle) { qdsp_hip_ssb_cf32_set_phase_inc(handle, deltaRe, deltaIm); }
    }

    int _mode = MODE_USB;
    float _sampleRate = 1.0f, _bandWidth = 0.0f;
    float deltaRe = 1.0f, deltaIm = 0.0f;
};

}  // namespace dsp
