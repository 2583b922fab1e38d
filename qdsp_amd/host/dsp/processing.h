// dsp/processing.h -- dsp::FrequencyXlator<T>, dsp::Squelch, dsp::AGC, dsp::FeedForwardAGC<T>, dsp::ComplexAGC and dsp::Threshold, HIP-backed
// (DelayImag is in dsp/psk_demod.h; the reference's other blocks in this header -- packer ... -- are not provided).
//
// Drop-in for src/dsp/processing.h:10-81.  init()/setSampleRate()/setFrequency() compute
// phaseDelta exactly as the reference does -- theta = (freq/sampleRate) * 2.0f * FL_M_PI in
// float, then the float cos/sin (processing.h:20,39,48) -- and hand the pair to the GPU
// NCO (qdsp_hip_xlate_cf32_*), which advances by arg(phaseDelta) per sample with a 64-bit
// fixed-point accumulator instead of VOLK's recursive float phasor.
// Every block here is a detail::hip_block (hip_block.h): setInput(), run() with its device links, `out` and the destructor are
// the base's; a block adds its constructors, init() and its setters.
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "block.h"
#include "filter.h"

namespace dsp {

template <class T>
class FrequencyXlator : public detail::hip_block<T, T> {
    static_assert(std::is_same<T, complex_t>::value, "FrequencyXlator is implemented for complex_t (as in the reference)");
    using hb = detail::hip_block<T, T>;
    using hb::setInput;     // (under the reference's name below)

public:
    FrequencyXlator() : hb(qdsp_hip_xlate_cf32_process_ex, qdsp_hip_xlate_cf32_destroy, "FrequencyXlator::run") {}
    FrequencyXlator(stream<complex_t>* in, float sampleRate, float freq) : FrequencyXlator() { init(in, sampleRate, freq); }

    void init(stream<complex_t>* in, float sampleRate, float freq) {
        _sampleRate = sampleRate;
        _freq = freq;
        computeDelta();
        const int rc = qdsp_hip_xlate_cf32_create(&this->handle, detail::hipDeviceForBlocks(), deltaRe, deltaIm, STREAM_BUFFER_SIZE);
        hb::attach(in, rc, "FrequencyXlator::init");
    }

    // (sic) the reference names its input setter setInputSize (processing.h:26)
    void setInputSize(stream<complex_t>* in) { hb::setInput(in); }

    void setSampleRate(float sampleRate) {
        _sampleRate = sampleRate;
        pushDelta();
    }
    float getSampleRate() { return _sampleRate; }

    void setFrequency(float freq) {
        _freq = freq;
        pushDelta();
    }
    float getFrequency() { return _freq; }

private:
    void computeDelta() {
        const float theta = (_freq / _sampleRate) * 2.0f * FL_M_PI;
        deltaRe = std::cos(theta);
        deltaIm = std::sin(theta);
    }
    // The reference changes phaseDelta while the worker runs ("No need to restart"); the
    // device NCO takes the new increment between two run() calls the same way.
    void pushDelta() {
        computeDelta();
        if (this->handle) { qdsp_hip_xlate_cf32_set_phase_inc(this->handle, deltaRe, deltaIm); }
    }

    float _sampleRate = 1.0f, _freq = 0.0f;
    float deltaRe = 1.0f, deltaIm = 0.0f;
};


// Squelch (src/dsp/processing.h:424-489): same constructors, init(), setInput(), setLevel(), getLevel() and `out`.  run() is one
// call into libqdsp_hip (qdsp_hip_squelch_process_ex) with the device links of the other blocks, so VFO -> Squelch -> demodulator
// hands its blocks over in device memory.  The mean of |x| is summed in FP64 on the device (include/qdsp_hip.h).
class Squelch : public detail::hip_block<complex_t, complex_t> {
    using hb = detail::hip_block<complex_t, complex_t>;

public:
    Squelch() : hb(qdsp_hip_squelch_process_ex, qdsp_hip_squelch_destroy, "Squelch::run") {}

    Squelch(stream<complex_t>* in, float level) : Squelch() { init(in, level); }

    void init(stream<complex_t>* in, float level) {
        _level = level;
        int rc = qdsp_hip_squelch_create(&handle, detail::hipDeviceForBlocks(), 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_squelch_set_level(handle, 0, _level); }
        hb::attach(in, rc, "Squelch::init");
    }

    void setLevel(float level) {
        paused([&] {
            _level = level;
            if (!handle) { return; }
            const int rc = qdsp_hip_squelch_set_level(handle, 0, _level);
            if (rc != 0) { detail::hipBlockFail("Squelch::setLevel", rc); }
        });
    }

    float getLevel() { return _level; }

private:
    float _level = -50.0f;
};

// AGC (src/dsp/processing.h:83-145): same constructors, init(), setInput(), setSampleRate(), setFallRate() and `out`.  The level
// lives on the device; _CorrectedFallRate = fallRate / sampleRate is computed by the library in float, as init() computes it.
class AGC : public detail::hip_block<float, float> {
    using hb = detail::hip_block<float, float>;

public:
    AGC() : hb(qdsp_hip_agc_process_ex, qdsp_hip_agc_destroy, "AGC::run") {}

    AGC(stream<float>* in, float fallRate, float sampleRate) : AGC() { init(in, fallRate, sampleRate); }

    void init(stream<float>* in, float fallRate, float sampleRate) {
        _sampleRate = sampleRate;
        _fallRate = fallRate;
        int rc = qdsp_hip_agc_create(&handle, detail::hipDeviceForBlocks(), 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_agc_set(handle, 0, _fallRate, _sampleRate); }
        hb::attach(in, rc, "AGC::init");
    }

    void setSampleRate(float sampleRate) { paused([&] { _sampleRate = sampleRate; push(); }); }

    void setFallRate(float fallRate) { paused([&] { _fallRate = fallRate; push(); }); }

private:
    void push() {
        if (!handle) { return; }
        const int rc = qdsp_hip_agc_set(handle, 0, _fallRate, _sampleRate);
        if (rc != 0) { detail::hipBlockFail("AGC::setFallRate", rc); }
    }

    float _fallRate = 0.0f;
    float _sampleRate = 1.0f;
};

// FeedForwardAGC<T> (src/dsp/processing.h:147-233), T = float or complex_t: same constructors, init(), setInput() and `out`.  The
// window is the reference's 1024 samples; the samples not yet output live on the device (qdsp_hip_ffagc_*).  run() publishes exactly
// the samples the call produced -- count - 1023 on the first emitting call, count afterwards -- and does not swap while the history
// fills (the reference publishes `count` there, of which only toProcess are written).
template <class T>
class FeedForwardAGC : public detail::hip_block<T, T> {
    static_assert(std::is_same<T, float>::value || std::is_same<T, complex_t>::value, "FeedForwardAGC: float or complex_t");
    using hb = detail::hip_block<T, T>;

public:
    FeedForwardAGC() : hb(qdsp_hip_ffagc_process_ex, qdsp_hip_ffagc_destroy, "FeedForwardAGC::run", true) {}

    FeedForwardAGC(stream<T>* in) : FeedForwardAGC() { init(in); }

    ~FeedForwardAGC() { hb::halt(); }    // the worker is in this class's run()

    void init(stream<T>* in) {
        const int kind = std::is_same<T, complex_t>::value ? QDSP_HIP_FFAGC_COMPLEX : QDSP_HIP_FFAGC_REAL;
        const int rc = qdsp_hip_ffagc_create(&this->handle, detail::hipDeviceForBlocks(), kind, 1, STREAM_BUFFER_SIZE, sampleCount);
        hb::attach(in, rc, "FeedForwardAGC::init");
    }

    int run() override {
        const int count = hb::take();
        if (count < 0) { return -1; }
        // (a call that only fills the history writes no output: nothing to hand over, no event to arm)
        const int outCount = hb::call(count, qdsp_hip_ffagc_out_size(this->handle, count) > 0);
        if (outCount < 0) { return -1; }
        if (outCount == 0) { return count; }
        return hb::publish(outCount) ? outCount : -1;
    }

private:
    int sampleCount = 1024;
};

// ComplexAGC (src/dsp/processing.h:235-298): same constructors, init(), setInput(), setSetPoint(), setMaxGain(), setRate() and
// `out`.  The gain lives on the device in FP64 (qdsp_hip_cagc_*); a setter acts from the next run().  The outputs follow the exact
// recurrence of the float parameters more closely than the reference's float loop does, so they are not that loop's bits
// (INTEGRATION.md).
class ComplexAGC : public detail::hip_block<complex_t, complex_t> {
    using hb = detail::hip_block<complex_t, complex_t>;

public:
    ComplexAGC() : hb(qdsp_hip_cagc_process_ex, qdsp_hip_cagc_destroy, "ComplexAGC::run") {}

    ComplexAGC(stream<complex_t>* in, float setPoint, float maxGain, float rate) : ComplexAGC() { init(in, setPoint, maxGain, rate); }

    void init(stream<complex_t>* in, float setPoint, float maxGain, float rate) {
        _setPoint = setPoint;
        _maxGain = maxGain;
        _rate = rate;
        int rc = qdsp_hip_cagc_create(&handle, detail::hipDeviceForBlocks(), 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_cagc_set(handle, 0, _setPoint, _maxGain, _rate); }
        hb::attach(in, rc, "ComplexAGC::init");
    }

    void setSetPoint(float setPoint) { paused([&] { _setPoint = setPoint; push(); }); }

    void setMaxGain(float maxGain) { paused([&] { _maxGain = maxGain; push(); }); }

    void setRate(float rate) { paused([&] { _rate = rate; push(); }); }

private:
    void push() {
        if (!handle) { return; }
        const int rc = qdsp_hip_cagc_set(handle, 0, _setPoint, _maxGain, _rate);
        if (rc != 0) { detail::hipBlockFail("ComplexAGC::set", rc); }
    }

    float _setPoint = 1.0f;
    float _maxGain = 10e4;
    float _rate = 10e-4;
};

// Threshold (src/dsp/processing.h:554-610): same constructors, init(), setInput(), setLevel(), getLevel() and `out`: one byte per
// float, out = (in > 0.0f), on the device (qdsp_hip_threshold_*).  As in the reference the level is stored and never used by run().
class Threshold : public detail::hip_block<float, uint8_t> {
    using hb = detail::hip_block<float, uint8_t>;

public:
    Threshold() : hb(qdsp_hip_threshold_process_ex, qdsp_hip_threshold_destroy, "Threshold::run") {}

    Threshold(stream<float>* in) : Threshold() { init(in); }

    void init(stream<float>* in) {
        const int rc = qdsp_hip_threshold_create(&handle, detail::hipDeviceForBlocks(), 1, STREAM_BUFFER_SIZE);
        hb::attach(in, rc, "Threshold::init");
    }

    void setLevel(float level) { _level = level; }

    float getLevel() { return _level; }

private:
    float _level = -50.0f;
};

}  // namespace dsp
