// dsp/processing.h -- dsp::FrequencyXlator<T>, dsp::Squelch, dsp::AGC, dsp::FeedForwardAGC<T> and dsp::ComplexAGC, HIP-backed
// (the reference's other blocks in this header -- DelayImag, packer ... -- are not provided).
//
// Drop-in for src/dsp/processing.h:10-81.  init()/setSampleRate()/setFrequency() compute
// phaseDelta exactly as the reference does -- theta = (freq/sampleRate) * 2.0f * FL_M_PI in
// float, then the float cos/sin (processing.h:20,39,48) -- and hand the pair to the GPU
// NCO (qdsp_hip_xlate_cf32_*), which advances by arg(phaseDelta) per sample with a 64-bit
// fixed-point accumulator instead of VOLK's recursive float phasor.
#pragma once
#include <cmath>
#include <type_traits>

#include "block.h"
#include "filter.h"

namespace dsp {

template <class T>
class FrequencyXlator : public generic_block<FrequencyXlator<T>> {
    static_assert(std::is_same<T, complex_t>::value, "FrequencyXlator is implemented for complex_t (as in the reference)");
    using base = generic_block<FrequencyXlator<T>>;

public:
    FrequencyXlator() {}
    FrequencyXlator(stream<complex_t>* in, float sampleRate, float freq) { init(in, sampleRate, freq); }

    ~FrequencyXlator() {
        const bool live = base::running;
        base::stop();
        if (live && _in) { _in->releaseConsumer(); }
        if (handle) { qdsp_hip_xlate_cf32_destroy(handle); }
    }

    void init(stream<complex_t>* in, float sampleRate, float freq) {
        _in = in;
        _sampleRate = sampleRate;
        _freq = freq;
        computeDelta();
        const int rc = qdsp_hip_xlate_cf32_create(&handle, detail::hipDeviceForBlocks(), deltaRe, deltaIm, STREAM_BUFFER_SIZE);
        if (rc != 0) { handle = nullptr; detail::hipBlockFail("FrequencyXlator::init", rc); }
        base::registerInput(_in);
        base::registerOutput(&out);
        _in->claimConsumer(handle != nullptr, true);
    }

    // (sic) the reference names its input setter setInputSize (processing.h:26)
    void setInputSize(stream<complex_t>* in) {
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
        _sampleRate = sampleRate;
        pushDelta();
    }
    float getSampleRate() { return _sampleRate; }

    void setFrequency(float freq) {
        _freq = freq;
        pushDelta();
    }
    float getFrequency() { return _freq; }

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
        const int rc = qdsp_hip_xlate_cf32_process_ex(handle, src, _in->linkIn(), count, dst, outLink);
        _in->flush();
        if (rc != 0) { return detail::hipBlockFail("FrequencyXlator::run", rc); }
        out.markWritten(outLink, evt);
        if (!out.swap(count)) { return -1; }
        return count;
    }

    stream<complex_t> out;

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
        if (handle) { qdsp_hip_xlate_cf32_set_phase_inc(handle, deltaRe, deltaIm); }
    }

    float _sampleRate = 1.0f, _freq = 0.0f;
    float deltaRe = 1.0f, deltaIm = 0.0f;
    stream<complex_t>* _in = nullptr;
    void* handle = nullptr;
    detail::done_events done;
};


// Squelch (src/dsp/processing.h:424-489): same constructors, init(), setInput(), setLevel(), getLevel() and `out`.  run() is one
// call into libqdsp_hip (qdsp_hip_squelch_process_ex) with the device links of the other blocks, so VFO -> Squelch -> demodulator
// hands its blocks over in device memory.  The mean of |x| is summed in FP64 on the device (include/qdsp_hip.h).
class Squelch : public generic_block<Squelch> {
    using base = generic_block<Squelch>;

public:
    Squelch() {}

    Squelch(stream<complex_t>* in, float level) { init(in, level); }

    ~Squelch() {
        const bool live = base::running;
        base::stop();
        if (live && _in) { _in->releaseConsumer(); }
        if (handle) { qdsp_hip_squelch_destroy(handle); }
    }

    void init(stream<complex_t>* in, float level) {
        _in = in;
        _level = level;
        int rc = qdsp_hip_squelch_create(&handle, detail::hipDeviceForBlocks(), 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_squelch_set_level(handle, 0, _level); }
        if (rc != 0) { handle = nullptr; detail::hipBlockFail("Squelch::init", rc); }
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

    void setLevel(float level) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        _level = level;
        if (handle) {
            const int rc = qdsp_hip_squelch_set_level(handle, 0, _level);
            if (rc != 0) { detail::hipBlockFail("Squelch::setLevel", rc); }
        }
        base::tempStart();
    }

    float getLevel() { return _level; }

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
        const int rc = qdsp_hip_squelch_process_ex(handle, src, _in->linkIn(), count, dst, outLink);
        _in->flush();
        if (rc != 0) { return detail::hipBlockFail("Squelch::run", rc); }
        out.markWritten(outLink, evt);
        if (!out.swap(count)) { return -1; }
        return count;
    }

    stream<complex_t> out;

private:
    float _level = -50.0f;
    stream<complex_t>* _in = nullptr;
    void* handle = nullptr;
    detail::done_events done;
};

// AGC (src/dsp/processing.h:83-145): same constructors, init(), setInput(), setSampleRate(), setFallRate() and `out`.  The level
// lives on the device; _CorrectedFallRate = fallRate / sampleRate is computed by the library in float, as init() computes it.
class AGC : public generic_block<AGC> {
    using base = generic_block<AGC>;

public:
    AGC() {}

    AGC(stream<float>* in, float fallRate, float sampleRate) { init(in, fallRate, sampleRate); }

    ~AGC() {
        const bool live = base::running;
        base::stop();
        if (live && _in) { _in->releaseConsumer(); }
        if (handle) { qdsp_hip_agc_destroy(handle); }
    }

    void init(stream<float>* in, float fallRate, float sampleRate) {
        _in = in;
        _sampleRate = sampleRate;
        _fallRate = fallRate;
        int rc = qdsp_hip_agc_create(&handle, detail::hipDeviceForBlocks(), 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_agc_set(handle, 0, _fallRate, _sampleRate); }
        if (rc != 0) { handle = nullptr; detail::hipBlockFail("AGC::init", rc); }
        base::registerInput(_in);
        base::registerOutput(&out);
        _in->claimConsumer(handle != nullptr, true);
    }

    void setInput(stream<float>* in) {
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

    void setFallRate(float fallRate) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        _fallRate = fallRate;
        push();
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
        const int rc = qdsp_hip_agc_process_ex(handle, src, _in->linkIn(), count, dst, outLink);
        _in->flush();
        if (rc != 0) { return detail::hipBlockFail("AGC::run", rc); }
        out.markWritten(outLink, evt);
        if (!out.swap(count)) { return -1; }
        return count;
    }

    stream<float> out;

private:
    void push() {
        if (!handle) { return; }
        const int rc = qdsp_hip_agc_set(handle, 0, _fallRate, _sampleRate);
        if (rc != 0) { detail::hipBlockFail("AGC::setFallRate", rc); }
    }

    float _fallRate = 0.0f;
    float _sampleRate = 1.0f;
    stream<float>* _in = nullptr;
    void* handle = nullptr;
    detail::done_events done;
};

// FeedForwardAGC<T> (src/dsp/processing.h:147-233), T = float or complex_t: same constructors, init(), setInput() and `out`.  The
// window is the reference's 1024 samples; the samples not yet output live on the device (qdsp_hip_ffagc_*).  run() publishes exactly
// the samples the call produced -- count - 1023 on the first emitting call, count afterwards -- and does not swap while the history
// fills (the reference publishes `count` there, of which only toProcess are written).
template <class T>
class FeedForwardAGC : public generic_block<FeedForwardAGC<T>> {
    static_assert(std::is_same<T, float>::value || std::is_same<T, complex_t>::value, "FeedForwardAGC: float or complex_t");
    using base = generic_block<FeedForwardAGC<T>>;

public:
    FeedForwardAGC() {}

    FeedForwardAGC(stream<T>* in) { init(in); }

    ~FeedForwardAGC() {
        const bool live = base::running;
        base::stop();
        if (live && _in) { _in->releaseConsumer(); }
        if (handle) { qdsp_hip_ffagc_destroy(handle); }
    }

    void init(stream<T>* in) {
        _in = in;
        const int kind = std::is_same<T, complex_t>::value ? QDSP_HIP_FFAGC_COMPLEX : QDSP_HIP_FFAGC_REAL;
        const int rc = qdsp_hip_ffagc_create(&handle, detail::hipDeviceForBlocks(), kind, 1, STREAM_BUFFER_SIZE, sampleCount);
        if (rc != 0) { handle = nullptr; detail::hipBlockFail("FeedForwardAGC::init", rc); }
        base::registerInput(_in);
        base::registerOutput(&out);
        _in->claimConsumer(handle != nullptr, true);
    }

    void setInput(stream<T>* in) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        base::unregisterInput(_in);
        _in->releaseConsumer();
        _in = in;
        _in->claimConsumer(handle != nullptr, true);
        base::registerInput(_in);
        base::tempStart();
    }

    int run() override {
        const int count = _in->read();
        if (count < 0) { return -1; }
        if (!handle) { return -1; }
        const bool emits = qdsp_hip_ffagc_out_size(handle, count) > 0;
        const bool inDev = _in->readOnDevice;
        const bool outDev = emits && out.consumerTakesDevice && out.ensureDevice(detail::hipDeviceForBlocks());
        const void* src = inDev ? static_cast<const void*>(_in->devReadBuf) : static_cast<const void*>(_in->readBuf);
        void* dst = outDev ? static_cast<void*>(out.devWriteBuf) : static_cast<void*>(out.writeBuf);
        void* evt = nullptr;
        // (a call that only fills the history writes no output: nothing to hand over, no event to arm)
        const int outLink = outDev ? out.linkOut(true) : (emits ? done.arm(handle, evt) : QDSP_HIP_LINK_HOST);
        const int outCount = qdsp_hip_ffagc_process_ex(handle, src, _in->linkIn(), count, dst, outLink);
        _in->flush();
        if (outCount < 0) { return detail::hipBlockFail("FeedForwardAGC::run", outCount); }
        if (outCount == 0) { return count; }
        out.markWritten(outLink, evt);
        if (!out.swap(outCount)) { return -1; }
        return outCount;
    }

    stream<T> out;

private:
    int sampleCount = 1024;
    stream<T>* _in = nullptr;
    void* handle = nullptr;
    detail::done_events done;
};

// ComplexAGC (src/dsp/processing.h:235-298): same constructors, init(), setInput(), setSetPoint(), setMaxGain(), setRate() and
// `out`.  The gain lives on the device in FP64 (qdsp_hip_cagc_*); a setter acts from the next run().  The outputs follow the exact
// recurrence of the float parameters more closely than the reference's float loop does, so they are not that loop's bits
// (INTEGRATION.md).
class ComplexAGC : public generic_block<ComplexAGC> {
    using base = generic_block<ComplexAGC>;

public:
    ComplexAGC() {}

    ComplexAGC(stream<complex_t>* in, float setPoint, float maxGain, float rate) { init(in, setPoint, maxGain, rate); }

    ~ComplexAGC() {
        const bool live = base::running;
        base::stop();
        if (live && _in) { _in->releaseConsumer(); }
        if (handle) { qdsp_hip_cagc_destroy(handle); }
    }

    void init(stream<complex_t>* in, float setPoint, float maxGain, float rate) {
        _in = in;
        _setPoint = setPoint;
        _maxGain = maxGain;
        _rate = rate;
        int rc = qdsp_hip_cagc_create(&handle, detail::hipDeviceForBlocks(), 1, STREAM_BUFFER_SIZE);
        if (rc == 0) { rc = qdsp_hip_cagc_set(handle, 0, _setPoint, _maxGain, _rate); }
        if (rc != 0) { handle = nullptr; detail::hipBlockFail("ComplexAGC::init", rc); }
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

    void setSetPoint(float setPoint) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        _setPoint = setPoint;
        push();
        base::tempStart();
    }

    void setMaxGain(float maxGain) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        _maxGain = maxGain;
        push();
        base::tempStart();
    }

    void setRate(float rate) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        _rate = rate;
        push();
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
        const int rc = qdsp_hip_cagc_process_ex(handle, src, _in->linkIn(), count, dst, outLink);
        _in->flush();
        if (rc != 0) { return detail::hipBlockFail("ComplexAGC::run", rc); }
        out.markWritten(outLink, evt);
        if (!out.swap(count)) { return -1; }
        return count;
    }

    stream<complex_t> out;

private:
    void push() {
        if (!handle) { return; }
        const int rc = qdsp_hip_cagc_set(handle, 0, _setPoint, _maxGain, _rate);
        if (rc != 0) { detail::hipBlockFail("ComplexAGC::set", rc); }
    }

    float _setPoint = 1.0f;
    float _maxGain = 10e4;
    float _rate = 10e-4;
    stream<complex_t>* _in = nullptr;
    void* handle = nullptr;
    detail::done_events done;
};

}  // namespace dsp
