// dsp/psk_demod.h -- dsp::DelayImag, dsp::PSKDemod<ORDER, OFFSET> and dsp::MSKDemod, HIP-backed.
//
// Drop-in for src/dsp/processing.h:300-344 and src/dsp/demodulator.h:499-682: the reference's constructors, init(), every setter,
// setInput(), start() / stop() and the public `out` (DelayImag: a stream; the demodulators: a pointer to one, as in the reference).
//   DelayImag   qdsp_hip_delay_imag_*: out[i] = {in[i].re, in[i - 1].im}, the carried imaginary part on the device.
//   PSKDemod    the reference registers five blocks (ComplexAGC, FIR<complex_t> over RRCTaps, CostasLoop<ORDER>, DelayImag when
//   MSKDemod    OFFSET, MMClockRecovery) and MSKDemod two (FloatFMDemod, MMClockRecovery<float>), a worker and two host buffers
//               each.  Here a demodulator is ONE block, one worker and one chain handle (qdsp_hip_psk_* / qdsp_hip_msk_*): a run()
//               is one library call that runs every stage on the device and hands over as many symbols as the block of samples
//               held.  Like MMClockRecovery::run it waits for the count, so the output link is the host buffer or the device
//               buffer, never a pipelined or deferred one.  A setter reaches its stage through qdsp_hip_*_stage and acts from the
//               next run(); parameters a stage refuses are reported (hipBlockErrors) and the previous ones are kept.
// Departures: MSKDemod's constructor forwards the three loop parameters (the reference's drops them); a ratio
// sampleRate / baudRate below the clock stage's parameter rule is refused at init(); an even RRC tap count uses the first `count`
// of the `count | 1` taps computed (what FIR<T> does with RRCTaps in this mirror and in the reference).
// Kept out of dsp/demodulator.h and dsp/processing.h so that what is built against those alone needs no new entry point.
#pragma once
#include <vector>

#include "block.h"
#include "hip_block.h"
#include "window.h"

namespace dsp {

class DelayImag : public detail::hip_block<complex_t, complex_t> {
    using hb = detail::hip_block<complex_t, complex_t>;

public:
    DelayImag() : hb(qdsp_hip_delay_imag_process_ex, qdsp_hip_delay_imag_destroy, "DelayImag::run") {}

    DelayImag(stream<complex_t>* in) : DelayImag() { init(in); }

    void init(stream<complex_t>* in) {
        const int rc = qdsp_hip_delay_imag_create(&handle, detail::hipDeviceForBlocks(), 1, STREAM_BUFFER_SIZE);
        hb::attach(in, rc, "DelayImag::init");
    }
};

namespace detail {
// The one block under a demodulator chain: complex_t in, symbols out, the count returned by the call.
template <class OUT>
class chain_block : public hip_block<complex_t, OUT> {
    using hb = hip_block<complex_t, OUT>;

public:
    chain_block(typename hb::process_fn p, typename hb::destroy_fn d, const char* who) : hb(p, d, who, true), ex(p), name(who) {}
    ~chain_block() { hb::halt(); }   // (the worker calls this class's run())

    void** slot() { return &this->handle; }
    void* chain() { return this->handle; }
    void attachTo(stream<complex_t>* in, int rc, const char* initWho) { hb::attach(in, rc, initWho); }
    // a setter's frame: the worker is parked while `change` runs
    template <class F> void change(F f) { hb::paused(f); }

    int run() override {
        const int count = hb::take();
        if (count < 0) { return -1; }
        stream<complex_t>* in = this->_in;
        const bool outDev = this->out.consumerTakesDevice && this->out.ensureDevice(hipDeviceForBlocks());
        const void* src = in->readOnDevice ? static_cast<const void*>(in->devReadBuf) : static_cast<const void*>(in->readBuf);
        void* dst = outDev ? static_cast<void*>(this->out.devWriteBuf) : static_cast<void*>(this->out.writeBuf);
        const int link = outDev ? QDSP_HIP_LINK_DEVICE : QDSP_HIP_LINK_HOST;
        const int rc = ex(this->handle, src, in->linkIn(), count, dst, link);
        in->flush();
        if (rc < 0) { return hipBlockFail(name, rc); }
        this->out.markWritten(link);
        return this->out.swap(rc) ? count : -1;
    }

private:
    typename hb::process_fn ex;
    const char* name;
};

// `call` on the stage `which` of a chain; a refusal is reported under `who`.  true: accepted.
template <class F> bool onStage(int (*stageOf)(void*, int, void**), void* chain, int which, const char* who, F call) {
    if (!chain) { return false; }
    void* s = nullptr;
    int rc = stageOf(chain, which, &s);
    if (rc == 0) { rc = call(s); }
    if (rc != 0) { hipBlockFail(who, rc); }
    return rc == 0;
}
}  // namespace detail

template <int ORDER, bool OFFSET>
class PSKDemod : public generic_hier_block<PSKDemod<ORDER, OFFSET>> {
    static_assert(ORDER == 2 || ORDER == 4 || ORDER == 8, "PSKDemod<ORDER>: ORDER is 2, 4 or 8");
    using hier = generic_hier_block<PSKDemod<ORDER, OFFSET>>;

public:
    PSKDemod() {}
    PSKDemod(stream<complex_t>* input, float sampleRate, float baudRate, int RRCTapCount = 32, float RRCAlpha = 0.32f, float agcRate = 10e-4, float costasLoopBw = 0.004f, float omegaGain = (0.01*0.01) / 4, float muGain = 0.01f, float omegaRelLimit = 0.005f) {
        init(input, sampleRate, baudRate, RRCTapCount, RRCAlpha, agcRate, costasLoopBw, omegaGain, muGain, omegaRelLimit);
    }

    ~PSKDemod() { hier::stop(); }

    void init(stream<complex_t>* input, float sampleRate, float baudRate, int RRCTapCount = 32, float RRCAlpha = 0.32f, float agcRate = 10e-4, float costasLoopBw = 0.004f, float omegaGain = (0.01*0.01) / 4, float muGain = 0.01f, float omegaRelLimit = 0.005f) {
        _RRCTapCount = RRCTapCount;
        _RRCAlpha = RRCAlpha;
        _sampleRate = sampleRate;
        _agcRate = agcRate;
        _costasLoopBw = costasLoopBw;
        _baudRate = baudRate;
        _omegaGain = omegaGain;
        _muGain = muGain;
        _omegaRelLimit = omegaRelLimit;

        taps.init(_RRCTapCount, _sampleRate, _baudRate, _RRCAlpha);
        loadTaps();
        const int rc = qdsp_hip_psk_create(block.slot(), detail::hipDeviceForBlocks(), ORDER, OFFSET ? 1 : 0, 1, STREAM_BUFFER_SIZE, coeffs.data(),
                                           (int)coeffs.size(), _agcRate, _costasLoopBw, _sampleRate / _baudRate, _omegaGain, _muGain, _omegaRelLimit);
        block.attachTo(input, rc, "PSKDemod::init");
        hier::registerBlock(&block);
        out = &block.out;
    }

    void setInput(stream<complex_t>* input) { block.setInput(input); }

    void setSampleRate(float sampleRate) {
        block.change([&] {
            taps.setSampleRate(sampleRate);
            if (retime("PSKDemod::setSampleRate", sampleRate / _baudRate)) { _sampleRate = sampleRate; }
            else { taps.setSampleRate(_sampleRate); }
        });
    }

    void setBaudRate(float baudRate) {
        block.change([&] {
            taps.setBaudRate(baudRate);
            if (retime("PSKDemod::setBaudRate", _sampleRate / baudRate)) { _baudRate = baudRate; }
            else { taps.setBaudRate(_baudRate); }
        });
    }

    void setRRCParams(int RRCTapCount, float RRCAlpha) {
        block.change([&] {
            taps.setTapCount(RRCTapCount);
            taps.setAlpha(RRCAlpha);
            if (pushTaps("PSKDemod::setRRCParams")) {
                _RRCTapCount = RRCTapCount;
                _RRCAlpha = RRCAlpha;
            } else {
                taps.setTapCount(_RRCTapCount);
                taps.setAlpha(_RRCAlpha);
            }
        });
    }

    void setAgcRate(float agcRate) {
        block.change([&] {
            if (stage(QDSP_HIP_PSK_AGC, "PSKDemod::setAgcRate", [&](void* s) { return qdsp_hip_cagc_set(s, 0, 1.0f, 65535, agcRate); })) { _agcRate = agcRate; }
        });
    }

    void setCostasLoopBw(float costasLoopBw) {
        block.change([&] {
            if (stage(QDSP_HIP_PSK_COSTAS, "PSKDemod::setCostasLoopBw", [&](void* s) { return qdsp_hip_costas_set_bandwidth(s, 0, costasLoopBw); })) {
                _costasLoopBw = costasLoopBw;
            }
        });
    }

    void setMMGains(float omegaGain, float myGain) {
        block.change([&] {
            if (stage(QDSP_HIP_PSK_CLOCK, "PSKDemod::setMMGains", [&](void* s) { return qdsp_hip_mmcr_set_gains(s, 0, omegaGain, myGain); })) {
                _omegaGain = omegaGain;
                _muGain = myGain;
            }
        });
    }

    void setOmegaRelLimit(float omegaRelLimit) {
        block.change([&] {
            if (stage(QDSP_HIP_PSK_CLOCK, "PSKDemod::setOmegaRelLimit", [&](void* s) { return qdsp_hip_mmcr_set_limit(s, 0, omegaRelLimit); })) {
                _omegaRelLimit = omegaRelLimit;
            }
        });
    }

    stream<complex_t>* out = NULL;

private:
    template <class F> bool stage(int which, const char* who, F call) { return detail::onStage(qdsp_hip_psk_stage, block.chain(), which, who, call); }

    // FIR<T>::loadTaps (dsp/filter.h): `count | 1` taps computed and normalised, the first `count` used
    void loadTaps() {
        const int n = taps.getTapCount();
        coeffs.assign(n > 0 ? (size_t)n + 1 : 1, 0.0f);
        taps.createTaps(coeffs.data(), n);
        coeffs.resize(n > 0 ? n : 0);
    }

    bool pushTaps(const char* who) {
        loadTaps();
        return stage(QDSP_HIP_PSK_RRC, who, [&](void* s) { return qdsp_hip_rowfir_set_taps(s, -1, coeffs.data(), (int)coeffs.size()); });
    }

    // a new rate ratio: the symbol period first (the stage that can refuse), then the taps of the same ratio
    bool retime(const char* who, float omega) {
        if (!stage(QDSP_HIP_PSK_CLOCK, who, [&](void* s) { return qdsp_hip_mmcr_set_omega(s, 0, omega); })) { return false; }
        return pushTaps(who);
    }

    detail::chain_block<complex_t> block{qdsp_hip_psk_process_ex, qdsp_hip_psk_destroy, "PSKDemod::run"};
    dsp::RRCTaps taps;
    std::vector<float> coeffs;

    int _RRCTapCount = 32;
    float _RRCAlpha = 0.32f;
    float _sampleRate = 1.0f;
    float _agcRate = 10e-4;
    float _baudRate = 1.0f;
    float _costasLoopBw = 0.004f;
    float _omegaGain = (0.01 * 0.01) / 4;
    float _muGain = 0.01f;
    float _omegaRelLimit = 0.005f;
};

class MSKDemod : public generic_hier_block<MSKDemod> {
    using hier = generic_hier_block<MSKDemod>;

public:
    MSKDemod() {}
    MSKDemod(stream<complex_t>* input, float sampleRate, float deviation, float baudRate, float omegaGain = (0.01*0.01) / 4, float muGain = 0.01f, float omegaRelLimit = 0.005f) {
        init(input, sampleRate, deviation, baudRate, omegaGain, muGain, omegaRelLimit);   // (the reference drops the last three)
    }

    ~MSKDemod() { hier::stop(); }

    void init(stream<complex_t>* input, float sampleRate, float deviation, float baudRate, float omegaGain = (0.01*0.01) / 4, float muGain = 0.01f, float omegaRelLimit = 0.005f) {
        _sampleRate = sampleRate;
        _deviation = deviation;
        _baudRate = baudRate;
        _omegaGain = omegaGain;
        _muGain = muGain;
        _omegaRelLimit = omegaRelLimit;

        const int rc = qdsp_hip_msk_create(block.slot(), detail::hipDeviceForBlocks(), 1, STREAM_BUFFER_SIZE, _sampleRate, _deviation,
                                           _sampleRate / _baudRate, _omegaGain, _muGain, _omegaRelLimit);
        block.attachTo(input, rc, "MSKDemod::init");
        hier::registerBlock(&block);
        out = &block.out;
    }

    void setInput(stream<complex_t>* input) { block.setInput(input); }

    void setSampleRate(float sampleRate) {
        block.change([&] {
            if (!stage(QDSP_HIP_MSK_CLOCK, "MSKDemod::setSampleRate", [&](void* s) { return qdsp_hip_mmcr_set_omega(s, 0, sampleRate / _baudRate); })) { return; }
            if (stage(QDSP_HIP_MSK_FM, "MSKDemod::setSampleRate", [&](void* s) { return qdsp_hip_demod_set_fm(s, 0, sampleRate, _deviation); })) {
                _sampleRate = sampleRate;
            }
        });
    }

    void setDeviation(float deviation) {
        block.change([&] {
            if (stage(QDSP_HIP_MSK_FM, "MSKDemod::setDeviation", [&](void* s) { return qdsp_hip_demod_set_fm(s, 0, _sampleRate, deviation); })) {
                _deviation = deviation;
            }
        });
    }

    // (as in MMClockRecovery::setOmega the limit is not applied here: it stays the one of init() / setOmegaRelLimit())
    void setBaudRate(float baudRate, float omegaRelLimit) {
        (void)omegaRelLimit;
        block.change([&] {
            if (stage(QDSP_HIP_MSK_CLOCK, "MSKDemod::setBaudRate", [&](void* s) { return qdsp_hip_mmcr_set_omega(s, 0, _sampleRate / baudRate); })) {
                _baudRate = baudRate;
            }
        });
    }

    void setMMGains(float omegaGain, float myGain) {
        block.change([&] {
            if (stage(QDSP_HIP_MSK_CLOCK, "MSKDemod::setMMGains", [&](void* s) { return qdsp_hip_mmcr_set_gains(s, 0, omegaGain, myGain); })) {
                _omegaGain = omegaGain;
                _muGain = myGain;
            }
        });
    }

    void setOmegaRelLimit(float omegaRelLimit) {
        block.change([&] {
            if (stage(QDSP_HIP_MSK_CLOCK, "MSKDemod::setOmegaRelLimit", [&](void* s) { return qdsp_hip_mmcr_set_limit(s, 0, omegaRelLimit); })) {
                _omegaRelLimit = omegaRelLimit;
            }
        });
    }

    stream<float>* out = NULL;

private:
    template <class F> bool stage(int which, const char* who, F call) { return detail::onStage(qdsp_hip_msk_stage, block.chain(), which, who, call); }

    detail::chain_block<float> block{qdsp_hip_msk_process_ex, qdsp_hip_msk_destroy, "MSKDemod::run"};

    float _sampleRate = 1.0f;
    float _deviation = 1.0f;
    float _baudRate = 1.0f;
    float _omegaGain = (0.01 * 0.01) / 4;
    float _muGain = 0.01f;
    float _omegaRelLimit = 0.005f;
};

}  // namespace dsp
