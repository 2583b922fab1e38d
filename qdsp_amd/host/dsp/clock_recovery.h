// dsp/clock_recovery.h -- dsp::MMClockRecovery<T> (T = float or complex_t), HIP-backed.
//
// Drop-in for src/dsp/clock_recovery.h:68-243: both constructors, init(), setOmega(), setGains(), setOmegaRelLimit(), setInput(),
// run() and `out`.  The loop -- mu, the dynamic omega, the position of the next symbol, the detector's memory and the last seven
// samples -- lives on the device (qdsp_hip_mmcr_*); a run() hands over as many symbols as the block of samples held.  The count is
// only known once the kernel has run, so run() waits for it: the output link is the host buffer or the device buffer, never a
// pipelined or deferred one, whatever the consumer would take.  A setter acts from the next run().  Departures:
// parameters outside the library's rule (finite, omega (1 - limit) - |muGain| >= 1, omega (1 + limit) + |muGain| < 2^20) are refused --
// the block reports the error and keeps the previous ones; setOmega() forms the bounds from the new omega (the reference's from the
// old one); the delay line starts as zeros; a NaN phase error stops
// the block's output until the next init().  EdgeTrigClockRecovery and MMClockRecovery<stereo_t> are not provided.
#pragma once
#include <type_traits>

#include "block.h"
#include "hip_block.h"

namespace dsp {

template <class T>
class MMClockRecovery : public detail::hip_block<T, T> {
    static_assert(std::is_same<T, complex_t>::value || std::is_same<T, float>::value, "MMClockRecovery<T>: T is complex_t or float");
    using hb = detail::hip_block<T, T>;

public:
    MMClockRecovery() : hb(qdsp_hip_mmcr_process_ex, qdsp_hip_mmcr_destroy, "MMClockRecovery::run", true) {}

    MMClockRecovery(stream<T>* in, float omega, float gainOmega, float muGain, float omegaRelLimit) : MMClockRecovery() {
        init(in, omega, gainOmega, muGain, omegaRelLimit);
    }

    void init(stream<T>* in, float omega, float gainOmega, float muGain, float omegaRelLimit) {
        _omega = omega;
        _gainOmega = gainOmega;
        _muGain = muGain;
        _omegaRelLimit = omegaRelLimit;
        const int rc = qdsp_hip_mmcr_create(&this->handle, detail::hipDeviceForBlocks(), std::is_same<T, complex_t>::value ? 1 : 0, 1,
                                            STREAM_BUFFER_SIZE, omega, gainOmega, muGain, omegaRelLimit);
        hb::attach(in, rc, "MMClockRecovery::init");
    }

    // (as in the reference the second argument is not used: the limit stays the one of init() / setOmegaRelLimit())
    void setOmega(float omega, float omegaRelLimit) {
        (void)omegaRelLimit;
        hb::paused([&] {
            if (!this->handle) { return; }
            const int rc = qdsp_hip_mmcr_set_omega(this->handle, 0, omega);
            if (rc == 0) { _omega = omega; }
            else { detail::hipBlockFail("MMClockRecovery::setOmega", rc); }
        });
    }

    void setGains(float omegaGain, float muGain) {
        hb::paused([&] {
            if (!this->handle) { return; }
            const int rc = qdsp_hip_mmcr_set_gains(this->handle, 0, omegaGain, muGain);
            if (rc == 0) { _gainOmega = omegaGain; _muGain = muGain; }
            else { detail::hipBlockFail("MMClockRecovery::setGains", rc); }
        });
    }

    void setOmegaRelLimit(float omegaRelLimit) {
        hb::paused([&] {
            if (!this->handle) { return; }
            const int rc = qdsp_hip_mmcr_set_limit(this->handle, 0, omegaRelLimit);
            if (rc == 0) { _omegaRelLimit = omegaRelLimit; }
            else { detail::hipBlockFail("MMClockRecovery::setOmegaRelLimit", rc); }
        });
    }

    int run() override {
        const int count = hb::take();
        if (count < 0) { return -1; }
        stream<T>* in = this->_in;
        const bool outDev = this->out.consumerTakesDevice && this->out.ensureDevice(detail::hipDeviceForBlocks());
        const void* src = in->readOnDevice ? static_cast<const void*>(in->devReadBuf) : static_cast<const void*>(in->readBuf);
        void* dst = outDev ? static_cast<void*>(this->out.devWriteBuf) : static_cast<void*>(this->out.writeBuf);
        const int link = outDev ? QDSP_HIP_LINK_DEVICE : QDSP_HIP_LINK_HOST;
        const int rc = qdsp_hip_mmcr_process_ex(this->handle, src, in->linkIn(), count, dst, link);
        in->flush();
        if (rc < 0) { return detail::hipBlockFail("MMClockRecovery::run", rc); }
        this->out.markWritten(link);
        return this->out.swap(rc) ? count : -1;
    }

private:
    float _omega = 1.0f, _gainOmega = 0.001f, _muGain = 1.0f, _omegaRelLimit = 0.005f;
};

}  // namespace dsp
