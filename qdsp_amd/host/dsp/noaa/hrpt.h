// dsp/noaa/hrpt.h -- dsp::noaa::HRPTDemux, HIP-backed.
//
// Drop-in for src/dsp/noaa/hrpt.h: both constructors, init(), setInput(), run(), TIPOut, AIPOut and AVHRRChan1Out .. 5Out.  The
// AVHRR split, the `minor` scan and the TIP / AIP gather run on the device (qdsp_hip_hrpt_*: hrpt_avhrr_kernel, hrpt_scan_kernel,
// hrpt_gather_kernel).  A read of `count` bytes holds count / 13863 whole frames; the library is called once per read, and every
// frame then goes out as in the reference: five TIPOut.swap(104) or five AIPOut.swap(104) where the frame carries them, then
// AVHRRChan1Out .. 5Out.swap(2048).
#pragma once
#include "demux_block.h"

namespace dsp {
namespace noaa {

class HRPTDemux : public detail::demux_block {
    using db = detail::demux_block;

public:
    static constexpr int frameBytes = 13863, minorFrame = 104, minorPerFrame = 5, pixels = 2048, planes = 5;

    HRPTDemux() : db(qdsp_hip_hrpt_destroy, frameBytes) {}

    HRPTDemux(stream<uint8_t>* in) : HRPTDemux() { init(in); }

    ~HRPTDemux() { db::halt(); }

    void init(stream<uint8_t>* in) {
        const int rc = qdsp_hip_hrpt_create(&handle, dsp::detail::hipDeviceForBlocks(), 1, maxItems());
        if (rc == 0) {
            avhrr.resize((size_t)maxItems() * planes * pixels);
            tip.resize((size_t)maxItems() * minorPerFrame * minorFrame);
            aip.resize(tip.size());
            slots.resize((size_t)maxItems());
        }
        db::attach(in, rc, "HRPTDemux::init");
        db::addOutput(&TIPOut);          // (the reference leaves these two out: its stop() cannot wake a swap() on them)
        db::addOutput(&AIPOut);
        db::addOutput(&AVHRRChan1Out);
        db::addOutput(&AVHRRChan2Out);
        db::addOutput(&AVHRRChan3Out);
        db::addOutput(&AVHRRChan4Out);
        db::addOutput(&AVHRRChan5Out);
    }

    int run() override {
        int count = 0;
        const int n = db::take(count);
        if (n < 0) { return -1; }
        const int rc = demux(n);
        _in->flush();                    // at the end of run(), as in the reference: a released input means its items are out
        return rc < 0 ? -1 : count;
    }

    stream<uint8_t> TIPOut;
    stream<uint8_t> AIPOut;

    stream<uint16_t> AVHRRChan1Out;
    stream<uint16_t> AVHRRChan2Out;
    stream<uint16_t> AVHRRChan3Out;
    stream<uint16_t> AVHRRChan4Out;
    stream<uint16_t> AVHRRChan5Out;

private:
    int demux(int n) {
        int rc = qdsp_hip_hrpt_process_ex(handle, db::src(), _in->linkIn(), n, avhrr.data(), QDSP_HIP_LINK_HOST);
        if (rc == 0 && n > 0) { rc = qdsp_hip_hrpt_get_tip(handle, 0, tip.data(), n * minorPerFrame); }
        if (rc >= 0 && n > 0) { rc = qdsp_hip_hrpt_get_aip(handle, 0, aip.data(), n * minorPerFrame); }
        if (rc >= 0 && n > 0) { rc = qdsp_hip_hrpt_get_frame_slots(handle, 0, slots.data(), n); }
        if (rc < 0) { return dsp::detail::hipBlockFail("HRPTDemux::run", rc); }
        stream<uint16_t>* chans[planes] = {&AVHRRChan1Out, &AVHRRChan2Out, &AVHRRChan3Out, &AVHRRChan4Out, &AVHRRChan5Out};
        for (int f = 0; f < n; f++) {
            if (slots[f] >= 0) {
                const bool isAip = (slots[f] >> 30) != 0;
                const uint8_t* from = (isAip ? aip.data() : tip.data()) + (size_t)(slots[f] & 0x3fffffff) * minorPerFrame * minorFrame;
                for (int i = 0; i < minorPerFrame; i++) {
                    if (!db::emit(isAip ? AIPOut : TIPOut, from + (size_t)i * minorFrame, minorFrame)) { return -1; }
                }
            }
            for (int c = 0; c < planes; c++) {
                if (!db::emit(*chans[c], avhrr.data() + ((size_t)c * n + f) * pixels, pixels)) { return -1; }
            }
        }
        return 0;
    }

    std::vector<uint16_t> avhrr;    // one read's planes: [5][n][2048]
    std::vector<uint8_t> tip, aip;   // its minor frames
    std::vector<int> slots;          // per frame: where its minor frames lie (qdsp_hip_hrpt_get_frame_slots)
};

}  // namespace noaa
}  // namespace dsp
