// dsp/noaa/tip.h -- dsp::noaa::TIPDemux and dsp::noaa::HIRSDemux, HIP-backed.
//
// Drop-in for src/dsp/noaa/tip.h: the constructors, init(), setInput(), run(), HIRSOut / SEMOut / DCSOut / SBUVOut and
// radChannels[20].  The byte gather of TIPDemux (qdsp_hip_tip_*: tip_kernel) and the element scan and field gather of HIRSDemux
// (qdsp_hip_hirs_*: hirs_scan_kernel, hirs_pack_kernel) run on the device; lastElement, newImageData and the line in progress live
// in the library's handle.  A read of `count` bytes holds count / 104 minor frames or count / 36 packets; the library is called
// once per read, and every item then goes out as in the reference: HIRSOut.swap(36), SEMOut.swap(2), DCSOut.swap(32),
// SBUVOut.swap(4) per minor frame; radChannels[0 .. 19].swap(56) per finished line.
#pragma once
#include "demux_block.h"

namespace dsp {
namespace noaa {

class TIPDemux : public detail::demux_block {
    using db = detail::demux_block;

public:
    static constexpr int minorFrame = 104, record = QDSP_HIP_TIP_RECORD_BYTES;

    TIPDemux() : db(qdsp_hip_tip_destroy, minorFrame) {}

    TIPDemux(stream<uint8_t>* in) : TIPDemux() { init(in); }

    ~TIPDemux() { db::halt(); }

    void init(stream<uint8_t>* in) {
        const int rc = qdsp_hip_tip_create(&handle, dsp::detail::hipDeviceForBlocks(), 1, maxItems());
        if (rc == 0) { records.resize((size_t)maxItems() * record); }
        db::attach(in, rc, "TIPDemux::init");
        db::addOutput(&HIRSOut);
        db::addOutput(&SEMOut);
        db::addOutput(&DCSOut);
        db::addOutput(&SBUVOut);
    }

    int run() override {
        int count = 0;
        const int n = db::take(count);
        if (n < 0) { return -1; }
        const int rc = demux(n);
        _in->flush();                    // at the end of run(), as in the reference: a released input means its items are out
        return rc < 0 ? -1 : count;
    }

    stream<uint8_t> HIRSOut;
    stream<uint8_t> SEMOut;
    stream<uint8_t> DCSOut;
    stream<uint8_t> SBUVOut;

private:
    int demux(int n) {
        const int rc = qdsp_hip_tip_process_ex(handle, db::src(), _in->linkIn(), n, records.data(), QDSP_HIP_LINK_HOST);
        if (rc != 0) { return dsp::detail::hipBlockFail("TIPDemux::run", rc); }
        for (int m = 0; m < n; m++) {
            const uint8_t* r = records.data() + (size_t)m * record;
            if (!db::emit(HIRSOut, r + QDSP_HIP_TIP_HIRS_OFFSET, QDSP_HIP_TIP_SEM_OFFSET - QDSP_HIP_TIP_HIRS_OFFSET)) { return -1; }
            if (!db::emit(SEMOut, r + QDSP_HIP_TIP_SEM_OFFSET, QDSP_HIP_TIP_DCS_OFFSET - QDSP_HIP_TIP_SEM_OFFSET)) { return -1; }
            if (!db::emit(DCSOut, r + QDSP_HIP_TIP_DCS_OFFSET, QDSP_HIP_TIP_SBUV_OFFSET - QDSP_HIP_TIP_DCS_OFFSET)) { return -1; }
            if (!db::emit(SBUVOut, r + QDSP_HIP_TIP_SBUV_OFFSET, record - QDSP_HIP_TIP_SBUV_OFFSET)) { return -1; }
        }
        return 0;
    }

    std::vector<uint8_t> records;    // one read's records
};

class HIRSDemux : public detail::demux_block {
    using db = detail::demux_block;

public:
    static constexpr int packet = 36, channels = 20, line = 56;

    HIRSDemux() : db(qdsp_hip_hirs_destroy, packet) {}

    HIRSDemux(stream<uint8_t>* in) : HIRSDemux() { init(in); }

    ~HIRSDemux() { db::halt(); }

    void init(stream<uint8_t>* in) {
        const int rc = qdsp_hip_hirs_create(&handle, dsp::detail::hipDeviceForBlocks(), 1, maxItems(), packet);
        if (rc == 0) { lines.resize(((size_t)maxItems() + 1) * channels * line); }
        db::attach(in, rc, "HIRSDemux::init");
        for (int i = 0; i < channels; i++) { db::addOutput(&radChannels[i]); }
    }

    int run() override {
        int count = 0;
        const int n = db::take(count);
        if (n < 0) { return -1; }
        const int rc = demux(n);
        _in->flush();                    // at the end of run(), as in the reference
        return rc < 0 ? -1 : count;
    }

    stream<uint16_t> radChannels[20];

private:
    int demux(int n) {
        const int got = qdsp_hip_hirs_process_ex(handle, db::src(), _in->linkIn(), n, lines.data(), QDSP_HIP_LINK_HOST);
        if (got < 0) { return dsp::detail::hipBlockFail("HIRSDemux::run", got); }
        const size_t plane = ((size_t)n + 1) * line;      // the planes of one call are out_size(n) lines apart
        for (int l = 0; l < got; l++) {
            for (int i = 0; i < channels; i++) {
                if (!db::emit(radChannels[i], lines.data() + (size_t)i * plane + (size_t)l * line, line)) { return -1; }
            }
        }
        return 0;
    }

    std::vector<uint16_t> lines;     // one read's finished lines: [20][n + 1][56]
};

}  // namespace noaa
}  // namespace dsp
