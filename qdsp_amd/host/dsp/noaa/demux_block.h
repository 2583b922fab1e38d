// dsp/noaa/demux_block.h -- what the three NOAA demultiplexers of this mirror share (hrpt.h, tip.h): one input stream<uint8_t>, one
// libqdsp_hip handle, several output streams.  A read of `count` bytes holds count / item whole items (the reference's case is
// exactly one; bytes behind the last whole item are dropped); the library is called once per read, with the input on the device
// where the neighbour is HIP-backed, and the results come back in one piece to the host, from where every item goes out with the
// reference's own sequence of swap()s.
#pragma once
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "../block.h"
#include "../hip_block.h"

namespace dsp {
namespace noaa {
namespace detail {

class demux_block : public generic_block<demux_block> {
protected:
    using base = generic_block<demux_block>;
    using destroy_fn = void (*)(void*);

    demux_block(destroy_fn d, int item) : destroyFn(d), item(item) {}

    // (a derived class calls halt() at the top of its destructor: the worker reads its members)
    ~demux_block() {
        halt();
        if (handle) { destroyFn(handle); }
    }

    void halt() {
        const bool live = base::running;
        base::stop();
        if (live && _in) { _in->releaseConsumer(); }
    }

    int maxItems() const { return STREAM_BUFFER_SIZE / item + 1; }

    // rc: what creating `handle` returned
    void attach(stream<uint8_t>* in, int rc, const char* who) {
        if (rc != 0) { handle = nullptr; dsp::detail::hipBlockFail(who, rc); }
        _in = in;
        base::registerInput(_in);
        _in->claimConsumer(handle != nullptr, true);
    }

    void addOutput(untyped_steam* s) { base::registerOutput(s); }

    // the next read: its whole items, or -1 to end the worker; `count` receives its bytes
    int take(int& count) {
        count = _in->read();
        if (count < 0 || !handle) { return -1; }
        return count / item;
    }
    const void* src() const { return _in->readOnDevice ? static_cast<const void*>(_in->devReadBuf) : static_cast<const void*>(_in->readBuf); }

    // n elements at `from` into the stream's write buffer and out; false: the block is being stopped
    template <class T> static bool emit(stream<T>& s, const T* from, int n) {
        memcpy(s.writeBuf, from, (size_t)n * sizeof(T));
        s.markWritten(QDSP_HIP_LINK_HOST);
        return s.swap(n);
    }

public:
    void setInput(stream<uint8_t>* in) {
        std::lock_guard<std::mutex> lck(base::ctrlMtx);
        base::tempStop();
        base::unregisterInput(_in);
        _in->releaseConsumer();
        _in = in;
        _in->claimConsumer(handle != nullptr, true);
        base::registerInput(_in);
        base::tempStart();
    }

protected:
    destroy_fn destroyFn;
    int item;
    stream<uint8_t>* _in = nullptr;
    void* handle = nullptr;
};

}  // namespace detail
}  // namespace noaa
}  // namespace dsp
