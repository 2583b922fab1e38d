// noaa_check -- the reference's NOAA HRPT demultiplexer graph on the C++ block mirror (dsp/noaa/hrpt.h, dsp/noaa/tip.h), file in,
// files out:
//
//   source of packed frames -> HRPTDemux -+-> AVHRRChan1Out .. 5Out -> sinks
//                                         +-> AIPOut -> sink
//                                         +-> TIPOut -> TIPDemux -+-> SEMOut, DCSOut, SBUVOut -> sinks
//                                                                 +-> HIRSOut -> HIRSDemux -> radChannels[0 .. 19] -> sinks
//
//   noaa_check <dev|host> <in> <outdir> <framesPerBlock>
//       <in>: frames of 13863 bytes (what a Deframer(110900) emits), back to back; a block of the graph holds <framesPerBlock> of
//       them (the reference's case is 1), the last block what is left.
//       host: a HandlerSource fills the stream's host buffers, as in the reference's program; dev: the source leaves its blocks in
//       the stream's device buffers, as a HIP-backed neighbour would (the link HRPTDemux asks for when it registers its input).
//       <outdir> receives one file per sink, 29 in all: avhrr1 .. avhrr5, aip, sem, dcs, sbuv, hirs01 .. hirs20.
// Every block of the graph runs as a worker.  The end is found along the chain: a demultiplexer releases its input only at the end
// of its run(), as the reference's does, so once the source has handed over its last block, a released stream means that the block
// behind it has emitted everything that block gave rise to.  Prints one line per output (items, elements, FNV-1a checksum) and
// "graph ok: ..." and returns 0 when every block has gone through.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include <dsp/noaa/hrpt.h>
#include <dsp/noaa/tip.h>
#include <dsp/sink.h>
#include <dsp/source.h>

using namespace dsp;

namespace {

std::vector<uint8_t> readAll(const char* path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<uint8_t> v((size_t)f.tellg());
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)v.size());
    return v;
}

// the frames in blocks; `done` once the last block has been handed over
struct Feed {
    std::vector<uint8_t> data;
    size_t pos = 0, block = 0;
    std::atomic<bool> done{false};
    std::atomic<long> blocks{0};

    size_t next() const { return std::min(block, data.size() - pos); }
    static int fill(uint8_t* dst, void* ctx) {
        Feed* f = static_cast<Feed*>(ctx);
        if (f->pos >= f->data.size()) { f->done = true; return -1; }
        const size_t n = f->next();
        memcpy(dst, f->data.data() + f->pos, n);
        f->pos += n;
        f->blocks++;
        return (int)n;
    }
};

// the same blocks left in the stream's device buffers
class DeviceSource : public generic_block<DeviceSource> {
public:
    DeviceSource(Feed* feed) : feed(feed) { generic_block<DeviceSource>::registerOutput(&out); }
    ~DeviceSource() { generic_block<DeviceSource>::stop(); }

    int run() override {
        if (feed->pos >= feed->data.size()) { feed->done = true; return -1; }
        const size_t n = feed->next();
        int link = QDSP_HIP_LINK_HOST;
        if (out.consumerTakesDevice && out.ensureDevice(detail::hipDeviceForBlocks())) {
            if (qdsp_hip_memcpy_h2d(detail::hipDeviceForBlocks(), out.devWriteBuf, feed->data.data() + feed->pos, n) != 0) { failed = true; return -1; }
            link = QDSP_HIP_LINK_DEVICE;
            deviceBlocks++;
        } else {
            memcpy(out.writeBuf, feed->data.data() + feed->pos, n);
        }
        feed->pos += n;
        feed->blocks++;
        out.markWritten(link);
        return out.swap((int)n) ? (int)n : -1;
    }

    stream<uint8_t> out;
    std::atomic<long> deviceBlocks{0};
    std::atomic<bool> failed{false};

private:
    Feed* feed;
};

template <class T> struct Tap {
    std::string name;
    int item = 0;
    std::ofstream file;
    std::atomic<long> items{0}, elems{0};
    std::atomic<bool> bad{false};
    uint64_t hash = 1469598103934665603ull;      // FNV-1a over the bytes (the sink's thread only, read after it has stopped)
    HandlerSink<T> sink;

    stream<T>* in;

    Tap(stream<T>* in, const std::string& dir, const std::string& name, int item) : name(name), item(item), in(in) {
        file.open(dir + "/" + name + ".bin", std::ios::binary);
        sink.init(in, push, this);
    }
    // the sink has taken the last item its producer handed over
    bool drained() { return in->waitFlushed(); }
    static void push(T* src, int count, void* ctx) {
        Tap* t = static_cast<Tap*>(ctx);
        if (count != t->item) { t->bad = true; }
        const unsigned char* b = reinterpret_cast<const unsigned char*>(src);
        for (size_t i = 0; i < (size_t)count * sizeof(T); i++) { t->hash = (t->hash ^ b[i]) * 1099511628211ull; }
        t->file.write(reinterpret_cast<const char*>(src), (std::streamsize)((size_t)count * sizeof(T)));
        t->items++;
        t->elems += count;
    }
    bool report() {
        file.close();
        printf("%-7s %8ld items %10ld elements  fnv1a %016llx\n", name.c_str(), items.load(), elems.load(), (unsigned long long)hash);
        return !bad.load() && (bool)file;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: noaa_check <dev|host> <in> <outdir> <framesPerBlock>\n");
        return 2;
    }
    const std::string link = argv[1], dir = argv[3];
    const long per = atol(argv[4]);
    if ((link != "dev" && link != "host") || per < 1 || per * noaa::HRPTDemux::frameBytes > STREAM_BUFFER_SIZE) {
        fprintf(stderr, "link: dev | host; framesPerBlock: 1 .. %d\n", (int)(STREAM_BUFFER_SIZE / noaa::HRPTDemux::frameBytes));
        return 2;
    }
    Feed feed;
    feed.data = readAll(argv[2]);
    feed.block = (size_t)per * noaa::HRPTDemux::frameBytes;
    const size_t total = feed.data.size();
    const auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
    long deviceBlocks = 0;
    bool tapsOk = true;
    {
        HandlerSource<uint8_t> hostSrc;
        std::unique_ptr<DeviceSource> devSrc;
        stream<uint8_t>* packedIn;
        if (link == "dev") {
            devSrc.reset(new DeviceSource(&feed));
            packedIn = &devSrc->out;
        } else {
            hostSrc.init(Feed::fill, &feed);
            packedIn = &hostSrc.out;
        }
        noaa::HRPTDemux demux(packedIn);
        if (link == "host") { packedIn->releaseConsumer(); }
        noaa::TIPDemux tipDemux(&demux.TIPOut);
        noaa::HIRSDemux hirsDemux(&tipDemux.HIRSOut);

        std::vector<std::unique_ptr<Tap<uint16_t>>> wide;
        std::vector<std::unique_ptr<Tap<uint8_t>>> narrow;
        stream<uint16_t>* av[5] = {&demux.AVHRRChan1Out, &demux.AVHRRChan2Out, &demux.AVHRRChan3Out, &demux.AVHRRChan4Out, &demux.AVHRRChan5Out};
        for (int c = 0; c < 5; c++) { wide.emplace_back(new Tap<uint16_t>(av[c], dir, "avhrr" + std::to_string(c + 1), 2048)); }
        narrow.emplace_back(new Tap<uint8_t>(&demux.AIPOut, dir, "aip", 104));
        narrow.emplace_back(new Tap<uint8_t>(&tipDemux.SEMOut, dir, "sem", 2));
        narrow.emplace_back(new Tap<uint8_t>(&tipDemux.DCSOut, dir, "dcs", 32));
        narrow.emplace_back(new Tap<uint8_t>(&tipDemux.SBUVOut, dir, "sbuv", 4));
        for (int i = 0; i < 20; i++) {
            char nm[16];
            snprintf(nm, sizeof(nm), "hirs%02d", i + 1);
            wide.emplace_back(new Tap<uint16_t>(&hirsDemux.radChannels[i], dir, nm, 56));
        }
        for (auto& t : wide) { t->sink.start(); }
        for (auto& t : narrow) { t->sink.start(); }
        hirsDemux.start();
        tipDemux.start();
        demux.start();
        if (devSrc) { devSrc->start(); } else { hostSrc.start(); }

        while (!feed.done.load() && hipBlockErrors() == 0 && !(devSrc && devSrc->failed.load())) { std::this_thread::sleep_for(std::chrono::microseconds(200)); }
        // the last block is in packedIn; each wait below ends when the block behind the stream has finished the run() that read it
        if (hipBlockErrors() == 0) {
            if (!packedIn->waitFlushed() || !demux.TIPOut.waitFlushed() || !tipDemux.HIRSOut.waitFlushed()) { rc = 4; }
            for (auto& t : wide) { if (!t->drained()) { rc = 4; } }
            for (auto& t : narrow) { if (!t->drained()) { rc = 4; } }
        }
        if (hipBlockErrors() > 0 || (devSrc && devSrc->failed.load())) { rc = 4; }
        if (devSrc) { devSrc->stop(); deviceBlocks = devSrc->deviceBlocks.load(); } else { hostSrc.stop(); }
        demux.stop();
        tipDemux.stop();
        hirsDemux.stop();
        for (auto& t : wide) { t->sink.stop(); }
        for (auto& t : narrow) { t->sink.stop(); }
        for (auto& t : wide) { tapsOk = t->report() && tapsOk; }
        for (auto& t : narrow) { tapsOk = t->report() && tapsOk; }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != 0) { fprintf(stderr, "a block failed\n"); return rc; }
    if (!tapsOk) { fprintf(stderr, "an item of the wrong size, or a file that could not be written\n"); return 5; }
    if ((link == "dev") != (deviceBlocks > 0)) { fprintf(stderr, "the link was not the one asked for\n"); return 6; }
    printf("graph ok: %zu bytes in, %ld blocks (%ld in device memory), %s link, %.1f ms\n", total, feed.blocks.load(), deviceBlocks, link.c_str(), ms);
    return 0;
}
