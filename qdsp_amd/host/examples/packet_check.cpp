// packet_check -- source -> FalconPacketSync -> sink of the C++ block mirror (dsp/falcon_packet.h), file in, file out.
//
//   packet_check <dev|host> <in> <out> <framesPerBlock>
//       <in>: frames of 1275 bytes (what FalconRS emits: a 4-byte header and 1191 data bytes are read of each), back to back; a
//       block of the graph holds <framesPerBlock> of them (the reference's case is 1), the last block what is left.
//       dev: the source leaves its blocks in the stream's device buffers, as a HIP-backed neighbour would (the link
//       FalconPacketSync asks for when it registers its input); host: the same graph over the host buffers.
//       <out> receives every packet, one per out.swap(): a little-endian uint32 length and then the bytes.
// The number of packets is not known in advance, so FalconPacketSync runs on the main thread, one run() per input block, while its
// neighbours run as workers.  Prints "graph ok: ..." and returns 0 when every block has gone through and the sink has taken the
// last packet.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include <dsp/falcon_packet.h>
#include <dsp/sink.h>

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

// the bytes of a file in blocks, in the stream's host buffers or -- where the consumer reads device memory -- in its device buffers
class FileSource : public generic_block<FileSource> {
public:
    FileSource(std::vector<uint8_t> bytes, size_t block, bool onDevice) : data(std::move(bytes)), block(block), onDevice(onDevice) {
        generic_block<FileSource>::registerOutput(&out);
    }
    ~FileSource() { generic_block<FileSource>::stop(); }

    int run() override {
        if (pos >= data.size()) { return -1; }
        const size_t n = std::min(block, data.size() - pos);
        int link = QDSP_HIP_LINK_HOST;
        if (onDevice && out.consumerTakesDevice && out.ensureDevice(detail::hipDeviceForBlocks())) {
            if (qdsp_hip_memcpy_h2d(detail::hipDeviceForBlocks(), out.devWriteBuf, data.data() + pos, n) != 0) { failed = true; return -1; }
            link = QDSP_HIP_LINK_DEVICE;
            deviceBlocks++;
        } else {
            memcpy(out.writeBuf, data.data() + pos, n);
        }
        pos += n;
        out.markWritten(link);
        return out.swap((int)n) ? (int)n : -1;
    }

    stream<uint8_t> out;
    std::atomic<long> deviceBlocks{0};
    std::atomic<bool> failed{false};

private:
    std::vector<uint8_t> data;
    size_t pos = 0, block;
    bool onDevice;
};

struct Writer {
    std::ofstream file;
    std::atomic<long> packets{0};
    std::atomic<bool> bad{false};
    static void push(uint8_t* src, int count, void* ctx) {
        Writer* w = static_cast<Writer*>(ctx);
        if (count < 1 || count > QDSP_HIP_FPKT_MAX_PACKET) { w->bad = true; return; }
        const uint32_t n = (uint32_t)count;
        const unsigned char le[4] = {(unsigned char)n, (unsigned char)(n >> 8), (unsigned char)(n >> 16), (unsigned char)(n >> 24)};
        w->file.write(reinterpret_cast<const char*>(le), 4);
        w->file.write(reinterpret_cast<const char*>(src), (std::streamsize)count);
        w->packets++;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: packet_check <dev|host> <in> <out> <framesPerBlock>\n");
        return 2;
    }
    const std::string link = argv[1];
    const long per = atol(argv[4]);
    if ((link != "dev" && link != "host") || per < 1 || per * FalconPacketSync::frameIn > STREAM_BUFFER_SIZE) {
        fprintf(stderr, "link: dev | host; framesPerBlock: 1 .. %d\n", (int)(STREAM_BUFFER_SIZE / FalconPacketSync::frameIn));
        return 2;
    }
    std::vector<uint8_t> bytes = readAll(argv[2]);
    const size_t total = bytes.size(), block = (size_t)per * FalconPacketSync::frameIn;
    const long nblocks = (long)((total + block - 1) / block);
    Writer w;
    w.file.open(argv[3], std::ios::binary);
    const auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
    long deviceBlocks = 0;
    {
        FileSource src(std::move(bytes), block, link == "dev");
        FalconPacketSync ps(&src.out);
        if (link == "host") { src.out.releaseConsumer(); }
        HandlerSink<uint8_t> sink(&ps.out, Writer::push, &w);
        sink.start();
        src.start();
        for (long b = 0; b < nblocks && rc == 0; b++) {
            if (ps.run() < 0) { fprintf(stderr, "FalconPacketSync::run failed at block %ld\n", b); rc = 4; }
        }
        if (rc == 0 && !ps.out.waitFlushed()) { rc = 4; }
        if (hipBlockErrors() > 0 || src.failed.load()) { rc = 4; }
        src.stop();
        sink.stop();
        deviceBlocks = src.deviceBlocks.load();
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    w.file.close();
    if (rc != 0) { fprintf(stderr, "a block failed\n"); return rc; }
    if (w.bad.load()) { fprintf(stderr, "a packet of an impossible size\n"); return 5; }
    if ((link == "dev") != (deviceBlocks > 0)) { fprintf(stderr, "the link was not the one asked for\n"); return 6; }
    printf("graph ok: %zu bytes in, %ld packets out, %ld blocks (%ld in device memory), %s link, %.1f ms\n", total, w.packets.load(), nblocks,
           deviceBlocks, link.c_str(), ms);
    return 0;
}
