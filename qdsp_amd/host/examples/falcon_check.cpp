// falcon_check -- source -> FalconRS -> sink of the C++ block mirror (dsp/falcon_fec.h), file in, file out.
//
//   falcon_check <dev|host> <in> <out> <framesPerBlock>
//       <in>: frames of 1279 bytes (a 4-byte sync word and five interleaved RS(255, 239) codewords), back to back; a block of the
//       graph holds <framesPerBlock> of them (the reference's case is 1), the last block what is left.
//       dev: the source leaves its blocks in the stream's device buffers, as a HIP-backed neighbour would (the link FalconRS
//       asks for when it registers its input); host: the same graph over the host buffers.
//       <out> receives every good frame, 1275 bytes, one per out.swap().
// The number of good frames is not known in advance, so FalconRS runs on the main thread, one run() per input block, while its
// neighbours run as workers.  Prints "graph ok: ..." and returns 0 when every block has gone through and the sink has taken the
// last frame.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include <dsp/falcon_fec.h>
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
    std::atomic<long> frames{0};
    std::atomic<bool> bad{false};
    static void push(uint8_t* src, int count, void* ctx) {
        Writer* w = static_cast<Writer*>(ctx);
        if (count != FalconRS::frameOut) { w->bad = true; }
        if (count > 0) { w->file.write(reinterpret_cast<const char*>(src), (std::streamsize)count); }
        w->frames++;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: falcon_check <dev|host> <in> <out> <framesPerBlock>\n");
        return 2;
    }
    const std::string link = argv[1];
    const long per = atol(argv[4]);
    if ((link != "dev" && link != "host") || per < 1 || per * FalconRS::frameIn > STREAM_BUFFER_SIZE) {
        fprintf(stderr, "link: dev | host; framesPerBlock: 1 .. %d\n", (int)(STREAM_BUFFER_SIZE / FalconRS::frameIn));
        return 2;
    }
    std::vector<uint8_t> bytes = readAll(argv[2]);
    const size_t total = bytes.size(), block = (size_t)per * FalconRS::frameIn;
    const long nblocks = (long)((total + block - 1) / block);
    Writer w;
    w.file.open(argv[3], std::ios::binary);
    const auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
    long deviceBlocks = 0;
    {
        FileSource src(std::move(bytes), block, link == "dev");
        FalconRS rs(&src.out);
        if (link == "host") { src.out.releaseConsumer(); }
        HandlerSink<uint8_t> sink(&rs.out, Writer::push, &w);
        sink.start();
        src.start();
        for (long b = 0; b < nblocks && rc == 0; b++) {
            if (rs.run() < 0) { fprintf(stderr, "FalconRS::run failed at block %ld\n", b); rc = 4; }
        }
        if (rc == 0 && !rs.out.waitFlushed()) { rc = 4; }
        if (hipBlockErrors() > 0 || src.failed.load()) { rc = 4; }
        src.stop();
        sink.stop();
        deviceBlocks = src.deviceBlocks.load();
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    w.file.close();
    if (rc != 0) { fprintf(stderr, "a block failed\n"); return rc; }
    if (w.bad.load()) { fprintf(stderr, "a frame of the wrong size\n"); return 5; }
    if ((link == "dev") != (deviceBlocks > 0)) { fprintf(stderr, "the link was not the one asked for\n"); return 6; }
    printf("graph ok: %zu bytes in, %ld frames out, %ld blocks (%ld in device memory), %s link, %.1f ms\n", total, w.frames.load(), nblocks,
           deviceBlocks, link.c_str(), ms);
    return 0;
}
