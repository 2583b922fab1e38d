// frame_check -- source -> [Threshold ->] Deframer -> sink graphs of the C++ block mirror (dsp/processing.h, dsp/deframing.h), file
// in, file out.
//
//   frame_check <b|f> <dev|host> <in> <out> <block> <frameLen> <syncFile>
//       b: the input file holds one bit per byte and goes to the Deframer directly (the link is the host buffer either way).
//       f: the input file holds float soft symbols: source -> Threshold -> Deframer.
//       dev: the Threshold hands its blocks to the Deframer in device memory (the link the blocks set up themselves);
//       host: the same graph with that link moved to the host buffers.
//       <syncFile>: the sync word, one bit per byte.  <out> receives the frames, ceil(frameLen / 8) bytes each, one per out.swap().
// The number of frames is not known in advance, so the Deframer runs on the main thread, one run() per input block, while its
// neighbours run as workers.  Prints "graph ok: ..." and returns 0 when every input block has gone through and the sink has taken
// the last frame.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include <dsp/deframing.h>
#include <dsp/processing.h>
#include <dsp/sink.h>
#include <dsp/source.h>

using namespace dsp;

namespace {

template <class T> std::vector<T> readAll(const char* path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    const size_t bytes = (size_t)f.tellg();
    f.seekg(0);
    std::vector<T> v(bytes / sizeof(T));
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <class T> struct Feed {
    std::vector<T> data;
    size_t pos = 0;
    int block = 1;
    static int pull(T* dst, void* ctx) {
        Feed* f = static_cast<Feed*>(ctx);
        if (f->pos >= f->data.size()) { return -1; }
        const size_t n = std::min<size_t>((size_t)f->block, f->data.size() - f->pos);
        memcpy(dst, f->data.data() + f->pos, n * sizeof(T));
        f->pos += n;
        return (int)n;
    }
};

struct Writer {
    std::ofstream file;
    std::atomic<long> frames{0};
    int frameBytes = 0;
    std::atomic<bool> bad{false};
    static void push(uint8_t* src, int count, void* ctx) {
        Writer* w = static_cast<Writer*>(ctx);
        if (count != w->frameBytes) { w->bad = true; }
        if (count > 0) { w->file.write(reinterpret_cast<const char*>(src), (std::streamsize)count); }
        w->frames++;
    }
};

// the Deframer on the calling thread: one run() per input block, then the sink's release of the last frame
int drive(Deframer& def, long nblocks) {
    for (long b = 0; b < nblocks; b++) {
        if (def.run() < 0) { fprintf(stderr, "Deframer::run failed at block %ld\n", b); return 4; }
    }
    if (!def.out.waitFlushed()) { return 4; }
    return hipBlockErrors() > 0 ? 4 : 0;
}

int runBytes(const char* inPath, Writer& w, int block, int frameLen, std::vector<uint8_t>& sync, size_t& total, long& nblocks) {
    Feed<uint8_t> feed;
    feed.data = readAll<uint8_t>(inPath);
    feed.block = block;
    total = feed.data.size();
    nblocks = (long)((feed.data.size() + block - 1) / block);
    HandlerSource<uint8_t> src(Feed<uint8_t>::pull, &feed);
    Deframer def(&src.out, frameLen, sync.data(), (int)sync.size());
    HandlerSink<uint8_t> sink(&def.out, Writer::push, &w);
    sink.start();
    src.start();
    const int rc = drive(def, nblocks);
    src.stop();
    sink.stop();
    return rc;
}

int runFloats(const char* inPath, Writer& w, int block, int frameLen, std::vector<uint8_t>& sync, bool hostLink, size_t& total, long& nblocks) {
    Feed<float> feed;
    feed.data = readAll<float>(inPath);
    feed.block = block;
    total = feed.data.size();
    nblocks = (long)((feed.data.size() + block - 1) / block);
    HandlerSource<float> src(Feed<float>::pull, &feed);
    Threshold thr(&src.out);
    thr.setLevel(3.0f);            // stored, without effect (as in the reference)
    Deframer def(&thr.out, frameLen, sync.data(), (int)sync.size());
    if (hostLink) { thr.out.releaseConsumer(); }   // the Threshold writes its host buffers, the Deframer uploads them
    HandlerSink<uint8_t> sink(&def.out, Writer::push, &w);
    sink.start();
    thr.start();
    src.start();
    const int rc = drive(def, nblocks);
    src.stop();
    thr.stop();
    sink.stop();
    return thr.getLevel() == 3.0f ? rc : 4;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 8) {
        fprintf(stderr, "usage: frame_check <b|f> <dev|host> <in> <out> <block> <frameLen> <syncFile>\n");
        return 2;
    }
    const std::string kind = argv[1], link = argv[2];
    if ((kind != "b" && kind != "f") || (link != "dev" && link != "host")) { fprintf(stderr, "kind: b | f; link: dev | host\n"); return 2; }
    const int block = atoi(argv[5]), frameLen = atoi(argv[6]);
    if (block < 1 || block > STREAM_BUFFER_SIZE) { fprintf(stderr, "block: 1 .. %d\n", (int)STREAM_BUFFER_SIZE); return 2; }
    std::vector<uint8_t> sync = readAll<uint8_t>(argv[7]);
    if (frameLen < 1 || sync.empty()) { fprintf(stderr, "frameLen >= 1 and a sync word of at least one byte\n"); return 2; }
    Writer w;
    w.frameBytes = (frameLen + 7) / 8;
    w.file.open(argv[4], std::ios::binary);
    size_t total = 0;
    long nblocks = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = kind == "b" ? runBytes(argv[3], w, block, frameLen, sync, total, nblocks)
                               : runFloats(argv[3], w, block, frameLen, sync, link == "host", total, nblocks);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    w.file.close();
    if (rc != 0) { fprintf(stderr, "a block failed\n"); return rc; }
    if (w.bad.load()) { fprintf(stderr, "a frame of the wrong size\n"); return 5; }
    printf("graph ok: %zu in, %ld frames out, %ld blocks, %s link, %.1f ms\n", total, w.frames.load(), nblocks, link.c_str(), ms);
    return 0;
}
