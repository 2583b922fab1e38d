// clock_check -- source -> FIR (one tap of 1.0) -> MMClockRecovery -> sink graphs of the C++ block mirror (dsp/clock_recovery.h),
// file in, file out.
//
//   clock_check <f|c> <dev|host> <in> <out> <block> <omega> [<gainOmega> <muGain> <omegaRelLimit>]
//       f: float samples and MMClockRecovery<float> (MSKDemod's); c: complex_t samples and MMClockRecovery<complex_t> (PSKDemod's).
//       dev: the FIR hands its blocks to the clock recovery in device memory (the link the blocks set up themselves);
//       host: the same graph with that link moved to the host buffers.
//       The FIR only puts a HIP-backed block in front: one tap of 1.0 copies its input bit for bit.  <out> receives the symbols;
//       the defaults of the other parameters are PSKDemod's (demodulator.h:566-682).
// Prints "graph ok: ..." and returns 0 when every input block has come out of the far end.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include <dsp/clock_recovery.h>
#include <dsp/filter.h>
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

// a file sink that counts the blocks it has written (a block may hold no symbol at all)
template <class T> struct Writer {
    std::ofstream file;
    std::atomic<long> blocks{0};
    std::atomic<long> samples{0};
    static void push(T* src, int count, void* ctx) {
        Writer* w = static_cast<Writer*>(ctx);
        if (count > 0) { w->file.write(reinterpret_cast<const char*>(src), (std::streamsize)count * sizeof(T)); }
        w->samples += count;
        w->blocks++;
    }
};

struct UnitTap : filter_window::generic_window {
    int getTapCount() override { return 1; }
    void createTaps(float* taps, int tapCount, float factor = 1.0f) override {
        (void)factor;
        if (tapCount > 0) { taps[0] = 1.0f; }
    }
};

template <class T>
int runGraph(const char* inPath, const char* outPath, int block, bool hostLink, float omega, float gainOmega, float muGain, float relLimit) {
    Feed<T> feed;
    feed.data = readAll<T>(inPath);
    feed.block = block;
    const long nblocks = (long)((feed.data.size() + block - 1) / block);
    HandlerSource<T> src(Feed<T>::pull, &feed);
    UnitTap one;
    FIR<T> fir(&src.out, &one);
    MMClockRecovery<T> rec(&fir.out, omega, gainOmega, muGain, relLimit);
    if (hostLink) { fir.out.releaseConsumer(); }   // the FIR writes its host buffers, the clock recovery uploads them
    Writer<T> w;
    w.file.open(outPath, std::ios::binary);
    HandlerSink<T> sink(&rec.out, Writer<T>::push, &w);
    sink.start();
    rec.start();
    fir.start();
    src.start();
    const auto t0 = std::chrono::steady_clock::now();
    while (w.blocks.load() < nblocks) {
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) { fprintf(stderr, "graph timed out\n"); return 3; }
        if (hipBlockErrors() > 0) { fprintf(stderr, "a block failed\n"); return 4; }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    src.stop();
    fir.stop();
    rec.stop();
    sink.stop();
    w.file.close();
    printf("graph ok: %zu in, %ld out, %ld blocks, %s link, %.1f ms\n", feed.data.size(), w.samples.load(), nblocks, hostLink ? "host" : "device", ms);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 7 && argc != 10) {
        fprintf(stderr, "usage: clock_check <f|c> <dev|host> <in> <out> <block> <omega> [<gainOmega> <muGain> <omegaRelLimit>]\n");
        return 2;
    }
    const std::string kind = argv[1], link = argv[2];
    if ((kind != "f" && kind != "c") || (link != "dev" && link != "host")) { fprintf(stderr, "kind: f | c; link: dev | host\n"); return 2; }
    const int block = atoi(argv[5]);
    if (block < 1 || block > STREAM_BUFFER_SIZE) { fprintf(stderr, "block: 1 .. %d\n", (int)STREAM_BUFFER_SIZE); return 2; }
    const float omega = (float)atof(argv[6]);
    const float gainOmega = argc == 10 ? (float)atof(argv[7]) : (0.01f * 0.01f) / 4.0f;
    const float muGain = argc == 10 ? (float)atof(argv[8]) : 0.01f;
    const float relLimit = argc == 10 ? (float)atof(argv[9]) : 0.005f;
    if (kind == "f") { return runGraph<float>(argv[3], argv[4], block, link == "host", omega, gainOmega, muGain, relLimit); }
    return runGraph<complex_t>(argv[3], argv[4], block, link == "host", omega, gainOmega, muGain, relLimit);
}
