// psk_check -- source -> FIR (one tap of 1.0) -> PSKDemod / MSKDemod -> sink graphs of the C++ block mirror (dsp/psk_demod.h), file in,
// file out.
//
//   psk_check <psk2|psk4|psk8|oqpsk|msk> <dev|host> <in> <out> <block> <sampleRate> <baudRate> [...]
//       psk2 / psk4 / psk8: PSKDemod<2 / 4 / 8, false>; oqpsk: PSKDemod<4, true>; msk: MSKDemod.  <in>: complex_t samples; <out>
//       receives the symbols (complex_t; msk: float).
//       dev: the FIR hands its blocks to the demodulator in device memory (the link the blocks set up themselves);
//       host: the same graph with that link moved to the host buffers.
//       The FIR only puts a HIP-backed block in front: one tap of 1.0 copies its input bit for bit.
//       [...] psk:  <RRCTapCount> <RRCAlpha> <agcRate> <costasLoopBw> <omegaGain> <muGain> <omegaRelLimit>
//             msk:  <deviation> <omegaGain> <muGain> <omegaRelLimit>
//       all of them or none; the defaults are the reference's (demodulator.h:499-682), the deviation's is sampleRate / 4.
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

#include <dsp/filter.h>
#include <dsp/psk_demod.h>
#include <dsp/sink.h>
#include <dsp/source.h>

using namespace dsp;

namespace {

std::vector<complex_t> readAll(const char* path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    const size_t bytes = (size_t)f.tellg();
    f.seekg(0);
    std::vector<complex_t> v(bytes / sizeof(complex_t));
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(complex_t)));
    return v;
}

struct Feed {
    std::vector<complex_t> data;
    size_t pos = 0;
    int block = 1;
    static int pull(complex_t* dst, void* ctx) {
        Feed* f = static_cast<Feed*>(ctx);
        if (f->pos >= f->data.size()) { return -1; }
        const size_t n = std::min<size_t>((size_t)f->block, f->data.size() - f->pos);
        memcpy(dst, f->data.data() + f->pos, n * sizeof(complex_t));
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

struct Args {
    const char *in, *out;
    int block;
    bool hostLink;
    float sampleRate, baudRate;
    int rrcTaps = 32;
    float rrcAlpha = 0.32f, agcRate = 10e-4, costasBw = 0.004f, deviation = 0.0f;
    float omegaGain = (0.01 * 0.01) / 4, muGain = 0.01f, relLimit = 0.005f;
};

// DEMOD: constructed by `make(&fir.out)`; SYM: its symbol type
template <class SYM, class MAKE>
int runGraph(const Args& a, MAKE make) {
    Feed feed;
    feed.data = readAll(a.in);
    feed.block = a.block;
    const long nblocks = (long)((feed.data.size() + a.block - 1) / a.block);
    HandlerSource<complex_t> src(Feed::pull, &feed);
    UnitTap one;
    FIR<complex_t> fir(&src.out, &one);
    auto demod = make(&fir.out);
    if (a.hostLink) { fir.out.releaseConsumer(); }   // the FIR writes its host buffers, the demodulator uploads them
    Writer<SYM> w;
    w.file.open(a.out, std::ios::binary);
    HandlerSink<SYM> sink(demod->out, Writer<SYM>::push, &w);
    sink.start();
    demod->start();
    fir.start();
    src.start();
    const auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
    while (w.blocks.load() < nblocks) {
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) { fprintf(stderr, "graph timed out\n"); rc = 3; break; }
        if (hipBlockErrors() > 0) { fprintf(stderr, "a block failed\n"); rc = 4; break; }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    src.stop();
    fir.stop();
    demod->stop();
    sink.stop();
    w.file.close();
    if (rc == 0) {
        printf("graph ok: %zu in, %ld out, %ld blocks, %s link, %.1f ms\n", feed.data.size(), w.samples.load(), nblocks, a.hostLink ? "host" : "device", ms);
    }
    delete demod;
    return rc;
}

template <int ORDER, bool OFFSET> int runPsk(const Args& a) {
    return runGraph<complex_t>(a, [&](stream<complex_t>* in) {
        return new PSKDemod<ORDER, OFFSET>(in, a.sampleRate, a.baudRate, a.rrcTaps, a.rrcAlpha, a.agcRate, a.costasBw, a.omegaGain, a.muGain, a.relLimit);
    });
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    const bool msk = mode == "msk";
    if (argc < 8 || (argc != 8 && argc != (msk ? 12 : 15))) {
        fprintf(stderr, "usage: psk_check <psk2|psk4|psk8|oqpsk|msk> <dev|host> <in> <out> <block> <sampleRate> <baudRate>\n"
                        "         [<RRCTapCount> <RRCAlpha> <agcRate> <costasLoopBw> <omegaGain> <muGain> <omegaRelLimit>]   (psk)\n"
                        "         [<deviation> <omegaGain> <muGain> <omegaRelLimit>]                                         (msk)\n");
        return 2;
    }
    const std::string link = argv[2];
    if (link != "dev" && link != "host") { fprintf(stderr, "link: dev | host\n"); return 2; }
    Args a;
    a.in = argv[3];
    a.out = argv[4];
    a.block = atoi(argv[5]);
    a.hostLink = link == "host";
    if (a.block < 1 || a.block > STREAM_BUFFER_SIZE) { fprintf(stderr, "block: 1 .. %d\n", (int)STREAM_BUFFER_SIZE); return 2; }
    a.sampleRate = (float)atof(argv[6]);
    a.baudRate = (float)atof(argv[7]);
    a.deviation = a.sampleRate / 4.0f;
    if (argc > 8) {
        int i = 8;
        if (msk) {
            a.deviation = (float)atof(argv[i++]);
        } else {
            a.rrcTaps = atoi(argv[i++]);
            a.rrcAlpha = (float)atof(argv[i++]);
            a.agcRate = (float)atof(argv[i++]);
            a.costasBw = (float)atof(argv[i++]);
        }
        a.omegaGain = (float)atof(argv[i++]);
        a.muGain = (float)atof(argv[i++]);
        a.relLimit = (float)atof(argv[i++]);
    }
    if (mode == "psk2") { return runPsk<2, false>(a); }
    if (mode == "psk4") { return runPsk<4, false>(a); }
    if (mode == "psk8") { return runPsk<8, false>(a); }
    if (mode == "oqpsk") { return runPsk<4, true>(a); }
    if (msk) {
        return runGraph<float>(a, [&](stream<complex_t>* in) {
            return new MSKDemod(in, a.sampleRate, a.deviation, a.baudRate, a.omegaGain, a.muGain, a.relLimit);
        });
    }
    fprintf(stderr, "mode: psk2 | psk4 | psk8 | oqpsk | msk\n");
    return 2;
}
