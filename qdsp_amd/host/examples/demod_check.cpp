// demod_check -- source -> VFO -> demodulator -> sink graphs of the C++ block mirror (qdsp_amd/host/dsp/demodulator.h), for
// the tests to compare with the restatement of src/dsp/demodulator.h applied to the VFO's own output.  A harness, not part of
// the product.
//
//   demod_check vfo <in.cf32> <out.cf32> <block> <offset> <inSR> <outSR> <bw>
//                   source -> VFO -> sink: what the demodulators below read
//   demod_check fm|fms|am|ssb <dev|host> <in.cf32> <out> <block> <offset> <inSR> <outSR> <bw> [<p1> [<p2>]]
//                   source -> VFO -> FloatFMDemod (fm, p1 = deviation) | FMDemod (fms: stereo_t out) | AMDemod (am) |
//                   SSBDemod (ssb, p1 = bandWidth, p2 = mode 0 USB / 1 LSB / 2 DSB) -> sink, at sample rate outSR.
//                   dev: the VFO hands its blocks to the demodulator in device memory (the links the blocks set up
//                   themselves); host: the same graph with that link moved to the host buffers.
//   demod_check deemp <dev|host> <in.cf32> <out> <block> <offset> <inSR> <outSR> <bw> <deviation> <tau>
//                   source -> VFO -> FMDemod -> BFMDeemp (dsp/deemp.h) -> sink; host: both links into and out of the FMDemod
//                   on the host buffers.
//   demod_check squelch <dev|host> <in.cf32> <out.cf32> <block> <offset> <inSR> <outSR> <bw> <level_db>
//                   source -> VFO -> Squelch (dsp/processing.h) -> sink
//   demod_check agc <dev|host> <in.cf32> <out> <block> <offset> <inSR> <outSR> <bw> <fall_rate>
//                   source -> VFO -> AMDemod -> AGC (dsp/processing.h) -> sink; host: both links into and out of the AMDemod on
//                   the host buffers.
//   demod_check ffagc <dev|host> <in.cf32> <out.cf32> <block> <offset> <inSR> <outSR> <bw>
//                   source -> VFO -> FeedForwardAGC<complex_t> (dsp/processing.h) -> sink: 1023 samples fewer out than the VFO gives
//                   (the harness counts one output block per input block and the block publishes nothing while it fills, so a
//                   <block> whose VFO output is below 1024 samples is refused)
//   demod_check cagc <dev|host> <in.cf32> <out.cf32> <block> <offset> <inSR> <outSR> <bw> <set_point> <max_gain> <rate>
//                   source -> VFO -> ComplexAGC (dsp/processing.h) -> sink
//   demod_check costas <dev|host> <in.cf32> <out.cf32> <block> <offset> <inSR> <outSR> <bw> <order> <loop_bandwidth>
//                   source -> VFO -> CostasLoop<order> (dsp/pll.h), order 2, 4 or 8 -> sink
//   demod_check sfm <in.cf32> <out> <block> <sampleRate> <deviation>
//                   source -> StereoFMDemod (dsp/stereo_demod.h) -> sink: the file is the demodulator's own input, read in blocks of
//                   <block> samples, one run() each; stereo_t out.
//   demod_check rebind <block> <before> <after>
//                   two sources of constant blocks, A = 1+0j and B = 2+0j; A -> Squelch (open) -> sink, and after <before> blocks
//                   have come out setInput() moves the running Squelch to B, until <after> blocks of B have come out.  Every
//                   block must be all A or all B, and no A may follow a B.  (How many blocks are lost across the switch is not
//                   fixed: the worker may be stopped with a block in hand.)
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

#include <dsp/deemp.h>
#include <dsp/demodulator.h>
#include <dsp/pll.h>
#include <dsp/processing.h>
#include <dsp/sink.h>
#include <dsp/source.h>
#include <dsp/stereo_demod.h>
#include <dsp/vfo.h>

using namespace dsp;

static std::vector<complex_t> readAll(const char* path) {
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

// a file sink that counts the blocks it has written
template <class T> struct Writer {
    std::ofstream file;
    std::atomic<long> blocks{0};
    std::atomic<long> samples{0};
    static void push(T* src, int count, void* ctx) {
        Writer* w = static_cast<Writer*>(ctx);
        w->file.write(reinterpret_cast<const char*>(src), (std::streamsize)count * sizeof(T));
        w->samples += count;
        w->blocks++;
    }
};

// source -> VFO -> [BLOCKS] -> sink; waits until every input block has come out the far end
template <class T, class MAKE>
static int runGraph(const char* inPath, const char* outPath, int block, float off, float inSR, float outSR, float bw, bool hostLink,
                    MAKE make) {
    Feed feed;
    feed.data = readAll(inPath);
    feed.block = block;
    const long nblocks = (long)((feed.data.size() + block - 1) / block);
    HandlerSource<complex_t> src(Feed::pull, &feed);
    VFO vfo(&src.out, off, inSR, outSR, bw);
    std::vector<generic_unnamed_block*> blks;      // in graph order
    stream<T>* last = make(vfo.out, blks);
    if (hostLink) { vfo.out->releaseConsumer(); }   // the VFO writes its host buffers, the demodulator uploads them
    Writer<T> w;
    w.file.open(outPath, std::ios::binary);
    HandlerSink<T> sink(last, Writer<T>::push, &w);
    sink.start();
    for (auto it = blks.rbegin(); it != blks.rend(); ++it) { (*it)->start(); }
    vfo.start();
    src.start();
    const auto t0 = std::chrono::steady_clock::now();
    while (w.blocks.load() < nblocks) {
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) { fprintf(stderr, "graph timed out\n"); return 3; }
        if (hipBlockErrors() > 0) { fprintf(stderr, "a block failed\n"); return 4; }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    src.stop();
    vfo.stop();
    for (auto* b : blks) { b->stop(); }
    sink.stop();
    for (auto it = blks.rbegin(); it != blks.rend(); ++it) { delete *it; }
    w.file.close();
    printf("graph ok: %zu in, %ld out, %ld blocks, %s link, %.1f ms\n", feed.data.size(), w.samples.load(), nblocks, hostLink ? "host" : "device", ms);
    return 0;
}

// source -> StereoFMDemod -> sink, every block of the file one run()
static int runStereo(const char* inPath, const char* outPath, int block, float sampleRate, float deviation) {
    Feed feed;
    feed.data = readAll(inPath);
    feed.block = block;
    const long nblocks = (long)((feed.data.size() + block - 1) / block);
    HandlerSource<complex_t> src(Feed::pull, &feed);
    StereoFMDemod demod(&src.out, sampleRate, deviation);
    Writer<stereo_t> w;
    w.file.open(outPath, std::ios::binary);
    HandlerSink<stereo_t> sink(&demod.out, Writer<stereo_t>::push, &w);
    sink.start();
    demod.start();
    src.start();
    const auto t0 = std::chrono::steady_clock::now();
    while (w.blocks.load() < nblocks) {
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) { fprintf(stderr, "graph timed out\n"); return 3; }
        if (hipBlockErrors() > 0) { fprintf(stderr, "a block failed\n"); return 4; }
    }
    src.stop();
    demod.stop();
    sink.stop();
    w.file.close();
    printf("graph ok: %zu in, %ld out, %ld blocks, %d pilot taps\n", feed.data.size(), w.samples.load(), nblocks, demod.getPilotTapCount());
    return 0;
}

// a source of blocks of one constant, and a sink that sorts the blocks it gets by that constant
struct Constant {
    complex_t value;
    int block;
    static int pull(complex_t* dst, void* ctx) {
        const Constant* c = static_cast<const Constant*>(ctx);
        std::fill(dst, dst + c->block, c->value);
        return c->block;
    }
};

struct Sorter {
    std::atomic<long> a{0}, b{0}, mixed{0}, aAfterB{0}, other{0};
    static void push(complex_t* src, int count, void* ctx) {
        Sorter* s = static_cast<Sorter*>(ctx);
        int na = 0, nb = 0;
        for (int i = 0; i < count; i++) {
            na += src[i].re == 1.0f && src[i].im == 0.0f;
            nb += src[i].re == 2.0f && src[i].im == 0.0f;
        }
        if (na == count) { s->a++; if (s->b.load() > 0) { s->aAfterB++; } }
        else if (nb == count) { s->b++; }
        else if (na + nb == count) { s->mixed++; }
        else { s->other++; }
    }
};

static int runRebind(int block, long before, long after) {
    if (block < 1 || block > STREAM_BUFFER_SIZE || before < 1 || after < 1) { fprintf(stderr, "rebind: <block> <before> <after>\n"); return 2; }
    Constant ca{complex_t{1.0f, 0.0f}, block}, cb{complex_t{2.0f, 0.0f}, block};
    HandlerSource<complex_t> srcA(Constant::pull, &ca), srcB(Constant::pull, &cb);
    Squelch sq(&srcA.out, -100.0f);      // |x| = 1 is 0 dB: open
    Sorter sorted;
    HandlerSink<complex_t> sink(&sq.out, Sorter::push, &sorted);
    sink.start();
    sq.start();
    srcA.start();
    srcB.start();
    const auto t0 = std::chrono::steady_clock::now();
    auto waitFor = [&](std::atomic<long>& n, long want) {
        while (n.load() < want) {
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) { fprintf(stderr, "graph timed out\n"); return 3; }
            if (hipBlockErrors() > 0) { fprintf(stderr, "a block failed\n"); return 4; }
        }
        return 0;
    };
    int rc = waitFor(sorted.a, before);
    if (rc == 0) {
        sq.setInput(&srcB.out);
        rc = waitFor(sorted.b, after);
    }
    srcA.stop();
    srcB.stop();
    sq.stop();
    sink.stop();
    if (rc != 0) { return rc; }
    const long mixed = sorted.mixed.load(), late = sorted.aAfterB.load(), other = sorted.other.load();
    if (mixed || late || other) {
        fprintf(stderr, "rebind: %ld mixed blocks, %ld blocks of A after a block of B, %ld blocks of neither\n", mixed, late, other);
        return 5;
    }
    printf("graph ok: %ld blocks of A, then %ld blocks of B\n", sorted.a.load(), sorted.b.load());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: see the header of demod_check.cpp\n"); return 2; }
    const std::string mode = argv[1];
    if (mode == "sfm") {
        if (argc < 7) { fprintf(stderr, "usage: see the header of demod_check.cpp\n"); return 2; }
        return runStereo(argv[2], argv[3], atoi(argv[4]), (float)atof(argv[5]), (float)atof(argv[6]));
    }
    if (mode == "rebind") {
        if (argc < 5) { fprintf(stderr, "usage: see the header of demod_check.cpp\n"); return 2; }
        return runRebind(atoi(argv[2]), atol(argv[3]), atol(argv[4]));
    }
    if (mode == "vfo" && argc >= 9) {
        const float off = (float)atof(argv[5]), inSR = (float)atof(argv[6]), outSR = (float)atof(argv[7]), bw = (float)atof(argv[8]);
        return runGraph<complex_t>(argv[2], argv[3], atoi(argv[4]), off, inSR, outSR, bw, false,
                                   [](stream<complex_t>* s, std::vector<generic_unnamed_block*>&) { return s; });
    }
    if (argc < 10) { fprintf(stderr, "usage: see the header of demod_check.cpp\n"); return 2; }
    const std::string link = argv[2];
    if (link != "dev" && link != "host") { fprintf(stderr, "link: dev | host\n"); return 2; }
    const bool hostLink = link == "host";
    const char* in = argv[3];
    const char* out = argv[4];
    const int block = atoi(argv[5]);
    const float off = (float)atof(argv[6]), inSR = (float)atof(argv[7]), outSR = (float)atof(argv[8]), bw = (float)atof(argv[9]);
    const float p1 = argc > 10 ? (float)atof(argv[10]) : 0.0f;
    const int p2 = argc > 11 ? atoi(argv[11]) : 0;
    // the demodulator block and its output stream
    auto with = [](auto* d, std::vector<generic_unnamed_block*>& blks) { blks.push_back(d); return &d->out; };
    if (mode == "fm")
        return runGraph<float>(in, out, block, off, inSR, outSR, bw, hostLink,
                               [&](stream<complex_t>* s, std::vector<generic_unnamed_block*>& b) { return with(new FloatFMDemod(s, outSR, p1), b); });
    if (mode == "fms")
        return runGraph<stereo_t>(in, out, block, off, inSR, outSR, bw, hostLink,
                                  [&](stream<complex_t>* s, std::vector<generic_unnamed_block*>& b) { return with(new FMDemod(s, outSR, p1), b); });
    if (mode == "am")
        return runGraph<float>(in, out, block, off, inSR, outSR, bw, hostLink,
                               [&](stream<complex_t>* s, std::vector<generic_unnamed_block*>& b) { return with(new AMDemod(s), b); });
    if (mode == "ssb")
        return runGraph<float>(in, out, block, off, inSR, outSR, bw, hostLink,
                               [&](stream<complex_t>* s, std::vector<generic_unnamed_block*>& b) { return with(new SSBDemod(s, outSR, p1, p2), b); });
    if (mode == "deemp" && argc > 11) {
        const float tau = (float)atof(argv[11]);
        return runGraph<stereo_t>(in, out, block, off, inSR, outSR, bw, hostLink,
                                  [&](stream<complex_t>* s, std::vector<generic_unnamed_block*>& b) {
                                      FMDemod* fm = new FMDemod(s, outSR, p1);
                                      b.push_back(fm);
                                      BFMDeemp* de = new BFMDeemp(&fm->out, outSR, tau);
                                      if (hostLink) { fm->out.releaseConsumer(); }
                                      return with(de, b);
                                  });
    }
    if (mode == "squelch" && argc > 10)
        return runGraph<complex_t>(in, out, block, off, inSR, outSR, bw, hostLink,
                                   [&](stream<complex_t>* s, std::vector<generic_unnamed_block*>& b) { return with(new Squelch(s, p1), b); });
    if (mode == "agc" && argc > 10)
        return runGraph<float>(in, out, block, off, inSR, outSR, bw, hostLink,
                               [&](stream<complex_t>* s, std::vector<generic_unnamed_block*>& b) {
                                   AMDemod* am = new AMDemod(s);
                                   b.push_back(am);
                                   AGC* agc = new AGC(&am->out, p1, outSR);
                                   if (hostLink) { am->out.releaseConsumer(); }
                                   return with(agc, b);
                               });
    if (mode == "ffagc") {
        if ((double)block * outSR / inSR < 1024.0) { fprintf(stderr, "ffagc: <block> * outSR / inSR must be at least 1024\n"); return 2; }
        return runGraph<complex_t>(in, out, block, off, inSR, outSR, bw, hostLink,
                                   [&](stream<complex_t>* s, std::vector<generic_unnamed_block*>& b) { return with(new FeedForwardAGC<complex_t>(s), b); });
    }
    if (mode == "cagc" && argc > 12) {
        const float maxGain = (float)atof(argv[11]), rate = (float)atof(argv[12]);
        return runGraph<complex_t>(in, out, block, off, inSR, outSR, bw, hostLink,
                                   [&](stream<complex_t>* s, std::vector<generic_unnamed_block*>& b) { return with(new ComplexAGC(s, p1, maxGain, rate), b); });
    }
    if (mode == "costas" && argc > 11) {
        const int order = (int)p1;
        const float loopBw = (float)atof(argv[11]);
        auto make = [&](auto* d) {
            return runGraph<complex_t>(in, out, block, off, inSR, outSR, bw, hostLink,
                                       [&](stream<complex_t>* s, std::vector<generic_unnamed_block*>& b) { d->init(s, loopBw); return with(d, b); });
        };
        if (order == 2) { return make(new CostasLoop<2>()); }
        if (order == 4) { return make(new CostasLoop<4>()); }
        if (order == 8) { return make(new CostasLoop<8>()); }
        fprintf(stderr, "costas: order 2, 4 or 8\n");
        return 2;
    }
    fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 2;
}
