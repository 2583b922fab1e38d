// TEST-ONLY driver for the handle table of qdsp_amd/csrc/stream_op.cpp under -fsanitize=thread, on the fake HIP runtime
// (fake_hip_runtime.cpp): workers create, look up and destroy dummy handles through the shape every unit uses (op_new, op_created,
// op_free) while probers look up foreign memory and the addresses the workers have just destroyed.  A live handle is always found
// under its own kind and only under it; foreign memory never is; a stale address is either refused or, once the allocator has
// handed it out again, another worker's live handle -- the probers never read it either way.  (The handles get no stream, events
// or staging: the fake runtime's own counters are not made for threads.)
#include "../../qdsp_amd/csrc/stream_op.h"

#include <stdio.h>

#include <atomic>
#include <thread>
#include <vector>

using namespace qh;

namespace {
struct Dummy : StreamOp {
    static constexpr OpKind kKind = OpKind::Cagc;
    int owner = -1;
};
struct Other : StreamOp {
    static constexpr OpKind kKind = OpKind::Costas;
};
int64_t no_launch(Dummy*, const void*, int64_t, int64_t, void*, int64_t, hipStream_t) { return 0; }
void drop(Dummy* d) {
    op_free(d, [] {});
}
}  // namespace

int main() {
    constexpr int kWorkers = 4, kProbers = 3, kRounds = 20000;
    std::atomic<bool> stop{false};
    std::atomic<long> bad{0}, stale_hits{0};
    std::atomic<void*> stale[kWorkers];
    for (auto& s : stale) s = nullptr;
    static char foreign[256];
    std::vector<std::thread> probers;
    for (int t = 0; t < kProbers; t++) {
        probers.emplace_back([&] {
            char on_stack[64] = {};
            while (!stop.load(std::memory_order_relaxed)) {
                if (as_stream_op(foreign) || as<Dummy>(foreign + 8) || as_stream_op(on_stack) || as<Other>(on_stack)) bad++;
                for (auto& s : stale) {
                    void* p = s.load(std::memory_order_relaxed);
                    if (as<Other>(p)) bad++;                        // no handle of that kind is ever made
                    if (as_stream_op(p) || as<Dummy>(p)) stale_hits++;   // (the address is in use again)
                }
            }
        });
    }
    std::vector<std::thread> workers;
    for (int t = 0; t < kWorkers; t++) {
        workers.emplace_back([&, t] {
            for (int i = 0; i < kRounds; i++) {
                void* h = nullptr;
                Dummy* d = nullptr;
                if (op_new<Dummy, no_launch>(&d, &h, true, 0, 1, 0) || as_stream_op(d) || op_created<drop>(&h, d, hipSuccess) || h != d) {
                    bad++;
                    return;
                }
                d->owner = t;
                if (as<Dummy>(h) != d || as_stream_op(h) != d || as<Other>(h) || as<Dummy>(h)->owner != t) bad++;
                drop(as<Dummy>(h));
                (void)as<Dummy>(h);                                 // (refused, or by now another worker's: not read)
                stale[t].store(h, std::memory_order_relaxed);
            }
        });
    }
    for (auto& t : workers) t.join();
    stop = true;
    for (auto& t : probers) t.join();
    if (bad.load()) { printf("FAIL: %ld wrong answers\n", bad.load()); return 1; }
    printf("stream_op race ok (%ld lookups met a reused address)\n", stale_hits.load());
    return 0;
}
