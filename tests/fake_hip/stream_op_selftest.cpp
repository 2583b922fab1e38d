// TEST-ONLY driver of qdsp_amd/csrc/stream_op.cpp against the fake synchronous HIP runtime (fake_hip_runtime.cpp), built with
// -fsanitize=address,undefined: a dummy operator (8 bytes in, 4 bytes out per sample, its launch a counted memcpy) through every
// pair of link codes, the error codes and their precedence, the timing loop, creation and release.  "Device" buffers are host
// memory here, so what arrives where can be compared byte for byte.
#include "../../qdsp_amd/csrc/stream_op.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>
#include <utility>
#include <vector>

extern "C" int fake_hip_live(void);
extern "C" void fake_hip_fail_malloc(int nth);

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

using namespace qh;

namespace {
constexpr int kMaxBlock = 64;
constexpr size_t kInEs = 8, kOutEs = 4;

struct Dummy : StreamOp {
    static constexpr OpKind kKind = OpKind::Level;
    int launches = 0;
    int64_t fail = 0;                      // what the next launches return instead of working
    const void* seen_in = nullptr;
    void* seen_out = nullptr;
    int64_t seen_count = -1, seen_in_stride = -1, seen_out_stride = -1;
    hipStream_t seen_stream = nullptr;
};

// the outputs are the leading bytes of the input; returns 0, or the output count where the handle has a hook for it
int64_t dummy_launch(Dummy* d, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    d->launches++;
    if (d->fail) return d->fail;
    const int64_t nout = d->out_count ? d->out_count(d, count) : count;
    d->seen_in = d_in;
    d->seen_out = d_out;
    d->seen_count = count;
    d->seen_in_stride = in_stride;
    d->seen_out_stride = out_stride;
    d->seen_stream = s;
    if (nout > 0) memcpy(d_out, d_in, (size_t)nout * d->out_es);
    return d->out_count ? nout : 0;
}

int64_t lag3(const StreamOp*, int64_t count) { return count > 3 ? count - 3 : 0; }

void drop(Dummy* d) {
    op_free(d, [] {});
}

// a create as the units write it: the shared head, the handle's own allocations, the shared tail
Dummy* make(int nchan, int max_block, bool hook) {
    void* h = &h;
    Dummy* d = nullptr;
    if (hook ? op_new<Dummy, dummy_launch, lag3>(&d, &h, true, 0, nchan, max_block) : op_new<Dummy, dummy_launch>(&d, &h, true, 0, nchan, max_block))
        return nullptr;
    if (h || op_created<drop>(&h, d, stream_op_init(d, 0, nchan, max_block, kInEs, kOutEs))) return nullptr;
    return static_cast<Dummy*>(h);
}

// one more type per kind, so that as<Other> can be asked of every kind
template <OpKind K>
struct Of : StreamOp {
    static constexpr OpKind kKind = K;
};
template <int K>
bool kind_is_told_apart() {
    Of<(OpKind)K> op;
    constexpr int other = K == (int)kLastOpKind ? 1 : K + 1;
    if (as_stream_op(&op) || as<Of<(OpKind)K>>(&op)) return false;                   // not registered: no handle
    stream_op_register(&op, (OpKind)K);
    const bool ok = as_stream_op(&op) == &op && as<Of<(OpKind)K>>(&op) == &op && !as<Of<(OpKind)other>>(&op);
    stream_op_unregister(&op);
    return ok && !as_stream_op(&op) && !as<Of<(OpKind)K>>(&op);
}
template <int... K>
bool kinds_are_told_apart(std::integer_sequence<int, K...>) {
    return (kind_is_told_apart<K + 1>() && ...);
}

int links() {
    const int base = fake_hip_live();
    Dummy* d = make(1, kMaxBlock, false);
    CHECK(d && as_stream_op(d) == d && fake_hip_live() == base + 5);     // a stream, two events, two staging buffers
    hipEvent_t ev = nullptr;
    CHECK(hipEventCreate(&ev) == hipSuccess);
    const hipStream_t shared = shared_stream(0);
    CHECK(shared && shared != d->stream && shared_stream(0) == shared && !shared_stream(-1) && !shared_stream(64));
    const int n = 40;
    std::vector<unsigned char> in(n * kInEs), out(n * kOutEs);
    int calls = 0;
    for (int il = QDSP_HIP_LINK_HOST; il <= QDSP_HIP_LINK_PIPELINED; il++) {
        for (int ol = QDSP_HIP_LINK_HOST; ol <= QDSP_HIP_LINK_HOST_DEFERRED; ol++) {
            for (size_t i = 0; i < in.size(); i++) in[i] = (unsigned char)(i * 7 + il * 31 + ol * 57 + 1);
            memset(out.data(), 0, out.size());
            memset(d->d_out, 0, kMaxBlock * kOutEs);
            const bool deferred = ol == QDSP_HIP_LINK_HOST_DEFERRED, out_host = ol == QDSP_HIP_LINK_HOST || deferred;
            if (deferred) {
                d->done_ev = nullptr;
                CHECK(stream_op_process_ex(d, in.data(), il, n, out.data(), ol) == QDSP_HIP_EINVAL && d->launches == calls);
                d->done_ev = ev;
            }
            const int recorded = *reinterpret_cast<int*>(ev);
            CHECK(stream_op_process_ex(d, in.data(), il, n, out.data(), ol) == 0);
            CHECK(d->launches == ++calls);                                         // exactly one launch per call
            CHECK(memcmp(out.data(), in.data(), n * kOutEs) == 0);                // the bytes arrive
            CHECK(d->seen_in == (il == QDSP_HIP_LINK_HOST ? d->d_in : (const void*)in.data()));   // staging for host sides only
            CHECK(d->seen_out == (out_host ? d->d_out : (void*)out.data()));
            if (il == QDSP_HIP_LINK_HOST) CHECK(memcmp(d->d_in, in.data(), in.size()) == 0);
            CHECK(d->seen_count == n && d->seen_in_stride == n && d->seen_out_stride == n);
            const bool pipelined = il == QDSP_HIP_LINK_PIPELINED || ol == QDSP_HIP_LINK_PIPELINED;
            CHECK(d->last_stream == (pipelined ? shared : d->stream) && d->seen_stream == d->last_stream);
            CHECK(*reinterpret_cast<int*>(ev) == recorded + (deferred ? 1 : 0));  // the completion event, behind deferred outputs only
        }
    }
    CHECK(calls == 12);
    // link codes out of range, in either position
    for (int bad : {-1, 3, 7}) CHECK(stream_op_process_ex(d, in.data(), bad, n, out.data(), QDSP_HIP_LINK_HOST) == QDSP_HIP_EINVAL);
    for (int bad : {-1, 4, 9}) CHECK(stream_op_process_ex(d, in.data(), QDSP_HIP_LINK_HOST, n, out.data(), bad) == QDSP_HIP_EINVAL);
    CHECK(stream_op_process_ex(d, in.data(), 0, -1, out.data(), 0) == QDSP_HIP_EINVAL);
    CHECK(stream_op_process_ex(d, nullptr, 0, n, out.data(), 0) == QDSP_HIP_EINVAL);
    CHECK(stream_op_process_ex(d, in.data(), 0, n, nullptr, 0) == QDSP_HIP_EINVAL);
    // count == 0: 0 before anything else happens, whatever the pointers
    const hipStream_t before = d->last_stream;
    for (int il = 0; il <= 2; il++)
        for (int ol = 0; ol <= 3; ol++) CHECK(stream_op_process_ex(d, nullptr, il, 0, nullptr, ol) == 0);
    CHECK(d->launches == calls && d->last_stream == before);
    // one sample more than max_block: refused wherever a side is on the host, taken between device sides
    std::vector<unsigned char> big_in((kMaxBlock + 1) * kInEs, 0x5a), big_out((kMaxBlock + 1) * kOutEs);
    for (int il = 0; il <= 2; il++) {
        for (int ol = 0; ol <= 3; ol++) {
            const bool host = il == QDSP_HIP_LINK_HOST || ol == QDSP_HIP_LINK_HOST || ol == QDSP_HIP_LINK_HOST_DEFERRED;
            const int64_t rc = stream_op_process_ex(d, big_in.data(), il, kMaxBlock + 1, big_out.data(), ol);
            CHECK(rc == (host ? QDSP_HIP_ESIZE : 0));
            if (!host) CHECK(d->launches == ++calls && memcmp(big_out.data(), big_in.data(), big_out.size()) == 0);
        }
    }
    CHECK(d->launches == calls);
    // a null `out` is an argument error, and so it comes before the size
    CHECK(stream_op_process_ex(d, big_in.data(), 0, kMaxBlock + 1, nullptr, 0) == QDSP_HIP_EINVAL);
    // the launch's own refusal comes through, and nothing is copied back
    d->fail = -77;
    memset(out.data(), 0, out.size());
    CHECK(stream_op_process_ex(d, in.data(), 0, n, out.data(), 0) == -77 && d->launches == ++calls && out[0] == 0 && out[n * kOutEs - 1] == 0);
    d->fail = 0;
    drop(d);
    // the host path is one channel
    Dummy* two = make(2, kMaxBlock, false);
    CHECK(two);
    for (int il = 0; il <= 2; il++) CHECK(stream_op_process_ex(two, in.data(), il, n, out.data(), 0) == QDSP_HIP_EINVAL);
    CHECK(two->launches == 0 && chan_ok(two, 1) && !chan_ok(two, 2) && !chan_ok(two, -1));
    CHECK(chan_first(-1) == 0 && chan_count(two, -1) == 2 && chan_first(1) == 1 && chan_count(two, 1) == 1);
    drop(two);
    CHECK(hipEventDestroy(ev) == hipSuccess);
    CHECK(fake_hip_live() == base + 1);                                            // (the shared stream lives as long as the library)
    return 0;
}

int output_count_hook() {
    Dummy* d = make(1, kMaxBlock, true);
    CHECK(d);
    std::vector<unsigned char> in(10 * kInEs), out(10 * kOutEs, 0);
    for (size_t i = 0; i < in.size(); i++) in[i] = (unsigned char)(200 - i);
    CHECK(stream_op_process_ex(d, in.data(), 0, 3, nullptr, 0) == 0 && d->launches == 1);       // nothing to emit: a null out is taken
    CHECK(stream_op_process_ex(d, in.data(), 0, 4, nullptr, 0) == QDSP_HIP_EINVAL && d->launches == 1);
    CHECK(stream_op_process_ex(d, nullptr, 0, 3, nullptr, 0) == QDSP_HIP_EINVAL);
    for (int ol = 0; ol <= 2; ol++) {
        memset(out.data(), 0, out.size());
        CHECK(stream_op_process_ex(d, in.data(), 0, 10, out.data(), ol) == 7);                     // the hook's value is the return value
        CHECK(d->seen_count == 10 && d->seen_in_stride == 10 && d->seen_out_stride == 7);
        CHECK(memcmp(out.data(), in.data(), 7 * kOutEs) == 0 && out[7 * kOutEs] == 0);          // and the number of samples copied back
    }
    // here the size is known before the output count is: ESIZE comes first
    std::vector<unsigned char> big((kMaxBlock + 1) * kInEs, 1);
    CHECK(stream_op_process_ex(d, big.data(), 0, kMaxBlock + 1, nullptr, 0) == QDSP_HIP_ESIZE);
    CHECK(stream_op_process_ex(d, nullptr, 2, 0, nullptr, 2) == 0 && d->launches == 4);
    drop(d);
    return 0;
}

int timing() {
    Dummy* d = make(3, 0, false);
    CHECK(d && !d->d_in && !d->d_out);                                             // max_block == 0: no staging
    std::vector<unsigned char> in(3 * 16 * kInEs, 3), out(3 * 16 * kOutEs);
    float ms = -1.0f;
    CHECK(stream_op_time(d, in.data(), 16, out.data(), nullptr, 0, &ms) == QDSP_HIP_EINVAL);
    CHECK(stream_op_time(d, in.data(), 16, out.data(), nullptr, -2, &ms) == QDSP_HIP_EINVAL);
    CHECK(stream_op_time(d, in.data(), 16, out.data(), nullptr, 5, nullptr) == QDSP_HIP_EINVAL);
    CHECK(d->launches == 0 && ms == -1.0f);
    CHECK(stream_op_time(d, in.data(), 16, out.data(), d->stream, 5, &ms) == 0 && d->launches == 5);
    CHECK(ms > 0.0f && ms < 0.002f && d->seen_count == 16 && d->seen_in_stride == 16 && d->seen_out_stride == 16 && d->seen_stream == d->stream);
    d->fail = -701;
    ms = -1.0f;
    CHECK(stream_op_time(d, in.data(), 16, out.data(), nullptr, 5, &ms) == -701 && d->launches == 6 && ms == -1.0f);
    drop(d);
    return 0;
}

int creation() {
    const int base = fake_hip_live();
    void* h = &h;
    CHECK(stream_op_check(nullptr, 0, 1, 0) == QDSP_HIP_EINVAL);
    CHECK(stream_op_check(&h, 0, 0, 0) == QDSP_HIP_EINVAL && stream_op_check(&h, 0, kDemodMaxChan + 1, 0) == QDSP_HIP_EINVAL);
    CHECK(stream_op_check(&h, 0, 1, -1) == QDSP_HIP_EINVAL);
    CHECK(stream_op_check(&h, 1, 1, 0) == QDSP_HIP_ENODEV && stream_op_check(&h, -1, 1, 0) == QDSP_HIP_ENODEV);   // one device here
    CHECK(stream_op_check(&h, 7, 0, 0) == QDSP_HIP_EINVAL);                        // EINVAL wins over ENODEV
    CHECK(stream_op_check(&h, 0, kDemodMaxChan, 0) == 0 && stream_op_check(&h, 0, 1, 1 << 30) == 0);
    // either staging buffer failing: nothing is left behind, and the handle is no handle any more
    for (int nth = 1; nth <= 2; nth++) {
        Dummy* d = new Dummy();
        fake_hip_fail_malloc(nth);
        CHECK(stream_op_init(d, 0, 1, kMaxBlock, kInEs, kOutEs) != hipSuccess);
        CHECK(fake_hip_live() == base && !d->stream && !d->ev0 && !d->ev1 && !d->d_in && !d->d_out && !as_stream_op(d));
        stream_op_release(d);                                                     // (what the operator's own free does next: harmless)
        CHECK(fake_hip_live() == base);
        delete d;
    }
    fake_hip_fail_malloc(0);
    // the shared head of a create: the operator's own refusal first, then the shared checks; *h is nulled in every case
    Dummy* none = nullptr;
    h = &h;
    CHECK((op_new<Dummy, dummy_launch>(&none, &h, false, 7, 1, 0)) == QDSP_HIP_EINVAL && !h && !none);
    h = &h;
    CHECK((op_new<Dummy, dummy_launch>(&none, &h, true, 7, 1, 0)) == QDSP_HIP_ENODEV && !h && !none);
    CHECK((op_new<Dummy, dummy_launch>(&none, nullptr, true, 0, 1, 0)) == QDSP_HIP_EINVAL && !none);
    // the shared tail: a failed create frees the handle, hands nothing out and never made it one
    CHECK((op_new<Dummy, dummy_launch>(&none, &h, true, 0, 1, 0)) == 0 && none && !h && !as_stream_op(none));
    CHECK(op_created<drop>(&h, none, hipErrorOutOfMemory) == -(int)hipErrorOutOfMemory && !h && !as_stream_op(none) && fake_hip_live() == base);
    // every kind of the enum: taken by as_stream_op and by as<> of its own kind, refused by as<> of another; only while registered
    CHECK(kinds_are_told_apart(std::make_integer_sequence<int, (int)kLastOpKind>()));
    struct Foreign { uint32_t magic; int pad[64]; } chan = {0x4348414eu, {0}}, engine = {0x51445350u, {0}}, math = {0x514d4154u, {0}};
    CHECK(!as_stream_op(nullptr) && !as_stream_op(&chan) && !as_stream_op(&engine) && !as_stream_op(&math));
    // memory that begins with a magic of the earlier scheme ("QLVL", "QDMD"): refused
    Foreign old_level = {0x514c564cu, {0}}, old_demod = {0x51444d44u, {0}};
    CHECK(!as_stream_op(&old_level) && !as<Dummy>(&old_level) && !as_stream_op(&old_demod));
    Dummy* d = make(1, 4, false);
    CHECK(d && as_stream_op(d) == static_cast<StreamOp*>(d) && as<Dummy>(d) == d && d->in_es == kInEs && d->out_es == kOutEs && d->max_block == 4);
    // unregistered: refused, though the memory is still a StreamOp; a second unregister does nothing
    stream_op_unregister(d);
    CHECK(!as_stream_op(d) && !as<Dummy>(d));
    stream_op_unregister(d);
    CHECK(!as_stream_op(d));
    stream_op_register(d, Dummy::kKind);
    CHECK(as<Dummy>(d) == d);
    // destroyed: the pointer is to freed memory, and the lookups refuse it without reading it (this build would report the read);
    // a second destroy -- the unit's free of what as<> returns -- is a call with null
    void* stale = d;
    drop(d);
    CHECK(!as_stream_op(stale) && !as<Dummy>(stale) && fake_hip_live() == base);
    drop(as<Dummy>(stale));
    CHECK(fake_hip_live() == base);
    return 0;
}

int uploads() {
    Dummy* d = make(2, 0, false);
    CHECK(d);
    const float src[2] = {1.5f, -2.5f};
    float dev[2] = {0.0f, 0.0f}, back[2] = {0.0f, 0.0f};
    CHECK(sync_upload(d, dev, src, sizeof(src)) == 0 && dev[0] == 1.5f && dev[1] == -2.5f);
    CHECK(sync_download(d, back, dev + 1, sizeof(float)) == 0 && back[0] == -2.5f && back[1] == 0.0f);
    CHECK(wait_stream(d->stream) == hipSuccess && wait_event(d->ev0, d->stream) == hipSuccess && wait_event(nullptr, d->stream) != hipSuccess);
    CHECK(mapped_host_ptr(dev) == nullptr);
    drop(d);
    return 0;
}
}  // namespace

int main() {
    static_assert(std::is_standard_layout<StreamOp>::value && !std::is_polymorphic<Dummy>::value,
                  "a handle is cast to the StreamOp it begins with and back (static_cast): no virtual functions, no second base");
    if (creation() || links() || output_count_hook() || timing() || uploads()) return 1;
    printf("stream_op ok\n");
    return 0;
}
