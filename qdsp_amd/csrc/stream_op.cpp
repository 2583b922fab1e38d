// stream_op.cpp -- the host path the per-row operators share (stream_op.h): handle head, creation and release, the block-graph
// entry point with its link protocol, the timing loop, and the waits / shared stream every host path of the library uses.
#include "stream_op.h"

#include <string.h>

#include <chrono>
#include <mutex>
#include <shared_mutex>
#include <unordered_map>

namespace qh {

// End-of-call wait of the host-pointer paths.  hipStreamSynchronize sleeps on an interrupt (~20 us to wake up),
// longer than the kernels of a reference-sized block take: poll the stream for a bounded time first
// (200 us).
hipError_t wait_stream(hipStream_t s) {
    static const int spin_us = 200;
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        do {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) return hipSuccess;
            if (q != hipErrorNotReady) return q;
        } while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(spin_us));
    }
    return hipStreamSynchronize(s);
}

// The same for the library's shared stream: wait for THIS call's work only (an event recorded behind it), not for
// whatever the upstream blocks have queued for later blocks in the meantime.
hipError_t wait_event(hipEvent_t ev, hipStream_t s) {
    hipError_t rc = hipEventRecord(ev, s);
    if (rc != hipSuccess) return rc;
    static const int spin_us = 200;
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        do {
            const hipError_t q = hipEventQuery(ev);
            if (q == hipSuccess) return hipSuccess;
            if (q != hipErrorNotReady) return q;
        } while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(spin_us));
    }
    return hipEventSynchronize(ev);
}

// (Ordering the two ends of a link with events instead -- every handle on its own stream, two events per device
// buffer of the stream<T>, hipStreamWaitEvent before and hipEventRecord behind each kernel -- was built and
// measured: the cross-stream dependencies cost more than the serialisation they remove; SineSource -> VFO 23 -> 27 us
// per block, Splitter -> 4 / 16 x VFO 80 -> 120 / 386 -> 615 us.)
// One in-order stream per device for "pipelined" device-resident links (QDSP_HIP_LINK_PIPELINED): a producer
// launches into it and hands its block over without waiting; the consumer launches into the same stream, so
// the GPU runs the two in launch order -- which is the order the stream<T> protocol imposes on the host threads
// (the consumer reads a block only after the producer swapped it in, the producer reuses a buffer only after
// the consumer flushed it, and both launch before they swap / flush).
hipStream_t shared_stream(int device) {
    static std::mutex m;
    static hipStream_t tab[64] = {};
    std::lock_guard<std::mutex> lk(m);
    if (device < 0 || device >= 64) return nullptr;
    if (!tab[device]) {
        if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&tab[device], hipStreamNonBlocking) != hipSuccess) tab[device] = nullptr;
    }
    return tab[device];
}

// The device address of a pinned host buffer the kernels may store into, or nullptr (pageable memory).  Asked on
// every call (~1 us): a remembered answer could outlive the buffer it was about.
void* mapped_host_ptr(void* p) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) return at.devicePointer;
    (void)hipGetLastError();   // (pageable memory: an error the runtime keeps otherwise)
    return nullptr;
}

namespace {
struct Entry {
    OpKind kind;
    int sub;
};
struct Registry {
    std::shared_mutex m;
    std::unordered_map<const void*, Entry> live;     // handle -> {kind, sub}
};
Registry& registry() {
    static Registry* r = new Registry();    // (never destroyed: a handle may be released from a static destructor)
    return *r;
}
// h if it is in the table and `ok` takes its entry; h itself is not read
template <class F>
StreamOp* lookup(void* h, F ok) {
    if (!h) return nullptr;
    Registry& r = registry();
    std::shared_lock<std::shared_mutex> lk(r.m);
    const auto it = r.live.find(h);
    return (it != r.live.end() && ok(it->second)) ? static_cast<StreamOp*>(h) : nullptr;
}
}  // namespace

void stream_op_register(StreamOp* d, OpKind kind, int sub) {
    Registry& r = registry();
    std::unique_lock<std::shared_mutex> lk(r.m);
    r.live[d] = Entry{kind, sub};
}

void stream_op_unregister(StreamOp* d) {
    Registry& r = registry();
    std::unique_lock<std::shared_mutex> lk(r.m);
    r.live.erase(d);
}

StreamOp* stream_op_lookup(void* h, OpKind kind, int sub) {
    return lookup(h, [kind, sub](const Entry& e) { return e.kind == kind && e.sub == sub; });
}

StreamOp* as_stream_op(void* h) {
    return lookup(h, [](const Entry&) { return true; });
}

int stream_op_check(void** h, int device, int nchan, int max_block) {
    if (!h || nchan < 1 || nchan > kDemodMaxChan || max_block < 0) return QDSP_HIP_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return QDSP_HIP_ENODEV;
    if (device < 0 || device >= ndev) return QDSP_HIP_ENODEV;
    HIPCHK(hipSetDevice(device));
    return 0;
}

hipError_t stream_op_init(StreamOp* d, int device, int nchan, int max_block, size_t in_es, size_t out_es) {
    d->device = device;
    d->nchan = nchan;
    d->max_block = max_block;
    d->in_es = in_es;
    d->out_es = out_es;
    hipError_t err = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipEventCreate(&d->ev0);
    if (err == hipSuccess) err = hipEventCreate(&d->ev1);
    if (err == hipSuccess && max_block > 0) err = hipMalloc(&d->d_in, (size_t)max_block * in_es);
    if (err == hipSuccess && max_block > 0) err = hipMalloc(&d->d_out, (size_t)max_block * out_es);
    if (err != hipSuccess) stream_op_release(d);
    return err;
}

void stream_op_release(StreamOp* d) {
    if (d->d_in) (void)hipFree(d->d_in);
    if (d->d_out) (void)hipFree(d->d_out);
    if (d->ev0) (void)hipEventDestroy(d->ev0);
    if (d->ev1) (void)hipEventDestroy(d->ev1);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    d->d_in = d->d_out = nullptr;
    d->ev0 = d->ev1 = nullptr;
    d->stream = d->last_stream = nullptr;
}

int64_t stream_op_process_ex(StreamOp* d, const void* in, int in_link, int count, void* out, int out_link) {
    // (an operator with an output count of its own may emit nothing and then takes a null `out`: asked below, once the count is known)
    if (d->nchan != 1 || count < 0 || (count > 0 && (!in || (!out && !d->out_count)))) return QDSP_HIP_EINVAL;
    if (in_link < QDSP_HIP_LINK_HOST || in_link > QDSP_HIP_LINK_PIPELINED || out_link < QDSP_HIP_LINK_HOST ||
        out_link > QDSP_HIP_LINK_HOST_DEFERRED)
        return QDSP_HIP_EINVAL;
    const bool deferred = out_link == QDSP_HIP_LINK_HOST_DEFERRED;
    if (deferred && !d->done_ev) return QDSP_HIP_EINVAL;
    const bool out_host = out_link == QDSP_HIP_LINK_HOST || deferred;
    if ((in_link == QDSP_HIP_LINK_HOST || out_host) && count > d->max_block) return QDSP_HIP_ESIZE;
    const int64_t nout = d->out_count ? d->out_count(d, count) : count;
    if (nout > 0 && !out) return QDSP_HIP_EINVAL;
    if (count == 0) return 0;
    HIPCHK(hipSetDevice(d->device));
    hipStream_t st = d->stream;
    if (in_link == QDSP_HIP_LINK_PIPELINED || out_link == QDSP_HIP_LINK_PIPELINED) {
        st = shared_stream(d->device);
        if (!st) return QDSP_HIP_ENOMEM;
    }
    if (d->last_stream && d->last_stream != st) HIPCHK(hipStreamSynchronize(d->last_stream));   // (links re-plumbed)
    d->last_stream = st;
    const void* src = in;
    if (in_link == QDSP_HIP_LINK_HOST) {
        HIPCHK(hipMemcpyAsync(d->d_in, in, (size_t)count * d->in_es, hipMemcpyHostToDevice, st));
        src = d->d_in;
    }
    const int64_t rc = d->launch(d, src, count, count, out_host ? d->d_out : out, nout, st);
    if (rc < 0) return rc;
    if (out_host && nout > 0) HIPCHK(hipMemcpyAsync(out, d->d_out, (size_t)nout * d->out_es, hipMemcpyDeviceToHost, st));
    if (deferred) {
        // the consumer waits for done_ev (stream<T>::read); a pipelined input has been ordered on the shared stream already
        HIPCHK(hipEventRecord(d->done_ev, st));
        if (in_link == QDSP_HIP_LINK_PIPELINED && mapped_host_ptr(out)) return rc;
        HIPCHK(hipEventSynchronize(d->done_ev));
        return rc;
    }
    if (!(out_link == QDSP_HIP_LINK_PIPELINED && in_link == QDSP_HIP_LINK_PIPELINED))
        HIPCHK(st == d->stream ? wait_stream(st) : wait_event(d->ev0, st));
    return rc;
}

// (d_out holds the outputs of the longest of the calls: `count` samples per row are enough)
int stream_op_time(StreamOp* d, const void* d_in, int64_t count, void* d_out, void* stream, int iters, float* ms) {
    if (iters <= 0 || !ms) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(hipEventRecord(d->ev0, s));
    for (int i = 0; i < iters; i++) {
        const int64_t rc = d->launch(d, d_in, count, count, d_out, count, s);
        if (rc < 0) return (int)rc;
    }
    HIPCHK(hipEventRecord(d->ev1, s));
    HIPCHK(hipEventSynchronize(d->ev1));
    float t = 0.0f;
    HIPCHK(hipEventElapsedTime(&t, d->ev0, d->ev1));
    *ms = t / (float)iters;
    return 0;
}

int sync_upload(StreamOp* d, void* dst, const void* src, size_t bytes) {
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}

int sync_download(StreamOp* d, void* dst, const void* src, size_t bytes) {
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace qh
