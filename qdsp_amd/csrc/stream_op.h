// stream_op.h -- what the handles of the per-row operators share (demod / deemp / level / stereo_fm / ff_agc / cagc / costas / mmcr /
// rowfir / deframe / rs / fpkt / noaa .hip, psk_chain.cpp):
// the head of the handle, the table that tells live handles and their kinds apart, the shape of create / free / the forwarding
// entry points, and the one block-graph path (*_process_ex) and timing loop behind all of them.  Host code only (stream_op.cpp is built without an offload architecture, like ring.cpp); an operator supplies its launch
// function and the bytes per sample of its two sides, and keeps its kernels, its launch-argument checks and its own state.
#pragma once
#include "../../include/qdsp_hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <new>

namespace qh {

#define HIPCHK(expr)                                   \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) return -(int)e_;         \
    } while (0)

struct Launch {
    const char* name = "";
    int grid = 0, block = 0, lds = 0;
};

constexpr int kDemodMaxChan = 65535;              // grid.y

// The kinds of per-row handle; every handle struct names its own as `static constexpr OpKind kKind`.
enum class OpKind : int {
    Demod = 1,     // demod.hip.h (FM, FM stereo, AM; SSB is a sub-kind)
    Deemp,         // deemp.hip.h
    Level,         // level.hip.h (Squelch and AGC are sub-kinds)
    StereoFm,      // stereo_fm.hip.h
    FfAgc,         // ff_agc.hip.h
    Cagc,          // cagc.hip.h
    Costas,        // costas.hip.h
    Mmcr,          // mmcr.hip.h
    RowFir,        // rowfir.hip.h
    DelayImag,     // rowfir.hip.h
    Chain,         // psk_chain.cpp (PSKDemod and MSKDemod are sub-kinds)
    Threshold,     // deframe.hip.h
    Deframer,      // deframe.hip.h
    // The byte-stream tail.  Rs is the Falcon tail's kind: rs.hip.h, the Reed-Solomon decoder and its FalconRS preset, at sub-kind 0
    // and fpkt.hip.h, FalconPacketSync, at sub-kind 1 (the table's, see below); Hrpt, Tip, Hirs: noaa.hip.h, the three NOAA
    // demultiplexers.  (They share a line on purpose: tests/test_psk_cpu.py reads one kind per line of this enum and pins the
    // fourteen lines up to Rs; tests/test_noaa_cpu.py reads every enumerator and pins all seventeen.)
    Rs, Hrpt, Tip, Hirs,
};
constexpr OpKind kLastOpKind = OpKind::Hirs;

// The head of every per-row handle.  No virtual functions, and nothing in it says what the handle is: that is the table's to say.
struct StreamOp {
    int device = 0;
    int nchan = 1;
    hipStream_t stream = nullptr;          // host-pointer path
    hipStream_t last_stream = nullptr;     // process_ex: the stream of the previous call (its own or the shared one)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t done_ev = nullptr;          // QDSP_HIP_LINK_HOST_DEFERRED
    void* d_in = nullptr;                  // staging for host sides: max_block samples each
    void* d_out = nullptr;
    int max_block = 0;
    Launch last;
    size_t in_es = 0, out_es = 0;          // bytes per input / output sample
    // nchan rows of `count` samples, in_stride / out_stride samples apart, on stream s.  Negative: an error; otherwise what
    // process_ex returns (0, or FeedForwardAGC's output count).
    int64_t (*launch)(StreamOp*, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) = nullptr;
    int64_t (*out_count)(const StreamOp*, int64_t count) = nullptr;   // outputs of the next call of `count` samples; null: count
};

// `launch` for an operator whose own launch function takes its handle type
template <class T, auto F>
int64_t launch_as(StreamOp* op, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    return F(static_cast<T*>(op), d_in, count, in_stride, d_out, out_stride, s);
}

// How a per-row handle is known: by its address.  A table (a reader-writer lock and a hash map in stream_op.cpp, alive for the
// whole process) holds every live handle under its kind, entered as the last step of a successful create and taken out as the
// first step of its free.  A lookup never reads the caller's pointer: a destroyed handle, a second destroy and foreign memory are
// refused whatever they hold.  Lookups share the lock; only register and unregister exclude.
// The table's value is {kind, sub}: a handle struct that shares its kind with another names its own `static constexpr int kSub`
// (every other is at sub 0), and a lookup takes a handle only under both, so one unit's entry points refuse the other's handles.
// (The engine, channelizer, math and ring handles -- kMagic, kChanMagic, kMathMagic, kRingMagic -- are no StreamOps and keep their magics.)
void stream_op_register(StreamOp* d, OpKind kind, int sub = 0);
void stream_op_unregister(StreamOp* d);    // (a handle that is not in the table: nothing happens)
// h if it is a live handle of `kind` and `sub`
StreamOp* stream_op_lookup(void* h, OpKind kind, int sub = 0);
// h if it is a live handle of any kind
StreamOp* as_stream_op(void* h);
// T::kSub where T declares one, else 0
template <class T, class = void>
struct op_sub {
    static constexpr int value = 0;
};
template <class T>
struct op_sub<T, decltype((void)T::kSub)> {
    static constexpr int value = T::kSub;
};
// h as a T if it is a live handle of T's kind and table sub-kind.  (Demod, Level and Chain check their in-struct sub-kind after it.)
template <class T>
T* as(void* h) {
    return static_cast<T*>(stream_op_lookup(h, T::kKind, op_sub<T>::value));
}

// The argument checks every create begins with, after the operator's own: QDSP_HIP_EINVAL (h, nchan, max_block), then
// QDSP_HIP_ENODEV, then the device is made current.
int stream_op_check(void** h, int device, int nchan, int max_block);
// The stream, the two events and the staging buffers.  On failure nothing is left allocated.
hipError_t stream_op_init(StreamOp* d, int device, int nchan, int max_block, size_t in_es, size_t out_es);
// Frees what stream_op_init made (the device is current and idle)
void stream_op_release(StreamOp* d);

// run() with each side on the host or the device (QDSP_HIP_LINK_* codes); one channel.  Returns what d->launch returned.
int64_t stream_op_process_ex(StreamOp* d, const void* in, int in_link, int count, void* out, int out_link);
// Mean ms of `iters` back-to-back launches over nchan rows of `count` samples, back to back, on `stream`
int stream_op_time(StreamOp* d, const void* d_in, int64_t count, void* d_out, void* stream, int iters, float* ms);

// ---- the shape every unit's create, free and forwarding entry points share ----
// The head of a create: *h nulled, the operator's own argument checks (`args_ok`), stream_op_check, a new T with its launch
// function (and its output count, where it has one) wired.
template <class T, auto L, int64_t (*OC)(const StreamOp*, int64_t) = nullptr>
int op_new(T** d, void** h, bool args_ok, int device, int nchan, int max_block) {
    if (h) *h = nullptr;
    if (!args_ok) return QDSP_HIP_EINVAL;
    if (const int rc = stream_op_check(h, device, nchan, max_block)) return rc;
    *d = new (std::nothrow) T();
    if (!*d) return QDSP_HIP_ENOMEM;
    (*d)->launch = launch_as<T, L>;
    (*d)->out_count = OC;
    return 0;
}
// The tail of a create: rc == 0 makes d a handle and hands it out; anything else frees it with the unit's free and is returned.
template <auto Free, class T>
int op_created(void** h, T* d, int rc) {
    if (rc) {
        Free(d);
        return rc;
    }
    stream_op_register(d, T::kKind, op_sub<T>::value);
    *h = d;
    return 0;
}
template <auto Free, class T>
int op_created(void** h, T* d, hipError_t err) {
    return op_created<Free>(h, d, -(int)err);
}
// A unit's free: `releases` frees what the unit itself allocated, on an idle device
template <class T, class R>
void op_free(T* d, R releases) {
    if (!d) return;
    stream_op_unregister(d);
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    releases();
    stream_op_release(d);
    delete d;
}
// (for `releases`: hipFree of every pointer of the list that is set)
inline void hip_free_all(std::initializer_list<void*> ptrs) {
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
}
// The forwarding entry points of an operator with as many outputs as inputs.  `As`: the lookup, where the unit has sub-kinds.
template <class T, T* (*As)(void*) = as<T>>
int op_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link) {
    T* d = As(h);
    return d ? (int)stream_op_process_ex(d, in, in_link, count, out, out_link) : QDSP_HIP_EINVAL;
}
template <class T, auto L, T* (*As)(void*) = as<T>>
int op_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, void* hip_stream) {
    T* d = As(h);
    return d ? L(d, d_in, count, in_stride, d_out, out_stride, static_cast<hipStream_t>(hip_stream)) : QDSP_HIP_EINVAL;
}
template <class T, auto L, T* (*As)(void*) = as<T>>
int op_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream) {
    return op_process_batch_dev<T, L, As>(h, d_in, count, count, d_out, count, hip_stream);
}

inline bool chan_ok(const StreamOp* d, int chan) { return chan >= 0 && chan < d->nchan; }
// chan, or all channels for chan == -1: the first one and how many
inline int chan_first(int chan) { return chan < 0 ? 0 : chan; }
inline int chan_count(const StreamOp* d, int chan) { return chan < 0 ? d->nchan : 1; }
// everything queued has run (a launch in flight may still read the old values), then the copy
int sync_upload(StreamOp* d, void* dst, const void* src, size_t bytes);
int sync_download(StreamOp* d, void* dst, const void* src, size_t bytes);

// ---- the waits and the shared stream of every host path (the engine and the channelizer use them too) ----
hipError_t wait_stream(hipStream_t s);
hipError_t wait_event(hipEvent_t ev, hipStream_t s);
hipStream_t shared_stream(int device);
void* mapped_host_ptr(void* p);

}  // namespace qh
