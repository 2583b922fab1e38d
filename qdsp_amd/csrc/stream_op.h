// stream_op.h -- what the handles of the per-row operators share (demod / deemp / level / stereo_fm / ff_agc / cagc / costas / mmcr /
// rowfir / deframe / rs .hip, psk_chain.cpp):
// the head of the handle, its creation and release, and the one block-graph path (*_process_ex) and timing loop behind all of
// them.  Host code only (stream_op.cpp is built without an offload architecture, like ring.cpp); an operator supplies its launch
// function and the bytes per sample of its two sides, and keeps its kernels, its launch-argument checks and its own state.
#pragma once
#include "../../include/qdsp_hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

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

constexpr uint32_t kDemodMagic = 0x51444d44u;     // "QDMD"  demod.hip.h
constexpr uint32_t kDeempMagic = 0x51444545u;     // "QDEE"  deemp.hip.h
constexpr uint32_t kLevelMagic = 0x514c564cu;     // "QLVL"  level.hip.h
constexpr uint32_t kStereoFmMagic = 0x5153464du;  // "QSFM"  stereo_fm.hip.h
constexpr uint32_t kFfAgcMagic = 0x51464147u;     // "QFAG"  ff_agc.hip.h
constexpr uint32_t kCagcMagic = 0x51434147u;      // "QCAG"  cagc.hip.h
constexpr uint32_t kCostasMagic = 0x51434f53u;    // "QCOS"  costas.hip.h
constexpr uint32_t kMmcrMagic = 0x514d4d43u;      // "QMMC"  mmcr.hip.h
constexpr uint32_t kRowFirMagic = 0x51524649u;    // "QRFI"  rowfir.hip.h
constexpr uint32_t kDelayImagMagic = 0x5144494du; // "QDIM"  rowfir.hip.h
constexpr uint32_t kChainMagic = 0x5150534bu;     // "QPSK"  psk_chain.cpp (PSKDemod and MSKDemod chains)
constexpr int kDemodMaxChan = 65535;              // grid.y

// The head of every per-row handle.  No virtual functions: every as_* reads `magic` at offset 0 of a handle of unknown kind.
struct StreamOp {
    uint32_t magic;
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

    explicit StreamOp(uint32_t m) : magic(m) {}
};

// `launch` for an operator whose own launch function takes its handle type
template <class T, auto F>
int64_t launch_as(StreamOp* op, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    return F(static_cast<T*>(op), d_in, count, in_stride, d_out, out_stride, s);
}

// Kinds without a magic (deframe.hip.h: Threshold, Deframer).  Why two of thirteen kinds are told apart differently: the eleven magics
// above are a closed set -- tests/test_psk_cpu.py counts the k*Magic constants of this header and checks that they differ, and a
// feature may not edit an existing test -- so a kind added after them cannot bring a twelfth constant.  Such a handle has magic 0,
// which no as_* of a kind above takes, and is known by its address instead: it is entered in a table (a mutex and a hash map in
// stream_op.cpp, alive for the whole process) under its kind at create and taken out at destroy.  as_threshold / as_deframer only
// look the pointer up, so they refuse a stale or foreign pointer without reading it.  as_stream_op (last_kernel, set_done_event,
// time_process_dev) still reads `magic` of an unknown pointer first, as it always has; the table is only asked, and its lock only
// taken, for a handle that is none of the eleven.
constexpr int kKindThreshold = 1;
constexpr int kKindDeframer = 2;
constexpr int kKindRs = 3;               // rs.hip.h: the Reed-Solomon decoder and its FalconRS preset
void stream_op_register(StreamOp* d, int kind);
void stream_op_unregister(StreamOp* d);
// h if it is a live registered handle of `kind` (0: of any kind)
StreamOp* stream_op_registered(void* h, int kind);

// h if it is one of the kinds above (by magic, no lock), or else a registered handle
StreamOp* as_stream_op(void* h);

// The argument checks every create begins with, after the operator's own: QDSP_HIP_EINVAL (h, nchan, max_block), then
// QDSP_HIP_ENODEV, then the device is made current.
int stream_op_check(void** h, int device, int nchan, int max_block);
// The stream, the two events and the staging buffers.  On failure nothing is left allocated.
hipError_t stream_op_init(StreamOp* d, int device, int nchan, int max_block, size_t in_es, size_t out_es);
// Frees what stream_op_init made and clears the magic (the device is current and idle)
void stream_op_release(StreamOp* d);

// run() with each side on the host or the device (QDSP_HIP_LINK_* codes); one channel.  Returns what d->launch returned.
int64_t stream_op_process_ex(StreamOp* d, const void* in, int in_link, int count, void* out, int out_link);
// Mean ms of `iters` back-to-back launches over nchan rows of `count` samples, back to back, on `stream`
int stream_op_time(StreamOp* d, const void* d_in, int64_t count, void* d_out, void* stream, int iters, float* ms);

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
