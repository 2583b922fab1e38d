// TEST-ONLY: the dozen HIP runtime entry points and the RCCL entry points qdsp_amd/csrc/ring.cpp uses, as synchronous host code, so
// that the ring's bookkeeping (four receive buffers in rotation, at most two posts outstanding, prev / zeros pointers, timing slots)
// runs under -fsanitize=address,undefined without a GPU (tests/test_sanitizers_cpu.py), and the few more that
// qdsp_amd/csrc/stream_op.cpp calls (copies as memcpy, queries that are always complete).  Built into two shared objects:
// libfakehip.so (-DFAKE_HIP, linked instead of libamdhip64) and librccl.so.1 (-DFAKE_RCCL: what ring.cpp dlopens; found first
// through LD_LIBRARY_PATH).  A "stream" executes everything at once, so an event is complete as soon as it is recorded; a
// one-rank communicator's ncclSend / ncclRecv pair is a memcpy at ncclGroupEnd.
#include <stdlib.h>
#include <string.h>

extern "C" {

#ifdef FAKE_HIP
// streams, events and buffers not yet given back, and the hipMalloc call (counted from 1) that is to fail next, for
// stream_op_selftest.cpp
static int g_live = 0, g_fail_malloc = 0;
int fake_hip_live(void) { return g_live; }
void fake_hip_fail_malloc(int nth) { g_fail_malloc = nth; }
static void* track(void* p) { if (p) g_live++; return p; }
static void untrack(void* p) { if (p) g_live--; free(p); }

int hipGetDeviceCount(int* n) { *n = 1; return 0; }
int hipSetDevice(int) { return 0; }
int hipDeviceSynchronize(void) { return 0; }
int hipGetLastError(void) { return 0; }
int hipStreamCreateWithFlags(void** s, unsigned) { *s = track(malloc(16)); return *s ? 0 : 2; }
int hipStreamDestroy(void* s) { untrack(s); return 0; }
int hipStreamSynchronize(void*) { return 0; }
int hipStreamQuery(void*) { return 0; }
int hipStreamWaitEvent(void*, void* e, unsigned) { return e ? 0 : 1; }
int hipEventCreateWithFlags(void** e, unsigned) { *e = track(calloc(1, 16)); return *e ? 0 : 2; }
int hipEventCreate(void** e) { return hipEventCreateWithFlags(e, 0); }
int hipEventDestroy(void* e) { untrack(e); return 0; }
int hipEventRecord(void* e, void*) { if (!e) return 1; *static_cast<int*>(e) += 1; return 0; }
int hipEventSynchronize(void* e) { return e ? 0 : 1; }
int hipEventQuery(void* e) { return e ? 0 : 1; }
int hipEventElapsedTime(float* ms, void* a, void* b) { if (!a || !b) return 1; *ms = 0.002f; return 0; }
int hipMalloc(void** p, size_t n) {
    *p = nullptr;
    if (g_fail_malloc > 0 && --g_fail_malloc == 0) return 2;
    *p = track(malloc(n ? n : 1));
    return *p ? 0 : 2;
}
int hipFree(void* p) { untrack(p); return 0; }
int hipMemset(void* p, int v, size_t n) { memset(p, v, n); return 0; }
int hipMemcpy(void* dst, const void* src, size_t n, int) { memcpy(dst, src, n); return 0; }
int hipMemcpyAsync(void* dst, const void* src, size_t n, int, void*) { memcpy(dst, src, n); return 0; }
// Always "not mapped": no buffer here is pinned, so the early return of a deferred output behind a pipelined input
// (stream_op_process_ex: mapped_host_ptr) is not taken.  That branch stays covered by the block-graph tests on the GPU only.
int hipPointerGetAttributes(void*, const void*) { return 1; }
#endif

#ifdef FAKE_RCCL
struct UniqueId { char internal[128]; };
struct Comm { int world, rank; };
static const void* g_send = nullptr;
static void* g_recv = nullptr;
static size_t g_send_n = 0, g_recv_n = 0;
static int g_depth = 0;
int ncclGetUniqueId(UniqueId* id) { memset(id->internal, 0x5a, sizeof id->internal); return 0; }
int ncclCommInitRank(Comm** c, int world, UniqueId, int rank) {
    if (world != 1 || rank != 0) return 5;      // the fake carries a one-rank ring only
    *c = static_cast<Comm*>(malloc(sizeof(Comm)));
    (*c)->world = world;
    (*c)->rank = rank;
    return 0;
}
int ncclCommDestroy(Comm* c) { free(c); return 0; }
int ncclGroupStart() { g_depth++; return 0; }
int ncclSend(const void* buf, size_t count, int, int peer, Comm* c, void*) { if (peer != 0 || !c) return 4; g_send = buf; g_send_n = count; return 0; }
int ncclRecv(void* buf, size_t count, int, int peer, Comm* c, void*) { if (peer != 0 || !c) return 4; g_recv = buf; g_recv_n = count; return 0; }
int ncclGroupEnd() {
    if (--g_depth == 0 && g_send && g_recv) {
        if (g_send_n != g_recv_n) return 4;
        memcpy(g_recv, g_send, g_send_n);
        g_send = nullptr;
        g_recv = nullptr;
    }
    return 0;
}
const char* ncclGetErrorString(int) { return "fake rccl error"; }
int ncclCommCount(Comm* c, int* n) { *n = c->world; return 0; }
int ncclCommUserRank(Comm* c, int* r) { *r = c->rank; return 0; }
int ncclCommCuDevice(Comm*, int* d) { *d = 0; return 0; }
int ncclGetVersion(int* v) { *v = 22203; return 0; }
#endif

}  // extern "C"
