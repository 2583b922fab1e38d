// rs.hip -- the Reed-Solomon decoder over rows of interleaved frames (design notes: rs.hip.h), and its C entry points.
#include "rs.hip.h"

#include <cstring>
#include <new>

namespace qk {

namespace {

__device__ __forceinline__ int rs_row_count(const int* in_counts, int row, int nframes) {
    if (!in_counts) return nframes;
    const int c = in_counts[row];
    return c < 0 ? 0 : (c < nframes ? c : nframes);
}

// what one lane wrote to LDS is read by the other lanes of its wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned wave_xor(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v ^= (unsigned)__shfl_xor((int)v, m);
    return v;
}

__device__ __forceinline__ int wrap255(int e) { return e >= 255 ? e - 255 : e; }

}  // namespace

__global__ __launch_bounds__(64 * kRsMaxDepth) void rs_decode_kernel(const RsArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_tab[kRsTab];
    __shared__ __attribute__((aligned(16))) unsigned char s_cw[kRsMaxDepth][256];
    __shared__ __attribute__((aligned(4))) unsigned char s_syn[kRsMaxDepth][32];    // syndromes
    __shared__ unsigned char s_lam[kRsMaxDepth][64];    // the locator's logarithms (0: a zero coefficient)
    __shared__ unsigned char s_om[kRsMaxDepth][32];     // the evaluator's logarithms
    __shared__ unsigned char s_root[kRsMaxDepth][64];
    __shared__ int s_bad;
    const int f = blockIdx.x, row = blockIdx.y, t = threadIdx.x, nt = blockDim.x;
    if (f >= rs_row_count(a.in_counts, row, a.nframes)) return;
    const unsigned char* s_exp = s_tab;
    const unsigned char* s_log = s_tab + 512;
    const unsigned char* s_imap = s_tab + 768;
    const unsigned char* s_omap = s_tab + 1024;
    const int I = a.depth;
    for (int j = t; j < kRsTab / 4; j += nt) reinterpret_cast<unsigned*>(s_tab)[j] = reinterpret_cast<const unsigned*>(a.tab)[j];
    if (t == 0) s_bad = 0;
    __syncthreads();
    {   // the frame, through the input map, one codeword per row of s_cw: cw[c][p] = in_map[d[p I + c]]
        const unsigned char* src = a.in + (long long)row * a.in_stride + (long long)f * a.frame_in + a.skip;
        const int mis = (int)((uintptr_t)src & 3);
        const unsigned* w = reinterpret_cast<const unsigned*>(src - mis);
        const int nb = 255 * I, nw = (mis + nb + 3) >> 2;
        for (int j = t; j < nw; j += nt) {
            const unsigned v = w[j];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int idx = 4 * j + b - mis;
                if (idx >= 0 && idx < nb) {
                    const int p = idx / I;
                    s_cw[idx - p * I][p] = s_imap[(v >> (8 * b)) & 255u];
                }
            }
        }
    }
    __syncthreads();
    const int wv = t >> 6, lane = t & 63;
    unsigned char* cw = s_cw[wv];
    const int nr = a.nroots;
    // ---- syndromes: S[i] = sum_k coeff[k] alpha^(gap (first_root + i) k), coeff[k] = cw[254 - k] ----
    unsigned any = 0;
    {
        int lc[4], e[4], st[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int k = 4 * lane + u;
            const unsigned c = k < 255 ? cw[254 - k] : 0u;
            lc[u] = c ? (int)s_log[c] : -1;
            e[u] = (a.g0 * k) % 255;
            st[u] = (a.gap * k) % 255;
        }
        for (int d = 0; 4 * d < nr; d++) {
            unsigned s4 = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                unsigned s = 0;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (lc[u] >= 0) s ^= s_exp[lc[u] + e[u]];
                    e[u] = wrap255(e[u] + st[u]);
                }
                if (4 * d + b < nr) s4 |= s << (8 * b);
            }
            s4 = wave_xor(s4);
            if (lane == 0) reinterpret_cast<unsigned*>(s_syn[wv])[d] = s4;
            any |= s4;
        }
    }
    wave_sync();
    int errs = 0;
    if (any) {
        // ---- the locator: lane j holds coefficient j of the locator (C) and of the last locator (B) ----
        unsigned C = lane == 0 ? 1u : 0u, B = C;
        int L = 0, ord = 0, lord = 0, delay = 1, ld_log = s_log[1];
        for (int i = 0; i < nr; i++) {
            unsigned p = 0;
            if (lane <= L && C) {
                const unsigned s = s_syn[wv][i - lane];
                if (s) p = s_exp[s_log[C] + s_log[s]];
            }
            const int d = __builtin_amdgcn_readfirstlane((int)wave_xor(p));
            if (!d) {
                delay++;
                continue;
            }
            const int sc = wrap255(255 + s_log[d] - ld_log);        // b d / last_d = exp[log b + sc]
            const int from = lane - delay;
            const unsigned bsrc = (unsigned)__shfl((int)B, from & 63);
            const unsigned term = (from >= 0 && from <= lord && bsrc) ? s_exp[s_log[bsrc] + sc] : 0u;
            if (2 * L <= i) {
                // the last locator shifted up by the delay and scaled: zeros below, its own old values above
                const unsigned bs = lane < delay ? 0u : (from <= lord ? term : B);
                const int top = lord + delay;
                if (lane <= top) {
                    const unsigned tmp = C;
                    C ^= bs;
                    B = tmp;
                } else {
                    B = bs;
                }
                lord = ord;
                ord = top;
                L = i + 1 - L;
                ld_log = s_log[d];
                delay = 1;
            } else {
                C ^= term;
                ord = lord + delay > ord ? lord + delay : ord;
                delay++;
            }
        }
        errs = ord;
        // ---- the locator's roots among all 256 elements, over its coefficients 0 .. ord ----
        s_lam[wv][lane] = (lane <= ord && C) ? s_log[C] : (unsigned char)0;
        wave_sync();
        const unsigned char* lam = s_lam[wv];
        const int top = ord < 63 ? ord : 63;
        int nroot = 0;
#pragma unroll 1
        for (int u = 0; u < 4; u++) {
            const int x = 64 * u + lane;
            bool r;
            if (x == 0) {
                r = lam[0] == 0;
            } else {
                const int lx = s_log[x];
                unsigned v = 0;
                int e = 0;
                for (int k = 0; k <= top; k++) {
                    const int ll = lam[k];
                    if (ll) v ^= s_exp[ll + e];
                    e = wrap255(e + lx);
                }
                r = v == 0;
            }
            const unsigned long long bal = __ballot(r);
            if (r) {
                const int rank = nroot + __popcll(bal & ((1ull << lane) - 1ull));
                if (rank < 64) s_root[wv][rank] = (unsigned char)x;
            }
            nroot += __popcll(bal);
        }
        if (nroot != ord) {
            errs = -1;
        } else {
            // ---- the evaluator S Lambda mod x^nr, then the value at every root ----
            if (lane < nr) {
                unsigned om = 0;
                const int hi = lane < top ? lane : top;
                for (int i = 0; i <= hi; i++) {
                    const int ll = lam[i];
                    const unsigned s = s_syn[wv][lane - i];
                    if (ll && s) om ^= s_exp[ll + s_log[s]];
                }
                s_om[wv][lane] = om ? s_log[om] : (unsigned char)0;
            }
            wave_sync();
            if (lane < ord) {
                const int x = s_root[wv][lane];          // never 0: the locator's constant term is 1
                const int lx = s_log[x];
                unsigned num = 0, den = 0;
                int e = 0;
                for (int k = 0; k < nr; k++) {
                    const int lo = s_om[wv][k];
                    if (lo) num ^= s_exp[lo + e];
                    e = wrap255(e + lx);
                }
                e = 0;
                for (int k = 1; k <= top; k += 2) {        // the formal derivative keeps the odd coefficients: Lambda[k] x^(k - 1)
                    const int ll = lam[k];
                    if (ll) den ^= s_exp[ll + e];
                    e = wrap255(wrap255(e + lx) + lx);
                }
                unsigned val = 0;
                if (num && den) {
                    const unsigned q = s_exp[255 + s_log[num] - s_log[den]];
                    const unsigned pw = s_exp[(lx * a.fpow) % 255];
                    val = s_exp[s_log[pw] + s_log[q]];
                }
                const int loc = ((255 - lx) * a.gap_inv) % 255;   // the coefficient; log 1 = 255 gives 0
                cw[254 - loc] ^= (unsigned char)val;
            }
        }
    }
    if (lane == 0) {
        if (errs < 0) s_bad = 1;
        if (a.errs) a.errs[((long long)row * a.nframes + f) * I + wv] = errs;
    }
    __syncthreads();
    const long long fi = (long long)row * a.nframes + f;
    if (s_bad) {
        if (t == 0) a.good[fi] = 0;
        return;
    }
    if (t == 0) a.good[fi] = 1;
    // out[i] = out_map[p < k ? msg[i % I][p] : 0] ^ xor[i], p = i / I: four bytes per lane and store
    unsigned* dst = reinterpret_cast<unsigned*>(a.scratch + fi * a.slot);
    const unsigned char* xr = a.tab + kRsTab;
    for (int j = t; 4 * j < a.frame_out; j += nt) {
        unsigned v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = 4 * j + b;
            if (i < a.frame_out) {
                const int p = i / I;
                const unsigned m = p < a.k ? s_cw[i - p * I][p] : 0u;
                v |= (unsigned)(s_omap[m] ^ xr[i]) << (8 * b);
            }
        }
        dst[j] = v;
    }
}

__global__ __launch_bounds__(kRsScanNT) void rs_scan_kernel(const RsArgs a) {
    __shared__ int wtot[kRsScanNT / 64];
    const int row = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n = rs_row_count(a.in_counts, row, a.nframes);
    const unsigned char* good = a.good + (long long)row * a.nframes;
    int* slots = a.slots + (long long)row * a.nframes;
    int running = 0;
    for (int base = 0; base < n; base += kRsScanNT) {
        const int i = base + t;
        const bool g = i < n && good[i];
        const unsigned long long bal = __ballot(g);
        if (lane == 0) wtot[wv] = __popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < kRsScanNT / 64; k++) {
            if (k < wv) off += wtot[k];
            tot += wtot[k];
        }
        if (i < n) slots[i] = g ? running + off + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
        running += tot;
        __syncthreads();
    }
    if (t == 0) a.counts[row] = running;
}

__global__ __launch_bounds__(kRsPackNT) void rs_pack_kernel(const RsArgs a) {
    const int f = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
    if (f >= rs_row_count(a.in_counts, row, a.nframes)) return;
    const long long fi = (long long)row * a.nframes + f;
    const int slot = a.slots[fi];
    if (slot < 0) return;
    const unsigned char* src = a.scratch + fi * a.slot;                      // 16-byte aligned
    unsigned char* dst = a.out + (long long)row * a.out_stride + (long long)slot * a.frame_out;
    const int fo = a.frame_out;
    int head = (int)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > fo) head = fo;
    const int nvec = (fo - head) >> 4, tail0 = head + 16 * nvec;
    if (t < head) dst[t] = src[t];
    const int sh = head & 3;
    for (int v = t; v < nvec; v += kRsPackNT) {
        const int off = head + 16 * v;
        const unsigned* w = reinterpret_cast<const unsigned*>(src + (off - sh));   // off + 20 - sh <= the slot's padded size
        const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
        *reinterpret_cast<uint4*>(dst + off) =
            make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh),
                       __builtin_amdgcn_alignbyte(w4, w3, sh));
    }
    if (t < fo - tail0) dst[tail0 + t] = src[tail0 + t];                    // fewer than 16
}

}  // namespace qk

namespace qh {

namespace {

bool spans_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}

constexpr int64_t kRsMaxFrames = (int64_t)1 << 22;     // per row and call

void rs_free(Rs* d) {
    op_free(d, [d] {
        hip_free_all({d->d_tab, d->d_scratch, d->d_good, d->d_slots, d->d_counts});
        if (d->h_count) (void)hipHostFree(d->h_count);
    });
}

// scratch slots, flags and output slots for calls of up to `frames` frames per row (a larger call than any before synchronises)
hipError_t rs_scratch(Rs* d, int64_t frames) {
    if (frames <= d->scratch_frames) return hipSuccess;
    hipError_t err = hipDeviceSynchronize();
    for (void* p : {(void*)d->d_scratch, (void*)d->d_good, (void*)d->d_slots})
        if (p) (void)hipFree(p);
    d->d_scratch = d->d_good = nullptr;
    d->d_slots = nullptr;
    d->scratch_frames = 0;
    const size_t n = (size_t)d->nchan * (size_t)frames;
    if (err == hipSuccess) err = hipMalloc(&d->d_scratch, n * (size_t)d->slot);
    if (err == hipSuccess) err = hipMalloc(&d->d_good, n);
    if (err == hipSuccess) err = hipMalloc(&d->d_slots, n * sizeof(int));
    if (err == hipSuccess) d->scratch_frames = frames;
    return err;
}

// exp, log, the two maps (null: the identity) and the XOR sequence (null: none) repeated over a frame's output bytes
void rs_fill_tab(Rs* d, const uint8_t* in_map, const uint8_t* out_map, const uint8_t* xr, int xor_len) {
    d->tab.assign((size_t)qk::kRsTab + (size_t)d->p.frame_out, 0);
    memcpy(d->tab.data(), d->field.exp, 512);
    memcpy(d->tab.data() + 512, d->field.log, 256);
    for (int i = 0; i < 256; i++) {
        d->tab[768 + i] = in_map ? in_map[i] : (unsigned char)i;
        d->tab[1024 + i] = out_map ? out_map[i] : (unsigned char)i;
    }
    if (xr)
        for (int i = 0; i < d->p.frame_out; i++) d->tab[(size_t)qk::kRsTab + i] = xr[i % xor_len];
}

bool rs_xor_ok(const Rs* d, const uint8_t* xr, int xor_len) { return !xr || (xor_len >= 1 && xor_len <= qrs::kN * d->p.depth); }

// strides in bytes
int rs_launch_counts(Rs* d, const void* d_in, int64_t nframes, int64_t in_stride, const int* d_in_counts, void* d_out, int64_t out_stride,
                     int* d_errs, hipStream_t s) {
    if (nframes < 0 || nframes > kRsMaxFrames || (nframes > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < nframes * d->p.frame_in || out_stride < nframes * d->p.frame_out) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    if (nframes == 0) {
        HIPCHK(hipMemsetAsync(d->d_counts, 0, (size_t)d->nchan * sizeof(int), s));
        return 0;
    }
    const size_t in_span = (size_t)(d->nchan - 1) * in_stride + (size_t)nframes * d->p.frame_in;
    const size_t out_span = (size_t)(d->nchan - 1) * out_stride + (size_t)nframes * d->p.frame_out;
    if (spans_overlap(d_in, in_span, d_out, out_span)) return QDSP_HIP_EINVAL;
    if (const hipError_t err = rs_scratch(d, nframes)) return -(int)err;
    qk::RsArgs a;
    a.in = static_cast<const unsigned char*>(d_in);
    a.in_counts = d_in_counts;
    a.out = static_cast<unsigned char*>(d_out);
    a.tab = d->d_tab;
    a.scratch = d->d_scratch;
    a.good = d->d_good;
    a.slots = d->d_slots;
    a.counts = d->d_counts;
    a.errs = d_errs;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.nframes = (int)nframes;
    a.depth = d->p.depth;
    a.skip = d->p.skip;
    a.nroots = d->p.num_roots;
    a.k = d->p.k;
    a.g0 = (d->p.root_gap * d->p.first_root) % 255;
    a.gap = d->p.root_gap;
    a.gap_inv = d->p.gap_inv;
    a.fpow = (d->p.first_root + 254) % 255;
    a.frame_in = d->p.frame_in;
    a.frame_out = d->p.frame_out;
    a.slot = d->slot;
    const dim3 grid((unsigned)nframes, (unsigned)d->nchan);
    hipLaunchKernelGGL(qk::rs_decode_kernel, grid, dim3(64 * d->p.depth), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(qk::rs_scan_kernel, dim3((unsigned)d->nchan), dim3(qk::kRsScanNT), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(qk::rs_pack_kernel, grid, dim3(qk::kRsPackNT), 0, s, a);
    HIPCHK(hipGetLastError());
    d->last = Launch{"rs_decode_kernel", (int)grid.x, 64 * d->p.depth, qk::kRsTab + qk::kRsMaxDepth * (256 + 32 + 64 + 32 + 64) + 4};
    if (d->nchan == 1) HIPCHK(hipMemcpyAsync(d->h_count, d->d_counts, sizeof(int), hipMemcpyDeviceToHost, s));   // process_ex reads it
    return 0;
}

// the shared host path: strides in frames
int rs_launch(Rs* d, const void* d_in, int64_t nframes, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    return rs_launch_counts(d, d_in, nframes, in_stride * d->p.frame_in, nullptr, d_out, out_stride * d->p.frame_out, nullptr, s);
}

int rs_create(void** h, int device, int nchan, int max_block, qrs::Params p, const uint8_t* in_map, const uint8_t* out_map, const uint8_t* xr,
              int xor_len) {
    if (h) *h = nullptr;
    qrs::Field field;
    if (!qrs::params_ok(p, field)) return QDSP_HIP_EINVAL;
    if (max_block > kRsMaxFrames) return QDSP_HIP_EINVAL;
    Rs* d = new (std::nothrow) Rs();
    if (!d) return QDSP_HIP_ENOMEM;
    d->p = p;
    d->field = field;
    if (!rs_xor_ok(d, xr, xor_len)) {
        delete d;
        return QDSP_HIP_EINVAL;
    }
    if (const int rc = stream_op_check(h, device, nchan, max_block)) {
        delete d;
        return rc;
    }
    d->slot = (p.frame_out + 15) / 16 * 16 + qk::kRsSlotPad;
    d->launch = launch_as<Rs, rs_launch>;
    hipError_t err = stream_op_init(d, device, nchan, max_block, (size_t)p.frame_in, (size_t)p.frame_out);
    d->nchan = nchan;
    rs_fill_tab(d, in_map, out_map, xr, xor_len);
    if (err == hipSuccess) err = hipMalloc(&d->d_tab, d->tab.size());
    if (err == hipSuccess) err = hipMemcpy(d->d_tab, d->tab.data(), d->tab.size(), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc(&d->d_counts, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipMemset(d->d_counts, 0, (size_t)nchan * sizeof(int));
    if (err == hipSuccess) err = hipHostMalloc(reinterpret_cast<void**>(&d->h_count), sizeof(int), hipHostMallocDefault);
    if (err == hipSuccess) err = rs_scratch(d, max_block > 0 ? max_block : 1);
    if (err == hipSuccess) {
        *d->h_count = 0;
        err = hipDeviceSynchronize();
    }
    return op_created<rs_free>(h, d, err);
}

}  // namespace

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_rs_create(void** h, int device, int nchan, int max_block, int prim_poly, int first_root, int root_gap, int num_roots, int depth,
                       int skip, int full_out, const uint8_t* in_map, const uint8_t* out_map, const uint8_t* xor_seq, int xor_len) {
    qrs::Params p;
    p.poly = prim_poly;
    p.first_root = first_root;
    p.root_gap = root_gap;
    p.num_roots = num_roots;
    p.depth = depth;
    p.skip = skip;
    p.full_out = full_out;
    return rs_create(h, device, nchan, max_block, p, in_map, out_map, xor_seq, xor_len);
}
int qdsp_hip_falcon_rs_create(void** h, int device, int nchan, int max_block) {
    uint8_t to_db[256], from_db[256], rnd[255];
    qrs::ccsds_dual_basis(to_db, from_db);
    qrs::ccsds_randomizer(rnd);
    return qdsp_hip_rs_create(h, device, nchan, max_block, qrs::kCcsdsPoly, 120, 11, 16, 5, 4, 1, from_db, to_db, rnd, 255);
}
int qdsp_hip_rs_set_maps(void* h, const uint8_t* in_map, const uint8_t* out_map, const uint8_t* xor_seq, int xor_len) {
    Rs* d = as<Rs>(h);
    if (!d || !rs_xor_ok(d, xor_seq, xor_len)) return QDSP_HIP_EINVAL;
    rs_fill_tab(d, in_map, out_map, xor_seq, xor_len);
    return sync_upload(d, d->d_tab, d->tab.data(), d->tab.size());
}
int64_t qdsp_hip_rs_out_size(void* h, int64_t nframes) {
    Rs* d = as<Rs>(h);
    return (d && nframes >= 0) ? nframes : QDSP_HIP_EINVAL;
}
int qdsp_hip_rs_frame_in_bytes(void* h) {
    Rs* d = as<Rs>(h);
    return d ? d->p.frame_in : QDSP_HIP_EINVAL;
}
int qdsp_hip_rs_frame_out_bytes(void* h) {
    Rs* d = as<Rs>(h);
    return d ? d->p.frame_out : QDSP_HIP_EINVAL;
}
int qdsp_hip_rs_process_batch_dev(void* h, const void* d_in, int64_t nframes, int64_t in_stride_bytes, const int* d_in_counts, void* d_out,
                                  int64_t out_stride_bytes, int* d_counts, int* d_errs, void* hip_stream) {
    Rs* d = as<Rs>(h);
    if (!d) return QDSP_HIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (const int rc = rs_launch_counts(d, d_in, nframes, in_stride_bytes, d_in_counts, d_out, out_stride_bytes, d_errs, s)) return rc;
    if (d_counts) HIPCHK(hipMemcpyAsync(d_counts, d->d_counts, (size_t)d->nchan * sizeof(int), hipMemcpyDeviceToDevice, s));
    return 0;
}
int qdsp_hip_rs_process_dev(void* h, const void* d_in, int64_t nframes, void* d_out, void* hip_stream) {
    Rs* d = as<Rs>(h);
    return d ? rs_launch(d, d_in, nframes, nframes, d_out, nframes, static_cast<hipStream_t>(hip_stream)) : QDSP_HIP_EINVAL;
}
int qdsp_hip_rs_get_counts(void* h, int* counts) {
    Rs* d = as<Rs>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    return sync_download(d, counts, d->d_counts, (size_t)d->nchan * sizeof(int));
}
int qdsp_hip_rs_process_ex(void* h, const void* in, int in_link, int nframes, void* out, int out_link) {
    Rs* d = as<Rs>(h);
    // the good-frame count is returned, so the call has to have run: an output link that hands over without waiting cannot be served
    if (!d || (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE)) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, nframes, out, out_link);
    if (rc < 0 || nframes == 0) return (int)rc;
    return *d->h_count;
}
int qdsp_hip_rs_process(void* h, const uint8_t* in, int nframes, uint8_t* out) {
    return qdsp_hip_rs_process_ex(h, in, QDSP_HIP_LINK_HOST, nframes, out, QDSP_HIP_LINK_HOST);
}
void qdsp_hip_rs_destroy(void* h) { rs_free(as<Rs>(h)); }

}  // extern "C"
