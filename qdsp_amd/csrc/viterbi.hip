// viterbi.hip -- the convolutional (Viterbi) decoder over rows of terminated frames (design notes: viterbi.hip.h), and its C entry points.
#include "viterbi.hip.h"

#include <mutex>
#include <new>
#include <unordered_set>

namespace qk {

namespace {

// what one lane wrote to LDS is read by the other lanes of its wave
__device__ __forceinline__ void vit_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned vit_lane_read(unsigned v, int lane) { return (unsigned)__builtin_amdgcn_readlane((int)v, lane); }

}  // namespace

template <int ORDER, int RATE, bool SOFT>
__global__ __launch_bounds__(64 * kVitWaves) void viterbi_decode_kernel(const VitArgs a) {
    constexpr int NS = 1 << (ORDER - 1);                  // states
    constexpr int SPL = NS > 64 ? NS / 64 : 1;            // states per lane
    constexpr int HALF = SPL / 2;
    constexpr int CAP = 20 * ORDER, MTB = 5 * ORDER;      // the history ring and the minimum traceback
    constexpr int RENORM = 65535 / (255 * RATE);
    constexpr int LOADS = SOFT ? 16 * RATE + 2 : 8;       // dwords of a block of 64 steps, the misaligned ends included
    constexpr unsigned SYM = RATE == 2 ? 0xffffu : 0xffffffu;
    static_assert(CAP <= 192 && SPL <= 4, "three slices per lane, four words per slice");
    __shared__ unsigned long long s_ring[kVitWaves][CAP * SPL];
    __shared__ unsigned long long s_bits[kVitWaves][32];  // one byte per decoded bit, at its position mod 256
    __shared__ unsigned s_stage[kVitWaves][16];           // decoded bytes, at their global address mod 64
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long* ring = s_ring[wv];
    unsigned char* bits = reinterpret_cast<unsigned char*>(s_bits[wv]);
    unsigned char* stage = reinterpret_cast<unsigned char*>(s_stage[wv]);
    const int sets = a.sets;

    // the lane's branch labels: state lane + 64 k from its low and its high predecessor (fill_table: polynomial i gives bit i)
    unsigned mlo[SPL], mhi[SPL];
#pragma unroll
    for (int k = 0; k < SPL; k++) {
        const unsigned j = (unsigned)lane + 64u * k;
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < RATE; i++) {
            const unsigned bl = __popc(j & a.poly[i]) & 1u, bh = __popc((j | NS) & a.poly[i]) & 1u;
            lo |= SOFT ? (bl ? 0xffu << (8 * i) : 0u) : bl << i;
            hi |= SOFT ? (bh ? 0xffu << (8 * i) : 0u) : bh << i;
        }
        mlo[k] = lo;
        mhi[k] = hi;
    }
    const int src0 = lane >> 1;                          // the lane of the predecessors of an even register (SPL 1: of the low one)
    const int src1 = SPL == 1 ? (lane >> 1) + NS / 2 : (lane >> 1) + 32;

    const long long total = (long long)a.nchan * a.nframes;
    for (long long item = (long long)blockIdx.x * kVitWaves + wv; item < total; item += (long long)gridDim.x * kVitWaves) {
        const int row = (int)(item / a.nframes), f = (int)(item - (long long)row * a.nframes);
        if (a.in_counts) {
            const int c = a.in_counts[row];
            if (f >= c) continue;                          // (c <= 0: no frame; f < nframes already)
        }
        const uintptr_t pa = (uintptr_t)(a.in + (long long)row * a.in_stride + (long long)f * a.frame_in), pend = pa + a.frame_in;
        const uintptr_t oa = (uintptr_t)(a.out + (long long)row * a.out_stride + (long long)f * a.frame_out);

        // the aligned dwords that hold the bytes of steps t0 .. t0 + 63, one per lane
        auto block_load = [&](int t0) -> unsigned {
            const uintptr_t first = pa + (SOFT ? (uintptr_t)t0 * RATE : ((uintptr_t)t0 * RATE) >> 3);
            const uintptr_t ad = (first & ~(uintptr_t)3) + 4u * lane;
            return (lane < LOADS && ad < pend) ? *reinterpret_cast<const unsigned*>(ad) : 0u;
        };
        // lane u: the packed symbols of step t0 + u -- soft: RATE bytes, first symbol lowest; hard: RATE bits, first bit lowest
        auto block_symbols = [&](unsigned w, int t0) -> unsigned {
            const uintptr_t first = pa + (SOFT ? (uintptr_t)t0 * RATE : ((uintptr_t)t0 * RATE) >> 3);
            const uintptr_t base = first & ~(uintptr_t)3;
            const unsigned q = (unsigned)(t0 + lane) * RATE;            // hard: the step's first bit
            const unsigned off = (unsigned)(pa + (SOFT ? q : q >> 3) - base);
            const unsigned w0 = (unsigned)__shfl((int)w, (int)(off >> 2)), w1 = (unsigned)__shfl((int)w, (int)(off >> 2) + 1);
            const unsigned v = (unsigned)((((unsigned long long)w1 << 32) | w0) >> (8 * (off & 3)));
            if (SOFT) return v & SYM;
            const unsigned win = (v & 0xffu) << 8 | ((v >> 8) & 0xffu);   // MSB first
            const unsigned g = (win >> (16 - (q & 7) - RATE)) & ((1u << RATE) - 1);
            return RATE == 2 ? ((g & 1) << 1 | g >> 1) : ((g & 1) << 2 | (g & 2) | g >> 2);
        };

        unsigned pm[SPL];
#pragma unroll
        for (int k = 0; k < SPL; k++) pm[k] = 0;
        int idx = 0, len = 0, n = 0, renorm = 0;          // ring slot of the next slice, slices held, steps processed, steps since a renormalisation
        int flushed = 0;                                  // output bytes stored

        // `L` slices back from the last one, from state s; the first `mtb` steps emit nothing.  Then what is whole of the output bytes.
        auto traceback = [&](unsigned s, int mtb, int L, bool final) {
            vit_wave_sync();
            // lane l's slices l, 64 + l and 128 + l steps back
            auto slices = [&](int r, unsigned long long(&d)[SPL]) {
                const int j = 64 * r + lane;
                int slot = idx - 1 - j;
                if (slot < 0) slot += CAP;
                if (slot < 0) slot = 0;                    // (j >= L: not used)
#pragma unroll
                for (int k = 0; k < SPL; k++) d[k] = j < L ? ring[slot * SPL + k] : 0ull;
            };
            // the serial part, `cnt` steps: the word of the state, its bit, the predecessor; bit l of the result: the decision of step l
            auto chain = [&](const unsigned long long(&d)[SPL], int cnt) -> unsigned long long {
                unsigned long long m = 0ull;
                const unsigned long long a0 = d[0], a1 = d[SPL > 1 ? 1 : 0], a2 = d[SPL > 2 ? 2 : 0], a3 = d[SPL > 3 ? 3 : 0];   // (values, not an indexed array)
                for (int l = 0; l < cnt; l++) {
                    unsigned long long v = a0;
                    if constexpr (SPL == 2) v = (s >> 6) & 1 ? a1 : a0;
                    if constexpr (SPL == 4) {
                        const unsigned long long v01 = (s >> 6) & 1 ? a1 : a0, v23 = (s >> 6) & 1 ? a3 : a2;
                        v = (s >> 7) & 1 ? v23 : v01;
                    }
                    const unsigned long long w = (unsigned long long)vit_lane_read((unsigned)(v >> 32), l) << 32 | vit_lane_read((unsigned)v, l);
                    const unsigned h = (unsigned)(w >> (s & 63)) & 1u;
                    s = (s >> 1) | (h << (ORDER - 2));
                    m |= (unsigned long long)h << l;
                }
                return m;
            };
            unsigned long long d0[SPL], d1[SPL], d2[SPL];
            slices(0, d0);
            slices(1, d1);
            slices(2, d2);
            unsigned long long hm[3];
            hm[0] = chain(d0, L < 64 ? L : 64);
            hm[1] = chain(d1, L - 64 < 64 ? L - 64 : 64);
            hm[2] = chain(d2, L - 128);
            // step j back decided bit n - 1 - j of the frame
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const int j = 64 * r + lane;
                if (j >= mtb && j < L) bits[(n - 1 - j) & 255] = (unsigned char)((hm[r] >> lane) & 1ull);
            }
            vit_wave_sync();
            const int b0 = (n - L) >> 3, b1 = (n - mtb) >> 3;          // bytes [b0, b1) are whole now
            if (b0 + lane < b1) {
                const unsigned long long x = s_bits[wv][(b0 + lane) & 31];
                const unsigned lo = (unsigned)x, hi = (unsigned)(x >> 32);
                const unsigned byte = (((lo * 0x08040201u) >> 24) & 15u) << 4 | (((hi * 0x08040201u) >> 24) & 15u);
                stage[(oa + b0 + lane) & 63] = (unsigned char)byte;
            }
            vit_wave_sync();
            const uintptr_t g0 = oa + flushed, g1 = oa + b1;
            uintptr_t lim = final ? g1 : (g1 & ~(uintptr_t)3);
            if (lim < g0) lim = g0;
            const uintptr_t ad = (g0 & ~(uintptr_t)3) + 4u * lane;
            if (ad < lim) {
                const uintptr_t lo = ad < g0 ? g0 : ad, hi = ad + 4 < lim ? ad + 4 : lim;
                if (hi - lo == 4) {
                    *reinterpret_cast<unsigned*>(ad) = s_stage[wv][(ad & 63) >> 2];
                } else {
                    for (uintptr_t b = lo; b < hi; b++) *reinterpret_cast<unsigned char*>(b) = stage[b & 63];
                }
            }
            flushed = (int)(lim - oa);
            vit_wave_sync();
        };

        unsigned cur = block_load(0);
        for (int t0 = 0; t0 < sets; t0 += 64) {
            const unsigned nxt = t0 + 64 < sets ? block_load(t0 + 64) : 0u;
            const unsigned ys = block_symbols(cur, t0);
            const int ne = sets - t0 < 64 ? sets - t0 : 64;
            for (int u = 0; u < ne; u++) {
                const int t = t0 + u;
                const unsigned y = vit_lane_read(ys, u);
                const bool warm = t < ORDER - 1;
                const bool tail = t >= sets - ORDER + 1;
                unsigned np[SPL];
                unsigned long long bal[SPL];
                unsigned pk[HALF > 0 ? HALF : 1];
                if (SPL > 1) {
#pragma unroll
                    for (int h = 0; h < HALF; h++) pk[h] = pm[h] | pm[h + HALF] << 16;
                }
#pragma unroll
                for (int k = 0; k < SPL; k++) {
                    unsigned lo, hi;
                    if (SPL == 1) {
                        lo = (unsigned)__shfl((int)pm[0], src0);
                        hi = (unsigned)__shfl((int)pm[0], src1);
                    } else {
                        const unsigned v = (unsigned)__shfl((int)pk[k >> 1], (k & 1) ? src1 : src0);
                        lo = v & 0xffffu;
                        hi = v >> 16;
                    }
                    unsigned le, he;
                    if (SOFT) {
                        le = __builtin_amdgcn_sad_u8(y, mlo[k], lo);
                        he = __builtin_amdgcn_sad_u8(y, mhi[k], hi);
                    } else {
                        le = __popc(y ^ mlo[k]) + lo;
                        he = __popc(y ^ mhi[k]) + hi;
                    }
                    le &= 0xffffu;
                    he &= 0xffffu;
                    const bool dec = !warm && he < le + (tail ? 1u : 0u);   // inner: low on a tie; tail: high on a tie
                    np[k] = t == 0 ? 0u : (dec ? he : le);                   // (set 0 counts for nothing: viterbi.hip.h, phases)
                    bal[k] = __ballot(dec);
                }
                if (!warm) {
                    unsigned long long w = bal[0];
#pragma unroll
                    for (int k = 1; k < SPL; k++)
                        if (lane == k) w = bal[k];
                    if (lane < SPL) ring[idx * SPL + lane] = w;
                    idx = idx + 1 == CAP ? 0 : idx + 1;
                    renorm++;
                    len++;
                    n++;
                    const bool ren = renorm == RENORM, tb = len == CAP;
                    if (ren || tb) {
                        // the best state among every skip-th, the lowest at the minimum
                        const unsigned skip = tail ? 1u << (ORDER - (sets - t)) : 1u;
                        unsigned key = ~0u;
#pragma unroll
                        for (int k = 0; k < SPL; k++) {
                            const unsigned st = (unsigned)lane + 64u * k;
                            const unsigned c = (st < (unsigned)NS && !(st & (skip - 1))) ? (np[k] << 16 | st) : ~0u;
                            key = c < key ? c : key;
                        }
#pragma unroll
                        for (int m = 32; m >= 1; m >>= 1) {
                            const unsigned o = (unsigned)__shfl_xor((int)key, m);
                            key = o < key ? o : key;
                        }
                        key = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
                        if (ren) {
                            renorm = 0;
#pragma unroll
                            for (int k = 0; k < SPL; k++) np[k] = (np[k] - (key >> 16)) & 0xffffu;
                        }
                        if (tb) {
                            traceback(key & 0xffffu, MTB, CAP, false);
                            len = MTB;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < SPL; k++) pm[k] = np[k];
            }
            cur = nxt;
        }
        traceback(0u, 0, len, true);                      // the flush: from state 0, every slice emits
    }
}

}  // namespace qk

namespace qh {

namespace {

// The live decoders, by address.  Entered last in create, removed first in destroy; a lookup never reads the caller's pointer.
std::mutex g_vit_mu;
std::unordered_set<const void*>& vit_live() {
    static auto* s = new std::unordered_set<const void*>();   // (alive for the whole process, like the per-row table)
    return *s;
}

Viterbi* as_viterbi(void* h) {
    if (!h) return nullptr;
    std::lock_guard<std::mutex> lk(g_vit_mu);
    return vit_live().count(h) ? static_cast<Viterbi*>(h) : nullptr;
}

bool spans_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}

constexpr int64_t kVitMaxFrames = (int64_t)1 << 22;       // per row and call

template <int ORDER, int RATE>
void vit_launch_as(const Viterbi* d, const qk::VitArgs& a, dim3 grid, hipStream_t s) {
    if (d->soft)
        hipLaunchKernelGGL((qk::viterbi_decode_kernel<ORDER, RATE, true>), grid, dim3(64 * qk::kVitWaves), 0, s, a);
    else
        hipLaunchKernelGGL((qk::viterbi_decode_kernel<ORDER, RATE, false>), grid, dim3(64 * qk::kVitWaves), 0, s, a);
}

// strides in bytes
int vit_launch_counts(Viterbi* d, const void* d_in, int64_t nframes, int64_t in_stride, const int* d_in_counts, void* d_out, int64_t out_stride,
                      hipStream_t s) {
    if (nframes < 0 || nframes > kVitMaxFrames || (nframes > 0 && (!d_in || !d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < nframes * d->frame_in || out_stride < nframes * d->frame_out) return QDSP_HIP_EINVAL;
    if (nframes == 0) return 0;
    const size_t in_span = (size_t)(d->nchan - 1) * in_stride + (size_t)nframes * d->frame_in;
    const size_t out_span = (size_t)(d->nchan - 1) * out_stride + (size_t)nframes * d->frame_out;
    if (spans_overlap(d_in, in_span, d_out, out_span)) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    qk::VitArgs a;
    a.in = static_cast<const unsigned char*>(d_in);
    a.in_counts = d_in_counts;
    a.out = static_cast<unsigned char*>(d_out);
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.nchan = d->nchan;
    a.nframes = (int)nframes;
    a.sets = d->sets;
    a.frame_in = d->frame_in;
    a.frame_out = d->frame_out;
    for (int i = 0; i < 3; i++) a.poly[i] = d->poly[i];
    const int64_t wgs = ((int64_t)d->nchan * nframes + qk::kVitWaves - 1) / qk::kVitWaves;
    const dim3 grid((unsigned)(wgs < qk::kVitMaxGrid ? wgs : qk::kVitMaxGrid));
    const int spl = d->order >= 8 ? 1 << (d->order - 7) : 1;
    if (d->rate == 2) {
        switch (d->order) {
            case 6: vit_launch_as<6, 2>(d, a, grid, s); break;
            case 7: vit_launch_as<7, 2>(d, a, grid, s); break;
            case 8: vit_launch_as<8, 2>(d, a, grid, s); break;
            default: vit_launch_as<9, 2>(d, a, grid, s); break;
        }
    } else {
        switch (d->order) {
            case 6: vit_launch_as<6, 3>(d, a, grid, s); break;
            case 7: vit_launch_as<7, 3>(d, a, grid, s); break;
            case 8: vit_launch_as<8, 3>(d, a, grid, s); break;
            default: vit_launch_as<9, 3>(d, a, grid, s); break;
        }
    }
    HIPCHK(hipGetLastError());
    d->last = Launch{"viterbi_decode_kernel", (int)grid.x, 64 * qk::kVitWaves, qk::kVitWaves * (160 * d->order * spl + 320)};
    return 0;
}

// the shared host path: strides in frames
int vit_launch(Viterbi* d, const void* d_in, int64_t nframes, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t s) {
    return vit_launch_counts(d, d_in, nframes, in_stride * d->frame_in, nullptr, d_out, out_stride * d->frame_out, s);
}

void vit_free(Viterbi* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    stream_op_release(d);
    delete d;
}

}  // namespace

const Launch* viterbi_last(void* h) {
    Viterbi* d = as_viterbi(h);
    return d ? &d->last : nullptr;
}

}  // namespace qh

using namespace qh;

extern "C" {

int qdsp_hip_viterbi_create(void** h, int device, int nchan, int max_block, int rate, int order, const uint16_t* poly, int sets, int soft) {
    if (h) *h = nullptr;
    if ((rate != 2 && rate != 3) || order < 6 || order > 9 || !poly || (soft != 0 && soft != 1)) return QDSP_HIP_EINVAL;
    if (sets < order + 7 || sets > 65536 || max_block > kVitMaxFrames) return QDSP_HIP_EINVAL;
    for (int i = 0; i < rate; i++)
        if (poly[i] >= (1u << order)) return QDSP_HIP_EINVAL;
    if (const int rc = stream_op_check(h, device, nchan, max_block)) return rc;
    Viterbi* d = new (std::nothrow) Viterbi();
    if (!d) return QDSP_HIP_ENOMEM;
    d->rate = rate;
    d->order = order;
    d->sets = sets;
    d->soft = soft;
    for (int i = 0; i < rate; i++) d->poly[i] = poly[i];
    d->frame_in = soft ? sets * rate : (sets * rate + 7) / 8;
    d->frame_out = (sets - order + 1) / 8;
    d->launch = launch_as<Viterbi, vit_launch>;
    const hipError_t err = stream_op_init(d, device, nchan, max_block, (size_t)d->frame_in, (size_t)d->frame_out);
    d->nchan = nchan;
    if (err != hipSuccess) {
        vit_free(d);
        return -(int)err;
    }
    {
        std::lock_guard<std::mutex> lk(g_vit_mu);
        vit_live().insert(d);
    }
    *h = d;
    return 0;
}
int qdsp_hip_viterbi_frame_in_bytes(void* h) {
    Viterbi* d = as_viterbi(h);
    return d ? d->frame_in : QDSP_HIP_EINVAL;
}
int qdsp_hip_viterbi_frame_out_bytes(void* h) {
    Viterbi* d = as_viterbi(h);
    return d ? d->frame_out : QDSP_HIP_EINVAL;
}
int qdsp_hip_viterbi_process_batch_dev(void* h, const void* d_in, int64_t nframes, int64_t in_stride_bytes, const int* d_in_counts, void* d_out,
                                       int64_t out_stride_bytes, void* hip_stream) {
    Viterbi* d = as_viterbi(h);
    if (!d) return QDSP_HIP_EINVAL;
    return vit_launch_counts(d, d_in, nframes, in_stride_bytes, d_in_counts, d_out, out_stride_bytes, static_cast<hipStream_t>(hip_stream));
}
int qdsp_hip_viterbi_process_dev(void* h, const void* d_in, int64_t nframes, void* d_out, void* hip_stream) {
    Viterbi* d = as_viterbi(h);
    return d ? vit_launch(d, d_in, nframes, nframes, d_out, nframes, static_cast<hipStream_t>(hip_stream)) : QDSP_HIP_EINVAL;
}
int qdsp_hip_viterbi_process_ex(void* h, const void* in, int in_link, int nframes, void* out, int out_link) {
    Viterbi* d = as_viterbi(h);
    return d ? (int)stream_op_process_ex(d, in, in_link, nframes, out, out_link) : QDSP_HIP_EINVAL;
}
int qdsp_hip_viterbi_process(void* h, const uint8_t* in, int nframes, uint8_t* out) {
    return qdsp_hip_viterbi_process_ex(h, in, QDSP_HIP_LINK_HOST, nframes, out, QDSP_HIP_LINK_HOST);
}
void qdsp_hip_viterbi_destroy(void* h) {
    if (!h) return;
    {
        std::lock_guard<std::mutex> lk(g_vit_mu);
        if (!vit_live().erase(h)) return;
    }
    vit_free(static_cast<Viterbi*>(h));
}

}  // extern "C"
