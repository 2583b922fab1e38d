// TEST-ONLY stand-in for qdsp_amd/csrc/rs.hip on the fake synchronous HIP runtime (fake_hip_runtime.cpp), so that falcon_check --
// dsp/falcon_fec.h over the real qdsp_amd/csrc/stream_op.cpp -- runs under -fsanitize=address,undefined without a GPU
// (tests/test_rs_cpu.py).  Same C entry points and handle plumbing as the library's, the tables of qdsp_amd/csrc/rs_tables.h; the
// "kernel" is a plain loop per codeword, scalar, in the order include/qdsp_hip.h states the decode.  One channel.  "Device" memory is
// host memory here.
#include "../../qdsp_amd/csrc/rs_tables.h"
#include "../../qdsp_amd/csrc/stream_op.h"

#include <string.h>

#include <new>
#include <vector>

using namespace qh;

namespace {

struct FakeRs : StreamOp {
    static constexpr OpKind kKind = OpKind::Rs;
    qrs::Params p;
    qrs::Field f;
    uint8_t in_map[256], out_map[256];
    std::vector<uint8_t> xr;
    int last_count = 0;
};
void drop(FakeRs* d) {
    op_free(d, [] {});
}

uint8_t mul(const qrs::Field& f, uint8_t a, uint8_t b) { return (a && b) ? f.exp[f.log[a] + f.log[b]] : 0; }
uint8_t dvd(const qrs::Field& f, uint8_t a, uint8_t b) { return (a && b) ? f.exp[255 + f.log[a] - f.log[b]] : 0; }     // x / 0 = 0
uint8_t pw(const qrs::Field& f, uint8_t a, int n) { return f.exp[((f.log[a] * n) % 255 + 255) % 255]; }

// one codeword in place; the symbols corrected, or -1
int decode_word(const FakeRs* d, uint8_t* word) {
    const qrs::Field& f = d->f;
    const int nr = d->p.num_roots;
    uint8_t coeff[255], syn[qrs::kMaxRoots];
    for (int i = 0; i < 255; i++) coeff[i] = word[254 - i];
    bool dirty = false;
    for (int i = 0; i < nr; i++) {
        uint8_t s = 0;
        for (int k = 0; k < 255; k++) s ^= mul(f, coeff[k], f.exp[(d->p.root_gap * (d->p.first_root + i) % 255 * k) % 255]);
        syn[i] = s;
        dirty |= s != 0;
    }
    if (!dirty) return 0;
    constexpr int W = 2 * qrs::kMaxRoots + 4;
    uint8_t C[W] = {1}, B[W] = {1};
    int L = 0, order = 0, lorder = 0, delay = 1;
    uint8_t last_d = 1;
    for (int i = 0; i < nr; i++) {
        uint8_t disc = syn[i];
        for (int j = 1; j <= L; j++) disc ^= mul(f, C[j], syn[i - j]);
        if (!disc) {
            delay++;
            continue;
        }
        if (2 * L <= i) {
            for (int j = lorder; j >= 0; j--) B[j + delay] = dvd(f, mul(f, B[j], disc), last_d);
            for (int j = delay - 1; j >= 0; j--) B[j] = 0;
            for (int j = 0; j <= lorder + delay; j++) {
                const uint8_t t = C[j];
                C[j] ^= B[j];
                B[j] = t;
            }
            const int t = order;
            order = lorder + delay;
            lorder = t;
            L = i + 1 - L;
            last_d = disc;
            delay = 1;
        } else {
            for (int j = lorder; j >= 0; j--) C[j + delay] ^= dvd(f, mul(f, B[j], disc), last_d);
            if (lorder + delay > order) order = lorder + delay;
            delay++;
        }
    }
    uint8_t roots[256];
    int nroots = 0;
    for (int x = 0; x < 256; x++) {
        uint8_t v = C[0];
        if (x)
            for (int j = 1; j <= order; j++) v ^= mul(f, C[j], pw(f, (uint8_t)x, j));
        if (!v) roots[nroots++] = (uint8_t)x;
    }
    if (nroots != order) return -1;
    uint8_t om[qrs::kMaxRoots] = {};
    for (int i = 0; i <= order; i++)
        for (int j = 0; i + j < nr; j++) om[i + j] ^= mul(f, C[i], syn[j]);
    for (int r = 0; r < nroots; r++) {
        const uint8_t x = roots[r];
        if (!x) continue;
        const uint8_t inv = dvd(f, 1, x);
        int loc = 0;
        for (int j = 0; j < 256; j++)
            if (pw(f, (uint8_t)j, d->p.root_gap) == inv) {
                loc = f.log[j];
                break;
            }
        uint8_t num = 0, den = 0;
        for (int k = 0; k < nr; k++) num ^= mul(f, om[k], pw(f, x, k));
        for (int k = 1; k <= order; k += 2) den ^= mul(f, C[k], pw(f, x, k - 1));
        coeff[loc] ^= mul(f, pw(f, x, d->p.first_root - 1), dvd(f, num, den));
    }
    for (int i = 0; i < 255; i++) word[i] = coeff[254 - i];
    return order;
}

int launch_counts(FakeRs* d, const void* d_in, int64_t nframes, int64_t in_stride, int64_t n, void* d_out, int64_t out_stride, int* d_errs) {
    if (nframes < 0 || (nframes > 0 && (!d_in || !d_out || d_in == d_out))) return QDSP_HIP_EINVAL;
    if (in_stride < nframes * d->p.frame_in || out_stride < nframes * d->p.frame_out) return QDSP_HIP_EINVAL;
    const int I = d->p.depth;
    const uint8_t* in = static_cast<const uint8_t*>(d_in);
    uint8_t* out = static_cast<uint8_t*>(d_out);
    d->last_count = 0;
    std::vector<uint8_t> cw((size_t)I * 255);
    for (int64_t fr = 0; fr < n; fr++) {
        const uint8_t* x = in + fr * d->p.frame_in + d->p.skip;
        for (int i = 0; i < 255 * I; i++) cw[(size_t)(i % I) * 255 + i / I] = d->in_map[x[i]];
        bool good = true;
        for (int c = 0; c < I; c++) {
            const int e = decode_word(d, cw.data() + (size_t)c * 255);
            if (d_errs) d_errs[fr * I + c] = e;
            good &= e >= 0;
        }
        if (!good) continue;
        uint8_t* y = out + (size_t)d->last_count * d->p.frame_out;
        for (int i = 0; i < d->p.frame_out; i++) {
            const int p = i / I;
            y[i] = d->out_map[p < d->p.k ? cw[(size_t)(i % I) * 255 + p] : 0] ^ d->xr[(size_t)i % d->xr.size()];
        }
        d->last_count++;
    }
    return 0;
}

int64_t launch(FakeRs* d, const void* d_in, int64_t nframes, int64_t in_stride, void* d_out, int64_t out_stride, hipStream_t) {
    return launch_counts(d, d_in, nframes, in_stride * d->p.frame_in, nframes, d_out, out_stride * d->p.frame_out, nullptr);
}

bool set_maps(FakeRs* d, const uint8_t* in_map, const uint8_t* out_map, const uint8_t* xr, int xor_len) {
    if (xr && (xor_len < 1 || xor_len > 255 * d->p.depth)) return false;
    for (int i = 0; i < 256; i++) {
        d->in_map[i] = in_map ? in_map[i] : (uint8_t)i;
        d->out_map[i] = out_map ? out_map[i] : (uint8_t)i;
    }
    if (xr) d->xr.assign(xr, xr + xor_len);
    else d->xr.assign(1, 0);
    return true;
}

}  // namespace

extern "C" {

int qdsp_hip_rs_create(void** h, int device, int nchan, int max_block, int prim_poly, int first_root, int root_gap, int num_roots, int depth,
                       int skip, int full_out, const uint8_t* in_map, const uint8_t* out_map, const uint8_t* xor_seq, int xor_len) {
    if (h) *h = nullptr;
    FakeRs* d = new (std::nothrow) FakeRs();
    if (!d) return QDSP_HIP_ENOMEM;
    d->p.poly = prim_poly;
    d->p.first_root = first_root;
    d->p.root_gap = root_gap;
    d->p.num_roots = num_roots;
    d->p.depth = depth;
    d->p.skip = skip;
    d->p.full_out = full_out;
    int rc = (nchan == 1 && qrs::params_ok(d->p, d->f) && set_maps(d, in_map, out_map, xor_seq, xor_len)) ? 0 : QDSP_HIP_EINVAL;
    if (!rc) rc = stream_op_check(h, device, nchan, max_block);
    if (!rc) {
        d->launch = launch_as<FakeRs, launch>;
        rc = -(int)stream_op_init(d, device, nchan, max_block, (size_t)d->p.frame_in, (size_t)d->p.frame_out);
    }
    return op_created<drop>(h, d, rc);
}
int qdsp_hip_falcon_rs_create(void** h, int device, int nchan, int max_block) {
    uint8_t to_db[256], from_db[256], rnd[255];
    qrs::ccsds_dual_basis(to_db, from_db);
    qrs::ccsds_randomizer(rnd);
    return qdsp_hip_rs_create(h, device, nchan, max_block, qrs::kCcsdsPoly, 120, 11, 16, 5, 4, 1, from_db, to_db, rnd, 255);
}
int qdsp_hip_rs_set_maps(void* h, const uint8_t* in_map, const uint8_t* out_map, const uint8_t* xor_seq, int xor_len) {
    FakeRs* d = as<FakeRs>(h);
    return (d && set_maps(d, in_map, out_map, xor_seq, xor_len)) ? 0 : QDSP_HIP_EINVAL;
}
int64_t qdsp_hip_rs_out_size(void* h, int64_t nframes) { return (as<FakeRs>(h) && nframes >= 0) ? nframes : QDSP_HIP_EINVAL; }
int qdsp_hip_rs_frame_in_bytes(void* h) {
    FakeRs* d = as<FakeRs>(h);
    return d ? d->p.frame_in : QDSP_HIP_EINVAL;
}
int qdsp_hip_rs_frame_out_bytes(void* h) {
    FakeRs* d = as<FakeRs>(h);
    return d ? d->p.frame_out : QDSP_HIP_EINVAL;
}
int qdsp_hip_rs_process_batch_dev(void* h, const void* d_in, int64_t nframes, int64_t in_stride_bytes, const int* d_in_counts, void* d_out,
                                  int64_t out_stride_bytes, int* d_counts, int* d_errs, void*) {
    FakeRs* d = as<FakeRs>(h);
    if (!d) return QDSP_HIP_EINVAL;
    const int64_t n = d_in_counts ? (d_in_counts[0] < 0 ? 0 : (d_in_counts[0] < nframes ? d_in_counts[0] : nframes)) : nframes;
    const int rc = launch_counts(d, d_in, nframes, in_stride_bytes, n, d_out, out_stride_bytes, d_errs);
    if (rc == 0 && d_counts) d_counts[0] = d->last_count;
    return rc;
}
int qdsp_hip_rs_process_dev(void* h, const void* d_in, int64_t nframes, void* d_out, void* s) {
    FakeRs* d = as<FakeRs>(h);
    return d ? (int)launch(d, d_in, nframes, nframes, d_out, nframes, static_cast<hipStream_t>(s)) : QDSP_HIP_EINVAL;
}
int qdsp_hip_rs_get_counts(void* h, int* counts) {
    FakeRs* d = as<FakeRs>(h);
    if (!d || !counts) return QDSP_HIP_EINVAL;
    counts[0] = d->last_count;
    return 0;
}
int qdsp_hip_rs_process_ex(void* h, const void* in, int in_link, int nframes, void* out, int out_link) {
    FakeRs* d = as<FakeRs>(h);
    if (!d || (out_link != QDSP_HIP_LINK_HOST && out_link != QDSP_HIP_LINK_DEVICE)) return QDSP_HIP_EINVAL;
    const int64_t rc = stream_op_process_ex(d, in, in_link, nframes, out, out_link);
    if (rc < 0 || nframes == 0) return (int)rc;
    return d->last_count;
}
int qdsp_hip_rs_process(void* h, const uint8_t* in, int nframes, uint8_t* out) {
    return qdsp_hip_rs_process_ex(h, in, QDSP_HIP_LINK_HOST, nframes, out, QDSP_HIP_LINK_HOST);
}
void qdsp_hip_rs_destroy(void* h) { drop(as<FakeRs>(h)); }

}  // extern "C"
