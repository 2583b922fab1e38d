// qdsp_hip.hip -- host side of libqdsp_hip.so: engine state + the extern "C" boundary
// declared in include/qdsp_hip.h.  gfx950 only; no CPU fallback exists anywhere in this
// library: without a HIP device every entry point returns an error.
#include "engine.hip.h"

namespace qh {

Engine* as_engine(void* h, Kind k) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || e->magic != kMagic || e->kind != k) return nullptr;
    return e;
}

long double turns_of(float re, float im) {
    // arg(phase_inc)/2pi in [0,1): the angle the reference's recursive phasor actually
    // advances by each sample is that of the ROUNDED float pair, not of the ideal theta.
    const long double two_pi = 6.283185307179586476925286766559005768L;
    long double t = atan2l((long double)im, (long double)re) / two_pi;
    t -= floorl(t);
    return t;
}
unsigned long long fx_of_turns(long double t) {
    t -= floorl(t);
    long double s = ldexpl(t, 64);
    if (s >= 18446744073709551615.0L) return 0ULL;
    return (unsigned long long)s;
}
void unit_of_fx(unsigned long long ph, long double mult, double* c, double* s) {
    // exp(j*2pi*frac(ph/2^64 * mult)) in long double, rounded to double
    const long double two_pi = 6.283185307179586476925286766559005768L;
    long double t = ldexpl((long double)ph, -64) * mult;
    t -= floorl(t);
    *c = (double)cosl(two_pi * t);
    *s = (double)sinl(two_pi * t);
}

// The same for the per-call NCO constants that only depend on the increment (step phasors, per-lane / per-row tables in
// the kernel arguments): memoised per thread -- a block's worker thread launches for one handle -- because at
// reference-sized calls 10-30 long-double sincos per call (1.5-4 us of host time) are as long as the kernel itself.
// 128 direct-mapped entries keyed by (increment, integer multiple); a retune simply misses.
void unit_of_fx_c(unsigned long long ph, long double mult, double* c, double* s) {
    struct Memo { unsigned long long ph; long long m; double c, s; bool ok; };
    static thread_local Memo memo[128];
    const long long m = (long long)mult;
    if ((long double)m != mult) { unit_of_fx(ph, mult, c, s); return; }
    const unsigned idx = (unsigned)(((ph * 0x9E3779B97F4A7C15ULL) ^ ((unsigned long long)m * 0xC2B2AE3D27D4EB4FULL)) >> 57);
    Memo& e = memo[idx];
    if (!(e.ok && e.ph == ph && e.m == m)) {
        unit_of_fx(ph, mult, &e.c, &e.s);
        e.ph = ph;
        e.m = m;
        e.ok = true;
    }
    *c = e.c;
    *s = e.s;
}

int64_t out_size(const Engine* e, int64_t count) {
    if (!e->has_filter) return count;
    return (count * e->L) / e->M;  // calcOutSize, resampling.h:95-97 (L = M = 1 for FIR)
}

int upload_taps(Engine* e, const float* taps, int ntaps) {
    // FIR: h[k] pairs with s[n - (ntaps-1) + k]  -> core with M=1, Q=ntaps, H=ntaps-1
    // resampler L==1: tapPhases[0][t] = taps[t]   -> core with M, Q=ceil(P/M), H=P
    // otherwise: [L][P] phase table, buildTapPhases (resampling.h:137-166)
    std::vector<float> host;
    const Plan plan = e->plan = plan_of(desc_of(e));
    if (e->d_taps_plain) { HIPCHK(hipFree(e->d_taps_plain)); e->d_taps_plain = nullptr; }
    if (plan.core) {
        const int K = e->P;
        const int Q = (K + e->M - 1) / e->M;
        host.assign((size_t)e->M * Q, 0.0f);
        for (int k = 0; k < K; k++) host[(size_t)(k % e->M) * Q + k / e->M] = taps[k];
    } else {
        host.assign((size_t)e->L * e->P, 0.0f);
        int cur = 0;
        for (int tap = 0; tap < e->P; tap++)
            for (int phase = 0; phase < e->L; phase++)
                host[(size_t)((e->L - 1) - phase) * e->P + tap] = (cur < ntaps) ? taps[cur++] : 0.0f;
    }
    if (e->d_taps) { HIPCHK(hipFree(e->d_taps)); e->d_taps = nullptr; }
    HIPCHK(hipMalloc(&e->d_taps, host.size() * sizeof(float)));
    HIPCHK(hipMemcpy(e->d_taps, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    if (e->d_taps_lm) { HIPCHK(hipFree(e->d_taps_lm)); e->d_taps_lm = nullptr; }
    if (plan.win) {
        // decim_win_kernel: hp[k + M*(R-1)] = h[k], zeros around (d_taps_lm doubles as its table)
        const int M = e->M, P = e->P, R = win_R(M, P), MR = M * R;
        const int nchunks = (M * (R - 1) + P + MR - 1) / MR;
        std::vector<float> w((size_t)nchunks * MR + (size_t)M * (R - 1) + 16, 0.0f);
        for (int k = 0; k < P; k++) w[(size_t)k + M * (R - 1)] = taps[k];
        HIPCHK(hipMalloc(&e->d_taps_lm, w.size() * sizeof(float)));
        HIPCHK(hipMemcpy(e->d_taps_lm, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (plan.lm) {
        // sub-filter c of resamp_lm_kernel: h_c = phases[(c*M) % L], stored branch-major [c][m][q] = h_c[q*M + m]
        const int L = e->L, M = e->M, P = e->P, Q = (P + M - 1) / M;
        std::vector<float> lm((size_t)L * M * Q, 0.0f);
        for (int c = 0; c < L; c++) {
            const float* hc = host.data() + (size_t)((c * M) % L) * P;
            for (int k = 0; k < P; k++) lm[((size_t)c * M + k % M) * Q + k / M] = hc[k];
        }
        // M == 1: the same taps transposed, [q][c], behind the first table
        const size_t n1 = lm.size();
        if (M == 1) {
            lm.resize(2 * n1);
            for (int c = 0; c < L; c++)
                for (int q = 0; q < Q; q++) lm[n1 + (size_t)q * L + c] = lm[(size_t)c * Q + q];
        }
        e->taps_lm_t_off = M == 1 ? n1 : 0;
        HIPCHK(hipMalloc(&e->d_taps_lm, lm.size() * sizeof(float)));
        HIPCHK(hipMemcpy(e->d_taps_lm, lm.data(), lm.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    // MFMA decimator (mf_dec.hip.h): A operand of set s, step (jj, a), lane l = tap row q = 16 s + l % 16, column 8 jj + 2 (l / 16) + a
    if (e->d_taps_mf) { HIPCHK(hipFree(e->d_taps_mf)); e->d_taps_mf = nullptr; }
    if (plan.mf.KJ) {
        const int KJ = plan.mf.KJ, QS = plan.mf.QS, Mk = plan.mf.keep2 ? e->M / 2 : e->M;
        std::vector<float> tk((size_t)QS * 2 * KJ * 64, 0.0f);
        for (int sset = 0; sset < QS; sset++)
            for (int jj = 0; jj < KJ; jj++)
                for (int a = 0; a < 2; a++)
                    for (int l = 0; l < 64; l++) {
                        const int q = 16 * sset + l % 16, col = 8 * jj + 2 * (l / 16) + a, k = Mk * q + col;
                        if (col < Mk && k < e->P) tk[((size_t)(sset * KJ + jj) * 2 + a) * 64 + l] = taps[k];
                    }
        HIPCHK(hipMalloc(&e->d_taps_mf, tk.size() * sizeof(float)));
        HIPCHK(hipMemcpy(e->d_taps_mf, tk.data(), tk.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    // rational MFMA resampler (rm_resamp.hip.h): the A operands of the plan's band matrix (rm_plan, select.cpp), in lane order
    if (e->d_taps_rm) { HIPCHK(hipFree(e->d_taps_rm)); e->d_taps_rm = nullptr; }
    if (plan.rm.ngrp) {
        const int L0 = e->L, M0 = e->M, P = e->P, L = plan.rm.J * L0, nblk = (L + 3) / 4;
        const int ngrp = plan.rm.ngrp, KB = plan.rm.KB, qpb = plan.rm.qpb;
        std::vector<float> tab((size_t)ngrp * KB * 64 + (size_t)2 * ngrp * 64, 0.0f);
        int* cbl = reinterpret_cast<int*>(tab.data() + (size_t)ngrp * KB * 64);
        int* meta = cbl + (size_t)ngrp * 64;
        for (int g = 0; g < ngrp; g++)
            for (int l = 0; l < 64; l++) {
                const int slot = l / 4;            // block slot of the step
                const int b = ngrp > 1 || qpb == 1 ? 16 * g + slot : slot % nblk;
                const int pq = ngrp > 1 || qpb == 1 ? 0 : slot / nblk;
                const bool live = b < nblk && pq < qpb;
                const int c0 = live ? rm_c0(b, L0, M0) : 0;
                cbl[g * 64 + l] = c0;
                meta[g * 64 + l] = live ? ((pq << 16) | b) : 0xffff;
                const int i = 4 * b + l % 4;
                if (!live || i >= L) continue;
                const int off = (int)(((long long)i * M0) / L0), ph = (int)(((long long)i * M0) % L0);
                for (int k = 0; k < KB; k++) {
                    const int col = c0 + k;
                    if (col >= off && col < off + P) tab[((size_t)g * KB + k) * 64 + l] = host[(size_t)ph * P + (col - off)];
                }
            }
        HIPCHK(hipMalloc(&e->d_taps_rm, tab.size() * sizeof(float)));
        HIPCHK(hipMemcpy(e->d_taps_rm, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}

// The phase table [1][P] of a handle whose d_taps is branch-major (interp 1, decimation <= 8): what resamp_any_kernel reads when
// QDSP_HIP_FORCE_ANY sends such a handle's call to it.  Built on first use, dropped with the taps.
int plain_taps(Engine* e) {
    if (e->d_taps_plain) return 0;
    if ((int)e->taps_host.size() != e->P || e->L != 1) return QDSP_HIP_EINVAL;
    HIPCHK(hipMalloc(&e->d_taps_plain, (size_t)e->P * sizeof(float)));
    HIPCHK(hipMemcpy(e->d_taps_plain, e->taps_host.data(), (size_t)e->P * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// (Re)configure the filter part.  History keeps its newest samples across a resize.
int configure(Engine* e, const float* taps, int ntaps, int interp, int decim) {
    if (!taps || ntaps <= 0 || interp <= 0 || decim <= 0) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    const int oldH = e->H;
    e->L = interp;
    e->M = decim;
    e->ntaps = ntaps;
    e->P = (ntaps + interp - 1) / interp;
    const int newH = (e->kind == KIND_FIR) ? ntaps - 1 : e->P;
    int rc = upload_taps(e, taps, ntaps);
    if (rc) return rc;
    e->taps_host.assign(taps, taps + ntaps);
    e->fft_ntaps = -1;
    e->f1k_ntaps = -1;
    e->pfb_ntaps = -1;
    const size_t bytes = (size_t)(newH > 0 ? newH : 1) * e->ch * sizeof(float);
    float* nh[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; i++) {
        HIPCHK(hipMalloc(&nh[i], bytes));
        HIPCHK(hipMemset(nh[i], 0, bytes));
    }
    if (e->d_hist[0] && oldH > 0 && newH > 0) {
        const int keep = oldH < newH ? oldH : newH;
        HIPCHK(hipMemcpy(nh[0] + (size_t)(newH - keep) * e->ch,
                         e->d_hist[e->cur] + (size_t)(oldH - keep) * e->ch,
                         (size_t)keep * e->ch * sizeof(float), hipMemcpyDeviceToDevice));
    }
    for (int i = 0; i < 2; i++)
        if (e->d_hist[i]) HIPCHK(hipFree(e->d_hist[i]));
    e->d_hist[0] = nh[0];
    e->d_hist[1] = nh[1];
    e->cur = 0;
    e->raw_valid = false;
    e->H = newH;
    e->hist_cap = newH;
    return 0;
}

void set_inc_now(Engine* e, float re, float im) {
    e->raw_valid = false;   // (a retune: the rotated history stays the truth, see launch_fft)
    e->inc_re = re;
    e->inc_im = im;
    e->dturns = turns_of(re, im);
    e->dphase = fx_of_turns(e->dturns);
    e->gm1 = (float)(hypotl((long double)re, (long double)im) - 1.0L);
}

// setters: stage the increment; the worker thread applies it between two calls, never in the middle of one
void set_inc(Engine* e, float re, float im) {
    unsigned int a, b;
    memcpy(&a, &re, 4);
    memcpy(&b, &im, 4);
    e->pending_inc.store(((unsigned long long)a << 32) | b, std::memory_order_release);
}
void apply_pending_inc(Engine* e) {
    const unsigned long long v = e->pending_inc.exchange(0ULL, std::memory_order_acq_rel);
    if (!v) return;
    const unsigned int a = (unsigned int)(v >> 32), b = (unsigned int)v;
    float re, im;
    memcpy(&re, &a, 4);
    memcpy(&im, &b, 4);
    set_inc_now(e, re, im);
}

int ensure_io(Engine* e, int max_block) {
    if (max_block <= 0) return 0;
    HIPCHK(hipSetDevice(e->device));
    const size_t in_bytes = (size_t)max_block * e->ch * sizeof(float);
    const size_t oc = (size_t)out_size(e, max_block) + 1;
    if (!e->d_in || max_block > e->max_block) {
        if (e->d_in) HIPCHK(hipFree(e->d_in));
        HIPCHK(hipMalloc(&e->d_in, in_bytes));
        e->max_block = max_block;
    }
    if (!e->d_out || oc > e->out_cap) {
        if (e->d_out) HIPCHK(hipFree(e->d_out));
        HIPCHK(hipMalloc(&e->d_out, oc * e->ch * sizeof(float)));
        e->out_cap = oc;
    }
    return 0;
}

int create(void** h, Kind kind, int device, int ch, bool rotate, bool has_filter, int max_block) {
    if (!h) return QDSP_HIP_EINVAL;
    *h = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return QDSP_HIP_ENODEV;
    if (device < 0 || device >= ndev) return QDSP_HIP_ENODEV;
    HIPCHK(hipSetDevice(device));
    Engine* e = new (std::nothrow) Engine();
    if (!e) return QDSP_HIP_ENOMEM;
    e->kind = kind;
    e->device = device;
    e->ch = ch;
    e->rotate = rotate;
    e->has_filter = has_filter;
    e->R = qk::knob(qk::K_R, 0);
    e->NT = qk::knob(qk::K_NT, 0);
    hipError_t err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipEventCreate(&e->ev0);
    if (err == hipSuccess) err = hipEventCreate(&e->ev1);
    if (err != hipSuccess) {
        // nothing created so far may outlive the failed handle
        if (e->ev1) (void)hipEventDestroy(e->ev1);
        if (e->ev0) (void)hipEventDestroy(e->ev0);
        if (e->stream) (void)hipStreamDestroy(e->stream);
        delete e;
        return -(int)err;
    }
    (void)max_block;      // (the staging buffers come with the first host-pointer call: ensure_io)
    *h = e;
    return 0;
}

void destroy(Engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    if (e->d_taps) (void)hipFree(e->d_taps);
    if (e->d_taps_plain) (void)hipFree(e->d_taps_plain);
    if (e->d_taps_lm) (void)hipFree(e->d_taps_lm);
    for (int i = 0; i < 2; i++)
        if (e->d_hist_raw[i]) (void)hipFree(e->d_hist_raw[i]);
    if (e->d_nco_tab) (void)hipFree(e->d_nco_tab);
    if (e->d_fft_H) (void)hipFree(e->d_fft_H);
    if (e->d_fft_TA) (void)hipFree(e->d_fft_TA);
    if (e->d_fft_TB) (void)hipFree(e->d_fft_TB);
    if (e->d_f1k_H) (void)hipFree(e->d_f1k_H);
    if (e->d_f1k_T) (void)hipFree(e->d_f1k_T);
    if (e->d_pfb) (void)hipFree(e->d_pfb);
    if (e->d_taps_mf) (void)hipFree(e->d_taps_mf);
    if (e->d_taps_rm) (void)hipFree(e->d_taps_rm);
    for (int i = 0; i < 2; i++)
        if (e->d_hist[i]) (void)hipFree(e->d_hist[i]);
    if (e->d_in) (void)hipFree(e->d_in);
    if (e->d_out) (void)hipFree(e->d_out);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->ev_up) (void)hipEventDestroy(e->ev_up);
    if (e->ev_kernel) (void)hipEventDestroy(e->ev_kernel);
    if (e->up_stream) (void)hipStreamDestroy(e->up_stream);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    e->magic = 0;
    delete e;
}

// ---- launches --------------------------------------------------------------------------

int nco_tables(Engine* e, long long S, int NT, int na, const double2** tab) {
    if (e->d_nco_tab && e->nco_key_dphase == e->dphase && e->nco_key_S == S && e->nco_key_NT == NT && e->nco_key_na >= na) {
        *tab = e->d_nco_tab;
        return 0;
    }
    if (na < 64) na = 64;
    std::vector<double2> h((size_t)256 + na + NT);
    for (int b = 0; b < 256; b++) unit_of_fx_c(e->dphase, (long double)b * (long double)S, &h[b].x, &h[b].y);
    for (int a2 = 0; a2 < na; a2++) unit_of_fx_c(e->dphase, 256.0L * (long double)a2 * (long double)S, &h[256 + a2].x, &h[256 + a2].y);
    for (int t = 0; t < NT; t++) unit_of_fx_c(e->dphase, (long double)t, &h[256 + na + t].x, &h[256 + na + t].y);
    HIPCHK(hipDeviceSynchronize());       // (rare: nothing in flight may still read the old tables)
    if (e->d_nco_tab) HIPCHK(hipFree(e->d_nco_tab));
    e->d_nco_tab = nullptr;
    HIPCHK(hipMalloc(&e->d_nco_tab, h.size() * sizeof(double2)));
    HIPCHK(hipMemcpy(e->d_nco_tab, h.data(), h.size() * sizeof(double2), hipMemcpyHostToDevice));
    e->nco_key_dphase = e->dphase;
    e->nco_key_S = S;
    e->nco_key_NT = NT;
    e->nco_key_na = na;
    *tab = e->d_nco_tab;
    return 0;
}

// NCO constants of stage_tile (kernels.hip.h) for a kernel staging with NT lanes; with the tile geometry (S samples
// between tiles, `first` = stream position staged by lane 0 of tile 0, ntiles) also the tile_phasor tables
template <class ARGS> int fill_stage_rot(Engine* e, ARGS& a, int NT, long long S, long long first, long long ntiles) {
    fill_stage_rot(a, NT);
    a.nco_tab = nullptr;
    if (!e->rotate) return 0;
    const int na = (int)((ntiles + 255) / 256) + 1;
    if (na > 65536) return 0;
    int rc = nco_tables(e, S, NT, na, &a.nco_tab);
    if (rc) return rc;
    a.nco_na = e->nco_key_na;
    const unsigned long long ph = a.phase0 + (unsigned long long)first * a.dphase;
    unit_of_fx(ph, 1.0L, &a.nco_e0.x, &a.nco_e0.y);
    return 0;
}

// what every direct-form kernel's arguments start from: the call's buffers, the two history buffers and the NCO state
template <class ARGS> void fill_call(ARGS& a, const Engine* e, const void* d_in, int64_t count, int64_t nout, void* d_out) {
    memset(&a, 0, sizeof(a));
    a.in = d_in;
    a.out = d_out;
    a.hist = e->d_hist[e->cur];
    a.hist_next = e->d_hist[e->cur ^ 1];
    a.count = count;
    a.nout = nout;
    a.phase0 = e->phase;
    a.dphase = e->dphase;
    a.gm1 = e->volk_gain ? e->gm1 : 0.0f;
}

// host copy of qk::slot (must match kernels.hip.h)
inline int qk_slot_host(int R, int v) { return (R % 2 == 0) ? v + v / R : v; }

template <int CH, int R, int NT, bool ROT, int MT>
int launch_core_t(Engine* e, qk::CoreArgs& a, hipStream_t s) {
    constexpr int TILE = NT * R;
    const int V = TILE + a.Q;
    int sb = qk_slot_host(R, V - 1) + 1;
    // Spread the M branch bases over the banks for the de-interleaving LDS writes.
    if (a.M > 1) {
        const int want = (a.M >= 16) ? 1 : 16 / a.M;
        while ((sb % 16) != (want % 16)) sb++;
    }
    a.sb = sb;
    const size_t lds = (size_t)a.M * sb * CH * sizeof(float);
    if (lds > (size_t)kMaxDynLds) return QDSP_HIP_EINVAL;
    a.nblocks = (int)((a.nout + TILE - 1) / TILE);
    a.vec = ((uintptr_t)a.in & 15) == 0;
    if (ROT) {
        { int rcn = fill_stage_rot(e, a, NT, (long long)TILE * a.M, -(long long)a.H, a.nblocks); if (rcn) return rcn; }
        unit_of_fx_c(a.dphase, 1.0L, &a.rot_one.x, &a.rot_one.y);
        unit_of_fx_c(a.dphase, (long double)(2 * NT), &a.rot_2nt.x, &a.rot_2nt.y);
    }
    hipLaunchKernelGGL((qk::fir_core_kernel<CH, R, NT, ROT, MT>), dim3(a.nblocks + 1), dim3(NT), lds, s, a);
    HIPCHK(hipGetLastError());
    e->last.name = "fir_core_kernel";
    e->last.grid = a.nblocks + 1;
    e->last.block = NT;
    e->last.lds = (int)lds;
    return 0;
}

template <int CH, bool ROT> int launch_core(Engine* e, qk::CoreArgs& a, hipStream_t s) {
    // Geometry: (R outputs per lane, NT lanes).  FIR (M == 1) is VALU-bound: a long
    // register window amortises the LDS read per tap.  Decimators stage M*TILE inputs per
    // tile, so TILE shrinks with M to stay inside the LDS budget.
    int R = e->R, NT = e->NT;
    if (R == 0 || NT == 0) {
        if (a.M == 1) { R = 8; NT = 256; }
        else if (a.M <= 2) { R = 8; NT = 128; }
        else if (a.M <= 8) { R = 4; NT = 128; }
        else { R = 4; NT = 64; }
    }
    const int mt = (a.M == 1 || a.M == 2 || a.M == 4 || a.M == 8) ? a.M : 0;
#define QK_CASE(r, nt, m) \
    if (R == r && NT == nt && mt == m) return launch_core_t<CH, r, nt, ROT, m>(e, a, s);
#define QK_GEOM(r, nt) QK_CASE(r, nt, 0) QK_CASE(r, nt, 2) QK_CASE(r, nt, 4) QK_CASE(r, nt, 8)
    QK_CASE(8, 256, 1)
    QK_CASE(16, 256, 1)
    QK_CASE(4, 256, 1)
    QK_GEOM(8, 256)
    QK_GEOM(4, 256)
    QK_GEOM(8, 128)
    QK_GEOM(4, 128)
    QK_GEOM(4, 64)
#undef QK_GEOM
#undef QK_CASE
    return QDSP_HIP_EINVAL;
}

template <int CH, bool ROT> int launch_win(Engine* e, const void* d_in, int64_t count, int64_t nout, void* d_out, hipStream_t s) {
    qk::WinArgs a;
    fill_call(a, e, d_in, count, nout, d_out);
    a.taps = e->d_taps_lm;
    a.P = e->H;                  // window start / history length: P for the resampler, ntaps-1 for FIR<T>
    a.ntaps = e->P;
    constexpr int NT = 256;
    auto go = [&](auto Mc, auto Rc) -> int {
        constexpr int M = decltype(Mc)::value, R = decltype(Rc)::value, MR = M * R;
        constexpr int TILE = NT * R;
        a.nchunks = (M * (R - 1) + e->P + MR - 1) / MR;
        const int U = TILE * M + a.nchunks * MR;
        const size_t lds = (size_t)(U + U / MR + 1) * CH * sizeof(float);
        if (lds > (size_t)kMaxDynLds) return QDSP_HIP_EINVAL;
        a.nblocks = (int)((nout + TILE - 1) / TILE);
        { int rcn = fill_stage_rot(e, a, NT, (long long)TILE * M, -(long long)a.P, a.nblocks); if (rcn) return rcn; }
        hipLaunchKernelGGL((qk::decim_win_kernel<CH, M, R, NT, ROT>), dim3(a.nblocks + 1), dim3(NT), lds, s, a);
        HIPCHK(hipGetLastError());
        e->last.name = "decim_win_kernel";
        e->last.grid = a.nblocks + 1;
        e->last.block = NT;
        e->last.lds = (int)lds;
        return 0;
    };
    using std::integral_constant;
    const int R = win_R(e->M, e->P);
#define QK_WIN(m, r) if (e->M == m && R == r) return go(integral_constant<int, m>{}, integral_constant<int, r>{});
    QK_WIN(1, 4) QK_WIN(1, 8)
    QK_WIN(2, 2) QK_WIN(2, 4) QK_WIN(2, 8)
    QK_WIN(3, 2) QK_WIN(3, 4)
    QK_WIN(4, 1) QK_WIN(4, 2) QK_WIN(4, 4)
    QK_WIN(5, 1) QK_WIN(5, 2) QK_WIN(5, 4)
    QK_WIN(6, 1) QK_WIN(6, 2)
    QK_WIN(7, 1)
    QK_WIN(8, 1) QK_WIN(8, 2)
    QK_WIN(10, 1) QK_WIN(12, 1) QK_WIN(16, 1)
#undef QK_WIN
    return QDSP_HIP_EINVAL;
}

template <int CH, bool ROT> int launch_lm(Engine* e, const void* d_in, int64_t count, int64_t nout, void* d_out, hipStream_t s) {
    qk::LmArgs a;
    fill_call(a, e, d_in, count, nout, d_out);
    a.taps = e->d_taps_lm;
    a.taps_t = e->d_taps_lm + e->taps_lm_t_off;
    a.M = e->M;
    a.P = e->P;
    a.Q = (e->P + e->M - 1) / e->M;
    for (int c = 0; c < e->L; c++) a.e[c] = (c * e->M) / e->L;
    constexpr int NT = 128;
    // R*L accumulators per lane: 10 .. 30 complex values
    auto go = [&](auto Rc, auto Lc) -> int {
        constexpr int R = decltype(Rc)::value, LL = decltype(Lc)::value;
        constexpr int TJ = NT * R;
        const int V = TJ + a.Q + 1;
        int sb = V;
        if ((sb & 15) == 0) sb += 1;                    // keep the M branch bases off one bank for the de-interleaving writes
        a.sb = sb;
        size_t lds = (size_t)a.M * sb * CH * sizeof(float);
        const size_t lds_out = (size_t)TJ * LL * CH * sizeof(float);      // the tile's outputs pass through LDS too
        if (lds < lds_out) lds = lds_out;
        if (lds > (size_t)kMaxDynLds) return QDSP_HIP_EINVAL;
        a.nblocks = (int)((nout + (long long)TJ * LL - 1) / ((long long)TJ * LL));
        { int rcn = fill_stage_rot(e, a, NT, (long long)TJ * a.M, -(long long)a.P, a.nblocks); if (rcn) return rcn; }
        hipLaunchKernelGGL((qk::resamp_lm_kernel<CH, R, NT, ROT, LL>), dim3(a.nblocks + 1), dim3(NT), lds, s, a);
        HIPCHK(hipGetLastError());
        e->last.name = "resamp_lm_kernel";
        e->last.grid = a.nblocks + 1;
        e->last.block = NT;
        e->last.lds = (int)lds;
        return 0;
    };
    using std::integral_constant;
    switch (e->L) {
        case 2: return go(integral_constant<int, 5>{}, integral_constant<int, 2>{});
        case 3: return go(integral_constant<int, 5>{}, integral_constant<int, 3>{});
        case 4: return go(integral_constant<int, 3>{}, integral_constant<int, 4>{});
        case 5: return go(integral_constant<int, 3>{}, integral_constant<int, 5>{});
        case 10: return go(integral_constant<int, 3>{}, integral_constant<int, 10>{});
        default: return QDSP_HIP_EINVAL;
    }
}

// Tile geometry of resamp_any_kernel into `a` (a.L / a.M / a.P / a.nout set by the caller); returns the dynamic LDS
// bytes, 0 if the taps of one phase do not fit.
size_t fill_any_geometry(qk::AnyArgs& a, int ch, bool* lt, bool* pad, int nchan) {
    constexpr int NT = 256;
    const AnyPlan pl = any_plan(a.L, a.M, a.P, ch, a.nout * nchan);   // (a batch launch runs nchan x nblocks tiles)
    if (pl.tile == 0) return 0;  // taps per phase beyond LDS
    *lt = pl.tap_bytes != 0;
    *pad = pl.pad;
    const long long tile = pl.tile;
    a.Pp = pl.Pp;
    a.tap_bytes = pl.tap_bytes;
    a.pad_inv = pl.pad ? (unsigned)((1ULL << 32) / (unsigned)a.M) + 1u : 0u;
    a.tile = (int)tile;
    a.ks_lanes = pl.ks_lanes;
    a.ks_shift = pl.ks_shift;
    a.ks_chunk = pl.ks_chunk;
    a.ks_red = (int)pl.span;
    a.nblocks = (int)((a.nout + tile - 1) / tile);
    a.step_d = (int)(((long long)NT * a.M) / a.L);
    a.step_p = (int)(((long long)NT * a.M) % a.L);
    return (size_t)a.tap_bytes + (size_t)(pl.span + (pl.ks_lanes ? NT : 0)) * ch * sizeof(float);
}

template <int CH, bool ROT> int launch_any(Engine* e, qk::AnyArgs& a, hipStream_t s) {
    constexpr int NT = 256;
    bool lt = false, pad = false;
    const size_t lds = fill_any_geometry(a, CH, &lt, &pad);
    if (lds == 0) return QDSP_HIP_EINVAL;  // taps per phase beyond LDS
    // persistent workgroups, 8 per CU (measured on the M = 50, 401-tap VFO, 32 KB of LDS each: 5 per CU -- what is
    // resident at once -- 0.41 ms per 2^27 samples, 8 .. 64 per CU 0.345-0.358)
    int nwg = 256 * 8;
    if (nwg > a.nblocks) nwg = a.nblocks;
    if (nwg < 1) nwg = 1;
    a.nwg = nwg;
    // full persistent grids only: a contiguous tile range per XCD (kernels.hip.h)
    a.xcd_tiles = (nwg >= 2048 && (nwg & 7) == 0) ? (a.nblocks + 7) / 8 : 0;
    fill_stage_rot(a, NT);
    if (pad) {
        if (lt) hipLaunchKernelGGL((qk::resamp_any_kernel<CH, NT, ROT, true, true>), dim3(nwg + 1), dim3(NT), lds, s, a);
        else hipLaunchKernelGGL((qk::resamp_any_kernel<CH, NT, ROT, false, true>), dim3(nwg + 1), dim3(NT), lds, s, a);
    } else {
        if (lt) hipLaunchKernelGGL((qk::resamp_any_kernel<CH, NT, ROT, true, false>), dim3(nwg + 1), dim3(NT), lds, s, a);
        else hipLaunchKernelGGL((qk::resamp_any_kernel<CH, NT, ROT, false, false>), dim3(nwg + 1), dim3(NT), lds, s, a);
    }
    HIPCHK(hipGetLastError());
    e->last.name = "resamp_any_kernel";
    e->last.grid = nwg + 1;
    e->last.block = NT;
    e->last.lds = (int)lds;
    return 0;
}

// ---- overlap-save FFT FIR -------------------------------------------------------------------
// Spectrum of a short sequence zero-padded to F = 2^m points, FP64 radix-2 (twiddles from sincosl, rounded once): what the
// overlap-save kernels multiply by.  The direct long-double DFT this replaces cost F x taps x87 operations -- 4-8 ms per
// handle at 4096 points and 256 taps, on creation and on every retune of a fused VFO; this is ~0.1 ms, and its error
// (1e-16 x log2 F) stays nine orders below the FP32 rounding of the result.
void host_spectrum(const std::vector<long double>& gr, const std::vector<long double>& gi, int F, std::vector<double>& re, std::vector<double>& im) {
    re.assign((size_t)F, 0.0);
    im.assign((size_t)F, 0.0);
    int bits = 0;
    while ((1 << bits) < F) bits++;
    for (size_t j = 0; j < gr.size() && j < (size_t)F; j++) {
        unsigned r = 0;
        for (int b = 0; b < bits; b++) r |= ((j >> b) & 1u) << (bits - 1 - b);
        re[r] = (double)gr[j];
        im[r] = (double)gi[j];
    }
    const long double two_pi = 6.283185307179586476925286766559005768L;
    std::vector<double> wr((size_t)F / 2), wi((size_t)F / 2);
    for (int i = 0; i < F / 2; i++) {
        wr[i] = (double)cosl(two_pi * (long double)i / F);
        wi[i] = (double)(-sinl(two_pi * (long double)i / F));
    }
    for (int len = 2; len <= F; len <<= 1) {
        const int half = len >> 1, step = F / len;
        for (int base = 0; base < F; base += len)
            for (int k = 0; k < half; k++) {
                const double cr = wr[(size_t)k * step], ci = wi[(size_t)k * step];
                const double xr = re[base + k + half], xi = im[base + k + half];
                const double tr = xr * cr - xi * ci, ti = xr * ci + xi * cr;
                re[base + k + half] = re[base + k] - tr;
                im[base + k + half] = im[base + k] - ti;
                re[base + k] += tr;
                im[base + k] += ti;
            }
    }
}

// g[j] = taps[N-1-j] (x exp(j (N-1-j) dphase) for the fused VFO: the mixer folded into the taps, fft_fir.hip.h) into the first N entries
void reversed_taps(const Engine* e, std::vector<long double>& gr, std::vector<long double>& gi) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    const int N = e->ntaps;
    for (int j = 0; j < N; j++) {
        const long double h = (long double)e->taps_host[N - 1 - j];
        long double c = 1.0L, sn = 0.0L;
        if (e->rotate) {
            const long double tt = ldexpl((long double)e->dphase, -64) * (long double)(N - 1 - j);
            c = cosl(two_pi * (tt - floorl(tt)));
            sn = sinl(two_pi * (tt - floorl(tt)));
        }
        gr[j] = h * c;
        gi[j] = h * sn;
    }
}

int fft_prepare(Engine* e) {
    // fused VFO: the spectrum is that of taps[k] * exp(j k dphase) (fft_fir.hip.h), so it follows the NCO
    const unsigned long long key_dphase = e->rotate ? e->dphase : 0;
    if (e->fft_ntaps == e->ntaps && e->fft_tw_ready && e->fft_dphase == key_dphase) return 0;
    constexpr int F = qk::kFftN;
    const long double two_pi = 6.283185307179586476925286766559005768L;
    std::vector<long double> cs, sn;
    if (!e->fft_tw_ready) {   // (the twiddle tables below: once per handle -- the flag, not a pointer: it is set only after every
                              // allocation and upload of the first-time block has succeeded)
        cs.resize(F);
        sn.resize(F);
        for (int i = 0; i < F; i++) {
            cs[i] = cosl(two_pi * (long double)i / F);
            sn[i] = sinl(two_pi * (long double)i / F);
        }
    }
    const int N = e->ntaps;
    // g[j] = taps[N-1-j]:  c[p] = sum_j g[j] s[p-j] = sum_k taps[k] s[p-(N-1)+k];
    // Hf[k] = sum_j g[j] exp(-j 2pi jk/F) / F
    // Hf and TA are uploaded twice, behind each other in one allocation: lane-major [256][16] (QDSP_HIP_FFT_TBL=0) and entry-major
    // [16][256] -- the same values; the lanes of a wave read 512 contiguous bytes of the second per instruction (FftArgs::HfT / TAT)
    std::vector<float2> Hp(2 * F), TA(2 * 256 * 16), TB(16 * 16);
    std::vector<long double> gr(N), gi(N);
    reversed_taps(e, gr, gi);
    std::vector<double> sre, sim;
    host_spectrum(gr, gi, F, sre, sim);
    for (int k = 0; k < F; k++) {
        const int k0 = k & 15, k1 = (k >> 4) & 15, k2 = k >> 8;
        Hp[(k0 * 16 + k1) * 16 + k2] = Hp[F + k2 * 256 + (k0 * 16 + k1)] = make_float2((float)(sre[k] / F), (float)(sim[k] / F));
    }
    if (!e->fft_tw_ready) {
        for (int t = 0; t < 256; t++)
            for (int k = 0; k < 16; k++) TA[t * 16 + k] = TA[F + k * 256 + t] = make_float2((float)cs[(t * k) % F], (float)(-sn[(t * k) % F]));
        for (int lo = 0; lo < 16; lo++)
            for (int k = 0; k < 16; k++) TB[lo * 16 + k] = make_float2((float)cs[(16 * lo * k) % F], (float)(-sn[(16 * lo * k) % F]));
        if (!e->d_fft_H) HIPCHK(hipMalloc(&e->d_fft_H, sizeof(float2) * 2 * F));
        if (!e->d_fft_TA) HIPCHK(hipMalloc(&e->d_fft_TA, sizeof(float2) * 2 * 256 * 16));
        if (!e->d_fft_TB) HIPCHK(hipMalloc(&e->d_fft_TB, sizeof(float2) * 16 * 16));
        HIPCHK(hipMemcpy(e->d_fft_TA, TA.data(), sizeof(float2) * TA.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(e->d_fft_TB, TB.data(), sizeof(float2) * TB.size(), hipMemcpyHostToDevice));
        e->fft_tw_ready = true;
    }
    HIPCHK(hipDeviceSynchronize());   // (retune / new taps: nothing in flight may still read the old spectrum)
    HIPCHK(hipMemcpy(e->d_fft_H, Hp.data(), sizeof(float2) * Hp.size(), hipMemcpyHostToDevice));
    e->fft_ntaps = N;
    e->fft_dphase = key_dphase;
    return 0;
}

// ---- overlap-save on 1024-point segments, one wave each (fft1k_fir.hip; which calls: fft1k_eligible, select.cpp) ----
int fft1k_prepare(Engine* e) {
    const unsigned long long key_dphase = e->rotate ? e->dphase : 0;
    if (e->f1k_ntaps == e->ntaps && e->f1k_tw_ready && e->f1k_dphase == key_dphase) return 0;
    constexpr int F = qk::kFft1kN;
    const long double two_pi = 6.283185307179586476925286766559005768L;
    std::vector<long double> cs, sn;
    if (!e->f1k_tw_ready) {   // (the twiddle tables below: once per handle; see fft_prepare for the flag)
        cs.resize(F);
        sn.resize(F);
        for (int i = 0; i < F; i++) {
            cs[i] = cosl(two_pi * (long double)i / F);
            sn[i] = sinl(two_pi * (long double)i / F);
        }
    }
    const int N = e->ntaps;
    // g[j] = taps[N-1-j] (x exp(j (N-1-j) dphase) for the fused VFO), Hf[k] = sum_j g[j] exp(-j 2pi jk/F) / F: as fft_prepare
    std::vector<long double> gr(N), gi(N);
    reversed_taps(e, gr, gi);
    std::vector<float2> Hp(F), T(64 * 16 + 4 * 16);
    std::vector<double> sre, sim;
    host_spectrum(gr, gi, F, sre, sim);
    for (int k = 0; k < F; k++) {
        const double re = sre[k], im = sim[k];
        // bin k = ka + 16 (4 g + s) + 256 kb0 sits with lane (ka << 2) | g, entry 4 s + kb0; tables are entry-major
        // ([entry][lane]: a wave's load of one entry is 512 contiguous bytes)
        const int ka = k & 15, kb1 = (k >> 4) & 15, kb0 = k >> 8;
        Hp[(4 * (kb1 & 3) + kb0) * 64 + ((ka << 2) | (kb1 >> 2))] = make_float2((float)(re / F), (float)(im / F));
    }
    if (!e->f1k_tw_ready) {
        for (int l = 0; l < 64; l++)
            for (int k = 0; k < 16; k++) T[k * 64 + l] = make_float2((float)cs[(l * k) % F], (float)(-sn[(l * k) % F]));
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 16; k++) T[1024 + k * 4 + j] = make_float2((float)cs[(16 * j * k) % F], (float)(-sn[(16 * j * k) % F]));
        if (!e->d_f1k_H) HIPCHK(hipMalloc(&e->d_f1k_H, sizeof(float2) * F));
        if (!e->d_f1k_T) HIPCHK(hipMalloc(&e->d_f1k_T, sizeof(float2) * T.size()));
        HIPCHK(hipMemcpy(e->d_f1k_T, T.data(), sizeof(float2) * T.size(), hipMemcpyHostToDevice));
        e->f1k_tw_ready = true;
    }
    HIPCHK(hipDeviceSynchronize());   // (retune / new taps: nothing in flight may still read the old spectrum)
    HIPCHK(hipMemcpy(e->d_f1k_H, Hp.data(), sizeof(float2) * F, hipMemcpyHostToDevice));
    e->f1k_ntaps = N;
    e->f1k_dphase = key_dphase;
    return 0;
}

int launch_xlate_inc(Engine* e, const void* d_in, int64_t count, void* d_out, unsigned long long phase0, unsigned long long dphase, float gm1,
                     hipStream_t s) {
    constexpr int NT = 256;
    if (count <= 0) return 0;
    qk::XlateArgs a;
    a.in = static_cast<const float2*>(d_in);
    a.out = static_cast<float2*>(d_out);
    a.count = count;
    a.phase0 = phase0;
    a.dphase = dphase;
    const long long npairs = (count + 1) / 2;
    long long grid = (npairs + NT - 1) / NT;
    // one pair per lane up to 2^27 samples: measured 0.345 ms per 2^27 samples against 0.46 ms with 16 blocks per CU
    // looping 64 times (the per-lane FP64 sincos is cheaper than the lost memory-level parallelism)
    { const long long cap = 256LL * 1024; if (grid > cap) grid = cap; }
    unit_of_fx_c(dphase, 1.0L, &a.rot_one.x, &a.rot_one.y);
    unit_of_fx_c(dphase, (long double)(2 * grid * NT), &a.rot_stride.x, &a.rot_stride.y);
    a.vec = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0;   // d_in == nullptr (SineSource) counts as aligned
    a.gm1 = gm1;
    hipLaunchKernelGGL((qk::xlate_kernel<NT>), dim3((unsigned)grid), dim3(NT), 0, s, a);
    HIPCHK(hipGetLastError());
    e->last.name = "xlate_kernel";
    e->last.grid = (int)grid;
    e->last.block = NT;
    e->last.lds = 0;
    return 0;
}

int launch_xlate(Engine* e, const void* d_in, int64_t count, void* d_out, hipStream_t s) {
    return launch_xlate_inc(e, d_in, count, d_out, e->phase, e->dphase, e->volk_gain ? e->gm1 : 0.0f, s);
}

// The overlap-save kernels of the fused VFO filter RAW samples while the handle keeps its history rotated (the direct
// kernels and *_set_history_dev use that form; a call may switch form with its size): the H samples are de-rotated once
// per call into a side buffer -- exp(-j phi(g)), g = -H .. -1 -- unless the previous overlap-save call left them there.
int raw_history(Engine* e, hipStream_t s, const float2** hist, float2** hist_raw_next) {
    *hist_raw_next = nullptr;
    if (!(e->rotate && e->H > 0)) return 0;
    if (!e->d_hist_raw[0] || e->hist_raw_cap < e->H) {
        for (int i = 0; i < 2; i++) {
            if (e->d_hist_raw[i]) HIPCHK(hipFree(e->d_hist_raw[i]));
            e->d_hist_raw[i] = nullptr;
            HIPCHK(hipMalloc(&e->d_hist_raw[i], (size_t)e->H * sizeof(float2)));
        }
        e->hist_raw_cap = e->H;
        e->raw_valid = false;
    }
    if (!e->raw_valid) {
        const unsigned long long ph_first = e->phase - (unsigned long long)e->H * e->dphase;   // phase of history sample 0
        const Launch keep = e->last;
        const int rc = launch_xlate_inc(e, e->d_hist[e->cur], e->H, e->d_hist_raw[e->cur], 0ULL - ph_first, 0ULL - e->dphase, 0.0f, s);
        e->last = keep;
        if (rc) return rc;
    }
    *hist = reinterpret_cast<const float2*>(e->d_hist_raw[e->cur]);
    *hist_raw_next = reinterpret_cast<float2*>(e->d_hist_raw[e->cur ^ 1]);
    return 0;
}

int launch_fft1k(Engine* e, const void* d_in, int64_t count, int64_t nout, void* d_out, hipStream_t s) {
    int rc = fft1k_prepare(e);
    if (rc) return rc;
    qk::FftArgs a;
    memset(&a, 0, sizeof(a));
    a.in = static_cast<const float2*>(d_in);
    a.out = static_cast<float2*>(d_out);
    a.hist = reinterpret_cast<const float2*>(e->d_hist[e->cur]);
    a.hist_keep = a.hist;
    a.hist_next = reinterpret_cast<float2*>(e->d_hist[e->cur ^ 1]);
    rc = raw_history(e, s, &a.hist, &a.hist_raw_next);
    if (rc) return rc;
    a.Hf = e->d_f1k_H;
    a.TA = e->d_f1k_T;
    a.TB = e->d_f1k_T + 1024;
    a.count = count;
    a.nout = nout;
    a.H = e->H;
    a.dec = 1;
    a.rot = e->rotate ? 1 : 0;
    a.decm = 1;
    a.ov = e->ntaps - 1;
    if (e->kind != KIND_FIR) {
        // resampler / VFO: y[n'] sits at stream position n' M - 1: segments start one sample early
        a.decm = e->M;
        a.decm_inv = (e->M >= 2 && (unsigned long long)(e->M + qk::kFft1kN) * (unsigned long long)e->M < (1ULL << 32)) ? (unsigned)((1ULL << 32) / (unsigned)e->M) + 1u : 0u;
        a.strided = 1;
        a.m_shift = -1;
        for (int sh = 0; sh <= 6; sh++)
            if (e->M == (1 << sh)) a.m_shift = sh;
        a.seg_shift = a.ov + 1;
        a.L = qk::kFft1kN - a.ov;
        a.nblocks = (int)((count + 1 + a.L - 1) / a.L);
    } else {
        a.seg_shift = a.ov;
        a.L = qk::kFft1kN - a.ov;
        a.nblocks = (int)((count + a.L - 1) / a.L);
    }
    if (e->ch == 1) {   // real data: one wave = a PAIR of real segments (re / im of one transform)
        a.real2 = 1;
        a.nblocks = (a.nblocks + 1) / 2;
    }
    a.nwg = a.nblocks;
    if (a.rot) {
        a.phase_in0 = e->phase;
        a.phase0 = e->phase - (unsigned long long)(e->ntaps - 1) * e->dphase;
        a.dphase = e->dphase;
        a.gm1 = e->volk_gain ? e->gm1 : 0.0f;
        if (!e->wtab1k_ok || e->wtab1k_dphase != e->dphase) {
            for (int i = 0; i < 16; i++) {
                double c, sn;
                unit_of_fx_c(e->dphase, (long double)(64 * i), &c, &sn);
                e->wtab1k[i] = make_float2((float)c, (float)sn);
            }
            e->wtab1k_dphase = e->dphase;
            e->wtab1k_ok = true;
        }
        memcpy(a.wtab, e->wtab1k, sizeof(a.wtab));
    }
    rc = qk::launch_fir_fft1k(a, s);
    if (rc) return rc;
    e->raw_valid = e->rotate && e->H > 0;   // (the caller flips cur: the raw hand-over then sits at d_hist_raw[cur])
    e->last.name = "fir_fft1k_kernel";
    e->last.grid = a.nblocks + (a.H + 63) / 64;
    e->last.block = 64;
    e->last.lds = (int)(16 * qk::kFft1kPitch * sizeof(float2));
    return 0;
}

// ---- polyphase overlap-save decimate-by-8 / -4 (pfb_dec.hip; which calls: pfb_eligible, select.cpp) ----
int pfb_prepare(Engine* e) {
    const unsigned long long key_dphase = e->rotate ? e->dphase : 0;
    if (e->pfb_ntaps == e->ntaps && e->pfb_M == e->M && e->d_pfb && e->pfb_dphase == key_dphase) return 0;
    constexpr int F = qk::kPfbF, D = qk::kPfbD, R = qk::kPfbRow;
    const long double two_pi = 6.283185307179586476925286766559005768L;
    const int N = e->ntaps, PH = pfb_phases(e->M), Q = pfb_Q(e->M, e->ntaps);
    // g[j] = taps[N-1-j] (x exp(j (N-1-j) dphase) for the fused VFO: the mixer folded into the taps, fft_fir.hip.h)
    std::vector<long double> gr((size_t)Q * D, 0.0L), gi((size_t)Q * D, 0.0L);
    reversed_taps(e, gr, gi);
    std::vector<long double> cs(F), ss(F);
    for (int i = 0; i < F; i++) { cs[i] = cosl(two_pi * i / F); ss[i] = sinl(two_pi * i / F); }
    std::vector<float2> tab((size_t)qk::kPfbTableElems + (size_t)(PH - 1) * qk::kPfbG1Elems, make_float2(0.0f, 0.0f));
    // G: row (k0*64 + kq*8 + c), element kg: spectrum of column c's filter gamma_c[q] = g[8q + 7 - c] at bin k0 + 8 kq + 64 kg, / 512
    for (int c = 0; c < D; c++) {
        std::vector<long double> cr((size_t)Q), ci((size_t)Q);
        for (int q = 0; q < Q; q++) {
            cr[q] = gr[D * q + (D - 1 - c)];
            ci[q] = gi[D * q + (D - 1 - c)];
        }
        std::vector<double> sre, sim;
        host_spectrum(cr, ci, F, sre, sim);      // (FP64 radix-2 FFT: see fft_prepare)
        for (int k = 0; k < F; k++) {
            const int k0 = k & 7, kq = (k >> 3) & 7, kg = k >> 6;
            tab[(size_t)((k0 * 64 + kq * 8 + c) * R + kg)] = make_float2((float)(sre[k] / F), (float)(sim[k] / F));
        }
    }
    if (PH == 2) {
        // G1: the odd outputs y4[2n' - 1]: window end 8n' - 5, i.e. the same taps four samples later, g_1 = 0 0 0 0 ++ g; the NCO phase of
        // that output is four samples behind the even one's (x exp(-j 4 dphase), folded in here).  Rows of 8 values, 16-byte chunk i of row
        // (k0, kq, c) stored at chunk i ^ ((kq*8 + c) >> 2 & 3): pfb_dec.hip reads it back the same way
        long double rc = 1.0L, rs = 0.0L;
        if (e->rotate) {
            const long double tt = ldexpl((long double)e->dphase, -64) * 4.0L;
            rc = cosl(two_pi * (tt - floorl(tt)));
            rs = -sinl(two_pi * (tt - floorl(tt)));
        }
        float2* G1 = tab.data() + qk::kPfbTableElems;
        for (int c = 0; c < D; c++) {
            std::vector<long double> cr((size_t)Q, 0.0L), ci((size_t)Q, 0.0L);
            for (int q = 0; q < Q; q++) {
                const int j = D * q + (D - 1 - c) - 4;       // index into g
                if (j < 0 || j >= N) continue;
                cr[q] = gr[j] * rc - gi[j] * rs;
                ci[q] = gr[j] * rs + gi[j] * rc;
            }
            std::vector<double> sre, sim;
            host_spectrum(cr, ci, F, sre, sim);
            for (int k = 0; k < F; k++) {
                const int k0 = k & 7, kq = (k >> 3) & 7, kg = k >> 6;
                const int row = k0 * 64 + kq * 8 + c, swz = ((kq * 8 + c) >> 2) & 3;
                G1[(size_t)row * 8 + 2 * ((kg >> 1) ^ swz) + (kg & 1)] = make_float2((float)(sre[k] / F), (float)(sim[k] / F));
            }
        }
    }
    float2* TW = tab.data() + 512 * R;     // row (k0*8 + kq), element g': W512^(g' (k0 + 8 kq))
    for (int k0 = 0; k0 < 8; k0++)
        for (int kq = 0; kq < 8; kq++)
            for (int g = 0; g < 8; g++) {
                const int idx = (g * (k0 + 8 * kq)) % F;
                TW[(k0 * 8 + kq) * R + g] = make_float2((float)cs[idx], (float)(-ss[idx]));
            }
    float2* TI1 = TW + 64 * R;             // row m, element alpha: exp(+j 2pi m alpha / 512)
    for (int m = 0; m < 64; m++)
        for (int al = 0; al < 8; al++) TI1[m * R + al] = make_float2((float)cs[(m * al) % F], (float)ss[(m * al) % F]);
    float2* TI2 = TI1 + 64 * R;            // row m0, element b0: exp(+j 2pi m0 b0 / 64)
    for (int m0 = 0; m0 < 8; m0++)
        for (int b0 = 0; b0 < 8; b0++) TI2[m0 * R + b0] = make_float2((float)cs[(8 * m0 * b0) % F], (float)ss[(8 * m0 * b0) % F]);
    float2* EL = TI2 + 8 * R;              // exp(j 2pi 8 l dphase): the NCO over a lane's element offset (fused VFO)
    for (int l = 0; l < 64; l++) {
        double c = 1.0, sn = 0.0;
        if (e->rotate) unit_of_fx_c(e->dphase, (long double)(8 * l), &c, &sn);
        EL[l] = make_float2((float)c, (float)sn);
    }
    if (!e->d_pfb) HIPCHK(hipMalloc(&e->d_pfb, ((size_t)qk::kPfbTableElems + qk::kPfbG1Elems) * sizeof(float2)));
    HIPCHK(hipDeviceSynchronize());   // (retune / new taps: nothing in flight may still read the old tables)
    HIPCHK(hipMemcpy(e->d_pfb, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice));
    e->pfb_ntaps = N;
    e->pfb_M = e->M;
    e->pfb_dphase = key_dphase;
    return 0;
}

int launch_pfb(Engine* e, const void* d_in, int64_t count, int64_t nout, void* d_out, hipStream_t s) {
    int rc = pfb_prepare(e);
    if (rc) return rc;
    qk::PfbArgs a;
    memset(&a, 0, sizeof(a));
    a.in = static_cast<const float2*>(d_in);
    a.out = static_cast<float2*>(d_out);
    a.hist = reinterpret_cast<const float2*>(e->d_hist[e->cur]);
    a.hist_keep = a.hist;
    a.hist_next = reinterpret_cast<float2*>(e->d_hist[e->cur ^ 1]);
    rc = raw_history(e, s, &a.hist, &a.hist_raw_next);
    if (rc) return rc;
    a.tables = e->d_pfb;
    a.count = count;
    a.nout = nout;
    a.H = e->H;
    a.PH = pfb_phases(e->M);
    a.Q = pfb_Q(e->M, e->ntaps);
    a.Lo = qk::kPfbF + 1 - a.Q;
    // column outputs n' the call needs: output n = PH n' - phi, n < nout  ->  n' <= ceil((nout - 1) / PH)
    const int64_t ncol = a.PH == 1 ? nout : (nout + a.PH - 2) / a.PH + 1;
    a.nseg = (int)((ncol + a.Lo - 1) / a.Lo);
    // persistent workgroups of 4 waves, one segment per wave at a time; 2 workgroups resident per CU (72 KB of LDS,
    // ~220 VGPRs), QDSP_HIP_PFB_WG_PER_CU queued per CU
    // (decimate by 4: 8 waves per workgroup -- they share the two spectrum tables, 159 KB of LDS -- one workgroup per CU)
    a.real = e->ch == 1 ? 1 : 0;
    const int wpw = 4 * a.PH;
    int nwg = 256 * qk::knob(qk::K_PFB_WG_PER_CU, 2) / a.PH;
    if (nwg > 1024) nwg = 1024;
    const int nunits = a.real ? (a.nseg + 1) / 2 : a.nseg;      // (real data: a wave takes a PAIR of segments at a time)
    const int need = (nunits + wpw - 1) / wpw;
    if (nwg > need) nwg = need;
    if (nwg < 1) nwg = 1;
    a.nwg = nwg;
    a.rot = e->rotate ? 1 : 0;
    if (a.rot) {
        a.phase_in0 = e->phase;
        a.phase0 = e->phase - (unsigned long long)(e->ntaps - 1) * e->dphase;
        a.dphase = e->dphase;
        a.gm1 = e->volk_gain ? e->gm1 : 0.0f;
        unit_of_fx_c(e->dphase, 8.0L * (long double)a.Lo * (long double)(wpw * nwg), &a.rot_step.x, &a.rot_step.y);
        if (wpw * nwg > 4096) return QDSP_HIP_EINVAL;     // (seg_pow covers wave indices below 2^12)
        unit_of_fx(a.phase0 - (unsigned long long)(8 * (a.Q - 1) + 1) * a.dphase, 1.0L, &a.pb_base.x, &a.pb_base.y);
        for (int k = 0; k < 12; k++) unit_of_fx_c(e->dphase, 8.0L * (long double)a.Lo * (long double)(1 << k), &a.seg_pow[k].x, &a.seg_pow[k].y);
        for (int b1 = 0; b1 < 8; b1++) {
            double c, sn;
            unit_of_fx_c(e->dphase, (long double)(512 * b1), &c, &sn);
            a.wtab[b1] = make_float2((float)c, (float)sn);
        }
    }
    rc = qk::launch_pfb_dec(a, s);
    if (rc) return rc;
    e->raw_valid = e->rotate && e->H > 0;   // (the caller flips cur: the raw hand-over then sits at d_hist_raw[cur])
    e->last.name = a.real ? (a.PH == 2 ? "pfb_dec4_real_kernel" : "pfb_dec8_real_kernel") : a.PH == 2 ? "pfb_dec4_kernel" : "pfb_dec8_kernel";
    e->last.grid = nwg + 1;
    e->last.block = qk::kPfbNT * a.PH;
    e->last.lds = (int)((qk::kPfbTableElems + (a.PH - 1) * qk::kPfbG1Elems + wpw * 64 * qk::kPfbRow + (a.PH - 1) * wpw * 64 * 9) * sizeof(float2));
    return 0;
}

// the 4096-point overlap-save kernels (fft_fir.hip)
int launch_fft(Engine* e, const void* d_in, int64_t count, int64_t nout, void* d_out, hipStream_t s) {
    int rc = fft_prepare(e);
    if (rc) return rc;
    qk::FftArgs a;
    memset(&a, 0, sizeof(a));
    a.in = static_cast<const float2*>(d_in);
    a.out = static_cast<float2*>(d_out);
    a.hist = reinterpret_cast<const float2*>(e->d_hist[e->cur]);
    a.hist_keep = a.hist;
    a.hist_next = reinterpret_cast<float2*>(e->d_hist[e->cur ^ 1]);
    rc = raw_history(e, s, &a.hist, &a.hist_raw_next);
    if (rc) return rc;
    a.Hf = e->d_fft_H;
    a.TA = e->d_fft_TA;
    a.TB = e->d_fft_TB;
    a.HfT = e->d_fft_H + qk::kFftN;
    a.TAT = e->d_fft_TA + qk::kFftN;
    a.tbl = qk::knob(qk::K_FFT_TBL, 1) ? 1 : 0;
    a.count = count;
    a.nout = nout;
    a.H = e->H;
    a.dec = fft_dec(desc_of(e));
    // Decimate by 2 on chip-filling calls (round 3, profiles/r03_tune_dec2.txt): the pruned inverse saves one radix-16 pass on half the
    // lanes but runs its last two passes on 128 of them behind two more barriers and stores 8 bytes per lane; the full inverse with every
    // other output kept is ahead from 2^25 samples (0.115 against 0.128 ms; 0.400 against 0.491 at 2^27), with the NCO from 2^26
    // (0.247 / 0.254; 0.472 / 0.505).  Decimations 4, 8, 16 keep the pruned form at every size (0.33 / 0.30 / 0.29 against 0.38 / 0.37 / 0.39).
    if (a.dec == 2 && e->ch == 2) {
        const int lim = qk::knob(qk::K_FFT_PRUNE2_MAX_COUNT, -1);
        // (re-measured once both forms ran four workgroups per CU where they can: 2^24 samples 0.0606 against 0.0623 ms, NCO from 2^25: 0.126 / 0.131)
        if (count >= (lim >= 0 ? (int64_t)lim : (int64_t)(e->rotate ? 1 << 25 : 1 << 24))) a.dec = 1;
    }
    a.rot = e->rotate ? 1 : 0;
    a.decm = 1;
    if (a.dec == 1 && e->kind != KIND_FIR) {
        // any-decimation resampler / VFO: y[n'] sits at stream position n'*M - 1.  Even overlap and
        // an even segment start (two samples before the first valid position) keep 16-byte loads.
        a.decm = e->M;
        a.decm_inv = (e->M >= 2 && (unsigned long long)(e->M + 4096) * (unsigned long long)e->M < (1ULL << 32)) ? (unsigned)((1ULL << 32) / (unsigned)e->M) + 1u : 0u;
        a.strided = 1;
        a.ov = (e->ntaps - 1 + 1) & ~1;
        a.seg_shift = a.ov + 2;
        a.L = qk::kFftN - a.ov;
        a.nblocks = (int)((count + 2 + a.L - 1) / a.L);
        a.vec = (((uintptr_t)d_in) & 15) == 0;
    } else if (a.dec == 1) {
        a.ov = (e->ntaps - 1 + 1) & ~1;   // FIR: out index == stream position; even so segments stay 16-byte aligned
        a.vec = ((((uintptr_t)d_in) | ((uintptr_t)d_out)) & 15) == 0;
        a.seg_shift = a.ov;
        a.L = qk::kFftN - a.ov;
        a.nblocks = (int)((count + a.L - 1) / a.L);
    } else {
        // resampler: y[n'] sits at stream position n'*dec - 1; segments start one sample early
        a.ov = ((e->ntaps - 1 + a.dec - 1) / a.dec) * a.dec;
        a.seg_shift = a.ov + 1;
        a.L = qk::kFftN - a.ov;
        const int per_block = a.L / a.dec;
        a.nblocks = (int)((nout + per_block - 1) / per_block);
    }
    if (e->ch == 1) {   // real data: one workgroup iteration = a PAIR of real segments
        a.real2 = 1;
        // 8-byte pair accesses: segments start on even samples (L, ov, seg_shift are even) of 8-byte aligned buffers
        a.vec = ((((uintptr_t)d_in) | ((uintptr_t)d_out)) & 7) == 0;
        a.nblocks = (a.nblocks + 1) / 2;
    }
    // FIR: 4 workgroups resident per CU (124 VGPRs, 37 KB LDS), 16 queued per CU for balance (the LDS-DMA kernels: a tapered grid, below).
    // Decimators work in groups of `dec` segments, 2 resident per CU (70 KB LDS).
    // (grouped only when the groups fill the chip -- measured crossover ~1000 groups, 2^25 samples at decimation 8 --
    // below that the segments run one per workgroup: a 1e6-sample block 10 us instead of 28)
    // FIR<complex_t> on aligned buffers: the LDS-DMA form (fir_fft_dma_kernel, fft_fir.hip)
    // The sample stream's cache policy in the LDS-DMA kernels (FftArgs::nt), by the overlap, as measured at 2^27 samples
    // (profiles/r06_fir256_taps.txt): non-temporal stores pay where every segment starts on a 64-byte boundary (overlap a multiple of 8
    // samples: - 2.1 % at 1000 taps, - 4.8 % at 57; 0 % at an overlap of 60, + 1.2 % at 62), the non-temporal DMA beside them only while
    // the two rows that stay cacheable hold the whole overlap (- 4.5 ... - 6.6 % up to 256; + 1.1 % at 2048).  QDSP_HIP_FFT_NT overrides.
    // (Buffers that are themselves not 64-byte aligned put the segments where an overlap of 62 puts them: plain accesses.)
    const bool on_64_bytes = a.ov % 8 == 0 && ((((uintptr_t)d_in) | ((uintptr_t)d_out)) & 63) == 0;
    a.nt = qk::knob(qk::K_FFT_NT, !on_64_bytes ? 0 : a.ov <= 256 ? 3 : 2);
    a.abl = qk::knob(qk::K_FFT_ABL, 0);
    a.stamps = reinterpret_cast<unsigned*>(qk::knobs_snapshot()->fft_stamps);   // diagnostic: scripts/stamp_fir_fft.py
    a.dma = (a.dec == 1 && !a.strided && !a.rot && e->ch == 2 && a.vec && a.ov <= 2048) ? qk::knob(qk::K_FFT_DMA, 1) : 0;   // 1: scalar arithmetic, 2: packed
    const bool grouped = a.dec >= 4 && (a.nblocks + a.dec - 1) / a.dec >= 1024;
    a.grouped = grouped ? 1 : 0;
    const int per_cu = qk::knob(qk::K_FFT_WG_PER_CU, grouped ? 4 : 16);
    const int units = grouped ? (a.nblocks + a.dec - 1) / a.dec : a.nblocks;
    int nwg = 256 * per_cu;
    if (nwg > units) nwg = units;
    // (QDSP_HIP_FFT_WG_PER_CU below 1: one workgroup walks every unit, as in launch_pfb and launch_rm -- a grid of none would leave the
    // segment loop a stride of 0.  A call with no unit at all keeps its grid of the hand-over workgroup alone.)
    if (nwg < 1 && units > 0) nwg = 1;
    a.n_long = nwg;   // (n_long, rounds: read by the LDS-DMA kernels only)
    a.rounds = (units + nwg - 1) / (nwg > 0 ? nwg : 1);
    if (a.dma) {   // tapered grid (fft_fir.hip.h): the resident workgroups (four per CU) are long, short ones follow
        const int slots_per_cu = qk::knob(qk::K_FFT_WG_PER_CU, 4);
        const int slots = 256 * (slots_per_cu < 1 ? 1 : slots_per_cu);   // (below 1 reads as 1: fft_taper_rounds divides by the slots)
        a.n_long = a.nblocks < slots ? a.nblocks : slots;
        a.rounds = qk::fft_taper_rounds(a.nblocks, slots);
        nwg = a.n_long + qk::fft_taper_short_count(a.nblocks, slots, a.rounds);
    }
    a.nwg = nwg;
    if (a.rot) {
        a.phase_in0 = e->phase;
        a.phase0 = e->phase - (unsigned long long)(e->ntaps - 1) * e->dphase;
        a.dphase = e->dphase;
        a.gm1 = e->volk_gain ? e->gm1 : 0.0f;
        // one workgroup's step between its units: nwg segments (per-segment kernel), nwg groups of dec segments (grouped)
        const long double step_mult = (long double)nwg * (long double)a.L * (long double)(grouped ? a.dec : 1);
        if (!e->rot_step_ok || e->rot_step_dphase != e->dphase || e->rot_step_mult != step_mult) {
            unit_of_fx_c(e->dphase, step_mult, &e->rot_step_val.x, &e->rot_step_val.y);
            e->rot_step_dphase = e->dphase;
            e->rot_step_mult = step_mult;
            e->rot_step_ok = true;
        }
        a.rot_step = e->rot_step_val;
        if (!e->wtab4k_ok || e->wtab4k_dphase != e->dphase) {
            for (int n2 = 0; n2 < 16; n2++) {
                double c, sn;
                unit_of_fx_c(e->dphase, (long double)(256 * n2), &c, &sn);
                e->wtab4k[n2] = make_float2((float)c, (float)sn);
            }
            e->wtab4k_dphase = e->dphase;
            e->wtab4k_ok = true;
        }
        memcpy(a.wtab, e->wtab4k, sizeof(a.wtab));
    }
    rc = qk::launch_fir_fft(a, nwg + 1, s);
    if (rc) return rc;
    e->raw_valid = e->rotate && e->H > 0;   // (the caller flips cur: the raw hand-over then sits at d_hist_raw[cur])
    e->last.name = a.dma == 2 ? "fir_fft_dmapk_kernel" : a.dma ? "fir_fft_dma_kernel" : "fir_fft_kernel";
    e->last.grid = nwg + 1;
    e->last.block = qk::kFftNT;
    e->last.lds = (int)(((grouped ? 2 : 1) * qk::kFftLdsElems + 16 * 17) * sizeof(float2));
    return 0;
}

// outputs per wave task: a task reads one tile of 16 rows beyond its own (T = 256: 6 %); small calls take shorter
// tasks so that a reference-sized block still spreads over the chip (1e6 samples at decimation 50: 20 000 outputs)
void mf_tasks(qk::MfArgs& a, int64_t nout, int nchan, bool rot, bool real) {
    long long T = nout * nchan / 2048;      // (one round of the chip: 3072 wave slots; 8192 left a 4M-sample call at T = 16 -- half of every task's reads its neighbour's -- and 18 us instead of 14)
    T = (T + 15) / 16 * 16;
    // (real data, round 4: 256 outputs per task on chip-filling calls -- decimate-by-50 0.118 -> 0.110 ms per 2^27 samples, by-200 -10 %, by-32 +1 %;
    // at 2^23 samples 128 keeps twice the tasks and decimate-by-16 a third quicker)
    const long long tmax = qk::knob(qk::K_MF_TASK_MAX, (rot || (real && a.count >= (1LL << 26))) ? 256 : 128);
    if (T > tmax) T = tmax;
    if (T < 16) T = 16;
    a.T = (int)T;
    a.ntasks = (int)((nout + T - 1) / T);
    a.minv = (unsigned)(((1ull << 32) + a.M - 1) / a.M);
    a.defer_store = (long long)a.count * nchan >= (1LL << 22);      // (profiles/r04_mf_deferred_store.txt)
}
// NCO tables: one tile (16 M samples) further in FP64, load i of a tile (64 i samples) in FP32
void mf_rot_tables(unsigned long long dphase, int M, int KJ, double2* step, float2* rot_k) {
    unit_of_fx_c(dphase, 16.0L * (long double)M, &step->x, &step->y);
    for (int k = 0; k < 2 * KJ; k++) {
        double c, sn;
        unit_of_fx_c(dphase, 64.0L * (long double)k, &c, &sn);
        rot_k[k] = make_float2((float)c, (float)sn);
    }
}

// FIR<complex_t> on reference-sized calls: the direct form arranged for latency (fir_lat.hip.h; fir_lat_eligible, select.cpp)
int launch_fir_lat(Engine* e, const void* d_in, int64_t count, void* d_out, hipStream_t s) {
    qk::FirLatArgs a;
    memset(&a, 0, sizeof(a));
    a.in = static_cast<const float2*>(d_in);
    a.out = static_cast<float2*>(d_out);
    a.hist = reinterpret_cast<const float2*>(e->d_hist[e->cur]);
    a.hist_next = reinterpret_cast<float2*>(e->d_hist[e->cur ^ 1]);
    a.taps = e->d_taps;
    a.count = count;
    a.N = e->ntaps;
    a.Np = (e->ntaps + 7) & ~7;
    a.nwaves = (int)((count + 63) / 64);
    const int rc = qk::launch_fir_lat(a, s);
    if (rc) return rc;
    e->last.name = "fir_lat_kernel";
    e->last.grid = (a.nwaves + 3) / 4 + 1;
    e->last.block = 256;
    e->last.lds = (int)qk::fir_lat_lds_bytes(a.Np);
    return 0;
}

int launch_rm(Engine* e, const void* d_in, int64_t count, int64_t nout, void* d_out, hipStream_t s) {
    qk::RmArgs a;
    memset(&a, 0, sizeof(a));
    a.in = static_cast<const float2*>(d_in);
    a.out = static_cast<float2*>(d_out);
    a.hist = reinterpret_cast<const float2*>(e->d_hist[e->cur]);
    a.hist_next = reinterpret_cast<float2*>(e->d_hist[e->cur ^ 1]);
    a.atab = e->d_taps_rm;
    a.count = count;
    a.nout = nout;
    a.L = e->plan.rm.J * e->L;          // (J merged periods)
    a.M = e->plan.rm.J * e->M;
    a.P = e->P;
    a.minv = (unsigned)(((1ull << 32) + a.M - 1) / a.M);
    a.qpb = e->plan.rm.qpb;
    a.ngrp = e->plan.rm.ngrp;
    a.KB = e->plan.rm.KB;
    a.ext = e->plan.rm.ext;
    a.pitch = e->plan.rm.pitch;
    a.G = e->plan.rm.G;
    a.total = 4 * a.G * a.M + a.ext;
    const long long nper = (nout + a.L - 1) / a.L;
    a.ntiles = (int)((nper + 4 * a.G - 1) / (4 * a.G));
    // waves QUEUED per SIMD (three are resident): more, shorter-lived waves than fit even out the tail and keep the tiles in flight closer
    // together in memory (round 3, scripts/tune_rm_waves.py, profiles/r03_tune_rm_waves.txt: 147/160 0.236 -> 0.224 ms per 2^26 samples,
    // interpolate-by-6 0.164 -> 0.130, 10/7 0.181 -> 0.179; the small decimating ratios are indifferent)
    int nwaves = 1024 * qk::knob(qk::K_RM_WAVES_PER_SIMD, e->M == 1 ? 12 : e->L >= 100 ? 8 : 6);
    if (nwaves > a.ntiles) nwaves = a.ntiles;
    if (nwaves < 1) nwaves = 1;
    a.nwaves = nwaves;
    if (e->rotate) {
        a.phase0 = e->phase;
        a.dphase = e->dphase;
        a.gm1 = e->volk_gain ? e->gm1 : 0.0f;
        unit_of_fx_c(e->dphase, (long double)nwaves * 4.0L * (long double)a.G * (long double)a.M, &a.rot_step.x, &a.rot_step.y);
        for (int k = 0; k < qk::kRmNE; k++) {
            double c, sn;
            unit_of_fx_c(e->dphase, 64.0L * (long double)k, &c, &sn);
            a.rot_k[k] = make_float2((float)c, (float)sn);
        }
    }
    const int rc = qk::launch_rm_resamp(a, e->rotate, e->ch == 1, s);
    if (rc) return rc < 0 && rc != -1 ? rc : QDSP_HIP_EINVAL;
    e->last.name = e->ch == 1 ? "resamp_mfma_real_kernel" : "resamp_mfma_kernel";
    e->last.grid = (nwaves + 3) / 4 + 1;
    e->last.block = 256;
    e->last.lds = (int)qk::rm_lds_bytes(a.ngrp, a.KB, a.G, a.pitch, e->ch == 1);
    return 0;
}

int launch_mf(Engine* e, const void* d_in, int64_t count, int64_t nout, void* d_out, hipStream_t s) {
    qk::MfArgs a;
    memset(&a, 0, sizeof(a));
    a.in = static_cast<const float2*>(d_in);
    a.out = static_cast<float2*>(d_out);
    a.hist = reinterpret_cast<const float2*>(e->d_hist[e->cur]);
    a.hist_next = reinterpret_cast<float2*>(e->d_hist[e->cur ^ 1]);
    a.tapk = e->d_taps_mf;
    a.count = count;
    a.nout = nout;
    a.P = e->P;
    a.M = e->plan.mf.keep2 ? e->M / 2 : e->M;
    a.keep2 = e->plan.mf.keep2;
    if (e->plan.mf.keep2) a.nout = 2 * nout - 1;      // (in the kernel's units: outputs of the decimator by M / 2)
    // the kernel's unguarded loads of an interior tile read 64 (2 KJ - 2) samples from the tile's start: they must lie inside the tile's own 16 M
    // (true for KJ = ceil(M / 8); a plan that pads KJ beyond that would read past the end of the input -- found the hard way, round 4)
    if (128 * (e->plan.mf.KJ - 1) > 16 * a.M) return QDSP_HIP_EINVAL;
    mf_tasks(a, a.nout, 1, e->rotate, e->ch == 1);
    if (e->rotate) {
        a.phase0 = e->phase;
        a.dphase = e->dphase;
        a.gm1 = e->volk_gain ? e->gm1 : 0.0f;
        mf_rot_tables(e->dphase, a.M, e->plan.mf.KJ, &a.rot_step, a.rot_k);
    }
    const int rc = qk::launch_mf_dec(a, e->plan.mf.KJ, e->rotate, qk::knob(qk::K_MF_DEPTH, (e->plan.mf.KJ <= 8 && !(e->rotate && e->plan.mf.KJ >= 5)) ? 2 : 1)      /* (fused VFO from decimation 33 on: one tile ahead = 118 VGPRs = four waves per SIMD, 1-3 % ahead of two tiles at three: 0.232 -> 0.229 ms at decimation 50; the plain decimator the other way round) */, e->plan.mf.QS, e->ch == 1, s);
    if (rc) return rc < 0 && rc != -1 ? rc : QDSP_HIP_EINVAL;
    e->last.name = e->ch == 1 ? "decim_mfma_real_kernel" : "decim_mfma_kernel";
    e->last.grid = (a.ntasks + 3) / 4 + 1;
    e->last.block = 256;
    e->last.lds = e->ch == 1 ? 4 * (16 * (8 * e->plan.mf.KJ + 4) + 64) * (int)sizeof(float) : 4 * (16 * (8 * e->plan.mf.KJ + 2) + 64) * (int)sizeof(float2);
    return 0;
}

// One run() worth of work on device pointers.  Returns the output count.
int64_t process_dev(Engine* e, const void* d_in, int64_t count, void* d_out, void* stream) {
    if (count < 0 || (count > 0 && ((!d_in && e->kind != KIND_SINE) || !d_out))) return QDSP_HIP_EINVAL;
    apply_pending_inc(e);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL == HIP's default stream
    const int64_t nout = out_size(e, count);
    int rc = 0;
    const Family family = select(desc_of(e), e->plan, count);
    switch (family) {
    case F_XLATE:
        rc = launch_xlate(e, d_in, count, d_out, s);
        break;
    case F_FIR_LAT:
        rc = launch_fir_lat(e, d_in, count, d_out, s);
        break;
    case F_MFMA_DECIM:
        rc = launch_mf(e, d_in, count, nout, d_out, s);
        break;
    case F_PFB:      // (the three overlap-save forms hand over the raw history as well: raw_history)
        rc = launch_pfb(e, d_in, count, nout, d_out, s);
        break;
    case F_FFT1K:
        rc = launch_fft1k(e, d_in, count, nout, d_out, s);
        break;
    case F_FFT4K:
        rc = launch_fft(e, d_in, count, nout, d_out, s);
        break;
    case F_WIN:
        if (e->ch == 2) rc = e->rotate ? launch_win<2, true>(e, d_in, count, nout, d_out, s) : launch_win<2, false>(e, d_in, count, nout, d_out, s);
        else rc = launch_win<1, false>(e, d_in, count, nout, d_out, s);
        break;
    case F_CORE: {
        qk::CoreArgs a;
        fill_call(a, e, d_in, count, nout, d_out);
        a.taps = e->d_taps;
        a.H = e->H;
        a.M = e->M;
        a.Q = (e->P + e->M - 1) / e->M;
        if (e->ch == 2) rc = e->rotate ? launch_core<2, true>(e, a, s) : launch_core<2, false>(e, a, s);
        else rc = launch_core<1, false>(e, a, s);
        break;
    }
    case F_MFMA_RATIONAL:
        rc = launch_rm(e, d_in, count, nout, d_out, s);
        break;
    case F_LM:
        if (e->ch == 2) rc = e->rotate ? launch_lm<2, true>(e, d_in, count, nout, d_out, s) : launch_lm<2, false>(e, d_in, count, nout, d_out, s);
        else rc = launch_lm<1, false>(e, d_in, count, nout, d_out, s);
        break;
    case F_ANY: {
        qk::AnyArgs a;
        fill_call(a, e, d_in, count, nout, d_out);
        a.phases = e->d_taps;
        if (e->plan.core) {
            // QDSP_HIP_FORCE_ANY set after the plan was made: d_taps is branch-major, this kernel reads the phase table
            rc = plain_taps(e);
            if (rc) return rc;
            a.phases = e->d_taps_plain;
        }
        a.L = e->L;
        a.M = e->M;
        a.P = e->P;
        if (e->ch == 2) rc = e->rotate ? launch_any<2, true>(e, a, s) : launch_any<2, false>(e, a, s);
        else rc = launch_any<1, false>(e, a, s);
        break;
    }
    }
    if (rc == 0 && family != F_XLATE) e->cur ^= 1;      // (every filter kernel writes the next history into the other buffer)
    if (family != F_PFB && family != F_FFT1K && family != F_FFT4K) e->raw_valid = false;   // (the direct kernels hand over the rotated history only)
    if (rc) return rc;
    if (e->rotate) e->phase += (unsigned long long)count * e->dphase;  // exact mod 2^64
    return nout;
}

// Host-pointer path: what a block's run() calls between _in->read() and out.swap().
int64_t process_host(Engine* e, const float* in, int count, float* out) {
    if (count < 0 || (count > 0 && (!in || !out))) return QDSP_HIP_EINVAL;
    if (count > e->max_block) {
        int rc = ensure_io(e, count);
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(e->device));
    const size_t in_bytes = (size_t)count * e->ch * sizeof(float);
    // (Round 4 re-measured pieces of one synchronous call on two streams -- upload stream + this one: 0.321 against 0.315 ms for a 1e6-sample FIR
    // block, 0.261 against 0.194 for the decimator: inside ONE call the two copy directions still do not overlap.  Across the calls of a block
    // graph they do: process_ex, Engine::up_stream.)
    if (e->up_stream && e->kernel_recorded) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_up, 0));   // (an earlier split upload of this handle)
    if (count) HIPCHK(hipMemcpyAsync(e->d_in, in, in_bytes, hipMemcpyHostToDevice, e->stream));
    const int64_t nout = process_dev(e, e->d_in, count, e->d_out, e->stream);
    if (nout < 0) return nout;
    if (nout)
        HIPCHK(hipMemcpyAsync(out, e->d_out, (size_t)nout * e->ch * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(wait_stream(e->stream));
    return nout;
}

// run() with each side on the host (pinned stream buffer) or already on the device (the
// device-resident companion of a stream): copies only where a side is on the host.
int64_t process_ex(Engine* e, const void* in, int in_dev, int count, void* out, int out_dev) {
    if (count < 0 || (count > 0 && (!in || !out))) return QDSP_HIP_EINVAL;
    // (a deferred host output is a host output: it goes through the staging buffer unless the kernel can store
    // straight into the pinned buffer)
    const bool out_host = out_dev == QDSP_HIP_LINK_HOST || out_dev == QDSP_HIP_LINK_HOST_DEFERRED;
    if ((!in_dev || out_host) && count > e->max_block) {
        int rc = ensure_io(e, count);
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(e->device));
    // in_dev / out_dev: 0 host, 1 device (complete / to be complete on return), 2 device through a pipelined link
    hipStream_t st = e->stream;
    if (in_dev == QDSP_HIP_LINK_PIPELINED || out_dev == QDSP_HIP_LINK_PIPELINED) {
        st = shared_stream(e->device);
        if (!st) return QDSP_HIP_ENOMEM;
    }
    if (e->last_stream && e->last_stream != st) HIPCHK(hipStreamSynchronize(e->last_stream));   // (links re-plumbed)
    e->last_stream = st;
    const void* src = in;
    // Host input + deferred host output into pinned memory (HandlerSource -> block -> sink on the mirror's pinned streams): see Engine::up_stream
    const bool split_upload = !in_dev && count > 0 && out_dev == QDSP_HIP_LINK_HOST_DEFERRED && e->done_ev && mapped_host_ptr(out) && mapped_host_ptr(const_cast<void*>(in)) &&
                              !qk::knob(qk::K_NO_SPLIT_UPLOAD, 0);
    if (split_upload) {
        if (!e->up_stream) {
            HIPCHK(hipStreamCreateWithFlags(&e->up_stream, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&e->ev_up, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&e->ev_kernel, hipEventDisableTiming));
        }
        if (e->kernel_recorded) HIPCHK(hipStreamWaitEvent(e->up_stream, e->ev_kernel, 0));      // the previous kernel has read d_in
        HIPCHK(hipMemcpyAsync(e->d_in, in, (size_t)count * e->ch * sizeof(float), hipMemcpyHostToDevice, e->up_stream));
        HIPCHK(hipEventRecord(e->ev_up, e->up_stream));
        HIPCHK(hipStreamWaitEvent(st, e->ev_up, 0));
        src = e->d_in;
    } else if (!in_dev) {
        // (an earlier split upload of this handle may still be in flight on the other stream: same staging buffer)
        if (e->up_stream && e->kernel_recorded) HIPCHK(hipStreamWaitEvent(st, e->ev_up, 0));
        if (count) HIPCHK(hipMemcpyAsync(e->d_in, in, (size_t)count * e->ch * sizeof(float), hipMemcpyHostToDevice, st));
        src = e->d_in;
    }
    // A small result headed for pinned, device-mapped host memory (a decimator's output in a stream<T> buffer) is
    // stored there by the kernel itself: posted writes over the link instead of a separate copy operation, which
    // costs ~10 us of latency per call whatever its size.
    const bool deferred = out_dev == QDSP_HIP_LINK_HOST_DEFERRED;
    if (deferred) {
        if (!e->done_ev) return QDSP_HIP_EINVAL;
        out_dev = QDSP_HIP_LINK_HOST;
    }
    void* dst = out_dev ? out : e->d_out;
    bool direct_out = false;
    if (!out_dev && count > 0) {
        const size_t out_bytes = (size_t)out_size(e, count) * e->ch * sizeof(float);
        if (out_bytes > 0 && out_bytes <= (size_t)(1 << 20)) {
            void* mapped = mapped_host_ptr(out);
            if (mapped) { dst = mapped; direct_out = true; }
        }
    }
    const int64_t nout = process_dev(e, src, count, dst, st);
    if (nout < 0) return nout;
    if (split_upload) {
        HIPCHK(hipEventRecord(e->ev_kernel, st));
        e->kernel_recorded = true;
    }
    if (!out_dev && !direct_out && nout)
        HIPCHK(hipMemcpyAsync(out, e->d_out, (size_t)nout * e->ch * sizeof(float), hipMemcpyDeviceToHost, st));
    // a block handed to a pipelined link need not be complete; a host input must have left its buffer, though
    if (deferred) {
        // the consumer waits (stream<T>::read does, on the event that travels with the buffer); only a host INPUT
        // and a pageable output (whose "async" copy is not) still need this call to wait
        HIPCHK(hipEventRecord(e->done_ev, st));
        // (a device input from a producer outside the shared stream must have been read before this call returns
        // and the block flushes it: only a pipelined input lets the call go without waiting)
        if (in_dev == QDSP_HIP_LINK_PIPELINED && (direct_out || nout == 0 || mapped_host_ptr(out))) return nout;
        if (split_upload) {
            // the input buffer is the caller's again once the upload has read it; the results travel behind done_ev
            HIPCHK(hipEventSynchronize(e->ev_up));
            return nout;
        }
        HIPCHK(hipEventSynchronize(e->done_ev));
        return nout;
    }
    if (!(out_dev == QDSP_HIP_LINK_PIPELINED && in_dev == QDSP_HIP_LINK_PIPELINED))
        HIPCHK(st == e->stream ? wait_stream(st) : wait_event(e->ev0, st));
    return nout;
}

int reset(Engine* e) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++)
        if (e->d_hist[i] && e->H > 0) HIPCHK(hipMemset(e->d_hist[i], 0, (size_t)e->H * e->ch * sizeof(float)));
    e->phase = 0;
    e->raw_valid = false;
    return 0;
}

int get_history(Engine* e, float* hist) {
    if (!hist) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    if (e->H > 0)
        HIPCHK(hipMemcpy(hist, e->d_hist[e->cur], (size_t)e->H * e->ch * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
int set_history(Engine* e, const float* hist) {
    if (!hist) return QDSP_HIP_EINVAL;
    e->raw_valid = false;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    if (e->H > 0)
        HIPCHK(hipMemcpy(e->d_hist[e->cur], hist, (size_t)e->H * e->ch * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// `d_hist` holds the H INPUT samples that precede the next call.  Engines with an NCO keep
// their history rotated (as the reference resampler's buffer holds the xlator's output), so
// those samples are rotated here with the phases they would have had: phase - H*dphase onward.
int set_history_dev(Engine* e, const void* d_hist, void* stream) {
    if (!d_hist) return QDSP_HIP_EINVAL;
    apply_pending_inc(e);
    e->raw_valid = false;
    HIPCHK(hipSetDevice(e->device));
    if (e->H <= 0) return 0;
    if (e->rotate && e->has_filter)
        return launch_xlate_inc(e, d_hist, e->H, e->d_hist[e->cur], e->phase - (unsigned long long)e->H * e->dphase, e->dphase, 0.0f,
                                static_cast<hipStream_t>(stream));
    HIPCHK(hipMemcpyAsync(e->d_hist[e->cur], d_hist, (size_t)e->H * e->ch * sizeof(float), hipMemcpyDeviceToDevice,
                          static_cast<hipStream_t>(stream)));
    return 0;
}

int get_phase(Engine* e, float* re, float* im) {
    if (!re || !im) return QDSP_HIP_EINVAL;
    double c, s;
    unit_of_fx(e->phase, 1.0L, &c, &s);
    *re = (float)c;
    *im = (float)s;
    return 0;
}
int set_phase(Engine* e, float re, float im) {
    if (re == 0.0f && im == 0.0f) return QDSP_HIP_EINVAL;
    e->raw_valid = false;
    e->phase = fx_of_turns(turns_of(re, im));
    return 0;
}

int time_process(Engine* e, const void* d_in, int64_t count, void* d_out, void* stream, int iters, float* ms) {
    if (iters <= 0 || !ms) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(hipEventRecord(e->ev0, s));
    for (int i = 0; i < iters; i++) {
        int64_t r = process_dev(e, d_in, count, d_out, stream);
        if (r < 0) return (int)r;
    }
    HIPCHK(hipEventRecord(e->ev1, s));
    HIPCHK(hipEventSynchronize(e->ev1));
    float t = 0.0f;
    HIPCHK(hipEventElapsedTime(&t, e->ev0, e->ev1));
    *ms = t / (float)iters;
    return 0;
}

Engine* any_engine(void* h) {
    Engine* e = static_cast<Engine*>(h);
    return (e && e->magic == kMagic) ? e : nullptr;
}

}  // namespace qh

using namespace qh;

// ==========================================================================================
// extern "C" boundary
// ==========================================================================================
extern "C" {

int qdsp_hip_abi_version(void) { return QDSP_HIP_ABI_VERSION; }

const char* qdsp_hip_error_string(int code) {
    if (code >= 0) return "success";
    switch (code) {
        case QDSP_HIP_EINVAL: return "qdsp_hip: invalid argument";
        case QDSP_HIP_ENOMEM: return "qdsp_hip: out of host memory";
        case QDSP_HIP_ESIZE: return "qdsp_hip: block larger than max_block";
        case QDSP_HIP_ENODEV: return "qdsp_hip: no usable HIP device";
        case QDSP_HIP_ERCCL: return "qdsp_hip: RCCL unavailable or an RCCL call failed (ring)";
        default: return hipGetErrorString((hipError_t)(-code));
    }
}

int qdsp_hip_device_count(int* count) {
    if (!count) return QDSP_HIP_EINVAL;
    *count = 0;
    HIPCHK(hipGetDeviceCount(count));
    return 0;
}

int qdsp_hip_device_info(int device, char* name, int name_len, char* arch, int arch_len, int* cus) {
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device));
    if (name && name_len > 0) { strncpy(name, p.name, name_len - 1); name[name_len - 1] = 0; }
    if (arch && arch_len > 0) { strncpy(arch, p.gcnArchName, arch_len - 1); arch[arch_len - 1] = 0; }
    if (cus) *cus = p.multiProcessorCount;
    return 0;
}

int qdsp_hip_host_alloc(void** p, size_t bytes) {
    if (!p) return QDSP_HIP_EINVAL;
    HIPCHK(hipHostMalloc(p, bytes, hipHostMallocDefault));
    return 0;
}
int qdsp_hip_host_free(void* p) { HIPCHK(hipHostFree(p)); return 0; }
int qdsp_hip_host_register(void* p, size_t bytes) { HIPCHK(hipHostRegister(p, bytes, hipHostRegisterDefault)); return 0; }
int qdsp_hip_host_unregister(void* p) { HIPCHK(hipHostUnregister(p)); return 0; }
int qdsp_hip_dev_alloc(int device, void** p, size_t bytes) {
    if (!p) return QDSP_HIP_EINVAL;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMalloc(p, bytes));
    return 0;
}
int qdsp_hip_dev_free(int device, void* p) { HIPCHK(hipSetDevice(device)); HIPCHK(hipFree(p)); return 0; }
int qdsp_hip_memcpy_h2d(int device, void* d, const void* h, size_t bytes) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return 0;
}
int qdsp_hip_memcpy_d2h(int device, void* h, const void* d, size_t bytes) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
    return 0;
}
int qdsp_hip_memcpy_d2d(int device, void* d_dst, const void* d_src, size_t bytes) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice));
    return 0;
}
// Copies for blocks that forward data between links (Splitter): ordered behind a pipelined input, not waited for
// when the destination link is pipelined too.
int qdsp_hip_memcpy_d2d_link(int device, void* d_dst, const void* d_src, size_t bytes, int in_link, int out_link) {
    HIPCHK(hipSetDevice(device));
    if (in_link != QDSP_HIP_LINK_PIPELINED && out_link != QDSP_HIP_LINK_PIPELINED) {
        HIPCHK(hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice));
        return 0;
    }
    hipStream_t st = shared_stream(device);
    if (!st) return QDSP_HIP_ENOMEM;
    HIPCHK(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, st));
    // Only a pipelined INPUT may be released with the copy still queued (its producer launches into this same
    // stream, behind the copy).  A plain device input comes from a producer on some other stream (Add / Multiply,
    // a host-fed Splitter): it reuses the buffer two blocks later whatever this stream has got to, so the copy
    // must have read it before the caller flushes.
    if (!(in_link == QDSP_HIP_LINK_PIPELINED && out_link == QDSP_HIP_LINK_PIPELINED)) HIPCHK(hipStreamSynchronize(st));
    return 0;
}
int qdsp_hip_memcpy_d2h_link(int device, void* h_dst, const void* d_src, size_t bytes, int in_link) {
    HIPCHK(hipSetDevice(device));
    if (in_link != QDSP_HIP_LINK_PIPELINED) {
        HIPCHK(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
        return 0;
    }
    hipStream_t st = shared_stream(device);
    if (!st) return QDSP_HIP_ENOMEM;
    HIPCHK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
int qdsp_hip_device_sync(int device) { HIPCHK(hipSetDevice(device)); HIPCHK(hipDeviceSynchronize()); return 0; }

// ---- filter-bearing operators: FIR, resampler, fused VFO ---------------------------------
#define QDSP_FILTER_COMMON(prefix, KIND)                                                          \
    int prefix##_reset(void* h) { Engine* e = as_engine(h, KIND); return e ? reset(e) : QDSP_HIP_EINVAL; } \
    int prefix##_history_len(void* h) { Engine* e = as_engine(h, KIND); return e ? e->H : QDSP_HIP_EINVAL; } \
    int prefix##_get_history(void* h, float* p) { Engine* e = as_engine(h, KIND); return e ? get_history(e, p) : QDSP_HIP_EINVAL; } \
    int prefix##_set_history(void* h, const float* p) { Engine* e = as_engine(h, KIND); return e ? set_history(e, p) : QDSP_HIP_EINVAL; } \
    int prefix##_history_dev(void* h, void** d) {                                                 \
        Engine* e = as_engine(h, KIND);                                                           \
        if (!e || !d) return QDSP_HIP_EINVAL;                                                     \
        *d = e->d_hist[e->cur];                                                                   \
        e->raw_valid = false; /* (the caller may write through the pointer) */                    \
        return 0;                                                                                 \
    }                                                                                             \
    int prefix##_set_history_dev(void* h, const void* d, void* s) {                               \
        Engine* e = as_engine(h, KIND);                                                           \
        return e ? set_history_dev(e, d, s) : QDSP_HIP_EINVAL;                                    \
    }                                                                                             \
    void prefix##_destroy(void* h) { Engine* e = as_engine(h, KIND); if (e) destroy(e); }

#define QDSP_FIR_API(prefix, CH)                                                                  \
    int prefix##_create(void** h, int device, const float* taps, int ntaps, int max_block) {      \
        int rc = create(h, KIND_FIR, device, CH, false, true, max_block);                         \
        if (rc) return rc;                                                                        \
        Engine* e = static_cast<Engine*>(*h);                                                     \
        rc = configure(e, taps, ntaps, 1, 1);                                                     \
        if (!rc) rc = ensure_io(e, max_block);                                                    \
        if (rc) { destroy(e); *h = nullptr; }                                                     \
        return rc;                                                                                \
    }                                                                                             \
    int prefix##_process(void* h, const float* in, int count, float* out) {                       \
        Engine* e = as_engine(h, KIND_FIR);                                                       \
        if (!e || e->ch != CH) return QDSP_HIP_EINVAL;                                            \
        int64_t r = process_host(e, in, count, out);                                              \
        return r < 0 ? (int)r : 0;                                                                \
    }                                                                                             \
    int prefix##_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* s) {    \
        Engine* e = as_engine(h, KIND_FIR);                                                       \
        if (!e || e->ch != CH) return QDSP_HIP_EINVAL;                                            \
        int64_t r = process_dev(e, d_in, count, d_out, s);                                        \
        return r < 0 ? (int)r : 0;                                                                \
    }                                                                                             \
    int prefix##_process_ex(void* h, const void* in, int in_dev, int count, void* out, int out_dev) { \
        Engine* e = as_engine(h, KIND_FIR);                                                       \
        if (!e || e->ch != CH) return QDSP_HIP_EINVAL;                                            \
        int64_t r = process_ex(e, in, in_dev, count, out, out_dev);                               \
        return r < 0 ? (int)r : 0;                                                                \
    }                                                                                             \
    int prefix##_set_taps(void* h, const float* taps, int ntaps) {                                \
        Engine* e = as_engine(h, KIND_FIR);                                                       \
        return e ? configure(e, taps, ntaps, 1, 1) : QDSP_HIP_EINVAL;                             \
    }                                                                                             \
    int prefix##_set_mode(void* h, int mode) {                                                    \
        Engine* e = as_engine(h, KIND_FIR);                                                       \
        if (!e || mode < 0 || mode > 2) return QDSP_HIP_EINVAL;                                   \
        e->fir_mode = mode;                                                                       \
        return 0;                                                                                 \
    }                                                                                             \
    QDSP_FILTER_COMMON(prefix, KIND_FIR)

QDSP_FIR_API(qdsp_hip_fir_cf32, 2)
QDSP_FIR_API(qdsp_hip_fir_f32, 1)

#define QDSP_DECIM_API(prefix, CH)                                                                \
    int prefix##_create(void** h, int device, const float* taps, int ntaps, int interp, int decim, int max_block) { \
        int rc = create(h, KIND_DECIM, device, CH, false, true, max_block);                       \
        if (rc) return rc;                                                                        \
        Engine* e = static_cast<Engine*>(*h);                                                     \
        rc = configure(e, taps, ntaps, interp, decim);                                            \
        if (!rc) rc = ensure_io(e, max_block);                                                    \
        if (rc) { destroy(e); *h = nullptr; }                                                     \
        return rc;                                                                                \
    }                                                                                             \
    int prefix##_process(void* h, const float* in, int count, float* out) {                       \
        Engine* e = as_engine(h, KIND_DECIM);                                                     \
        if (!e || e->ch != CH) return QDSP_HIP_EINVAL;                                            \
        return (int)process_host(e, in, count, out);                                              \
    }                                                                                             \
    int64_t prefix##_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* s) { \
        Engine* e = as_engine(h, KIND_DECIM);                                                     \
        if (!e || e->ch != CH) return QDSP_HIP_EINVAL;                                            \
        return process_dev(e, d_in, count, d_out, s);                                             \
    }                                                                                             \
    int prefix##_process_ex(void* h, const void* in, int in_dev, int count, void* out, int out_dev) { \
        Engine* e = as_engine(h, KIND_DECIM);                                                     \
        if (!e || e->ch != CH) return QDSP_HIP_EINVAL;                                            \
        return (int)process_ex(e, in, in_dev, count, out, out_dev);                               \
    }                                                                                             \
    int prefix##_configure(void* h, const float* taps, int ntaps, int interp, int decim) {        \
        Engine* e = as_engine(h, KIND_DECIM);                                                     \
        if (!e) return QDSP_HIP_EINVAL;                                                           \
        int rc = configure(e, taps, ntaps, interp, decim);                                        \
        if (!rc && e->max_block) { int mb = e->max_block; e->max_block = 0; rc = ensure_io(e, mb); } \
        return rc;                                                                                \
    }                                                                                             \
    int64_t prefix##_out_size(void* h, int64_t count) {                                           \
        Engine* e = as_engine(h, KIND_DECIM);                                                     \
        return e ? out_size(e, count) : QDSP_HIP_EINVAL;                                          \
    }                                                                                             \
    int prefix##_set_mode(void* h, int mode) {                                                    \
        Engine* e = as_engine(h, KIND_DECIM);                                                     \
        if (!e || mode < 0 || mode > 2) return QDSP_HIP_EINVAL;                                   \
        e->fir_mode = mode;                                                                       \
        return 0;                                                                                 \
    }                                                                                             \
    QDSP_FILTER_COMMON(prefix, KIND_DECIM)

QDSP_DECIM_API(qdsp_hip_decim_cf32, 2)
QDSP_DECIM_API(qdsp_hip_decim_f32, 1)

// ---- FrequencyXlator ----------------------------------------------------------------------
int qdsp_hip_xlate_cf32_create(void** h, int device, float inc_re, float inc_im, int max_block) {
    if (inc_re == 0.0f && inc_im == 0.0f) return QDSP_HIP_EINVAL;
    int rc = create(h, KIND_XLATE, device, 2, true, false, max_block);
    if (rc) return rc;
    Engine* e = static_cast<Engine*>(*h);
    set_inc_now(e, inc_re, inc_im);
    rc = ensure_io(e, max_block);
    if (rc) { destroy(e); *h = nullptr; }
    return rc;
}
int qdsp_hip_xlate_cf32_process(void* h, const float* in, int count, float* out) {
    Engine* e = as_engine(h, KIND_XLATE);
    if (!e) return QDSP_HIP_EINVAL;
    int64_t r = process_host(e, in, count, out);
    return r < 0 ? (int)r : 0;
}
int qdsp_hip_xlate_cf32_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* s) {
    Engine* e = as_engine(h, KIND_XLATE);
    if (!e) return QDSP_HIP_EINVAL;
    int64_t r = process_dev(e, d_in, count, d_out, s);
    return r < 0 ? (int)r : 0;
}
int qdsp_hip_xlate_cf32_process_ex(void* h, const void* in, int in_dev, int count, void* out, int out_dev) {
    Engine* e = as_engine(h, KIND_XLATE);
    if (!e) return QDSP_HIP_EINVAL;
    int64_t r = process_ex(e, in, in_dev, count, out, out_dev);
    return r < 0 ? (int)r : 0;
}
int qdsp_hip_xlate_cf32_set_phase_inc(void* h, float re, float im) {
    Engine* e = as_engine(h, KIND_XLATE);
    if (!e || (re == 0.0f && im == 0.0f)) return QDSP_HIP_EINVAL;
    set_inc(e, re, im);
    return 0;
}
int qdsp_hip_xlate_cf32_get_phase(void* h, float* re, float* im) {
    Engine* e = as_engine(h, KIND_XLATE);
    return e ? get_phase(e, re, im) : QDSP_HIP_EINVAL;
}
int qdsp_hip_xlate_cf32_set_phase(void* h, float re, float im) {
    Engine* e = as_engine(h, KIND_XLATE);
    return e ? set_phase(e, re, im) : QDSP_HIP_EINVAL;
}
int qdsp_hip_xlate_cf32_advance(void* h, int64_t n) {
    Engine* e = as_engine(h, KIND_XLATE);
    if (!e) return QDSP_HIP_EINVAL;
    apply_pending_inc(e);
    e->phase += (unsigned long long)n * e->dphase;
    e->raw_valid = false;
    return 0;
}
int qdsp_hip_xlate_cf32_set_volk_gain(void* h, int on) {
    Engine* e = as_engine(h, KIND_XLATE);
    if (!e) return QDSP_HIP_EINVAL;
    e->volk_gain = on != 0;
    return 0;
}
void qdsp_hip_xlate_cf32_destroy(void* h) { Engine* e = as_engine(h, KIND_XLATE); if (e) destroy(e); }

// ---- SineSource -----------------------------------------------------------------------------
int qdsp_hip_sine_cf32_create(void** h, int device, float inc_re, float inc_im, int max_block) {
    if (inc_re == 0.0f && inc_im == 0.0f) return QDSP_HIP_EINVAL;
    int rc = create(h, KIND_SINE, device, 2, true, false, max_block);
    if (rc) return rc;
    Engine* e = static_cast<Engine*>(*h);
    set_inc_now(e, inc_re, inc_im);
    rc = ensure_io(e, max_block);
    if (rc) { destroy(e); *h = nullptr; }
    return rc;
}
int qdsp_hip_sine_cf32_generate(void* h, int count, void* out, int out_on_device) {
    Engine* e = as_engine(h, KIND_SINE);
    if (!e || count < 0 || (count > 0 && !out)) return QDSP_HIP_EINVAL;
    if ((out_on_device == QDSP_HIP_LINK_HOST || out_on_device == QDSP_HIP_LINK_HOST_DEFERRED) && count > e->max_block) {
        int rc = ensure_io(e, count);
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    if (out_on_device == QDSP_HIP_LINK_PIPELINED) {
        st = shared_stream(e->device);
        if (!st) return QDSP_HIP_ENOMEM;
    }
    if (e->last_stream && e->last_stream != st) HIPCHK(hipStreamSynchronize(e->last_stream));
    e->last_stream = st;
    const bool deferred = out_on_device == QDSP_HIP_LINK_HOST_DEFERRED;
    if (deferred) {
        if (!e->done_ev) return QDSP_HIP_EINVAL;
        out_on_device = QDSP_HIP_LINK_HOST;
    }
    void* dst = out_on_device ? out : e->d_out;
    const int64_t r = process_dev(e, nullptr, count, dst, st);
    if (r < 0) return (int)r;
    if (!out_on_device && count)
        HIPCHK(hipMemcpyAsync(out, e->d_out, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    if (deferred) {
        HIPCHK(hipEventRecord(e->done_ev, st));
        if (count == 0 || mapped_host_ptr(out)) return 0;
        HIPCHK(hipEventSynchronize(e->done_ev));
        return 0;
    }
    if (out_on_device != QDSP_HIP_LINK_PIPELINED) HIPCHK(wait_stream(st));
    return 0;
}
int qdsp_hip_sine_cf32_generate_dev(void* h, int64_t count, void* d_out, void* stream) {
    Engine* e = as_engine(h, KIND_SINE);
    if (!e) return QDSP_HIP_EINVAL;
    const int64_t r = process_dev(e, nullptr, count, d_out, stream);
    return r < 0 ? (int)r : 0;
}
int qdsp_hip_sine_cf32_set_phase_inc(void* h, float re, float im) {
    Engine* e = as_engine(h, KIND_SINE);
    if (!e || (re == 0.0f && im == 0.0f)) return QDSP_HIP_EINVAL;
    set_inc(e, re, im);
    return 0;
}
int qdsp_hip_sine_cf32_get_phase(void* h, float* re, float* im) {
    Engine* e = as_engine(h, KIND_SINE);
    return e ? get_phase(e, re, im) : QDSP_HIP_EINVAL;
}
int qdsp_hip_sine_cf32_set_volk_gain(void* h, int on) {
    Engine* e = as_engine(h, KIND_SINE);
    if (!e) return QDSP_HIP_EINVAL;
    e->volk_gain = on != 0;
    return 0;
}
void qdsp_hip_sine_cf32_destroy(void* h) { Engine* e = as_engine(h, KIND_SINE); if (e) destroy(e); }

// ---- fused VFO ------------------------------------------------------------------------------
int qdsp_hip_xlate_fir_decim_cf32_create(void** h, int device, const float* taps, int ntaps, int interp,
                                         int decim, float inc_re, float inc_im, int max_block) {
    if (inc_re == 0.0f && inc_im == 0.0f) return QDSP_HIP_EINVAL;
    int rc = create(h, KIND_VFO, device, 2, true, true, max_block);
    if (rc) return rc;
    Engine* e = static_cast<Engine*>(*h);
    set_inc_now(e, inc_re, inc_im);
    rc = configure(e, taps, ntaps, interp, decim);
    if (!rc) rc = ensure_io(e, max_block);
    if (rc) { destroy(e); *h = nullptr; }
    return rc;
}
int qdsp_hip_xlate_fir_decim_cf32_process(void* h, const float* in, int count, float* out) {
    Engine* e = as_engine(h, KIND_VFO);
    return e ? (int)process_host(e, in, count, out) : QDSP_HIP_EINVAL;
}
int64_t qdsp_hip_xlate_fir_decim_cf32_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* s) {
    Engine* e = as_engine(h, KIND_VFO);
    return e ? process_dev(e, d_in, count, d_out, s) : QDSP_HIP_EINVAL;
}
int qdsp_hip_xlate_fir_decim_cf32_process_ex(void* h, const void* in, int in_dev, int count, void* out, int out_dev) {
    Engine* e = as_engine(h, KIND_VFO);
    return e ? (int)process_ex(e, in, in_dev, count, out, out_dev) : QDSP_HIP_EINVAL;
}
int qdsp_hip_xlate_fir_decim_cf32_configure(void* h, const float* taps, int ntaps, int interp, int decim) {
    Engine* e = as_engine(h, KIND_VFO);
    if (!e) return QDSP_HIP_EINVAL;
    int rc = configure(e, taps, ntaps, interp, decim);
    if (!rc && e->max_block) { int mb = e->max_block; e->max_block = 0; rc = ensure_io(e, mb); }
    return rc;
}
int qdsp_hip_xlate_fir_decim_cf32_set_phase_inc(void* h, float re, float im) {
    Engine* e = as_engine(h, KIND_VFO);
    if (!e || (re == 0.0f && im == 0.0f)) return QDSP_HIP_EINVAL;
    set_inc(e, re, im);
    return 0;
}
int qdsp_hip_xlate_fir_decim_cf32_get_phase(void* h, float* re, float* im) {
    Engine* e = as_engine(h, KIND_VFO);
    return e ? get_phase(e, re, im) : QDSP_HIP_EINVAL;
}
int qdsp_hip_xlate_fir_decim_cf32_set_phase(void* h, float re, float im) {
    Engine* e = as_engine(h, KIND_VFO);
    return e ? set_phase(e, re, im) : QDSP_HIP_EINVAL;
}
int qdsp_hip_xlate_fir_decim_cf32_advance(void* h, int64_t n) {
    Engine* e = as_engine(h, KIND_VFO);
    if (!e) return QDSP_HIP_EINVAL;
    apply_pending_inc(e);
    e->phase += (unsigned long long)n * e->dphase;
    e->raw_valid = false;
    return 0;
}
int qdsp_hip_xlate_fir_decim_cf32_set_volk_gain(void* h, int on) {
    Engine* e = as_engine(h, KIND_VFO);
    if (!e) return QDSP_HIP_EINVAL;
    e->volk_gain = on != 0;
    return 0;
}
int qdsp_hip_xlate_fir_decim_cf32_set_mode(void* h, int mode) {
    Engine* e = as_engine(h, KIND_VFO);
    if (!e || mode < 0 || mode > 2) return QDSP_HIP_EINVAL;
    e->fir_mode = mode;
    return 0;
}
int64_t qdsp_hip_xlate_fir_decim_cf32_out_size(void* h, int64_t count) {
    Engine* e = as_engine(h, KIND_VFO);
    return e ? out_size(e, count) : QDSP_HIP_EINVAL;
}
QDSP_FILTER_COMMON(qdsp_hip_xlate_fir_decim_cf32, KIND_VFO)

}  // extern "C"
