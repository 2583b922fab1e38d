// select.cpp -- kernel selection and filter planning (select.h): the rules, the measured tables and the measurements behind them.
#include "select.h"
#include "knobs.h"
#include <vector>

namespace qh {

namespace {

// fir_core_kernel (de-interleaved tile): FIR and decimations up to 8.  From 9 on the general kernel with its
// staged-as-it-lies tile is 2-3x faster (scripts/tune_large_decim.py: M = 9..16, 31-255 taps: 0.12-0.38 ms per
// 2^26 samples against 0.26-0.54).
bool use_core(const HandleDesc& d) { return d.L == 1 && d.M <= 8 && !qk::knob(qk::K_FORCE_ANY, 0); }

int win_limit(int M) {
    static const int limit[17] = {0, 7, 150, 150, 160, 200, 256, 160, 200, 0, 192, 0, 224, 0, 0, 0, 256};
    return M >= 0 && M <= 16 ? limit[M] : 0;
}
bool use_win(const HandleDesc& d, const Exceptions& x) {
    if (!d.has_filter || d.L != 1) return false;
    const int M = d.M;
    if (!((M >= 1 && M <= 8) || M == 10 || M == 12 || M == 16)) return false;
    // where the overlap-save forms take over (per 2^26 samples they run 0.25 / 0.19 / 0.15 / 0.17 ms at decimation
    // 2 / 4 / 8 / 16 -- pruned inverse -- and 0.20-0.21 ms at every other decimation: full inverse, strided store)
    // ([1] = FIR<T> and equal-rate resamplers below the overlap-save threshold: 0.22 ms against 0.25 de-interleaved)
    const int max_taps = qk::knob(qk::K_WIN_MAX_TAPS, win_limit(M));
    return d.P <= max_taps && qk::knob(qk::K_NO_WIN, 0) == 0 && !(x.veto & VETO_WIN);
}

// interp / decim pairs served by resamp_lm_kernel (kernels.hip.h)
bool use_lm(const HandleDesc& d) {
    if (d.kind == KIND_FIR || !d.has_filter) return false;
    if (!(d.L == 2 || d.L == 3 || d.L == 4 || d.L == 5 || d.L == 10)) return false;
    return d.M >= 1 && d.M <= 8 && qk::knob(qk::K_NO_LM, 0) == 0;
}

// Shapes the MFMA decimator (mf_dec.hip.h) serves: complex data, interp 1, at most 16 taps per polyphase column (the 16
// rows of the A operand), decimation up to 128 (a tile of 16 rows is prefetched in registers).  Its time hardly depends
// on the tap count (0.21-0.25 ms per 2^27 samples from decimation 14 up, profiles/r02_tune_mf.md); below decimation 14
// the tiles get small and it only wins over the strided-window / general kernels from ~12 taps per unit of decimation,
// and the strided-window kernel keeps the short filters at decimation 16.
Plan::Mf mf_plan(const HandleDesc& d) {
    const Plan::Mf none;
    // (ch == 1, round 4: PolyphaseResampler<float> -- decim_mfma_real_kernel, the same plan on float rows)
    if ((d.ch != 2 && d.ch != 1) || (d.ch == 1 && d.rotate) || d.L != 1 || !d.has_filter || d.kind == KIND_FIR) return none;
    const int M = d.M, P = d.P;
    if (M < qk::knob(qk::K_MF_MIN_DECIM, 9)) return none;
    // decimations 130-256 (even): the kernel runs rows of M / 2 samples -- the decimator by M / 2 with the same taps -- and
    // keeps every other output; twice the matrix work for the outputs that count, on a unit that has the room
    const int k2 = (M > 8 * qk::kMfMaxKJ && M <= 16 * qk::kMfMaxKJ && M % 2 == 0) ? 1 : 0;
    const int Mk = k2 ? M / 2 : M;
    if (Mk > 8 * qk::kMfMaxKJ) return none;
    const int Q = (P + Mk - 1) / Mk;                  // taps per column: one set of 16 rows of the A operand, or two
    if (Q > qk::kMfMaxQ) return none;
    if (Q > 16 && M < 12) return none;       // (two tap sets on rows of < 12 samples: 0.44 ms per 2^27 at decimation 10 against 0.36 overlap-save, round 3)
    if (M < 14 && P < 12 * M) return none;
    if (P < M) return none;                           // (fewer taps than the decimation: most of each row meets no tap, the general kernel is 5-16 % ahead)
    if (use_win(d, Exceptions()) && P < 6 * M) return none;
    return Plan::Mf{(Mk + 7) / 8, Q > 16 ? 2 : 1, k2};
}

// Rational MFMA resampler (rm_resamp.hip.h): the banded period matrix W[i][c] = phases[(i M) % L][c - (i M) / L], cut
// into blocks of 4 rows (16 blocks per MFMA step) with one band per block, in the lane order of the A operand.
// Periods too short to hold their band in one row are merged J at a time (L' = J L, M' = J M: the same operator).
Plan::Rm rm_plan(const HandleDesc& d) {
    Plan::Rm rm;
    // Where it pays (profiles/r02_tune_rm.md): periods of at least 9 blocks (interp >= 33: 48 kHz <-> 44.1 kHz runs 1.25-1.5x
    // faster than through the general direct kernel), pure interpolators, and the decimating side of the small ratios
    // resamp_lm_kernel serves (decim >= 5, and 10/3: 1.2-2.2x at up to ~24 taps per phase).  Other short periods share a step
    // between period quads and run within +-15 % of the general kernel, which keeps them (QDSP_HIP_RM_MIN_INTERP lowers
    // the bar).
    bool rm_wanted = d.L >= qk::knob(qk::K_RM_MIN_INTERP, 33) || (d.M == 1 && d.L >= 6 && !use_lm(d));
    if (use_lm(d) && d.L >= 2)
        rm_wanted = rm_wanted || (d.M >= 5 && d.P <= (d.L == 10 ? 36 : 24)) || (d.L == 10 && d.M >= 3 && d.P <= 24);
    // Round 3 (scripts/sweep_rm_grid.py, profiles/r03_sweep_rm_grid.txt: 130 ratios x 8-32 taps per phase on 2^26-sample calls): the block
    // form is ahead of the general direct kernel on nearly every ratio from 14 taps per phase on (x 0.5-0.9 of its time; 72 of 79 ratios at
    // 14 taps per phase, 60 at 12 with losses up to x 1.25, at 8 anything from x 0.7 to x 1.4), and of resamp_lm_kernel on its decimating side up to 32 taps per phase (3/8: x 0.49, 5/8:
    // x 0.53, 4/7: x 0.61) and on 4/3, 5/3, 5/4 from 16 taps per phase (x 0.73-0.97); resamp_lm_kernel keeps decimations 1-2,
    // 2/3 and 3/4 (x 1.05-2.2).  These plans only serve chip-filling calls (rm_min_count): their reference-sized calls stay where
    // round 2's survey put them.
    if (!rm_wanted && d.L >= 2 && !qk::knob(qk::K_NO_RM_EXT, 0)) {
        bool ext;
        if (use_lm(d))
            ext = (d.M >= 5 && d.P <= 36) || (d.L == 10 && d.M >= 3 && d.P <= 36) ||
                  ((d.M == 3 || d.M == 4) && d.L >= 4 && d.P >= 16 && d.P <= 32);      // (3/4: x 0.90-0.94 at 16 / 24 taps per phase, x 1.2 at 20: left alone)
        else      // (7/6, 9/7, 9/8 at 16 taps per phase: x 1.04-1.17, the only losers of that column)
            ext = d.M >= 2 && d.P >= 14 && !(d.P < 20 && ((d.L == 7 && d.M == 6) || (d.L == 9 && (d.M == 7 || d.M == 8))));
        if (ext) {
            rm_wanted = true;
            rm.big_only = true;
        }
    }
    // (ch == 1, round 4: PolyphaseResampler<float> -- resamp_mfma_real_kernel, the same plan on float tiles.  Against the real-data forms of the other
    // kernels -- scripts/sweep_real_rational.py forced, profiles/r04_real_rational.txt -- it wins on chip-filling calls at every tap count (147/160 with
    // 8 / 12 taps per phase: x 0.63 / 0.54 of their time) but for 33/32 below 14 taps per phase (x 1.05-1.10); small calls: rm_min_count)
    if (d.ch == 1 && rm_wanted && d.P < 14 && d.L >= 33 && d.L < 48) rm_wanted = false;
    if (!((d.ch == 2 || (d.ch == 1 && !d.rotate)) && rm_wanted && d.has_filter && d.kind != KIND_FIR && !use_core(d) && d.M < (1 << 16))) return rm;
    const int L0 = d.L, M0 = d.M, P = d.P;
    for (int J = 1; J <= 64; J++) {
        const int L = J * L0, M = J * M0, nblk = (L + 3) / 4;
        if (nblk > 16 * qk::kRmMaxGrp || 4 * M > 64 * qk::kRmNE) break;
        const int qpb = nblk <= 8 ? 16 / nblk : 1, ngrp = (nblk + 15) / 16;
        std::vector<int> c0((size_t)nblk);      // first band column of block b (rm_c0)
        int KB = 1, reach = 0;
        for (int b = 0; b < nblk; b++) {
            const int i0 = 4 * b, i1 = (i0 + 3 < L - 1) ? i0 + 3 : L - 1;
            c0[b] = rm_c0(b, L0, M0);
            const int need = (int)(((long long)i1 * M0) / L0) + P - c0[b];
            if (need > KB) KB = need;
        }
        if (KB > qk::kRmMaxKB) break;
        for (int b = 0; b < nblk; b++)
            if (c0[b] + KB > reach) reach = c0[b] + KB;
        const int ext = reach > M ? reach - M : 0;
        if (ext > M) continue;                     // a row must hold its band with one neighbour's head: merge more periods
        // used fraction of the 16 blocks of a step: below ~0.6 the general direct kernel is the faster one
        const double used = (double)(nblk * qpb) / (16.0 * ngrp);
        if (used < 0.6) continue;                  // (more merged periods may fill the steps better)
        int pitch = M + ext;
        pitch += (pitch & 1) ^ 1;                  // odd: the four periods of a quad start on different banks
        if (d.ch == 1) {      // (complex data: the same search changes nothing -- 0.4155 / 0.4378 / 0.4394 against 0.4139 / 0.4415 / 0.4431 ms, alternated)
            // Real data: the B operand of a step is one ds_read_b32 per lane -- 32-lane groups, bank = sample index mod 32 -- from sample
            // (period l % 4) * pitch + c0[block l / 4] + k.  PMC of resamp_mfma_real_kernel at the odd pitch: LDS 70 % busy, a third of it bank
            // conflicts (profiles/r04_pmc_resamp_mfma_real.json).  Of the 32 pitches from M + ext on, take the one whose lane groups meet the
            // fewest busy banks (the float tiles are half the size of the complex ones: the longer rows cost nothing that matters).
            int best_cost = 1 << 30;
            for (int cand = M + ext; cand < M + ext + 32; cand++) {
                int cost = 0;
                for (int g = 0; g < ngrp; g++)
                    for (int half = 0; half < 2; half++) {
                        int busy[32] = {0}, worst = 0;
                        for (int l = 32 * half; l < 32 * half + 32; l++) {
                            const int slot = l / 4;
                            const int b = ngrp > 1 || qpb == 1 ? 16 * g + slot : slot % nblk;
                            const int pq = ngrp > 1 || qpb == 1 ? 0 : slot / nblk;
                            const int sidx = ((4 * pq + l % 4) * cand + (b < nblk ? c0[b] : 0)) & 31;
                            if (++busy[sidx] > worst) worst = busy[sidx];
                        }
                        cost += worst;
                    }
                if (cost < best_cost) { best_cost = cost; pitch = cand; }
            }
        }
        // period quads per tile: as many as the register prefetch (kRmNE samples per lane) holds, a multiple of qpb
        int G = (64 * qk::kRmNE - ext) / (4 * M);
        if (G > 16) G = 16;
        G -= G % qpb;
        if (G < 1 || qk::rm_lds_bytes(ngrp, KB, G, pitch, d.ch == 1) > 64 * 1024) continue;
        rm = Plan::Rm{ngrp, KB, ext, pitch, G, J, qpb, rm.big_only};
        break;
    }
    return rm;
}

// explicit settings (set_mode, QDSP_HIP_FIR_MODE) outrank the table's per-call mode
int mode_of(const HandleDesc& d, const Exceptions& x) {
    if (d.fir_mode) return d.fir_mode;
    const int k = qk::knob(qk::K_FIR_MODE, 0);
    return k ? k : x.mode;
}

// ---- FIR<complex_t>, AUTO: which kernel family serves a call of `count` samples with `ntaps` taps -------------------------------------------
// Round 4: this one choice is DATA, not an if-chain.  scripts/sweep_fir_table.py times the four families on a grid of
// call sizes x tap counts (each forced with QDSP_HIP_FIR_PICK), scripts/gen_dispatch_table.py turns the committed sweep
// (profiles/r04_sweep_fir_table.txt) into dispatch_table.inc -- one byte per cell: the fastest family -- tests/test_capi_cpu.py checks that the
// table is the sweep's, tests/test_gpu_dispatch.py re-measures a fixed sample of cells and fails when the default is > 10 % behind an alternative.
// A call takes the nearest cell (log2 of the count, log of the taps); a family that cannot serve the shape (structural limits in the *_eligible
// predicates) hands the call back to the rule chain.
#include "dispatch_table.inc"
// The switch settings the decimator sweep tries (scripts/sweep_decim_table.py lists them in the same order): what each one vetoes / which mode it sets.
constexpr int kDecimSettingVeto[16] = {0, VETO_WIN, VETO_FFT1K, VETO_WIN | VETO_FFT1K, 0, 0, VETO_PFB, VETO_PFB, VETO_MF, 0, 0, 0, 0, 0, 0, 0};
constexpr int kDecimSettingMode[16] = {0, 0, 0, 0, 1, 2, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0};
#include "decim_table.inc"
int decim_table_setting(int rot, int M, int ntaps, int64_t count) {   // rot: the table's class -- 0 complex decimator, 1 fused VFO, 2 real data
    if (qk::knob(qk::K_NO_DECIM_TABLE, 0) || count <= 0 || rot >= kDecimTabClasses) return 0;
    // the decimation's row: below 10 the swept decimation itself or none (the kernel families change from one small decimation to the next: 6 on
    // 5's row lost 40 % where the rules were right); from 10 on -- general direct kernel, overlap-save, MFMA decimator at every decimation -- the
    // swept decimation nearest on a log scale (12 -> 10, 40 -> 32, 80 -> 64), inside the swept range.  The settings only take kernels AWAY from
    // the rule chain or name the family, so a neighbour's setting is always valid; tests/test_gpu_dispatch.py holds unswept decimations to
    // the same 10 % as swept ones.
    if (M < kDecimTabM[0] || M > kDecimTabM[kDecimTabMs - 1] || ntaps < kDecimTabTaps[0] / 2) return 0;
    int mi = -1;
    for (int i = 0; i < kDecimTabMs; i++)
        if (kDecimTabM[i] == M) mi = i;
    for (int i = 1; i < kDecimTabMs && mi < 0; i++)
        if (kDecimTabM[i - 1] >= 10 && M > kDecimTabM[i - 1] && M < kDecimTabM[i])
            mi = (long long)M * M >= (long long)kDecimTabM[i - 1] * kDecimTabM[i] ? i : i - 1;      // (the geometric mean is the border)
    if (mi < 0) return 0;
    int lg = 0;
    while ((int64_t(1) << (lg + 1)) <= count) lg++;
    if (count - (int64_t(1) << lg) > (int64_t(1) << lg) * 0.41421356) lg++;
    int row = lg - kDecimTabLog2Min;
    row = row < 0 ? 0 : row >= kDecimTabRows ? kDecimTabRows - 1 : row;
    int col = 0;
    for (int c = 1; c < kDecimTabCols; c++)
        if ((double)ntaps * ntaps >= (double)kDecimTabTaps[c - 1] * kDecimTabTaps[c]) col = c;
    return kDecimTab[rot][mi][row][col];
}
int fir_table_pick(int64_t count, int ntaps) {
    if (count <= 0 || ntaps < kFirPickTaps[0]) return PICK_NONE;
    int lg = 0;
    while ((int64_t(1) << (lg + 1)) <= count) lg++;                   // floor(log2 count)
    if (count - (int64_t(1) << lg) > (int64_t(1) << lg) * 0.41421356) lg++;   // nearest power of two on a log scale (sqrt 2)
    int row = lg - kFirPickLog2Min;
    row = row < 0 ? 0 : row >= kFirPickRows ? kFirPickRows - 1 : row;
    int col = 0;
    for (int c = 1; c < kFirPickCols; c++)                            // nearest grid point on a log scale: the geometric mean is the border
        if ((double)ntaps * ntaps >= (double)kFirPickTaps[c - 1] * kFirPickTaps[c]) col = c;
    return kFirPick[row][col];
}

// Large decimations (the VFO's usual job: 2.4 Msps -> 48 kHz is M = 50) with the few taps per output such
// filters have: the general direct kernel streams the input once and does P/M MACs per input sample, while the
// overlap-save form pays a full 4096-point transform pair whatever M (0.20-0.22 ms per 2^26 samples, 0.25-0.28
// with the fused NCO).  Measured (scripts/tune_large_decim.py, M = 9..250, 31..1001 taps): the direct form takes
// 0.12-0.17 ms up to ~9 taps per input-sample-of-decimation and ~320 taps (tiles shrink with M: LDS holds
// tile * M samples), and the NCO costs it 0.015 ms instead of 0.055; 2-way bank conflicts (M = 2 mod 4) move
// the crossover down.
bool any_direct_wins(const HandleDesc& d) {
    if (d.L != 1 || d.ch != 2) return false;
    const AnyPlan pl = any_plan(1, d.M, d.P, d.ch);
    if (pl.tile == 0) return false;
    // tiles of 64 outputs and fewer (M >= 64 or so) split every output's taps over 4-16 lanes: 0.12-0.26 ms up to
    // 2001 taps at ~8 taps per unit of decimation (the reference VFO's own design rule) against 0.22-0.41
    if (pl.ks_lanes) return d.P <= (d.rotate ? 12 : 10) * d.M;
    const int per_m = (d.M & 3) == 2 ? (d.rotate ? 10 : 7) : (d.rotate ? 15 : 9);
    const int max_taps = d.rotate ? 512 : 320;
    return d.P <= per_m * d.M && d.P <= max_taps;
}

// ---- overlap-save on 1024-point segments, one wave each (fft1k_fir.hip) --------------------------------
// Reference-sized calls: a lone 4096-point segment takes its workgroup ~12 us whatever else runs (8 barriers), so a
// call that cannot fill the chip four workgroups deep is better off as 4x as many independent one-wave segments.
// Bounds: complex data, interp 1, taps up to half a segment; calls from the first size the 4096-point form is
// picked for up to QDSP_HIP_FFT1K_MAX_COUNT (measured crossover, scripts/tune_call_size.py).
bool fft1k_eligible(const HandleDesc& d, const Exceptions& x, int64_t count) {
    if (d.L != 1 || d.ntaps < 2 || d.ntaps > 769) return false;   // (769 taps: a quarter of every segment is new)
    if (d.kind != KIND_FIR && d.kind != KIND_DECIM && d.kind != KIND_VFO) return false;
    if (d.ch != 2 && (d.kind == KIND_VFO || d.rotate || qk::knob(qk::K_NO_FFT1K_REAL, 0))) return false;   // real data: two real segments per wave
    const int mode = mode_of(d, x);
    if (mode != 0 || qk::knob(qk::K_NO_FFT1K, 0) || (x.veto & VETO_FFT1K)) return false;
    if (x.pick) return x.pick == PICK_FFT1K;
    const int forced = qk::knob(qk::K_FFT1K_MAX_COUNT, -1);
    if (forced >= 0) return count <= forced;
    // measured crossovers against the 4096-point kernels (scripts/tune_fft1k.py, profiles/r02_tune_fft1k.txt): the
    // overlap grows with the taps (1024 - ntaps + 1 new points per segment), decimations 2 / 4 / 8 / 16 have the
    // pruned inverse on the other side, the fused NCO costs this form 32 more complex products per lane
    if (d.ch == 1) {
        // real data (two real segments per wave): the other side is fir_fft_kernel<1, false, REAL> with its full inverse at every
        // decimation -- 256 taps: FIR 59.6 against 69.9 us at 2^25 samples, decimate-by-8 115.8 against 152.2 at 2^26
        if (d.ntaps > 513) return count <= (1 << 20);
        if (d.kind == KIND_FIR) return count <= (d.ntaps <= 128 ? 1 << 27 : d.ntaps <= 288 ? 1 << 25 : d.ntaps <= 416 ? 1 << 24 : 1 << 23);
        return count <= (d.ntaps <= 288 ? 1 << 27 : d.ntaps <= 416 ? 1 << 26 : 1 << 25);
    }
    const bool pruned = d.kind != KIND_FIR && (d.M == 2 || d.M == 4 || d.M == 8 || d.M == 16);
    int64_t lim = d.ntaps <= 128 ? 6 << 20 : d.ntaps <= 288 ? 4 << 20 : d.ntaps <= 416 ? 3 << 20 : d.ntaps <= 513 ? 2 << 20 : pruned ? 1 << 18 : 1 << 19;
    if (pruned && d.ntaps <= 513) lim = d.ntaps <= 288 ? 3 << 20 : 3 << 19;
    if (d.rotate && (pruned || d.ntaps > 288) && d.ntaps <= 513) lim = 3 << 19;
    return count <= lim;
}

constexpr int kFftMaxTaps = 2049;   // keeps >= 2048 valid outputs per 4096-point block

bool fft_eligible(const HandleDesc& d, const Exceptions& x, int64_t count) {
    if (!fft_dec(d)) return false;
    int mode = mode_of(d, x);
    if (mode == 1) return false;
    if (mode == 2) return true;
    if (x.pick) return x.pick == PICK_FFT1K || x.pick == PICK_FFT4K;
    // auto: calls big enough to fill the chip with 4096-point segments, and filters past the measured
    // crossover of the two forms
    // real data (two segments per transform, 305 Gs/s whatever the taps at 2^26 samples): the direct form
    // moves half the bytes per sample and stays ahead to ~96 taps (445 Gs/s at 63, 164 at 256); a real
    // decimator keeps 1/M of a full inverse, so the direct form wins until ~32 taps per branch
    // (decimate-by-8, 256 taps: 324 vs 321 Gs/s)
    int min_taps;
    if (d.ch == 1) {
        // Chip-filling calls (round 3, profiles/r03_sweep_real.txt, 2^27 real samples): the overlap-save form costs 0.23-0.28 ms at any
        // length; against it the direct form stays ahead to 64 taps (FIR), 128-192 taps at decimation 2-5, 384 at decimation 8, the
        // strided-window kernel to its own limits at decimation 10 / 12 / 16 -- and nothing else serves the decimations in between:
        // round 2's 32 taps per unit of decimation left decimate-by-10 with 256 taps on the general kernel at 0.56 ms (now 0.26).
        const bool big = count >= (1 << 22);
        min_taps = qk::knob(qk::K_FFT_MIN_TAPS_REAL, big && d.M == 1 ? 64 : 96);
        if (d.M > 1) {
            int need = 32 * d.M;
            if (big) {
                static const int t[9] = {0, 0, 144, 128, 192, 176, 224, 224, 384};
                // (swept: decimations 1-5, 8, 10, 12, 16 -- profiles/r03_sweep_real.txt; past 16 the round-2 rule stays: ADVICE round 3)
                need = d.M <= 8 ? t[d.M] : win_limit(d.M) ? win_limit(d.M) + 1 : d.M <= 16 ? 128 : 32 * d.M;
            }
            if (min_taps < need) min_taps = need;
        }
    } else if (d.M == 1 && d.kind != KIND_FIR) {
        // equal-rate resampler / pure xlating FIR: full inverse + per-element store (0.52 ms per 2^27 samples)
        // against the tile-per-block direct form (0.51 ms at 7 taps, 0.63 at 63)
        min_taps = 24;
    } else if (d.M == 1) {
        // FIR: the overlap-save kernel (a copy-speed 4.8 TB/s whatever the taps) beats the tile-per-block
        // direct form from 8 taps on (2^26 samples: 0.222 vs 0.256 ms at 7 taps, 0.225 vs 0.394 at 127)
        min_taps = 8;
        // reference-sized calls (<= 1e6 samples, stream.h:7) are latency-bound: one 4096-point segment takes ~9 us
        // whatever the taps, the direct form 4.7 / 5.7 us at 31 / 63 taps (8.3 at 1e6 samples) and 11-16 us at 256
        // (round 2: with one-wave 1024-point segments -- fft1k_fir.hip -- the small calls cross over at ~24 taps:
        // 31 taps x 1e6 samples 6.8 us against 7.2, 95 taps x 262144 5.7 against 6.9; profiles/r02_tune_fft1k.txt)
        if (count < (1 << 21) && min_taps < 96) min_taps = qk::knob(qk::K_FFT_MIN_TAPS_SMALL, fft1k_eligible(d, x, count) ? 24 : 96);
    } else {
        if (d.M >= 9 && !use_win(d, x) && any_direct_wins(d)) return false;
        // decimators (scripts/tune_small.py, profiles/r01_tune_small.txt): the direct form slows down with the
        // decimation (LDS-capacity-bound de-interleaved tiles): M = 2 / 4 / 5 it wins to ~110 taps
        // (0.20 / 0.16 / 0.18 ms vs 0.24 / 0.18 / 0.22), from M = 7 the overlap-save form wins at any length
        // (M = 8: 0.16 vs 0.25-0.29 ms; M = 16: 0.17 vs 0.45-0.49 ms)
        const int dflt = d.M >= 7 ? 2 : 112;
        min_taps = qk::knob(qk::K_FFT_MIN_TAPS_DECIM, dflt);
    }
    // (below 2^16 samples a 4096-point segment per workgroup leaves most of the chip idle; one-wave segments go down to 2^14)
    // (... and further where the alternative is fir_core_kernel on a long filter: 256-400 taps at decimation 3 / 8, 2048-16 000
    // samples: 10-13 us against 5.6-5.9; the FIR itself has fir_lat_kernel there)
    // Long filters outside that kernel's range (more than 769 taps): the direct kernels cost 4-7.5e-6 us per tap and
    // sample (1500 taps x 4096 samples: 49 us; 1000 taps at decimation 7: 29 us up to 65 534 samples), one 4096-point
    // segment 9.5-12 us whatever it holds: from 2^21 tap-samples on the segment wins (the decimators' direct kernel does not
    // get cheaper with the decimation: its time follows the taps a lane walks through)
    int64_t min_count = 1 << 16;
    if (fft1k_eligible(d, x, count)) {
        // (FIR<complex_t> has fir_lat_kernel below 2^24 tap-samples; FIR<float> only fir_core_kernel: 3.4 us + 4e-6 per tap and sample)
        if (d.kind != KIND_FIR) min_count = 64;
        else if (d.ch == 2) min_count = d.ntaps > 320 ? 64 : 1 << 14;
        else min_count = (1 << 19) / d.ntaps < 1024 ? 1024 : (1 << 19) / d.ntaps;
    }
    if (min_count == (1 << 16) && d.ntaps >= 256) {
        const int64_t by_work = (1 << 21) / d.ntaps;
        min_count = by_work < 1024 ? 1024 : by_work;
    }
    return d.ntaps >= min_taps && count >= ((int)min_count);
}

// ---- polyphase overlap-save decimate-by-8 (pfb_dec.hip) ---------------------------------------------
// Serves PolyphaseResampler<complex_t> / the fused VFO with interp 1, decim 8 on calls big enough to fill the chip
// with one segment per wave (8 waves per CU: measured crossover against the per-segment fir_fft_kernel<8> in
// scripts/tune_call_size.py).
// (round 3: decimate by 4 as TWO output phases over the same eight columns, pfb_dec.hip: taps per column counted with the odd
// outputs' four-sample delay)
bool pfb_eligible(const HandleDesc& d, const Exceptions& x, int64_t count) {
    // (ch == 1, round 4: PolyphaseResampler<float> at decimation 8 / 4 -- pfb_dec8_real_kernel / pfb_dec4_real_kernel, two real segments per set of transforms)
    const bool real8 = d.ch == 1 && !d.rotate && (d.M == qk::kPfbD || d.M == 4) && d.kind == KIND_DECIM;
    if ((d.ch != 2 && !real8) || d.L != 1 || (d.M != qk::kPfbD && d.M != 4) || d.ntaps < 2) return false;
    if (d.kind != KIND_DECIM && d.kind != KIND_VFO) return false;
    if (pfb_Q(d.M, d.ntaps) > qk::kPfbMaxQ) return false;
    if (qk::knob(qk::K_NO_PFB, 0) || (x.veto & VETO_PFB)) return false;
    // measured crossover (scripts/tune_pfb_threshold.py, 256 taps): a lone segment takes a wave ~7 us (15 us per call
    // with the table load) where fir_fft_kernel<8> needs 8 us, so the per-segment kernels keep the reference-sized
    // calls; from 2^23 samples (decimator) / 2^24 (fused VFO) on this form is ahead, 1.2x at 2^27
    // (never below one segment: the kernel's prefetch reads whole 4096-sample segments from a clamped in-range start)
    if (count < qk::kPfbSeg) return false;
    // (decimate by 4, profiles/r03_tune_pfb4.txt: level with fir_fft_dec_kernel<4> at 2^25 samples, 0.166 against 0.181 ms at 2^26, 0.312 against 0.330 at 2^27)
    return count >= (int64_t)qk::knob(qk::K_PFB_MIN_COUNT, d.M == 4 ? 1 << 26 : (d.rotate || real8) ? 1 << 24 : 1 << 23);      // (real data: pairs of segments)
}

// FIR<complex_t> on reference-sized calls: the direct form arranged for latency (fir_lat.hip.h), bit-identical to
// fir_core_kernel.  Per call at 256 taps the overlap-save kernel takes 9.0-9.3 us at 16 384-262 144 samples and
// fir_core_kernel 11.3+ (profiles/r02_tune_call_size.txt).
bool fir_lat_eligible(const HandleDesc& d, const Exceptions& x, int64_t count) {
    if (d.kind != KIND_FIR || d.ch != 2 || !d.has_filter || d.L != 1 || d.M != 1) return false;
    if (d.ntaps > 1024 || qk::knob(qk::K_NO_FIR_LAT, 0)) return false;
    if (x.pick) return x.pick == PICK_LAT && count > 0;      // the measured table has spoken (dispatch_table.inc)
    // (a wave walks all taps of its 64 outputs: 600 taps take 9.3 us on 4096 samples, the one-wave overlap-save kernel 5.6)
    if (d.ntaps > 320 && fft1k_eligible(d, x, count)) return false;
    // measured: 2.5 us + 1.7e-7 us per tap and sample (63 / 127 / 256 taps at 65 536 samples: 2.9 / 3.6 / 5.3 us); what it
    // competes with is the overlap-save kernel (~9 us up to 262 144 samples) from 96 taps on, fir_core_kernel (5.7-6.1 us) below
    // -- and, for up to 769 taps, the one-wave-per-segment overlap-save kernel (5.2-5.9 us up to 262 144 samples whatever the taps)
    const int64_t limit = qk::knob(qk::K_FIR_LAT_MAX_WORK, d.ntaps > 769 ? 1 << 25 : 1 << 24);
    return count > 0 && count * (int64_t)d.ntaps <= limit;
}

// Smallest call the MFMA kernels take (profiles/r02_tune_call_size_mfma.txt).  Their waves set up operand tables, slot
// maps and an FP64 phasor before the first tile and then walk their tiles one after the other, so on a reference-sized
// block (<= 1e6 samples, src/dsp/stream.h:7) the general direct kernel is 1-3 us quicker wherever a wave's tile is large
// (decimations past 32, periods of >= 33 outputs); the crossover sits at 2-5e6 samples -- 1.4e7 for the decimations
// run at half the row length -- and from there on the MFMA kernels are 1.3-2x faster.  Short rows (decimation <= 32)
// and the small rational ratios are quicker at every size.
int64_t mf_min_count(const HandleDesc& d, const Plan::Mf& mf) {
    const int v = qk::knob(qk::K_MF_MIN_COUNT, -1);
    if (v >= 0) return v;
    if (mf.keep2) return 1 << 24;
    // (filters of at most three taps per unit of decimation: two or three tap rows of the operand in use -- the general kernel is 10-25 % ahead at
    // 2^22 samples, level at 2^24; profiles/r03_sweep_mid.txt)
    if (d.P <= 3 * d.M) return 8 << 20;
    if (mf.QS == 2 || mf.KJ > 4) return 3 << 20;
    return 0;
}
int64_t rm_min_count(const HandleDesc& d, const Plan::Rm& rm) {
    const int v = qk::knob(qk::K_RM_MIN_COUNT, -1);
    if (v >= 0) return v;
    // (profiles/r03_sweep_rm_grid.txt, second part: decimating ratios are ahead from 2^22 input samples; interpolating ones -- whose work follows
    // the OUTPUT count -- only from ~10 million inputs: 8/3 at 6.3 million x 1.2, at 12.6 million x 0.9)
    int64_t base = rm.big_only ? (d.L > d.M ? 12 << 20 : 1 << 22) : (d.L >= 33 ? 6 << 20 : 0);
    if (d.ch == 1) {
        // real data (profiles/r04_real_rational.txt): interpolating ratios only pay from 2^25 samples on (6/1 at 2^20: 2-3.3x slower than the general
        // kernel, at 2^23 1.07-1.23x, at 2^26 0.53-0.74x; 48/5 at 2^23 1.09-1.33x; 160/147 level at 2^23); the decimating ones at every size up
        // to 19 taps per phase, from 2^22 samples beyond that (3/8 with 20 taps per phase at 2^20: 1.31x)
        if (d.L > d.M && base < (1 << 25)) base = 1 << 25;
        if (d.L < d.M && d.P >= 20 && base < (1 << 22)) base = 1 << 22;
    }
    return base;
}

// Reference-sized calls of the small-interpolation resamplers: resamp_lm_kernel gives every lane R x L accumulators over all
// P taps -- the throughput form (0.27-0.30 ms per 2^26 samples where the general kernel needs 0.43-0.60) -- so a call
// too small to fill the chip takes as long as ONE lane's chain: 6.5 us at 32 taps per phase, 14 us at 67 (3/7, 200
// taps), 24-28 us at 128 (5/8, 640 taps) or on 10/7, whatever the size up to ~1e6 samples.  The general kernel with
// its call-sized tiles (any_plan) takes 4.0-4.7 us there and grows with outputs x taps.  Measured crossovers
// (profiles/r02_tune_small_resamp.txt), in outputs of the call: 16 384 x taps per phase at decimation 3-4, 2x that from
// decimation 5, 2.5x at decimation 1-2, never beyond 2^20 outputs; filters under 16 taps per phase stay (3.8-4.5 us).
// (interp 10, decim 7 past the MFMA kernel's tap range: the general kernel at every size -- 0.58 against 0.74 ms per 2^26)
bool lm_yields_to_any(const HandleDesc& d, int64_t nout) {
    if (qk::knob(qk::K_NO_LM_SMALL_CALL_RULE, 0)) return false;
    if (d.L == 10 && d.M == 7) return true;
    if (d.P < 16) return false;
    int64_t lim = (int64_t)d.P * (d.M >= 5 ? 32768 : d.M >= 3 ? 16384 : 40960);
    if (lim > (1 << 20)) lim = 1 << 20;
    return nout <= lim;
}

// The strided-window decimator on reference-sized calls: 6.0-8.2 us per call at 95-127 taps (decimation 2 / 4 / 8) where
// the one-wave overlap-save kernel takes 5.5 whatever the taps; from ~1e6 samples on the window kernel is ahead again
// (profiles/r02_tune_fft1k.txt).
bool win_yields_to_fft1k(const HandleDesc& d, const Exceptions& x, int64_t count) {
    if (d.ch != 2 || d.ntaps < 96 || count > (1 << 19)) return false;   // (real data: 5.6-6.8 us against 7.1-8.3)
    return fft1k_eligible(d, x, count);
}

// The strided-window decimator on chip-filling calls (round 3, scripts/tune_dec_small.py, profiles/r03_tune_win_vs_fft.txt, 2^27 samples):
// its time grows with the taps (decimation 2: 0.32 ms at 48 taps, 0.53 at 128) while the overlap-save forms cost the same at any
// length -- 0.48 / 0.38 / 0.33 ms at decimation 2 / 3 / 4, pfb_dec8_kernel 0.24-0.25 at decimation 8 -- so past the measured
// crossovers the big calls go there (decimation 8, 160 taps: 0.30 -> 0.25 ms, fused VFO 0.35 -> 0.25; decimation 2, 144 taps:
// 0.57 -> 0.48).  use_win()'s limits, measured on 2^26-sample calls in round 1, keep the smaller calls.
bool win_yields_to_fft_big(const HandleDesc& d, const Exceptions& x, int64_t count) {
    if (d.ch != 2) return false;
    const int M = d.M, P = d.P;
    if (M == 8) return pfb_eligible(d, x, count) && P >= (d.rotate ? 56 : 88);
    // (at 2^24 samples the window kernel is still ahead at decimation 3-5 -- 0.046-0.049 against 0.053-0.055 ms at 112-160 taps --
    // and level at decimation 2)
    if (M == 2) return count >= (1 << 24) && P >= 104;
    if (M == 3 || M == 4) return count >= (1 << 26) && P >= 104;
    if (M == 5) return count >= (1 << 26) && !d.rotate && P >= 152;
    if (M == 6) return count >= (1 << 26) && !d.rotate && P >= 208;      // (256 taps: 0.455 against 0.37 ms; level at 192)
    return false;
}

// Real data, chip-filling calls (same sweep): the de-interleaved direct kernel moves 4-byte samples at decimation 2 / 4 faster than the
// strided window does (decimation 2: 0.14-0.25 against 0.18-0.36 ms at 32-128 taps; decimation 4: 0.12-0.18 against 0.15-0.23), and from
// ~100 taps at decimation 5 / 8.
bool real_win_yields_to_core_big(const HandleDesc& d, int64_t count) {
    if (d.ch != 1 || count < (1 << 22) || !use_core(d)) return false;
    return d.M == 2 || d.M == 4 || (d.M == 5 && d.P >= 96) || (d.M == 8 && d.P >= 128);
}

}  // namespace

// decimators served by decim_win_kernel (kernels.hip.h): interp 1, short filters.  Outputs per lane and the
// tap limit from scripts/tune_win.py / tune_small.py (2^26 samples): chunks of M*R <= 10 samples are the sweet
// spot; past ~100-128 taps the overlap-save kernels take over (their pruned forms at M = 4, 8, 16 earlier).
int win_R(int M, int P) {
    const int r = qk::knob(qk::K_WIN_R, 0);      // experiments: 1, 2, 4 or 8 where instantiated
    if (r == 1 || r == 2 || r == 4 || r == 8) return r;
    if (M == 1) return 8;
    if (M <= 3) return 4;
    if (M == 4) return P > 96 ? 4 : 2;
    if (M <= 6) return 2;
    if (M == 8) return P > 63 ? 2 : 1;
    return 1;
}

// DEC the overlap-save kernel would run with for this engine, 0 if it cannot: 1 = full inverse
// (the FIR, and any other integer decimation through a strided store), 2/4/8/16 = pruned inverse.
int fft_dec(const HandleDesc& d) {
    if (d.L != 1 || d.ntaps < 2 || d.ntaps > kFftMaxTaps) return 0;
    if (d.ch == 1) {
        // real data: two real segments per complex transform (full inverse; decimators keep every M-th output)
        if (d.kind == KIND_FIR) return 1;
        if (d.kind == KIND_DECIM) return 1;
        return 0;
    }
    if (d.kind == KIND_FIR) return 1;
    if (d.kind == KIND_DECIM || d.kind == KIND_VFO) {
        if (d.M == 2 || d.M == 4 || d.M == 8 || d.M == 16) return d.M;
        return 1;   // any other decimation, 1 included (the pure xlating FIR / a resampler at equal rates)
    }
    return 0;
}

// Tile plan of resamp_any_kernel: phase-table pitch and bytes in LDS (0: table stays in memory), padded layout,
// outputs per tile (0: the taps of one phase do not fit) and the LDS elements a tile stages.
AnyPlan any_plan(int L, int M, int P, int ch, long long nout) {
    constexpr int NT = 256;
    AnyPlan p;
    // the phase table rides in LDS when it leaves at least half of the budget to the samples
    p.Pp = (P + 3) & ~3;
    if (((p.Pp >> 2) & 1) == 0) p.Pp += 4;
    const long long tap_bytes = (long long)L * p.Pp * (long long)sizeof(float);
    const bool lt = tap_bytes <= kMaxDynLds / 2;
    p.tap_bytes = lt ? (int)tap_bytes : 0;
    // Tile = as many outputs as keep the staged input span inside what is left of the LDS budget.
    const long long max_elems = (kMaxDynLds - p.tap_bytes) / (ch * (int)sizeof(float));
    long long tile = (long long)8 * NT;
    // interp 1 with a decimation that is a multiple of 4: lane windows M samples apart share LDS banks (4-way and
    // worse) -> one pad element per M samples
    p.pad = L == 1 && (M & 3) == 0 && M <= 65536;
    auto span_of = [&](long long t) {
        const long long sp = ((t - 1) * M) / L + P + 2;
        return p.pad ? sp + sp / M + 1 : sp;
    };
    // interp 1 with a tile of at most a quarter of the workgroup: NT / tile lanes share an output's taps (NT partial
    // sums behind the samples).  Two lanes per output (tile 128) measured no better than one: the extra barrier
    // and LDS round trip cost what the halved tap loop saves (M = 50, 201 taps: 0.162 vs 0.145 ms).
    constexpr int kSplitTile = NT / 4;
    const bool ks_ok = L == 1 && P >= 64;
    auto need = [&](long long t) { return span_of(t) + ((ks_ok && t <= kSplitTile) ? NT : 0); };
    while (tile > 1 && need(tile) > max_elems) tile /= 2;
    // reference-sized calls (nout known): 2048 outputs per tile leave a 1e6-sample block of a 24/125 audio resampler on 94
    // workgroups and a 16 384-sample one on 2 (10.3 us per call whatever the size); one to four outputs per lane spread it
    if (nout >= 0) {
        const long long want = qk::knob(qk::K_ANY_SMALL_CALL_TILES, 512);   // (256 .. 4096 measured: 147/160 at 1e6 samples 9.5 / 9.1 / 10.0 / 11.2 us)
        while (tile > NT && (nout + tile - 1) / tile < want) tile /= 2;
        // large decimations (taps split over the lanes of an output): down to 16 outputs per tile = 16 lanes per output, as long
        // as a lane keeps 16 taps -- the VFO's 401 taps / 50 on a 1e6-sample block: 100 dependent MACs per lane -> 25
        if (ks_ok && want > 0) {
            if (tile > kSplitTile && (nout + kSplitTile - 1) / kSplitTile <= 768 && P >= 64) tile = kSplitTile;
            // (... and as long as the halved tiles still fit one round of the chip: the NCO variant keeps 3 workgroups per CU
            // resident, and a 769th workgroup waits for a whole round -- 401-513 taps / 40-64 on 1e6 samples: 9.4-9.5 us with
            // 783-978 tiles against 7.3-7.4 with 392-490)
            const long long tmin = 16;
            while (tile > tmin && tile <= kSplitTile && (nout + tile - 1) / tile < want && (nout + tile / 2 - 1) / (tile / 2) <= 768 &&
                   P / (2 * NT / tile) >= 16)
                tile /= 2;
        }
    }
    // a half-workgroup tile with a long tap loop: the quarter tile with four lanes per output is faster (M = 50,
    // 401 taps: 0.24 -> 0.17 ms) unless it stages too little per lane (M = 32: 9 samples in batches of 8)
    if (ks_ok && tile == 2 * kSplitTile && P >= 192 && M >= 40) tile = kSplitTile;
    p.tile = need(tile) > max_elems ? 0 : tile;
    p.span = span_of(tile);
    p.ks_lanes = p.ks_shift = p.ks_chunk = 0;
    if (ks_ok && p.tile >= 1 && p.tile <= kSplitTile && (p.tile & (p.tile - 1)) == 0) {
        p.ks_lanes = (int)(NT / p.tile);
        while ((1 << p.ks_shift) < p.tile) p.ks_shift++;
        p.ks_chunk = (((P + p.ks_lanes - 1) / p.ks_lanes) + 3) & ~3;
    }
    return p;
}

// Planned with the rule chain alone: a handle's tables do not depend on the calls it serves.
Plan plan_of(const HandleDesc& d) {
    Plan p;
    p.core = use_core(d);
    p.win = use_win(d, Exceptions());
    p.lm = use_lm(d);
    p.mf = mf_plan(d);
    p.rm = rm_plan(d);
    return p;
}

Exceptions call_exceptions(const HandleDesc& d, int64_t count) {
    Exceptions x;
    const bool cplx_dec = (d.kind == KIND_DECIM || d.kind == KIND_VFO) && d.ch == 2 && d.M >= 2;
    const bool real_any = (d.kind == KIND_DECIM || d.kind == KIND_FIR) && d.ch == 1 && !d.rotate;
    if ((cplx_dec || real_any) && d.has_filter && d.L == 1 && d.fir_mode == 0 && qk::knob(qk::K_FIR_MODE, 0) == 0) {
        // Integer decimators and the fused VFO on complex data, FIR / decimators on real data: the rule chain decides, EXCEPT where the measured table
        // (decim_table.inc <- profiles/r04_sweep_decim_table.txt, scripts/gen_dispatch_table.py) found one of eight switch settings more than
        // 4 % faster in the call's cell.  QDSP_HIP_DECIM_SETTING = 1..8 forces a setting (the sweep, the regression test), 0 = rules only.
        const int forced = qk::knob(qk::K_DECIM_SETTING, -1);
        const int setting = forced >= 0 ? forced : decim_table_setting(real_any ? 2 : d.rotate ? 1 : 0, d.M, d.ntaps, count);
        x.veto = kDecimSettingVeto[setting & 15];
        x.mode = kDecimSettingMode[setting & 15];
    }
    if (d.kind == KIND_FIR && d.ch == 2 && d.has_filter && mode_of(d, x) == 0) {
        const int forced = qk::knob(qk::K_FIR_PICK, 0);               // 1..4: the sweep and the regression test force a family
        x.pick = forced >= PICK_LAT && forced <= PICK_FFT4K ? forced : qk::knob(qk::K_NO_FIR_TABLE, 0) ? PICK_NONE : fir_table_pick(count, d.ntaps);
        // (QDSP_HIP_FFT1K_MAX_COUNT, the tests' way of pinning the 4096-point kernels at oracle-sized inputs, outranks the table)
        if (x.pick == PICK_FFT1K && !forced) {
            const int cap = qk::knob(qk::K_FFT1K_MAX_COUNT, -1);
            if ((cap >= 0 && count > cap) || qk::knob(qk::K_NO_FFT1K, 0)) x.pick = PICK_FFT4K;
        }
        // structural limits of the family named: none for the direct form; the others fall back to the rule chain
        if ((x.pick == PICK_LAT && d.ntaps > 1024) || (x.pick == PICK_FFT1K && d.ntaps > 769) ||
            ((x.pick == PICK_FFT1K || x.pick == PICK_FFT4K) && !fft_dec(d)))
            x.pick = PICK_NONE;
    }
    return x;
}

// The rule chain, first match wins.  A family needs both its rule at call time and its table from plan time: the switches may have
// changed in between (QDSP_HIP_FORCE_ANY set after the plan was made), and a handle never launches on a table it does not hold.
Family select(const HandleDesc& d, const Plan& plan, int64_t count) {
    if (!d.has_filter) return F_XLATE;
    const Exceptions x = call_exceptions(d, count);
    const int64_t nout = (count * d.L) / d.M;      // calcOutSize, resampling.h:95-97 (L = M = 1 for FIR)
    const bool automatic = mode_of(d, x) == 0;
    if (automatic && fir_lat_eligible(d, x, count)) return F_FIR_LAT;
    // large integer decimations (the VFO's usual job) as an FP32 matrix product on the MFMA units (mf_dec.hip.h)
    if (plan.mf.KJ && automatic && nout > 0 && count >= mf_min_count(d, plan.mf) && !qk::knob(qk::K_NO_MF, 0) && !(x.veto & VETO_MF)) return F_MFMA_DECIM;
    // AUTO only: QDSP_HIP_FIR_DIRECT keeps meaning fir_core_kernel (the form the bit-exactness tests pin),
    // QDSP_HIP_FIR_FFT the overlap-save kernels
    const bool win = automatic && plan.win && use_win(d, x);
    if (fft_eligible(d, x, count) && !(win && !win_yields_to_fft1k(d, x, count) && !win_yields_to_fft_big(d, x, count)))
        return pfb_eligible(d, x, count) ? F_PFB : fft1k_eligible(d, x, count) ? F_FFT1K : F_FFT4K;
    if (win && !real_win_yields_to_core_big(d, count)) return F_WIN;
    if (plan.core && use_core(d)) return F_CORE;      // (plan.core: d_taps has this kernel's layout -- a handle planned under QDSP_HIP_FORCE_ANY has not)
    // rational ratios with interp >= 6 (48 kHz <-> 44.1 kHz is 147 / 160) on the MFMA units (rm_resamp.hip.h)
    if (plan.rm.ngrp && automatic && nout > 0 && count >= rm_min_count(d, plan.rm) && !qk::knob(qk::K_NO_RM, 0)) return F_MFMA_RATIONAL;
    if (plan.lm && use_lm(d) && !(automatic && lm_yields_to_any(d, nout))) return F_LM;
    return F_ANY;
}

bool has_dedicated_form(const HandleDesc& d, int64_t count) {
    return fft_eligible(d, Exceptions(), count) || use_win(d, Exceptions()) || use_core(d) || use_lm(d);
}

}  // namespace qh
