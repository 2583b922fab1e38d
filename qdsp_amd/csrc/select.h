// select.h -- which kernel serves a call, and which tables a handle needs for it: pure functions of the handle's description, its
// plan, the call's size and the QDSP_HIP_* switches (knobs.h).  Plain C++ -- no HIP header, no kernel header -- so that a box
// without a GPU compiles and runs it (tests/fake_hip/select_selftest.cpp recomputes tests/golden/dispatch_map.txt with it).
// Nothing here writes anywhere but its return value.
//   plan_of(d)              once per configure(): the tap tables to build and the geometry of the MFMA plans (upload_taps fills them)
//   call_exceptions(d, n)   per call: what the measured tables (dispatch_table.inc, decim_table.inc) and the forcing switches say
//                           against the rule chain for a call of n samples; every predicate takes them as an argument
//   select(d, plan, n)      per call: the family process_dev launches
#pragma once
#include "kconst.h"
#include <stdint.h>

namespace qh {

enum Kind : int { KIND_FIR = 1, KIND_DECIM = 2, KIND_XLATE = 3, KIND_VFO = 4, KIND_CHAN = 5, KIND_SINE = 6 };

// What selection reads of a handle.
struct HandleDesc {
    Kind kind;
    int ch;                   // floats per sample
    bool rotate, has_filter;
    int L, M;                 // interp, decim
    int ntaps;                // prototype length
    int P;                    // taps per phase = ceil(ntaps / L)
    int fir_mode;             // 0 auto, 1 direct form, 2 overlap-save FFT (set_mode)
};

// Which forms of the taps a handle holds (upload_taps builds exactly these), with the geometry of the two MFMA plans.
struct Plan {
    bool core = false;        // d_taps in fir_core_kernel's branch-major layout (otherwise the phase table [L][P])
    bool win = false;         // decim_win_kernel's padded table
    bool lm = false;          // resamp_lm_kernel's sub-filter table
    struct Mf { int KJ = 0, QS = 1, keep2 = 0; } mf;      // MFMA decimator (mf_dec.hip.h), KJ == 0: none
    struct Rm {               // rational MFMA resampler (rm_resamp.hip.h), ngrp == 0: none
        int ngrp = 0, KB = 0, ext = 0, pitch = 0, G = 0, J = 1, qpb = 1;
        bool big_only = false;      // plan admitted by the round-3 extension of the rule: chip-filling calls only (rm_min_count)
    } rm;
};

// Per-call exceptions to the rule chain; default-constructed = the rule chain alone.
enum { VETO_WIN = 1, VETO_FFT1K = 2, VETO_PFB = 4, VETO_MF = 8 };
enum FirPick { PICK_NONE = 0, PICK_LAT = 1, PICK_CORE = 2, PICK_FFT1K = 3, PICK_FFT4K = 4 };
struct Exceptions {
    int veto = 0;             // integer decimators / fused VFO / real data, AUTO: kernels the measured table (decim_table.inc) takes away
    int mode = 0;             // ... or the mode it sets (explicit settings outrank it: mode_of)
    int pick = PICK_NONE;     // FIR<complex_t>, AUTO: the family the measured table (dispatch_table.inc) names, PICK_NONE = the rule chain
};

enum Family { F_XLATE, F_FIR_LAT, F_MFMA_DECIM, F_PFB, F_FFT1K, F_FFT4K, F_WIN, F_CORE, F_MFMA_RATIONAL, F_LM, F_ANY };

struct AnyPlan { int Pp, tap_bytes; bool pad; long long tile, span; int ks_lanes, ks_shift, ks_chunk; };

Plan plan_of(const HandleDesc& d);
Exceptions call_exceptions(const HandleDesc& d, int64_t count);
Family select(const HandleDesc& d, const Plan& plan, int64_t count);
AnyPlan any_plan(int L, int M, int P, int ch, long long nout = -1);

// chan_batch_wins (chan_ops.hip): a channel of this description has a kernel of its own that beats the general one on chip-filling calls
bool has_dedicated_form(const HandleDesc& d, int64_t count);

// geometry the launches share with the rules
int win_R(int M, int P);
int fft_dec(const HandleDesc& d);
inline int rm_c0(int b, int L0, int M0) { return (int)(((long long)(4 * b) * M0) / L0); }      // first band column of block b of the period matrix
inline int pfb_phases(int M) { return M == 4 ? 2 : 1; }
inline int pfb_Q(int M, int ntaps) { return (ntaps + M * (pfb_phases(M) - 1) + qk::kPfbD - 1) / qk::kPfbD; }

}  // namespace qh
