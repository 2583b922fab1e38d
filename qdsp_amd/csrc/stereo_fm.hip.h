// stereo_fm.hip.h -- StereoFMDemod (src/dsp/demodulator.h:189-330) over nchan channel rows (gfx950).  One run() of the reference is
//   m = FloatFMDemod(in);  f = FIR<float>(m, BlackmanBandpassWindow(1000, 1000, 19000, sampleRate));  p = AGC(f, 20, sampleRate);
//   d = p * p;  s = m * d;  out = {m + s, m - s}
// and has no loop that carries a value from one sample to the next but the FM phase.  Here one call is three ordinary launches on
// one stream, blockIdx.y = channel, tile = kDemodNT lanes x kDemodSpl consecutive samples as in demod.hip / level.hip:
//   fm_demod_kernel    (demod.hip, unchanged) writes the library-owned scratch m[nchan][count]
//   pilot_fir_kernel   f[i] = sum_k taps[k] m[i - (T - 1) + k], direct form.  A workgroup stages its 2048 + T - 1 inputs in LDS (the
//                      halo from the carried history where the tile starts before sample T - 1 of the call); a lane keeps a
//                      sliding register window over its 8 outputs: per 4 taps one 16-byte LDS read and 32 FMAs.  The taps are
//                      read with a wave-uniform index (scalar loads).  Every output is the same chain acc = fmaf(taps[k], x, acc),
//                      k = 0 .. T - 1 from +0.0f, so its bits are a function of the taps and the T samples under them alone.
//                      Lane l reads the 16-byte slots 2 l + k / 4: in a ds_read_b128 lane group two lanes meet on every other slot
//                      (2-way), by instruction counts 8 LDS cycles per wave and read against 128 VALU cycles for the 32 FMAs that
//                      follow it, so the plain map stays and no lane pays address arithmetic for a swizzle.  Measured
//                      (profiles/stereo_fm_rates.txt): on chip-filling calls the FMAs run at 0.9 to 1.0 of the v_fmac_f32 issue rate.
//                      One FP64 partial per workgroup: the maximum of its f under `x > m` from -inf (level_partial_kernel's rule).
//                      The workgroups over the last T - 1 samples write the next history (slot cur ^ 1; readers see slot cur).
//   stereo_mix_kernel  every workgroup folds its channel's partials in the same order, applies AGC's level update (agc_level of
//                      level.hip.h, cfr = 20.0f / sampleRate) and stores the matrix, every operation rounded to float; workgroup 0
//                      of a channel writes the next level.
// No workgroup waits for another.  m and f stay in library-owned scratch rows (16-byte aligned, `sstride` floats apart).
#pragma once
#include "level.hip.h"

namespace qk {

constexpr int kPilotMaxTaps = 4096;
constexpr int kPilotTile = kDemodNT * kDemodSpl;                  // outputs per workgroup
constexpr int kPilotLds = kPilotTile + kPilotMaxTaps + 16;        // floats: the tile, the halo, and the window's read-ahead

struct PilotArgs {
    const float* m;             // [nchan][sstride]
    float* f;                   // [nchan][sstride]
    const float* taps;          // [T], shared by all channels
    const float* hist;          // [nchan][T - 1] slot cur: the last T - 1 samples of m before this call
    float* hist_next;           // [nchan][T - 1] slot cur ^ 1
    double* part;               // [nchan][tiles]
    long long count, sstride;
    int T;
    int tiles;
};

struct MixArgs {
    const float* m;             // [nchan][sstride]
    const float* f;
    float* out;                 // stereo_t rows, out_stride samples apart
    const float* cfr;           // [nchan] 20.0f / sampleRate
    const float* level;         // [nchan] slot cur
    float* level_next;          // [nchan] slot cur ^ 1
    const double* part;         // [nchan][tiles]
    long long count, sstride, out_stride;
    int tiles;
    int vec;                    // 1: every output row 16-byte aligned
};

}  // namespace qk

namespace qh {

struct StereoFm : StreamOp {
    static constexpr OpKind kKind = OpKind::StereoFm;
    int ntaps = 0;
    float* d_phase[2] = {nullptr, nullptr};   // FM phase, history and level: read from slot cur, written to cur ^ 1
    float* d_hist[2] = {nullptr, nullptr};
    float* d_level[2] = {nullptr, nullptr};
    int cur = 0;
    float* d_speed = nullptr;              // [nchan] phasorSpeed
    float* d_cfr = nullptr;                // [nchan] 20.0f / sampleRate
    float* d_taps = nullptr;               // [kPilotMaxTaps]
    std::vector<float> speed, cfr;
    float* d_m = nullptr;                  // scratch rows, grown to the largest call seen
    float* d_f = nullptr;
    double* d_part = nullptr;
    long long scratch_cap = 0;             // samples per row
    long long last_count = 0, last_sstride = 0;
};

}  // namespace qh
