// rs_tables.h -- the host-side tables of the Reed-Solomon decoder (rs.hip.h): GF(2^8) exp / log, the parameter checks of
// qdsp_hip_rs_create, and the two CCSDS tables FalconRS uses, from their closed forms.  Plain C++, no HIP: the library and the
// tests' plain-loop fake both build their tables here.
#pragma once
#include <stdint.h>
#include <string.h>

namespace qrs {

constexpr int kN = 255;            // symbols per codeword: full-length codewords only
constexpr int kMaxRoots = 32;
constexpr int kMaxDepth = 8;
constexpr int kMaxSkip = 64;

// exp[i] = alpha^i for i < 512 (the wrap-around saves the modulo after adding two logarithms); log[alpha^i] = i for i = 1 .. 255,
// so log[1] = 255 and log[0] = 0 (never a valid logarithm: 0 marks a zero coefficient wherever logarithms are stored).
struct Field {
    uint8_t exp[512];
    uint8_t log[256];
};

// false: `poly` is not a primitive polynomial of degree 8 (9 bits, alpha = x generates all 255 non-zero elements)
inline bool field_build(int poly, Field& f) {
    if (poly < 0x100 || poly > 0x1ff) return false;
    memset(&f, 0, sizeof(f));
    unsigned e = 1;
    f.exp[0] = 1;
    for (int i = 1; i < 512; i++) {
        e <<= 1;
        if (e > 255) e ^= (unsigned)poly;
        f.exp[i] = (uint8_t)e;
        if (i < 256) f.log[e] = (uint8_t)i;
    }
    bool seen[256] = {};
    for (int i = 0; i < 255; i++) {
        const int v = f.exp[i];
        if (v == 0 || seen[v]) return false;
        seen[v] = true;
    }
    return true;
}

inline uint8_t field_mul(const Field& f, uint8_t a, uint8_t b) { return (a && b) ? f.exp[f.log[a] + f.log[b]] : 0; }

// g with (g * gap) % 255 == 1, or 0 where gcd(gap, 255) != 1
inline int gap_inverse(int gap) {
    for (int g = 1; g < 255; g++)
        if ((g * gap) % 255 == 1) return g;
    return 0;
}

struct Params {
    int poly = 0, first_root = 0, root_gap = 0, num_roots = 0, depth = 0, skip = 0, full_out = 0;
    int k = 0;                // message symbols per codeword
    int gap_inv = 0;
    int frame_in = 0;         // skip + 255 * depth
    int frame_out = 0;        // (full_out ? 255 : k) * depth
};

// the checks of qdsp_hip_rs_create on the code's parameters; fills the derived values
inline bool params_ok(Params& p, Field& f) {
    if (!field_build(p.poly, f)) return false;
    if (p.first_root < 0 || p.first_root > 255 || p.root_gap < 1 || p.root_gap > 254) return false;
    p.gap_inv = gap_inverse(p.root_gap);
    if (!p.gap_inv) return false;
    if (p.num_roots < 2 || p.num_roots > kMaxRoots || p.depth < 1 || p.depth > kMaxDepth || p.skip < 0 || p.skip > kMaxSkip) return false;
    if (p.full_out != 0 && p.full_out != 1) return false;
    p.k = kN - p.num_roots;
    p.frame_in = p.skip + kN * p.depth;
    p.frame_out = (p.full_out ? kN : p.k) * p.depth;
    return true;
}

// ---- CCSDS (FalconRS): primitive polynomial 0x187, first root 120, root gap 11, 16 roots, depth 5 behind a 4-byte sync word ----
constexpr int kCcsdsPoly = 0x187;

// The pseudo-randomiser: s[n + 8] = s[n] ^ s[n + 3] ^ s[n + 5] ^ s[n + 7] from eight ones, MSB first, 255 bytes (0xFF 0x48 0x0E ...)
inline void ccsds_randomizer(uint8_t out[255]) {
    uint8_t s[255 * 8 + 8];
    for (int i = 0; i < 8; i++) s[i] = 1;
    for (int n = 0; n + 8 < 255 * 8; n++) s[n + 8] = s[n] ^ s[n + 3] ^ s[n + 5] ^ s[n + 7];
    for (int b = 0; b < 255; b++) {
        unsigned v = 0;
        for (int j = 0; j < 8; j++) v = (v << 1) | s[8 * b + j];
        out[b] = (uint8_t)v;
    }
}

// Conventional -> dual basis: bit (7 - j) of to_db[x] is Tr(alpha^(117 j mod 255) x), Tr(y) = y + y^2 + ... + y^128 over 0x187;
// from_db is its inverse
inline void ccsds_dual_basis(uint8_t to_db[256], uint8_t from_db[256]) {
    Field f;
    field_build(kCcsdsPoly, f);
    for (int x = 0; x < 256; x++) {
        unsigned v = 0;
        for (int j = 0; j < 8; j++) {
            uint8_t y = field_mul(f, f.exp[(117 * j) % 255], (uint8_t)x), tr = 0;
            for (int i = 0; i < 8; i++) {
                tr ^= y;
                y = field_mul(f, y, y);
            }
            v |= (unsigned)(tr & 1) << (7 - j);     // (the trace lies in GF(2): 0 or 1)
        }
        to_db[x] = (uint8_t)v;
    }
    for (int x = 0; x < 256; x++) from_db[to_db[x]] = (uint8_t)x;
}

}  // namespace qrs
