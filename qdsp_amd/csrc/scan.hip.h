// scan.hip.h -- what the rows run as a prefix scan share (deemp.hip, cagc.hip): the scan of one tile and the chunk geometry.
// A map type M supplies M::identity(), compose(later, earlier) and shfl_up(m, d).
#pragma once
#include "demod.hip.h"

namespace qk {

// tiles of kDemodNT lanes x kDemodSpl samples in a row of `count`
__host__ __device__ __forceinline__ long long scan_tiles_of(long long count) {
    return (count + (long long)kDemodNT * kDemodSpl - 1) / ((long long)kDemodNT * kDemodSpl);
}

// tiles (>= 1) -> T tiles per chunk and G chunks per row: one chunk for rows of at most row_tiles, else at most kAmMaxParts chunks
inline void scan_chunks(long long tiles, int row_tiles, long long* T, int* G) {
    const long long g0 = tiles <= row_tiles ? 1 : (tiles < kAmMaxParts ? tiles : kAmMaxParts);
    *T = (tiles + g0 - 1) / g0;
    *G = (int)((tiles + *T - 1) / *T);
}

// One tile: from every lane's own map, the map of all lanes before it (*ex) and of the whole tile (returned).  Hillis-Steele
// over the 64 lanes of a wave by cross-lane moves, then the kDemodNT / 64 wave totals through `wt`; always the same tree.
template <class M> __device__ __forceinline__ M tile_scan(const M& p, M* wt, M* ex) {
    constexpr int NW = kDemodNT / 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    M inc = p;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const M q = shfl_up(inc, d);
        if (lane >= d) inc = compose(inc, q);
    }
    if (lane == 63) wt[w] = inc;
    __syncthreads();
    M e = shfl_up(inc, 1);
    if (lane == 0) e = M::identity();
    M pre = M::identity(), tot = M::identity();
#pragma unroll
    for (int k = 0; k < NW; k++) {
        const M t = wt[k];
        if (k < w) pre = compose(t, pre);
        tot = compose(t, tot);
    }
    *ex = compose(e, pre);
    __syncthreads();   // (wt is written again by the next tile)
    return tot;
}

}  // namespace qk
