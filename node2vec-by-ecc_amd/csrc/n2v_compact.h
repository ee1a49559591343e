// The one stable compaction of the library (eccsplit: select / nodes / pairs; ecccons: join / feature rows) — gfx950.
// Three launches: ballots per tile -> one-workgroup exclusive scan of the tile counts (and the total) -> the same ballots
// again, every kept element written at tile offset + kept elements before it.  Workgroups meet only at the launch
// boundaries, so the output does not depend on the order in which they run.
#pragma once
#include "n2v_common.h"
#include "n2v_sim.h"

namespace n2v {

constexpr int COMPACT_TILE = N2V_ECCSPLIT_TILE;          // elements per workgroup of the compaction passes

// P: test(k) keeps element k; emit(k, slot) writes a kept element; skip(k) sees a dropped one.

template <class P>
__global__ void __launch_bounds__(256) compact_count_kernel(P p, int64_t n, int64_t* __restrict__ tile_cnt) {
    __shared__ int wave_cnt[4];
    const int t = threadIdx.x;
    int c = 0;
    for (int it = 0; it < COMPACT_TILE / 256; ++it) {
        const int64_t k = (int64_t)blockIdx.x * COMPACT_TILE + it * 256 + t;
        c += __popcll(__ballot(k < n && p.test(k)));                     // the wavefront's count, in every lane
    }
    if ((t & 63) == 0) wave_cnt[t >> 6] = c;
    __syncthreads();
    if (t == 0) tile_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// exclusive scan of the tile counts in place; *count = their sum
static __global__ void __launch_bounds__(256) compact_scan_kernel(int64_t* __restrict__ tile_cnt, int64_t n_tiles, int64_t* __restrict__ count) {
    __shared__ int64_t part[256];
    const int t = threadIdx.x;
    const int64_t per = (n_tiles + 255) / 256;
    const int64_t lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += tile_cnt[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) { const int64_t v = part[i]; part[i] = run; run += v; }
        *count = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t i = lo; i < hi; ++i) { const int64_t v = tile_cnt[i]; tile_cnt[i] = run; run += v; }
}

template <class P>
__global__ void __launch_bounds__(256) compact_scatter_kernel(P p, int64_t n, const int64_t* __restrict__ tile_off) {
    __shared__ int wave_cnt[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int64_t base = tile_off[blockIdx.x];                                 // kept elements before this tile
    for (int it = 0; it < COMPACT_TILE / 256; ++it) {
        const int64_t k = (int64_t)blockIdx.x * COMPACT_TILE + it * 256 + t;
        const bool keep = k < n && p.test(k);
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; ++w) { before += w < wave ? wave_cnt[w] : 0; total += wave_cnt[w]; }
        __syncthreads();
        if (keep) p.emit(k, base + before + __popcll(b & ((1ull << lane) - 1)));
        else if (k < n) p.skip(k);
        base += total;
    }
}

template <class P>
void compact(const P& p, int64_t n, int64_t* scratch, int64_t* count, hipStream_t s) {
    const int64_t n_tiles = (n + COMPACT_TILE - 1) / COMPACT_TILE;
    compact_count_kernel<P><<<(unsigned)n_tiles, 256, 0, s>>>(p, n, scratch);
    compact_scan_kernel<<<1, 256, 0, s>>>(scratch, n_tiles, count);
    compact_scatter_kernel<P><<<(unsigned)n_tiles, 256, 0, s>>>(p, n, scratch);
}

}  // namespace n2v
