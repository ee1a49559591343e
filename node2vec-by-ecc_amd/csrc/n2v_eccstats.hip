// Eccentricity statistics: the per-item weights of EccenKNN (ir / ie / ire / ier) and the per-user ue — gfx950 (MI355X).
// C-ABI: include/n2v_sim.h.
//
// Reference: src/utils.py:53-153, a chain of pandas group-bys and merges over the ratings (uid, id, feedback, timewindow).
// Here it is a few segmented passes over the rows.  Every floating-point sum has ONE stated order (tests/
// eccstats_reference.py) and the kernels keep it, so their output is the restatement's bit for bit (the library is built
// with -ffp-contract=off): no float atomics and no tree reductions anywhere a rounded sum is formed.
//   groups     rows sorted by the (item, timewindow) key -> group number of every row, group boundaries, unum, the groups
//              of every item; three passes (heads per tile, scan of the tiles, numbering) with integer arithmetic only.
//   irg        irg[g] = table[unum[g]]: -log(count) comes from a host-built table (n2v_eccstats_log_table, the host's
//              libm log, which is Python's math.log); the device's log is not promised to equal it.
//   segsum     CSR segments: sum a[k] and sum a[k] * g[idx[k]], left to right.  Segments shorter than 64 take one lane each;
//              a longer one takes one wavefront, which loads 64 elements coalesced (the next 64 already in flight) and adds
//              them one after the other through v_readlane, so the serial part is the adds alone.
//   moments    global sum / mean / sum of squared deviations in the fixed two-level order: one wavefront per chunk of 4096
//              elements (the same readlane chain), then one wavefront over the chunk sums.  min / max by an order key.
//   finish     elementwise z, zero-one, product, quotient, quotient with +-inf -> 0.
#include <cmath>

#include "n2v_common.h"
#include "n2v_sim.h"

namespace {

constexpr int CHUNK = N2V_ECCSTATS_CHUNK;
constexpr int LONG_SEG = 64;      // a segment of at least this many elements takes a wavefront
constexpr int TILE = 2048;        // rows per workgroup of the group passes
constexpr int LONG_BLOCKS = 2048; // workgroups (4 wavefronts each) that share the long segments

// ---- the in-order chain -------------------------------------------------------------------------------------------------

__device__ __forceinline__ double lane_value(double v, int j) {           // j wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}
// acc += v[lane 0], v[lane 1], ... v[lane cnt - 1], one rounded add each; every lane ends with the same acc
__device__ __forceinline__ void chain(double& acc, double v, int cnt) {
    if (cnt == 64) {
#pragma unroll
        for (int j = 0; j < 64; ++j) acc = acc + lane_value(v, j);
    } else {
        for (int j = 0; j < cnt; ++j) acc = acc + lane_value(v, j);
    }
}
__device__ __forceinline__ void chain2(double& a0, double v0, double& a1, double v1, int cnt) {
    if (cnt == 64) {
#pragma unroll
        for (int j = 0; j < 64; ++j) { a0 = a0 + lane_value(v0, j); a1 = a1 + lane_value(v1, j); }
    } else {
        for (int j = 0; j < cnt; ++j) { a0 = a0 + lane_value(v0, j); a1 = a1 + lane_value(v1, j); }
    }
}

// ---- groups -------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool is_head(const int64_t* __restrict__ key, int64_t k) { return k == 0 || key[k] != key[k - 1]; }

__global__ void __launch_bounds__(256) heads_count_kernel(const int64_t* __restrict__ key, int64_t n, int64_t* __restrict__ tile_heads) {
    __shared__ int wave_cnt[4];
    const int t = threadIdx.x;
    int c = 0;
    for (int it = 0; it < TILE / 256; ++it) {
        const int64_t k = (int64_t)blockIdx.x * TILE + it * 256 + t;
        c += __popcll(__ballot(k < n && is_head(key, k)));              // the wavefront's count, in every lane
    }
    if ((t & 63) == 0) wave_cnt[t >> 6] = c;
    __syncthreads();
    if (t == 0) tile_heads[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// exclusive scan of the tile counts in place; counts[0] = number of groups, counts[1] = 0 (the largest unum comes later)
__global__ void __launch_bounds__(256) tile_scan_kernel(int64_t* __restrict__ tile_heads, int64_t n_tiles, int64_t* __restrict__ counts) {
    __shared__ int64_t part[256];
    const int t = threadIdx.x;
    const int64_t per = (n_tiles + 255) / 256;
    const int64_t lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += tile_heads[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) { const int64_t v = part[i]; part[i] = run; run += v; }
        counts[0] = run;
        counts[1] = 0;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t i = lo; i < hi; ++i) { const int64_t v = tile_heads[i]; tile_heads[i] = run; run += v; }
}

struct GroupArgs {
    const int64_t* key; const int64_t* perm; int64_t n; int64_t n_tw; int64_t n_items; const int64_t* tile_off;
    const int64_t* counts; int32_t* row_group; int64_t* group_begin; int64_t* item_gptr;
};

__global__ void __launch_bounds__(256) groups_number_kernel(GroupArgs a) {
    __shared__ int wave_cnt[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int64_t base = a.tile_off[blockIdx.x];                               // heads before this tile
    const int64_t n_groups = a.counts[0];
    for (int it = 0; it < TILE / 256; ++it) {
        const int64_t k = (int64_t)blockIdx.x * TILE + it * 256 + t;
        const bool head = k < a.n && is_head(a.key, k);
        const unsigned long long b = __ballot(head);
        if (lane == 0) wave_cnt[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; ++w) { before += w < wave ? wave_cnt[w] : 0; total += wave_cnt[w]; }
        __syncthreads();
        if (k < a.n) {
            const int64_t g = base + before + __popcll(b & ((2ull << lane) - 1)) - 1;   // heads up to and including k
            const int64_t p = a.perm[k];
            if (p >= 0 && p < a.n) a.row_group[p] = (int32_t)g;
            if (head) {
                a.group_begin[g] = k;
                const int64_t item = a.key[k] / a.n_tw, prev = k == 0 ? -1 : a.key[k - 1] / a.n_tw;
                const int64_t top = item < a.n_items ? item : a.n_items - 1;
                for (int64_t j = prev + 1 > 0 ? prev + 1 : 0; j <= top; ++j) a.item_gptr[j] = g;   // items without rows: empty
            }
            if (k == a.n - 1) {
                a.group_begin[n_groups] = a.n;
                const int64_t item = a.key[k] / a.n_tw;
                for (int64_t j = item + 1 > 0 ? item + 1 : 0; j <= a.n_items; ++j) a.item_gptr[j] = n_groups;
            }
        }
        base += total;
    }
}

__global__ void __launch_bounds__(256) unum_kernel(const int64_t* __restrict__ group_begin, int64_t* __restrict__ counts,
                                                   int64_t n, int64_t* __restrict__ unum) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n_groups = counts[0];
    long long c = 0;
    if (g < n_groups && g < n) { c = group_begin[g + 1] - group_begin[g]; unum[g] = c; }
    for (int off = 32; off; off >>= 1) { const long long o = __shfl_xor(c, off, 64); c = o > c ? o : c; }
    if ((threadIdx.x & 63) == 0 && c > 0) atomicMax(reinterpret_cast<long long*>(counts + 1), c);   // an integer: any order
}

__global__ void __launch_bounds__(256) irg_kernel(const int64_t* __restrict__ unum, int64_t n_groups, const double* __restrict__ table,
                                                  int64_t table_len, double* __restrict__ irg, int32_t* __restrict__ status) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const int64_t c = unum[g];
    if (c >= 1 && c < table_len) irg[g] = table[c];
    else { irg[g] = __builtin_nan(""); atomicOr(status, 1); }             // a count the table does not hold
}

// ---- segment sums -------------------------------------------------------------------------------------------------------

struct SegArgs {
    const int64_t* seg_ptr; int64_t n_seg; const int64_t* perm; const double* a; int64_t n_a; const int32_t* idx;
    const double* g; int64_t n_g; int mean; double* out_sum; double* out_wsum; int32_t* n_long; int32_t* long_list;
};

// element k of the concatenated segments: a[p] and a[p] * g[idx[p]], p = perm[k] (or k); anything out of range is a NaN
__device__ __forceinline__ void seg_element(const SegArgs& s, int64_t k, double& av, double& wv) {
    const int64_t p = s.perm ? s.perm[k] : k;
    av = __builtin_nan(""); wv = av;
    if (p < 0 || p >= s.n_a) return;
    av = s.a[p];
    if (!s.g) return;
    const int64_t j = s.idx ? (int64_t)s.idx[p] : p;
    if (j >= 0 && j < s.n_g) wv = av * s.g[j];                            // rounded before it is added
}

__device__ __forceinline__ void seg_store(const SegArgs& s, int64_t seg, int64_t len, double sum, double wsum) {
    if (s.out_sum) s.out_sum[seg] = s.mean ? sum / (double)len : sum;
    if (s.out_wsum) s.out_wsum[seg] = wsum;
}

__global__ void __launch_bounds__(256) seg_short_kernel(SegArgs s) {
    const int64_t seg = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (seg >= s.n_seg) return;
    const int64_t beg = s.seg_ptr[seg], end = s.seg_ptr[seg + 1], len = end - beg;
    if (len >= LONG_SEG) {                                                // a wavefront's: queue it (integer atomic; any order)
        s.long_list[atomicAdd(s.n_long, 1)] = (int32_t)seg;
        return;
    }
    double sum = 0.0, wsum = 0.0;
    for (int64_t k = beg; k < end; ++k) {
        double av, wv;
        seg_element(s, k, av, wv);
        sum = sum + av; wsum = wsum + wv;
    }
    seg_store(s, seg, len, sum, wsum);
}

__global__ void __launch_bounds__(256) seg_long_kernel(SegArgs s) {
    const int lane = threadIdx.x & 63;
    const int n_long = *s.n_long;
    const int n_waves = gridDim.x * 4;
    for (int w = n2v::uni(blockIdx.x * 4 + (threadIdx.x >> 6)); w < n_long; w += n_waves) {
        const int64_t seg = n2v::uni(s.long_list[w]);
        const int64_t beg = n2v::uni64(s.seg_ptr[seg]), end = n2v::uni64(s.seg_ptr[seg + 1]);
        double sum = 0.0, wsum = 0.0, av = 0.0, wv = 0.0, av2 = 0.0, wv2 = 0.0;
        if (beg + lane < end) seg_element(s, beg + lane, av, wv);
        for (int64_t base = beg; base < end; base += 64) {
            const int64_t nb = base + 64;
            if (nb + lane < end) seg_element(s, nb + lane, av2, wv2);     // in flight while this chunk is added
            const int cnt = end - base < 64 ? (int)(end - base) : 64;
            if (s.g) chain2(sum, av, wsum, wv, cnt);
            else chain(sum, av, cnt);
            av = av2; wv = wv2;
        }
        if (lane == 0) seg_store(s, seg, end - beg, sum, wsum);
    }
}

// ---- moments ------------------------------------------------------------------------------------------------------------

// larger double <=> larger key, -0.0 below +0.0; not for NaN
__device__ __forceinline__ unsigned long long total_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// stats: [0] sum [1] mean [2] sum of squared deviations [3] var [4] std [5] min [6] max [7] n
// partial: [0, n_chunks) chunk sums, [n_chunks, 2 n_chunks) chunk minima, [2 n_chunks, 3 n_chunks) chunk maxima
template <int DEV>
__global__ void __launch_bounds__(64) chunk_kernel(const double* __restrict__ x, int64_t n, int64_t n_chunks,
                                                   const double* __restrict__ stats, double* __restrict__ partial) {
    const int lane = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * CHUNK;
    const int left = n - c0 < CHUNK ? (int)(n - c0) : CHUNK;              // > 0
    const double m = DEV ? stats[1] : 0.0;
    double acc = 0.0;
    unsigned long long kmin = ~0ull, kmax = 0ull;
    bool nan = false;
    for (int b = 0; b < CHUNK / 64; b += 8) {
        if (b * 64 >= left) break;
        double v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int e = (b + r) * 64 + lane;
            v[r] = 0.0;
            if (e < left) {
                const double xv = x[c0 + e];
                if (DEV) { const double d = xv - m; v[r] = d * d; }
                else {
                    v[r] = xv;
                    if (xv != xv) nan = true;
                    else { const unsigned long long k = total_key(xv); kmin = k < kmin ? k : kmin; kmax = k > kmax ? k : kmax; }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int rest = left - (b + r) * 64;
            chain(acc, v[r], rest >= 64 ? 64 : (rest > 0 ? rest : 0));
        }
    }
    if (!DEV) {
        for (int off = 32; off; off >>= 1) {
            const unsigned long long a = __shfl_xor(kmin, off, 64), z = __shfl_xor(kmax, off, 64);
            kmin = a < kmin ? a : kmin; kmax = z > kmax ? z : kmax;
        }
        nan = __ballot(nan) != 0ull;
    }
    if (lane == 0) {
        partial[blockIdx.x] = acc;
        if (!DEV) {
            partial[n_chunks + blockIdx.x] = nan ? __builtin_nan("") : key_value(kmin);
            partial[2 * n_chunks + blockIdx.x] = nan ? __builtin_nan("") : key_value(kmax);
        }
    }
}

template <int DEV>
__global__ void __launch_bounds__(64) total_kernel(const double* __restrict__ partial, int64_t n_chunks, int64_t n,
                                                   double* __restrict__ stats) {
    const int lane = threadIdx.x;
    double acc = 0.0, v = 0.0, v2 = 0.0;
    unsigned long long kmin = ~0ull, kmax = 0ull;
    bool nan = false;
    if (lane < n_chunks) v = partial[lane];
    for (int64_t base = 0; base < n_chunks; base += 64) {
        if (base + 64 + lane < n_chunks) v2 = partial[base + 64 + lane];
        if (!DEV && base + lane < n_chunks) {
            const double lo = partial[n_chunks + base + lane], hi = partial[2 * n_chunks + base + lane];
            if (lo != lo || hi != hi) nan = true;
            else {
                const unsigned long long a = total_key(lo), z = total_key(hi);
                kmin = a < kmin ? a : kmin; kmax = z > kmax ? z : kmax;
            }
        }
        chain(acc, v, n_chunks - base < 64 ? (int)(n_chunks - base) : 64);
        v = v2;
    }
    if (!DEV) {
        for (int off = 32; off; off >>= 1) {
            const unsigned long long a = __shfl_xor(kmin, off, 64), z = __shfl_xor(kmax, off, 64);
            kmin = a < kmin ? a : kmin; kmax = z > kmax ? z : kmax;
        }
        nan = __ballot(nan) != 0ull;
    }
    if (lane != 0) return;
    if (!DEV) {
        stats[0] = acc;
        stats[1] = acc / (double)n;
        stats[5] = nan ? __builtin_nan("") : key_value(kmin);
        stats[6] = nan ? __builtin_nan("") : key_value(kmax);
        stats[7] = (double)n;
    } else {
        const double var = acc / (double)n;
        stats[2] = acc;
        stats[3] = var;
        stats[4] = sqrt(var);
    }
}

// ---- finish -------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) finish_kernel(int op, const double* __restrict__ a, const double* __restrict__ b,
                                                     const double* __restrict__ stats, int64_t n, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    double r;
    switch (op) {
    case N2V_ECCSTATS_Z: r = x - (stats[1] / stats[4]); break;           // x - (mean / std): the reference's precedence
    case N2V_ECCSTATS_ZERO_ONE: r = (x - stats[5]) / (stats[6] - stats[5]); break;
    case N2V_ECCSTATS_MUL: r = x * b[i]; break;
    case N2V_ECCSTATS_DIV: r = x / b[i]; break;
    default: r = x / b[i]; if (r == __builtin_inf() || r == -__builtin_inf()) r = 0.0; break;   // N2V_ECCSTATS_DIV_INF0
    }
    out[i] = r;
}

}  // namespace

extern "C" {

int n2v_eccstats_log_table(int64_t len, double* table) {
    if (len < 1 || !table) return n2v::fail(N2V_ERR_INVALID, "eccstats_log_table: len=%lld", (long long)len);
    table[0] = std::nan("");
    for (int64_t c = 1; c < len; ++c) table[c] = -std::log((double)c);
    return N2V_OK;
}

int64_t n2v_eccstats_groups_scratch(int64_t n) { return n < 1 ? 0 : (n + TILE - 1) / TILE; }

int n2v_eccstats_groups(const int64_t* key_sorted, const int64_t* perm, int64_t n, int64_t n_tw, int64_t n_items,
                        int64_t* scratch, int32_t* row_group, int64_t* group_begin, int64_t* unum, int64_t* item_gptr,
                        int64_t* counts, void* stream) {
    if (n < 1 || n > 0x7fffffff || n_tw < 1 || n_items < 1)
        return n2v::fail(N2V_ERR_INVALID, "eccstats_groups: n=%lld (1 .. 2^31-1) n_tw=%lld n_items=%lld", (long long)n, (long long)n_tw, (long long)n_items);
    if (!key_sorted || !perm || !scratch || !row_group || !group_begin || !unum || !item_gptr || !counts)
        return n2v::fail(N2V_ERR_INVALID, "eccstats_groups: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_tiles = (n + TILE - 1) / TILE;
    heads_count_kernel<<<(unsigned)n_tiles, 256, 0, s>>>(key_sorted, n, scratch);
    tile_scan_kernel<<<1, 256, 0, s>>>(scratch, n_tiles, counts);
    GroupArgs a{key_sorted, perm, n, n_tw, n_items, scratch, counts, row_group, group_begin, item_gptr};
    groups_number_kernel<<<(unsigned)n_tiles, 256, 0, s>>>(a);
    unum_kernel<<<n2v::grid_for(n, 256), 256, 0, s>>>(group_begin, counts, n, unum);
    return n2v::check_launch("eccstats_groups");
}

int n2v_eccstats_irg(const int64_t* unum, int64_t n_groups, const double* log_table, int64_t table_len, double* irg,
                     int32_t* status, void* stream) {
    if (n_groups < 1 || n_groups > 0x7fffffff || table_len < 1)
        return n2v::fail(N2V_ERR_INVALID, "eccstats_irg: n_groups=%lld table_len=%lld", (long long)n_groups, (long long)table_len);
    if (!unum || !log_table || !irg || !status) return n2v::fail(N2V_ERR_INVALID, "eccstats_irg: null pointer");
    irg_kernel<<<n2v::grid_for(n_groups, 256), 256, 0, (hipStream_t)stream>>>(unum, n_groups, log_table, table_len, irg, status);
    return n2v::check_launch("eccstats_irg");
}

int n2v_eccstats_segsum(const int64_t* seg_ptr, int64_t n_seg, const int64_t* perm, const double* a, int64_t n_a,
                        const int32_t* idx, const double* g, int64_t n_g, int32_t mean, int32_t* scratch, double* out_sum,
                        double* out_wsum, void* stream) {
    if (n_seg < 1 || n_seg > 0x7fffffff || n_a < 1 || (g && n_g < 1))
        return n2v::fail(N2V_ERR_INVALID, "eccstats_segsum: n_seg=%lld n_a=%lld n_g=%lld", (long long)n_seg, (long long)n_a, (long long)n_g);
    if (!seg_ptr || !a || !scratch || (!out_sum && !out_wsum) || (out_wsum && !g))
        return n2v::fail(N2V_ERR_INVALID, "eccstats_segsum: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(scratch, 0, sizeof(int32_t), s) != hipSuccess) return n2v::fail(N2V_ERR_HIP, "eccstats_segsum: memset failed");
    SegArgs sa{seg_ptr, n_seg, perm, a, n_a, idx, out_wsum ? g : nullptr, n_g, mean, out_sum, out_wsum, scratch, scratch + 1};
    seg_short_kernel<<<n2v::grid_for(n_seg, 256), 256, 0, s>>>(sa);
    const int64_t blocks = (n_seg + 3) / 4 < LONG_BLOCKS ? (n_seg + 3) / 4 : LONG_BLOCKS;
    seg_long_kernel<<<(unsigned)blocks, 256, 0, s>>>(sa);
    return n2v::check_launch("eccstats_segsum");
}

int64_t n2v_eccstats_moments_scratch(int64_t n) { return n < 1 ? 0 : 3 * ((n + CHUNK - 1) / CHUNK); }

int n2v_eccstats_moments(const double* x, int64_t n, double* scratch, double* stats, void* stream) {
    if (n < 1) return n2v::fail(N2V_ERR_INVALID, "eccstats_moments: n=%lld", (long long)n);
    if (!x || !scratch || !stats) return n2v::fail(N2V_ERR_INVALID, "eccstats_moments: null pointer");
    const int64_t n_chunks = (n + CHUNK - 1) / CHUNK;
    if (n_chunks > 0x7fffffff) return n2v::fail(N2V_ERR_INVALID, "eccstats_moments: n=%lld too large", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    chunk_kernel<0><<<(unsigned)n_chunks, 64, 0, s>>>(x, n, n_chunks, stats, scratch);
    total_kernel<0><<<1, 64, 0, s>>>(scratch, n_chunks, n, stats);
    chunk_kernel<1><<<(unsigned)n_chunks, 64, 0, s>>>(x, n, n_chunks, stats, scratch);
    total_kernel<1><<<1, 64, 0, s>>>(scratch, n_chunks, n, stats);
    return n2v::check_launch("eccstats_moments");
}

int n2v_eccstats_finish(int32_t op, const double* a, const double* b, const double* stats, int64_t n, double* out, void* stream) {
    if (n < 1) return n2v::fail(N2V_ERR_INVALID, "eccstats_finish: n=%lld", (long long)n);
    if (op < N2V_ECCSTATS_Z || op > N2V_ECCSTATS_DIV_INF0) return n2v::fail(N2V_ERR_INVALID, "eccstats_finish: op %d", op);
    const bool needs_stats = op == N2V_ECCSTATS_Z || op == N2V_ECCSTATS_ZERO_ONE;
    if (!a || !out || (needs_stats ? !stats : !b)) return n2v::fail(N2V_ERR_INVALID, "eccstats_finish: null pointer");
    finish_kernel<<<n2v::grid_for(n, 256), 256, 0, (hipStream_t)stream>>>(op, a, b, stats, n, out);
    return n2v::check_launch("eccstats_finish");
}

}  // extern "C"
