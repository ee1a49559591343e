// Random forests on binned features (include/n2v_sim.h, n2v_forest_*): the last stage of src/main_ecc.py:160-202.
// The definition is tests/forest_reference.py; every accumulated quantity is an integer, so the tables equal it bit for bit.
//
//   edges      one wavefront per feature over its sorted column: count the distinct values; at most n_bins of them: all but
//              the first, else the distinct ones among the n_bins - 1 quantile picks.  Ballot compaction keeps the order.
//   bin        one thread per (sample, feature): binary search of the number of edges <= x.
//   bootstrap  one thread per draw, int32 atomic add on the drawn sample's weight.
//   hist       the hot path.  Samples stay partitioned by node (order[], seg[]); a workgroup takes PIECE positions of the
//              batch and a tile of features, and for each node its piece meets: zero LDS, accumulate with LDS integer
//              atomics (threads = sample slots x features of the tile, so one sample's tile is one contiguous read and the
//              lanes of one sample hit different addresses), flush the non-zero cells with global integer atomics.
//   split      one wavefront per (node, feature): each lane scans 4 consecutive bins, a wave scan joins them, the score of
//              every threshold, a wave argmax (higher score, then lower bin), the next occupied bin for the gap middle.
//              Then one thread per node takes the features in ascending order (strictly greater wins).
//   route      flags (left / right per position), a scan outside, then the scatter: a stable partition per split node.
//   predict    one lane per (sample, value column): walks every tree in ascending order, adds the leaf value, divides.
#include <cmath>
#include <cstdint>

#include "n2v_common.h"
#include "n2v_sim.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr int PIECE = N2V_FOREST_PIECE;
constexpr int HIST_LDS = N2V_FOREST_HIST_LDS;
constexpr int KEY_SHIFT = 12;                       // F <= 4096: a feature's key is (philox word << 12) | feature

int feature_tile(int n_bins, int n_classes) {
    const int per_feature = n_bins * (n_classes > 0 ? 4 * n_classes : 12);
    int tile = 64;
    while (tile > 1 && tile * per_feature > HIST_LDS) tile >>= 1;
    return tile;
}

// the largest m in [0, n_seg) with seg[m] <= p; segments are not empty
__device__ __forceinline__ int segment_of(const int32_t* __restrict__ seg, int n_seg, int p) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(BLOCK) void check_x_kernel(const double* __restrict__ x, int64_t count, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < count && x[i] != x[i]) atomicOr(status, N2V_FOREST_BAD_NAN);
}

__global__ __launch_bounds__(BLOCK) void check_u8_kernel(const uint8_t* __restrict__ a, int64_t count, int32_t limit,
                                                         int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < count && (int32_t)a[i] >= limit) atomicOr(status, N2V_FOREST_BAD_BIN);
}

__global__ __launch_bounds__(BLOCK) void check_i32_kernel(const int32_t* __restrict__ a, int64_t count, int32_t limit, int32_t bit,
                                                          int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < count && (a[i] < 0 || a[i] >= limit)) atomicOr(status, bit);
}

__global__ __launch_bounds__(BLOCK) void check_tree_kernel(const int32_t* __restrict__ feature, const int32_t* __restrict__ threshold,
                                                           const int32_t* __restrict__ left, const int64_t* __restrict__ tree_ptr,
                                                           int32_t n_trees, int32_t n_features, int32_t n_bins,
                                                           int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= tree_ptr[n_trees]) return;
    int lo = 0, hi = n_trees - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tree_ptr[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const int64_t local = i - tree_ptr[lo], size = tree_ptr[lo + 1] - tree_ptr[lo];
    const int32_t l = left[i];
    if (l == -1) return;
    int32_t bad = 0;
    if (l <= local || (int64_t)l + 1 >= size) bad |= N2V_FOREST_BAD_CHILD;
    if (feature[i] < 0 || feature[i] >= n_features) bad |= N2V_FOREST_BAD_FEATURE;
    if (threshold[i] < 0 || threshold[i] >= n_bins) bad |= N2V_FOREST_BAD_BIN;
    if (bad) atomicOr(status, bad);
}

// ---- bins ---------------------------------------------------------------------------------------------------------------

// lane-ordered compaction of one flag per lane: returns this lane's slot and advances *count (uniform)
__device__ __forceinline__ int wave_slot(bool keep, int& count) {
    const uint64_t mask = __ballot(keep);
    const int lane = threadIdx.x & (WAVE - 1);
    const int slot = count + __popcll(mask & ((1ull << lane) - 1ull));
    count += __popcll(mask);
    return slot;
}

__global__ __launch_bounds__(WAVE) void edges_kernel(const double* __restrict__ xs, int64_t n, int32_t n_bins, double* __restrict__ edges,
                                                     int32_t* __restrict__ n_edges) {
    const int lane = threadIdx.x;
    const double* col = xs + (int64_t)blockIdx.x * n;
    double* out = edges + (int64_t)blockIdx.x * (n_bins - 1);
    int64_t distinct = 0;
    for (int64_t i = lane; i < n; i += WAVE) distinct += (i == 0 || col[i] != col[i - 1]) ? 1 : 0;
    for (int d = 32; d; d >>= 1) distinct += __shfl_xor(distinct, d, WAVE);
    int count = 0;
    if (distinct <= n_bins) {
        for (int64_t base = 1; base < n; base += WAVE) {
            const int64_t i = base + lane;
            const bool keep = i < n && col[i] != col[i - 1];
            const int slot = wave_slot(keep, count);
            if (keep) out[slot] = col[i];                     // slot < distinct - 1 <= n_bins - 1
        }
    } else {
        for (int base = 1; base < n_bins; base += WAVE) {
            const int b = base + lane;
            bool keep = false;
            double q = 0.0;
            if (b < n_bins) {
                q = col[((int64_t)b * n) / n_bins];
                keep = b == 1 || q != col[((int64_t)(b - 1) * n) / n_bins];
            }
            const int slot = wave_slot(keep, count);
            if (keep) out[slot] = q;
        }
    }
    if (lane == 0) n_edges[blockIdx.x] = count;
}

__global__ __launch_bounds__(BLOCK) void bin_kernel(const double* __restrict__ x, int64_t count, int32_t n_features, int32_t n_bins,
                                                    const double* __restrict__ edges, const int32_t* __restrict__ n_edges,
                                                    uint8_t* __restrict__ bins, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count) return;
    const int f = (int)(i % n_features);
    const double v = x[i];
    if (v != v) {
        atomicOr(status, N2V_FOREST_BAD_NAN);
        bins[i] = 0;
        return;
    }
    const double* e = edges + (int64_t)f * (n_bins - 1);
    int lo = 0, hi = n_edges[f];
    hi = hi < 0 ? 0 : (hi > n_bins - 1 ? n_bins - 1 : hi);
    while (lo < hi) {                                          // the number of edges <= v
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    bins[i] = (uint8_t)lo;
}

__global__ __launch_bounds__(BLOCK) void bootstrap_kernel(uint64_t seed, uint32_t tree, int64_t n, int32_t* __restrict__ w) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    uint32_t r[4];
    n2v::philox4x32_10(seed, (uint32_t)k, (uint32_t)((uint64_t)k >> 32), tree, N2V_FOREST_STREAM_BOOT, r);
    atomicAdd(&w[((uint64_t)r[0] * (uint64_t)n) >> 32], 1);
}

__global__ __launch_bounds__(BLOCK) void quantise_kernel(const double* __restrict__ y, int64_t n, double scale, int64_t* __restrict__ yq,
                                                         unsigned long long* __restrict__ max_abs, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double q = rint(y[i] * scale);
    if (!(fabs(q) < 9007199254740992.0)) {                     // NaN, infinity or beyond 2^53
        atomicOr(status, N2V_FOREST_BAD_TARGET);
        yq[i] = 0;
        return;
    }
    const int64_t v = (int64_t)q;
    yq[i] = v;
    atomicMax(max_abs, (unsigned long long)(v < 0 ? -v : v));
}

__global__ __launch_bounds__(BLOCK) void keys_kernel(uint64_t seed, uint32_t tree, uint32_t node0, int64_t count, int32_t n_features,
                                                     int64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count) return;
    const uint32_t j = (uint32_t)(i % n_features), v = node0 + (uint32_t)(i / n_features);
    uint32_t r[4];
    n2v::philox4x32_10(seed, v, j, tree, N2V_FOREST_STREAM_FEAT, r);
    keys[i] = (int64_t)(((uint64_t)r[0] << KEY_SHIFT) | j);
}

// ---- histogram ------------------------------------------------------------------------------------------------------------

// Global layout: regressor int64 [node][feature][bin][2] = (count, sum); classifier int32 [node][feature][bin][class].
// LDS layout: cell = bin * tile + feature of the tile; regressor int64 sums[cells] then int32 counts[cells]; classifier
// int32 [cells][K].
template <bool CLS>
__global__ __launch_bounds__(BLOCK) void hist_kernel(const uint8_t* __restrict__ bins, int32_t n_features, int32_t f_count,
                                                     int32_t n_bins, int32_t K, const int32_t* __restrict__ order,
                                                     const int32_t* __restrict__ seg, int32_t node0, int32_t node1,
                                                     const int32_t* __restrict__ w, const int64_t* __restrict__ yq,
                                                     const int32_t* __restrict__ cls, int32_t tile, void* __restrict__ hist) {
    extern __shared__ int64_t lds64[];
    const int tid = threadIdx.x;
    const int f0 = blockIdx.y * tile;
    const int nf = f_count - f0 < tile ? f_count - f0 : tile;
    const int cells = tile * n_bins;
    int64_t* lsum = lds64;
    int32_t* lcnt = CLS ? (int32_t*)lds64 : (int32_t*)(lds64 + cells);
    const int words = CLS ? cells * K : cells;
    const int pos_end = seg[node1];
    int p = seg[node0] + (int)blockIdx.x * PIECE;
    const int p1 = p + PIECE < pos_end ? p + PIECE : pos_end;
    if (p >= p1) return;
    const int slots = BLOCK / tile, slot = tid / tile, f = tid % tile;
    int m = node0 + segment_of(seg + node0, node1 - node0, p);
    while (p < p1) {
        const int e = seg[m + 1] < p1 ? seg[m + 1] : p1;
        for (int i = tid; i < words; i += BLOCK) lcnt[i] = 0;
        if (!CLS)
            for (int i = tid; i < cells; i += BLOCK) lsum[i] = 0;
        __syncthreads();
        if (f < nf) {
            for (int q = p + slot; q < e; q += slots) {
                const int s = order[q];
                const int32_t wv = w[s];
                if (wv == 0) continue;
                const int b = bins[(int64_t)s * n_features + f0 + f];        // < n_bins: checked before the fit
                const int cell = b * tile + f;
                if (CLS) {
                    atomicAdd(&lcnt[cell * K + cls[s]], wv);                 // cls[s] < K: checked before the fit
                } else {
                    atomicAdd(&lcnt[cell], wv);
                    atomicAdd((unsigned long long*)&lsum[cell], (unsigned long long)((int64_t)wv * yq[s]));
                }
            }
        }
        __syncthreads();
        const int64_t node_base = (int64_t)(m - node0) * f_count;
        for (int i = tid; i < words; i += BLOCK) {
            const int32_t c = lcnt[i];
            if (c == 0) continue;                                            // a cell with no count has no sum either
            const int cell = CLS ? i / K : i;
            const int ff = cell % tile, b = cell / tile;
            if (ff >= nf) continue;
            const int64_t at = (node_base + f0 + ff) * n_bins + b;
            if (CLS) {
                atomicAdd((int32_t*)hist + at * K + (i - cell * K), c);
            } else {
                atomicAdd((unsigned long long*)hist + at * 2, (unsigned long long)c);
                atomicAdd((unsigned long long*)hist + at * 2 + 1, (unsigned long long)lsum[i]);
            }
        }
        __syncthreads();
        p = e;
        ++m;
    }
}

// ---- split ----------------------------------------------------------------------------------------------------------------

template <typename T>
__device__ __forceinline__ T wave_inclusive(T v) {
    const int lane = threadIdx.x & (WAVE - 1);
    for (int d = 1; d < WAVE; d <<= 1) {
        const T o = __shfl_up(v, d, WAVE);
        if (lane >= d) v += o;
    }
    return v;
}

// One wavefront per (node, feature).  best_score / best_thr: [node][feature], best_thr -1 without a valid split.  The
// wavefront of feature 0 also writes the node's count, its parent term and its value.
template <bool CLS>
__global__ __launch_bounds__(BLOCK) void split_kernel(const void* __restrict__ hist, int32_t nodes, int32_t f_count, int32_t n_bins,
                                                      int32_t K, int32_t min_leaf, int32_t leaf_only, const double* __restrict__ gtab,
                                                      int64_t gtab_len, uint64_t seed, uint32_t tree, uint32_t node_id0,
                                                      const int64_t* __restrict__ key_limit, double y_scale,
                                                      double* __restrict__ best_score, int32_t* __restrict__ best_thr,
                                                      int64_t* __restrict__ node_count, double* __restrict__ node_parent,
                                                      double* __restrict__ value) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t pair = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
    if (pair >= (int64_t)nodes * f_count) return;
    const int m = (int)(pair / f_count), f = (int)(pair % f_count);
    bool selected = !leaf_only;
    if (selected && key_limit) {
        uint32_t r[4];
        n2v::philox4x32_10(seed, node_id0 + (uint32_t)m, (uint32_t)f, tree, N2V_FOREST_STREAM_FEAT, r);
        selected = (int64_t)(((uint64_t)r[0] << KEY_SHIFT) | (uint32_t)f) <= key_limit[m];
    }
    if (!selected && f != 0) {
        if (lane == 0) {
            best_score[pair] = 0.0;
            best_thr[pair] = -1;
        }
        return;
    }
    const int b0 = lane * 4;
    double score[4];
    bool valid[4], occupied[4];
    double parent;
    int64_t count;
    if (CLS) {
        const int32_t* h = (const int32_t*)hist + pair * n_bins * K;
        int64_t nL[4] = {0, 0, 0, 0};
        double sL[4] = {0.0, 0.0, 0.0, 0.0}, sR[4] = {0.0, 0.0, 0.0, 0.0}, sP = 0.0;
        int64_t total = 0;
        for (int j = 0; j < 4; ++j) occupied[j] = false;
        for (int c = 0; c < K; ++c) {
            int32_t v[4];
            int32_t mine = 0;
            for (int j = 0; j < 4; ++j) {
                v[j] = b0 + j < n_bins ? h[(int64_t)(b0 + j) * K + c] : 0;
                mine += v[j];
                occupied[j] = occupied[j] || v[j] > 0;
            }
            const int32_t incl = wave_inclusive(mine);
            const int32_t tot = __shfl(incl, WAVE - 1, WAVE);
            int32_t run = incl - mine;
            for (int j = 0; j < 4; ++j) {
                run += v[j];
                nL[j] += run;
                sL[j] = sL[j] + gtab[run < gtab_len ? run : gtab_len - 1];
                sR[j] = sR[j] + gtab[tot - run < gtab_len ? tot - run : gtab_len - 1];
            }
            total += tot;
            sP = sP + gtab[tot < gtab_len ? tot : gtab_len - 1];
            if (f == 0 && lane == 0) value[(int64_t)(node_id0 + m) * K + c] = (double)tot;
        }
        count = total;
        const int64_t lim = gtab_len - 1;
        parent = -(gtab[total < lim ? total : lim] - sP);
        for (int j = 0; j < 4; ++j) {
            const int64_t nR = total - nL[j];
            valid[j] = b0 + j < n_bins - 1 && nL[j] >= min_leaf && nR >= min_leaf;
            score[j] = -(((gtab[nL[j] < lim ? nL[j] : lim] - sL[j]) + gtab[nR < lim ? nR : lim]) - sR[j]);
        }
        if (f == 0 && lane == 0)
            for (int c = 0; c < K; ++c) value[(int64_t)(node_id0 + m) * K + c] = value[(int64_t)(node_id0 + m) * K + c] / (double)total;
    } else {
        const int64_t* h = (const int64_t*)hist + pair * n_bins * 2;
        int64_t cn[4], sm[4], mine_n = 0, mine_s = 0;
        for (int j = 0; j < 4; ++j) {
            cn[j] = b0 + j < n_bins ? h[(int64_t)(b0 + j) * 2] : 0;
            sm[j] = b0 + j < n_bins ? h[(int64_t)(b0 + j) * 2 + 1] : 0;
            mine_n += cn[j];
            mine_s += sm[j];
            occupied[j] = cn[j] > 0;
        }
        const int64_t incl_n = wave_inclusive(mine_n), incl_s = wave_inclusive(mine_s);
        const int64_t total = __shfl(incl_n, WAVE - 1, WAVE), S = __shfl(incl_s, WAVE - 1, WAVE);
        int64_t nL = incl_n - mine_n, SL = incl_s - mine_s;
        for (int j = 0; j < 4; ++j) {
            nL += cn[j];
            SL += sm[j];
            const int64_t nR = total - nL, SR = S - SL;
            valid[j] = b0 + j < n_bins - 1 && nL >= min_leaf && nR >= min_leaf;
            const double sl = (double)SL, sr = (double)SR;
            score[j] = valid[j] ? (sl * sl) / (double)nL + (sr * sr) / (double)nR : 0.0;
        }
        count = total;
        parent = ((double)S * (double)S) / (double)total;
        if (f == 0 && lane == 0) value[node_id0 + m] = ((double)S / (double)total) / y_scale;
    }
    if (f == 0 && lane == 0) {
        node_count[m] = count;
        node_parent[m] = parent;
    }
    // the lane's best, then the wave's: higher score, then lower bin
    double bs = 0.0;
    int bb = 0x7fffffff;
    for (int j = 0; j < 4; ++j)
        if (valid[j] && selected && (bb == 0x7fffffff || score[j] > bs)) {
            bs = score[j];
            bb = b0 + j;
        }
    for (int d = 32; d; d >>= 1) {
        const double os = __shfl_xor(bs, d, WAVE);
        const int ob = __shfl_xor(bb, d, WAVE);
        if (ob != 0x7fffffff && (bb == 0x7fffffff || os > bs || (os == bs && ob < bb))) {
            bs = os;
            bb = ob;
        }
    }
    int next = 0x7fffffff;                                   // the next occupied bin after the winner
    for (int j = 3; j >= 0; --j)
        if (occupied[j] && b0 + j > bb) next = b0 + j;
    for (int d = 32; d; d >>= 1) {
        const int o = __shfl_xor(next, d, WAVE);
        next = o < next ? o : next;
    }
    if (lane == 0) {
        const bool have = bb != 0x7fffffff && next != 0x7fffffff;
        best_score[pair] = have ? bs : 0.0;
        best_thr[pair] = have ? (bb + next - 1) / 2 : -1;
    }
}

__global__ __launch_bounds__(BLOCK) void choose_kernel(int32_t nodes, int32_t f_count, int32_t min_split, int32_t leaf_only,
                                                       const double* __restrict__ best_score, const int32_t* __restrict__ best_thr,
                                                       const int64_t* __restrict__ node_count, const double* __restrict__ node_parent,
                                                       int32_t node_id0, int32_t* __restrict__ feature, int32_t* __restrict__ threshold,
                                                       int32_t* __restrict__ left, int32_t* __restrict__ split) {
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    if (m >= nodes) return;
    int bf = -1, bt = -1;
    double bs = 0.0;
    if (!leaf_only && node_count[m] >= min_split) {
        for (int f = 0; f < f_count; ++f) {
            const int t = best_thr[(int64_t)m * f_count + f];
            const double s = best_score[(int64_t)m * f_count + f];
            if (t >= 0 && (bf < 0 || s > bs)) {
                bf = f;
                bt = t;
                bs = s;
            }
        }
        if (bf >= 0 && !(bs > node_parent[m])) bf = bt = -1;
    }
    feature[node_id0 + m] = bf;
    threshold[node_id0 + m] = bt;
    left[node_id0 + m] = -1;
    split[m] = bf >= 0 ? 1 : 0;
}

// ---- route ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void route_flags_kernel(const uint8_t* __restrict__ bins, int32_t n_features,
                                                            const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                            int32_t n_seg, const int32_t* __restrict__ split,
                                                            const int32_t* __restrict__ feature, const int32_t* __restrict__ threshold,
                                                            int32_t node_id0, int32_t* __restrict__ flags) {
    const int n_pos = seg[n_seg];
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n_pos) return;
    const int m = segment_of(seg, n_seg, p);
    int32_t l = 0, r = 0;
    if (split[m]) {
        const bool go = (int32_t)bins[(int64_t)order[p] * n_features + feature[node_id0 + m]] <= threshold[node_id0 + m];
        l = go ? 1 : 0;
        r = 1 - l;
    }
    flags[p] = l;
    flags[n_pos + p] = r;
}

// flags / sums: int32[2][n_pos], sums the inclusive scan of flags along each row; rank: the inclusive scan of split.
__global__ __launch_bounds__(BLOCK) void route_scatter_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                              int32_t n_seg, const int32_t* __restrict__ split,
                                                              const int32_t* __restrict__ rank, const int32_t* __restrict__ flags,
                                                              const int32_t* __restrict__ sums, int32_t node_id0, int32_t next_id0,
                                                              int32_t n_split, int32_t n_next, int32_t* __restrict__ left,
                                                              int32_t* __restrict__ new_order, int32_t* __restrict__ new_seg) {
    const int n_pos = seg[n_seg];
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n_pos) return;
    if (p == 0) new_seg[2 * n_split] = n_next;
    const int m = segment_of(seg, n_seg, p);
    if (!split[m]) return;
    const int32_t* sl = sums;
    const int32_t* sr = sums + n_pos;
    const int b = seg[m], e = seg[m + 1];
    const int lb = b ? sl[b - 1] : 0, rb = b ? sr[b - 1] : 0, le = sl[e - 1];
    const int dest = flags[p] ? rb + sl[p] - 1 : le + sr[p] - 1;
    if (dest >= 0 && dest < n_next) new_order[dest] = order[p];
    if (p == b) {
        const int r = rank[m] - 1;
        if (r >= 0 && r < n_split) {
            new_seg[2 * r] = lb + rb;
            new_seg[2 * r + 1] = le + rb;
            left[node_id0 + m] = next_id0 + 2 * r;
        }
    }
}

// ---- predict --------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void predict_kernel(const uint8_t* __restrict__ bins, int64_t n, int32_t n_features,
                                                        const int32_t* __restrict__ feature, const int32_t* __restrict__ threshold,
                                                        const int32_t* __restrict__ left, const double* __restrict__ value,
                                                        const int64_t* __restrict__ tree_ptr, int32_t n_trees, int32_t width,
                                                        int32_t max_depth, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n * width) return;
    const int64_t s = i / width;
    const int c = (int)(i % width);
    const uint8_t* row = bins + s * n_features;
    double acc = 0.0;
    for (int t = 0; t < n_trees; ++t) {
        const int64_t base = tree_ptr[t];
        int32_t node = 0;
        for (int d = 0; d < max_depth; ++d) {
            const int32_t l = left[base + node];
            if (l < 0) break;
            node = (int32_t)row[feature[base + node]] <= threshold[base + node] ? l : l + 1;
        }
        acc = acc + value[(base + node) * width + c];
    }
    out[i] = acc / (double)n_trees;
}

__global__ __launch_bounds__(BLOCK) void argmax_kernel(const double* __restrict__ proba, int64_t n, int32_t K, int32_t* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n) return;
    int best = 0;
    for (int c = 1; c < K; ++c)
        if (proba[s * K + c] > proba[s * K + best]) best = c;
    out[s] = best;
}

bool bad_shape(int64_t n, int64_t n_features, int64_t n_bins, int64_t K) {
    return n < 1 || n > 0x7fffffff || n_features < 1 || n_features > N2V_FOREST_MAX_FEATURES || n_bins < 2 ||
           n_bins > N2V_FOREST_MAX_BINS || K < 0 || K == 1 || K > N2V_FOREST_MAX_CLASSES || n * n_features > 0x7fffffffffffll;
}

}  // namespace

extern "C" {

int32_t n2v_forest_feature_tile(int32_t n_bins, int32_t n_classes) {
    if (n_bins < 2 || n_bins > N2V_FOREST_MAX_BINS || n_classes < 0 || n_classes > N2V_FOREST_MAX_CLASSES) return 0;
    return feature_tile(n_bins, n_classes);
}

int n2v_forest_glog_table(int64_t len, double* table) {
    if (len < 1 || !table) return n2v::fail(N2V_ERR_INVALID, "forest_glog_table: len=%lld", (long long)len);
    table[0] = 0.0;
    for (int64_t a = 1; a < len; ++a) table[a] = (double)a * std::log((double)a);
    return N2V_OK;
}

int n2v_forest_check_x(const double* x, int64_t count, int32_t* status, void* stream) {
    if (count < 1 || !x || !status) return n2v::fail(N2V_ERR_INVALID, "forest_check_x: count=%lld", (long long)count);
    check_x_kernel<<<n2v::grid_for(count, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(x, count, status);
    return n2v::check_launch("forest_check_x");
}

int n2v_forest_check_bins(const uint8_t* bins, int64_t count, int32_t n_bins, int32_t* status, void* stream) {
    if (count < 1 || !bins || !status || n_bins < 2 || n_bins > N2V_FOREST_MAX_BINS)
        return n2v::fail(N2V_ERR_INVALID, "forest_check_bins: count=%lld n_bins=%d", (long long)count, n_bins);
    check_u8_kernel<<<n2v::grid_for(count, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(bins, count, n_bins, status);
    return n2v::check_launch("forest_check_bins");
}

int n2v_forest_check_classes(const int32_t* cls, int64_t count, int32_t n_classes, int32_t* status, void* stream) {
    if (count < 1 || !cls || !status || n_classes < 2 || n_classes > N2V_FOREST_MAX_CLASSES)
        return n2v::fail(N2V_ERR_INVALID, "forest_check_classes: count=%lld n_classes=%d", (long long)count, n_classes);
    check_i32_kernel<<<n2v::grid_for(count, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(cls, count, n_classes, N2V_FOREST_BAD_CLASS, status);
    return n2v::check_launch("forest_check_classes");
}

int n2v_forest_check_tree(const int32_t* feature, const int32_t* threshold, const int32_t* left, const int64_t* tree_ptr,
                          int32_t n_trees, int64_t n_nodes, int32_t n_features, int32_t n_bins, int32_t* status, void* stream) {
    if (n_trees < 1 || n_nodes < n_trees || n_nodes > 0x7fffffff || bad_shape(1, n_features, n_bins, 0))
        return n2v::fail(N2V_ERR_INVALID, "forest_check_tree: n_trees=%d n_nodes=%lld n_features=%d n_bins=%d", n_trees,
                         (long long)n_nodes, n_features, n_bins);
    if (!feature || !threshold || !left || !tree_ptr || !status) return n2v::fail(N2V_ERR_INVALID, "forest_check_tree: null pointer");
    check_tree_kernel<<<n2v::grid_for(n_nodes, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(feature, threshold, left, tree_ptr, n_trees,
                                                                                        n_features, n_bins, status);
    return n2v::check_launch("forest_check_tree");
}

int n2v_forest_edges(const double* xs, int64_t n, int32_t n_features, int32_t n_bins, double* edges, int32_t* n_edges, void* stream) {
    if (bad_shape(n, n_features, n_bins, 0))
        return n2v::fail(N2V_ERR_INVALID, "forest_edges: n=%lld n_features=%d n_bins=%d", (long long)n, n_features, n_bins);
    if (!xs || !edges || !n_edges) return n2v::fail(N2V_ERR_INVALID, "forest_edges: null pointer");
    edges_kernel<<<n_features, WAVE, 0, (hipStream_t)stream>>>(xs, n, n_bins, edges, n_edges);
    return n2v::check_launch("forest_edges");
}

int n2v_forest_bin(const double* x, int64_t n, int32_t n_features, int32_t n_bins, const double* edges, const int32_t* n_edges,
                   uint8_t* bins, int32_t* status, void* stream) {
    if (bad_shape(n, n_features, n_bins, 0))
        return n2v::fail(N2V_ERR_INVALID, "forest_bin: n=%lld n_features=%d n_bins=%d", (long long)n, n_features, n_bins);
    if (!x || !edges || !n_edges || !bins || !status) return n2v::fail(N2V_ERR_INVALID, "forest_bin: null pointer");
    bin_kernel<<<n2v::grid_for(n * n_features, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(x, n * n_features, n_features, n_bins, edges,
                                                                                        n_edges, bins, status);
    return n2v::check_launch("forest_bin");
}

int n2v_forest_bootstrap(uint64_t seed, int32_t tree, int64_t n, int32_t* w, void* stream) {
    if (n < 1 || n > 0x7fffffff || tree < 0 || !w) return n2v::fail(N2V_ERR_INVALID, "forest_bootstrap: n=%lld tree=%d", (long long)n, tree);
    if (hipMemsetAsync(w, 0, sizeof(int32_t) * n, (hipStream_t)stream) != hipSuccess) return n2v::check_launch("forest_bootstrap");
    bootstrap_kernel<<<n2v::grid_for(n, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(seed, (uint32_t)tree, n, w);
    return n2v::check_launch("forest_bootstrap");
}

int n2v_forest_quantise(const double* y, int64_t n, int32_t y_bits, int64_t* yq, int64_t* max_abs, int32_t* status, void* stream) {
    if (n < 1 || n > 0x7fffffff || y_bits < 0 || y_bits > 52 || !y || !yq || !max_abs || !status)
        return n2v::fail(N2V_ERR_INVALID, "forest_quantise: n=%lld y_bits=%d", (long long)n, y_bits);
    if (hipMemsetAsync(max_abs, 0, sizeof(int64_t), (hipStream_t)stream) != hipSuccess) return n2v::check_launch("forest_quantise");
    quantise_kernel<<<n2v::grid_for(n, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(y, n, std::ldexp(1.0, y_bits), yq,
                                                                                (unsigned long long*)max_abs, status);
    return n2v::check_launch("forest_quantise");
}

int n2v_forest_feature_keys(uint64_t seed, int32_t tree, int32_t node_id0, int32_t nodes, int32_t n_features, int64_t* keys,
                            void* stream) {
    if (tree < 0 || node_id0 < 0 || nodes < 1 || n_features < 1 || n_features > N2V_FOREST_MAX_FEATURES || !keys)
        return n2v::fail(N2V_ERR_INVALID, "forest_feature_keys: tree=%d node_id0=%d nodes=%d n_features=%d", tree, node_id0, nodes,
                         n_features);
    const int64_t count = (int64_t)nodes * n_features;
    keys_kernel<<<n2v::grid_for(count, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(seed, (uint32_t)tree, (uint32_t)node_id0, count,
                                                                                n_features, keys);
    return n2v::check_launch("forest_feature_keys");
}

int n2v_forest_hist(const uint8_t* bins, int64_t n, int32_t n_features, int32_t f_count, int32_t n_bins, int32_t n_classes,
                    const int32_t* order, const int32_t* seg, int32_t node0, int32_t node1, int64_t n_positions, const int32_t* w,
                    const int64_t* yq, const int32_t* cls, void* hist, void* stream) {
    if (bad_shape(n, n_features, n_bins, n_classes) || f_count < 1 || f_count > n_features || node0 < 0 || node1 <= node0 ||
        n_positions < 1 || n_positions > n)
        return n2v::fail(N2V_ERR_INVALID, "forest_hist: n=%lld n_features=%d f_count=%d n_bins=%d n_classes=%d nodes %d .. %d "
                         "n_positions=%lld", (long long)n, n_features, f_count, n_bins, n_classes, node0, node1, (long long)n_positions);
    if (!bins || !order || !seg || !w || !hist || (n_classes ? !cls : !yq)) return n2v::fail(N2V_ERR_INVALID, "forest_hist: null pointer");
    const int tile = feature_tile(n_bins, n_classes);
    const size_t cell_bytes = n_classes ? 4 * (size_t)n_classes : 12;
    const size_t hist_bytes = (size_t)(node1 - node0) * f_count * n_bins * (n_classes ? 4 * (size_t)n_classes : 16);
    if (hipMemsetAsync(hist, 0, hist_bytes, (hipStream_t)stream) != hipSuccess) return n2v::check_launch("forest_hist");
    const dim3 grid(n2v::grid_for(n_positions, PIECE), (f_count + tile - 1) / tile);
    const size_t lds = (size_t)tile * n_bins * cell_bytes;
    if (n_classes)
        hist_kernel<true><<<grid, BLOCK, lds, (hipStream_t)stream>>>(bins, n_features, f_count, n_bins, n_classes, order, seg, node0,
                                                                     node1, w, yq, cls, tile, hist);
    else
        hist_kernel<false><<<grid, BLOCK, lds, (hipStream_t)stream>>>(bins, n_features, f_count, n_bins, n_classes, order, seg, node0,
                                                                      node1, w, yq, cls, tile, hist);
    return n2v::check_launch("forest_hist");
}

int n2v_forest_split(const void* hist, int32_t nodes, int32_t f_count, int32_t n_bins, int32_t n_classes, int32_t min_samples_split,
                     int32_t min_samples_leaf, int32_t leaf_only, const double* gtab, int64_t gtab_len, uint64_t seed, int32_t tree,
                     int32_t node_id0, const int64_t* key_limit, int32_t y_bits, double* best_score, int32_t* best_thr,
                     int64_t* node_count, double* node_parent, int32_t* feature, int32_t* threshold, int32_t* left, double* value,
                     int32_t* split, void* stream) {
    if (nodes < 1 || bad_shape(1, f_count, n_bins, n_classes) || min_samples_leaf < 1 || min_samples_split < 0 || tree < 0 ||
        node_id0 < 0 || y_bits < 0 || y_bits > 52 || (n_classes && gtab_len < 1))
        return n2v::fail(N2V_ERR_INVALID, "forest_split: nodes=%d f_count=%d n_bins=%d n_classes=%d min_samples_leaf=%d", nodes, f_count,
                         n_bins, n_classes, min_samples_leaf);
    if (!hist || !best_score || !best_thr || !node_count || !node_parent || !feature || !threshold || !left || !value || !split ||
        (n_classes && !gtab))
        return n2v::fail(N2V_ERR_INVALID, "forest_split: null pointer");
    const int64_t pairs = (int64_t)nodes * f_count;
    const unsigned grid = n2v::grid_for(pairs, BLOCK / WAVE);
    if (n_classes)
        split_kernel<true><<<grid, BLOCK, 0, (hipStream_t)stream>>>(hist, nodes, f_count, n_bins, n_classes, min_samples_leaf, leaf_only,
                                                                    gtab, gtab_len, seed, (uint32_t)tree, (uint32_t)node_id0, key_limit,
                                                                    1.0, best_score, best_thr, node_count, node_parent, value);
    else
        split_kernel<false><<<grid, BLOCK, 0, (hipStream_t)stream>>>(hist, nodes, f_count, n_bins, n_classes, min_samples_leaf, leaf_only,
                                                                     gtab, gtab_len, seed, (uint32_t)tree, (uint32_t)node_id0, key_limit,
                                                                     std::ldexp(1.0, y_bits), best_score, best_thr, node_count,
                                                                     node_parent, value);
    if (int rc = n2v::check_launch("forest_split")) return rc;
    choose_kernel<<<n2v::grid_for(nodes, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(nodes, f_count, min_samples_split, leaf_only, best_score,
                                                                                  best_thr, node_count, node_parent, node_id0, feature,
                                                                                  threshold, left, split);
    return n2v::check_launch("forest_split");
}

int n2v_forest_route_flags(const uint8_t* bins, int64_t n, int32_t n_features, const int32_t* order, const int32_t* seg, int32_t n_seg,
                           int64_t n_positions, const int32_t* split, const int32_t* feature, const int32_t* threshold,
                           int32_t node_id0, int32_t* flags, void* stream) {
    if (n < 1 || n > 0x7fffffff || n_features < 1 || n_seg < 1 || n_positions < 1 || n_positions > n || node_id0 < 0)
        return n2v::fail(N2V_ERR_INVALID, "forest_route_flags: n=%lld n_seg=%d n_positions=%lld", (long long)n, n_seg, (long long)n_positions);
    if (!bins || !order || !seg || !split || !feature || !threshold || !flags) return n2v::fail(N2V_ERR_INVALID, "forest_route_flags: null pointer");
    route_flags_kernel<<<n2v::grid_for(n_positions, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(bins, n_features, order, seg, n_seg, split,
                                                                                             feature, threshold, node_id0, flags);
    return n2v::check_launch("forest_route_flags");
}

int n2v_forest_route_scatter(const int32_t* order, const int32_t* seg, int32_t n_seg, int64_t n_positions, const int32_t* split,
                             const int32_t* rank, const int32_t* flags, const int32_t* sums, int32_t node_id0, int32_t next_id0,
                             int32_t n_split, int64_t n_next, int32_t* left, int32_t* new_order, int32_t* new_seg, void* stream) {
    if (n_seg < 1 || n_positions < 1 || n_positions > 0x7fffffff || n_split < 1 || n_split > n_seg || n_next < 1 || n_next > n_positions ||
        node_id0 < 0 || next_id0 <= node_id0)
        return n2v::fail(N2V_ERR_INVALID, "forest_route_scatter: n_seg=%d n_positions=%lld n_split=%d n_next=%lld", n_seg,
                         (long long)n_positions, n_split, (long long)n_next);
    if (!order || !seg || !split || !rank || !flags || !sums || !left || !new_order || !new_seg)
        return n2v::fail(N2V_ERR_INVALID, "forest_route_scatter: null pointer");
    route_scatter_kernel<<<n2v::grid_for(n_positions, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(order, seg, n_seg, split, rank, flags, sums,
                                                                                               node_id0, next_id0, n_split, (int32_t)n_next,
                                                                                               left, new_order, new_seg);
    return n2v::check_launch("forest_route_scatter");
}

int n2v_forest_predict(const uint8_t* bins, int64_t n, int32_t n_features, const int32_t* feature, const int32_t* threshold,
                       const int32_t* left, const double* value, const int64_t* tree_ptr, int32_t n_trees, int32_t width,
                       int32_t max_depth, double* out, void* stream) {
    if (n < 1 || n > 0x7fffffff || n_features < 1 || n_features > N2V_FOREST_MAX_FEATURES || n_trees < 1 || width < 1 ||
        width > N2V_FOREST_MAX_CLASSES || max_depth < 0 || max_depth > N2V_FOREST_MAX_DEPTH)
        return n2v::fail(N2V_ERR_INVALID, "forest_predict: n=%lld n_features=%d n_trees=%d width=%d max_depth=%d", (long long)n,
                         n_features, n_trees, width, max_depth);
    if (!bins || !feature || !threshold || !left || !value || !tree_ptr || !out) return n2v::fail(N2V_ERR_INVALID, "forest_predict: null pointer");
    predict_kernel<<<n2v::grid_for(n * width, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(bins, n, n_features, feature, threshold, left, value,
                                                                                       tree_ptr, n_trees, width, max_depth, out);
    return n2v::check_launch("forest_predict");
}

int n2v_forest_argmax(const double* proba, int64_t n, int32_t n_classes, int32_t* out, void* stream) {
    if (n < 1 || n > 0x7fffffff || n_classes < 2 || n_classes > N2V_FOREST_MAX_CLASSES || !proba || !out)
        return n2v::fail(N2V_ERR_INVALID, "forest_argmax: n=%lld n_classes=%d", (long long)n, n_classes);
    argmax_kernel<<<n2v::grid_for(n, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(proba, n, n_classes, out);
    return n2v::check_launch("forest_argmax");
}

}  // extern "C"
