// Eccentricity split: ue -> n bins of users -> one bipartite user-item CSR graph per bin — gfx950 (MI355X).
// C-ABI: include/n2v_sim.h.
//
// Reference: src/utils.py:305-312 (mark_n), :382-405 (split_and_save_edgelist / save_edgelist) and the graph that
// src/main.py:66-80 reads back from each file.  Here the rows stay on the device and a graph is a chain of passes with
// the sorts (torch) between them.  Integer arithmetic only; a weight is moved by its bytes and never added.
//   sort_key   fp64 -> int64 that orders as the stated rule does: -0.0 ties with +0.0, NaN after +inf.
//   mark       bin[order[r]] = n if n_users / n == 0 else min(r / (n_users / n) + 1, n).
//   compaction the one stable compaction behind select / nodes / pairs, three launches as n2v_eccstats_groups: ballots
//              per tile -> one-workgroup exclusive scan of the tile counts (and the total) -> the same ballots again,
//              every kept element written at tile offset + kept elements before it.  Workgroups meet only at the
//              launch boundaries, so the output does not depend on the order in which they run.
//   first      first appearance: 64-bit integer atomicMin of 2k (user) and 2k + 1 (item) over the selected rows; the
//              word is read first and the atomic skipped when it is already smaller (a popular item meets 10^5 rows).
//   ranks      dense id of every node slot from the sort of the node names; start_order from the sort of first.
//   keys       dense_u * N + dense_i of every selected row.
//   fill       sorted entries -> row_ptr / col / w.
#include "n2v_common.h"
#include "n2v_compact.h"
#include "n2v_sim.h"

namespace {

constexpr int TILE = n2v::COMPACT_TILE;                  // elements per workgroup of the compaction passes
constexpr long long NONE = 0x7fffffffffffffffll;         // N2V_ECCSPLIT_NONE: a node no selected row names
constexpr int64_t LIMIT = 0x7fffffff;                    // every size is below 2^31

// ---- sort key and mark ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) sort_key_kernel(const int64_t* __restrict__ bits, int64_t n, int64_t* __restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long b = bits[i], mag = b & 0x7fffffffffffffffll;
    long long k;
    if (mag > 0x7ff0000000000000ll) k = NONE;            // NaN, any sign or payload: last
    else if (mag == 0) k = 0;                            // -0.0 and +0.0: a tie
    else k = b >= 0 ? b : (b ^ 0x7fffffffffffffffll);    // negative: the larger magnitude is the smaller key
    key[i] = k;
}

__global__ void __launch_bounds__(256) mark_kernel(const int64_t* __restrict__ order, int64_t n_users, int64_t n_bins,
                                                   int32_t* __restrict__ bin) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_users) return;
    const int64_t u = order[r], repeat = n_users / n_bins;
    if (u < 0 || u >= n_users) return;
    const int64_t b = repeat == 0 ? n_bins : (r / repeat + 1 < n_bins ? r / repeat + 1 : n_bins);
    bin[u] = (int32_t)b;
}

// ---- the stable compaction: n2v_compact.h ------------------------------------------------------------------------------

using n2v::compact;

struct SelectP {
    const int64_t* user; const int32_t* bin; int64_t n_users; int32_t which; int64_t* rows;
    __device__ bool test(int64_t k) const {
        if (which == 0) return true;
        const int64_t u = user[k];
        return u >= 0 && u < n_users && bin[u] == which;
    }
    __device__ void emit(int64_t k, int64_t slot) const { rows[slot] = k; }
    __device__ void skip(int64_t) const {}
};

struct NodeP {
    const int64_t* first; int64_t n_users; const int64_t* user_names; const int64_t* item_names;
    int64_t* node_name; int64_t* node_first; int32_t* slot_of;
    __device__ bool test(int64_t j) const { return first[j] != NONE; }
    __device__ void emit(int64_t j, int64_t slot) const {
        node_name[slot] = j < n_users ? user_names[j] : item_names[j - n_users];
        node_first[slot] = first[j];
        slot_of[j] = (int32_t)slot;
    }
    __device__ void skip(int64_t j) const { slot_of[j] = -1; }
};

struct PairP {
    const int64_t* key; const int64_t* perm; const int64_t* rows; const int64_t* w_bits; int64_t n; int64_t n_rows;
    int64_t n_nodes; int64_t* ekey; int64_t* ew_bits;
    __device__ bool test(int64_t t) const { return t == n - 1 || key[t] != key[t + 1]; }       // the LAST of its run
    __device__ void emit(int64_t t, int64_t slot) const {
        const int64_t kt = key[t], a = kt / n_nodes, b = kt - a * n_nodes;
        int64_t k = perm[t];
        k = k < 0 ? 0 : (k < n ? k : n - 1);
        int64_t row = rows ? rows[k] : k;
        row = row < 0 ? 0 : (row < n_rows ? row : n_rows - 1);
        const int64_t wv = w_bits[row];
        ekey[2 * slot] = kt;              ew_bits[2 * slot] = wv;            // u -> i
        ekey[2 * slot + 1] = b * n_nodes + a; ew_bits[2 * slot + 1] = wv;    // i -> u
    }
    __device__ void skip(int64_t) const {}
};

// ---- first appearance -------------------------------------------------------------------------------------------------

__device__ __forceinline__ void lower(int64_t* p, long long v) {
    if (*reinterpret_cast<const volatile long long*>(p) > v) atomicMin(reinterpret_cast<long long*>(p), v);
}

__global__ void __launch_bounds__(256) first_kernel(const int64_t* __restrict__ rows, const int64_t* __restrict__ n_sel, int64_t cap,
                                                    const int64_t* __restrict__ user, const int64_t* __restrict__ item,
                                                    int64_t n_rows, int64_t n_users, int64_t n_items, int64_t* first) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t n = n_sel ? *n_sel : cap;
    n = n < cap ? n : cap;
    if (t >= n) return;
    const int64_t k = rows ? rows[t] : t;
    if (k < 0 || k >= n_rows) return;
    const int64_t u = user[k], i = item[k];
    if (u >= 0 && u < n_users) lower(first + u, 2 * k);
    if (i >= 0 && i < n_items) lower(first + n_users + i, 2 * k + 1);
}

// ---- ranks, keys, fill ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) rank_kernel(const int64_t* __restrict__ perm_name, int64_t n_nodes, int32_t* __restrict__ rank) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_nodes) return;
    const int64_t slot = perm_name[r];
    if (slot >= 0 && slot < n_nodes) rank[slot] = (int32_t)r;
}

__global__ void __launch_bounds__(256) start_order_kernel(const int64_t* __restrict__ perm_first, const int32_t* __restrict__ rank,
                                                          int64_t n_nodes, int32_t* __restrict__ start_order) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_nodes) return;
    const int64_t slot = perm_first[j];
    if (slot >= 0 && slot < n_nodes) start_order[j] = rank[slot];
}

struct KeyArgs {
    const int64_t* rows; int64_t n_sel; const int64_t* user; const int64_t* item; int64_t n_rows; int64_t n_users; int64_t n_items;
    const int32_t* slot_of; const int32_t* rank; int64_t n_nodes; int64_t* key;
};

__global__ void __launch_bounds__(256) keys_kernel(KeyArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_sel) return;
    int64_t out = 0;                                                     // a row outside its promise: the pair (0, 0)
    const int64_t k = a.rows ? a.rows[t] : t;
    if (k >= 0 && k < a.n_rows) {
        const int64_t u = a.user[k], i = a.item[k];
        if (u >= 0 && u < a.n_users && i >= 0 && i < a.n_items) {
            const int64_t su = a.slot_of[u], si = a.slot_of[a.n_users + i];
            if (su >= 0 && su < a.n_nodes && si >= 0 && si < a.n_nodes) out = (int64_t)a.rank[su] * a.n_nodes + a.rank[si];
        }
    }
    a.key[t] = out;
}

__global__ void __launch_bounds__(256) fill_kernel(const int64_t* __restrict__ ekey, const int64_t* __restrict__ perm, int64_t nnz,
                                                   const int64_t* __restrict__ ew_bits, int64_t n_nodes, int64_t* __restrict__ row_ptr,
                                                   int32_t* __restrict__ col, int64_t* __restrict__ w_bits) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int64_t kt = ekey[e];
    int64_t r = kt / n_nodes;
    const int64_t c = kt - r * n_nodes;
    r = r < 0 ? 0 : (r < n_nodes ? r : n_nodes - 1);
    int64_t prev = e == 0 ? -1 : ekey[e - 1] / n_nodes;
    prev = prev < -1 ? -1 : (prev < n_nodes ? prev : n_nodes - 1);
    const int64_t p = perm[e];
    col[e] = (int32_t)c;
    w_bits[e] = ew_bits[p < 0 ? 0 : (p < nnz ? p : nnz - 1)];
    for (int64_t j = prev + 1; j <= r; ++j) row_ptr[j] = e;              // rows without entries: empty
    if (e == nnz - 1) for (int64_t j = r + 1; j <= n_nodes; ++j) row_ptr[j] = nnz;
}

bool small(int64_t v) { return v >= 1 && v <= LIMIT; }

}  // namespace

extern "C" {

int32_t n2v_eccsplit_tile(void) { return TILE; }

int64_t n2v_eccsplit_scratch(int64_t n) { return n < 1 ? 0 : (n + TILE - 1) / TILE; }

int n2v_eccsplit_sort_key(const double* ue, int64_t n, int64_t* key, void* stream) {
    if (n == 0) return N2V_OK;
    if (!small(n)) return n2v::fail(N2V_ERR_INVALID, "eccsplit_sort_key: n=%lld (0 .. 2^31-1)", (long long)n);
    if (!ue || !key) return n2v::fail(N2V_ERR_INVALID, "eccsplit_sort_key: null pointer");
    sort_key_kernel<<<n2v::grid_for(n, 256), 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const int64_t*>(ue), n, key);
    return n2v::check_launch("eccsplit_sort_key");
}

int n2v_eccsplit_mark(const int64_t* order, int64_t n_users, int64_t n_bins, int32_t* bin, void* stream) {
    if (n_users == 0) return N2V_OK;
    if (!small(n_users) || !small(n_bins))
        return n2v::fail(N2V_ERR_INVALID, "eccsplit_mark: n_users=%lld n_bins=%lld (1 .. 2^31-1)", (long long)n_users, (long long)n_bins);
    if (!order || !bin) return n2v::fail(N2V_ERR_INVALID, "eccsplit_mark: null pointer");
    mark_kernel<<<n2v::grid_for(n_users, 256), 256, 0, (hipStream_t)stream>>>(order, n_users, n_bins, bin);
    return n2v::check_launch("eccsplit_mark");
}

int n2v_eccsplit_select(const int64_t* user, int64_t n_rows, const int32_t* bin, int64_t n_users, int32_t which, int64_t* scratch,
                        int64_t* rows, int64_t* count, void* stream) {
    if (!count) return n2v::fail(N2V_ERR_INVALID, "eccsplit_select: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int64_t), s) != hipSuccess) return n2v::fail(N2V_ERR_HIP, "eccsplit_select: memset failed");
        return N2V_OK;
    }
    if (!small(n_rows) || !small(n_users) || which < 0)
        return n2v::fail(N2V_ERR_INVALID, "eccsplit_select: n_rows=%lld n_users=%lld which=%d", (long long)n_rows, (long long)n_users, which);
    if (!user || !bin || !scratch || !rows) return n2v::fail(N2V_ERR_INVALID, "eccsplit_select: null pointer");
    compact(SelectP{user, bin, n_users, which, rows}, n_rows, scratch, count, s);
    return n2v::check_launch("eccsplit_select");
}

int n2v_eccsplit_first(const int64_t* rows, const int64_t* n_sel, int64_t cap, const int64_t* user, const int64_t* item,
                       int64_t n_rows, int64_t n_users, int64_t n_items, int64_t* first, void* stream) {
    if (cap == 0) return N2V_OK;
    if (!small(cap) || cap > n_rows || !small(n_rows) || !small(n_users) || !small(n_items) || n_users + n_items > LIMIT)
        return n2v::fail(N2V_ERR_INVALID, "eccsplit_first: cap=%lld n_rows=%lld n_users=%lld n_items=%lld", (long long)cap,
                         (long long)n_rows, (long long)n_users, (long long)n_items);
    if (!user || !item || !first) return n2v::fail(N2V_ERR_INVALID, "eccsplit_first: null pointer");
    first_kernel<<<n2v::grid_for(cap, 256), 256, 0, (hipStream_t)stream>>>(rows, n_sel, cap, user, item, n_rows, n_users, n_items, first);
    return n2v::check_launch("eccsplit_first");
}

int n2v_eccsplit_nodes(const int64_t* first, int64_t n_users, int64_t n_items, const int64_t* user_names, const int64_t* item_names,
                       int64_t* scratch, int64_t* node_name, int64_t* node_first, int32_t* slot_of, int64_t* count, void* stream) {
    if (!count) return n2v::fail(N2V_ERR_INVALID, "eccsplit_nodes: null pointer");
    if (n_users == 0 && n_items == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int64_t), (hipStream_t)stream) != hipSuccess) return n2v::fail(N2V_ERR_HIP, "eccsplit_nodes: memset failed");
        return N2V_OK;
    }
    if (n_users < 0 || n_items < 0 || n_users > LIMIT || n_items > LIMIT || n_users + n_items > LIMIT)
        return n2v::fail(N2V_ERR_INVALID, "eccsplit_nodes: n_users=%lld n_items=%lld", (long long)n_users, (long long)n_items);
    if (!first || !user_names || !item_names || !scratch || !node_name || !node_first || !slot_of || !count)
        return n2v::fail(N2V_ERR_INVALID, "eccsplit_nodes: null pointer");
    compact(NodeP{first, n_users, user_names, item_names, node_name, node_first, slot_of}, n_users + n_items, scratch, count,
            (hipStream_t)stream);
    return n2v::check_launch("eccsplit_nodes");
}

int n2v_eccsplit_ranks(const int64_t* perm_name, const int64_t* perm_first, int64_t n_nodes, int32_t* rank, int32_t* start_order,
                       void* stream) {
    if (n_nodes == 0) return N2V_OK;
    if (!small(n_nodes)) return n2v::fail(N2V_ERR_INVALID, "eccsplit_ranks: n_nodes=%lld", (long long)n_nodes);
    if (!perm_name || !perm_first || !rank || !start_order) return n2v::fail(N2V_ERR_INVALID, "eccsplit_ranks: null pointer");
    hipStream_t s = (hipStream_t)stream;
    rank_kernel<<<n2v::grid_for(n_nodes, 256), 256, 0, s>>>(perm_name, n_nodes, rank);
    start_order_kernel<<<n2v::grid_for(n_nodes, 256), 256, 0, s>>>(perm_first, rank, n_nodes, start_order);
    return n2v::check_launch("eccsplit_ranks");
}

int n2v_eccsplit_keys(const int64_t* rows, int64_t n_sel, const int64_t* user, const int64_t* item, int64_t n_rows, int64_t n_users,
                      int64_t n_items, const int32_t* slot_of, const int32_t* rank, int64_t n_nodes, int64_t* key, void* stream) {
    if (n_sel == 0) return N2V_OK;
    if (!small(n_sel) || n_sel > n_rows || !small(n_rows) || !small(n_users) || !small(n_items) || !small(n_nodes))
        return n2v::fail(N2V_ERR_INVALID, "eccsplit_keys: n_sel=%lld n_rows=%lld n_users=%lld n_items=%lld n_nodes=%lld",
                         (long long)n_sel, (long long)n_rows, (long long)n_users, (long long)n_items, (long long)n_nodes);
    if (!user || !item || !slot_of || !rank || !key) return n2v::fail(N2V_ERR_INVALID, "eccsplit_keys: null pointer");
    KeyArgs a{rows, n_sel, user, item, n_rows, n_users, n_items, slot_of, rank, n_nodes, key};
    keys_kernel<<<n2v::grid_for(n_sel, 256), 256, 0, (hipStream_t)stream>>>(a);
    return n2v::check_launch("eccsplit_keys");
}

int n2v_eccsplit_pairs(const int64_t* key_sorted, const int64_t* perm, int64_t n_sel, const int64_t* rows, const double* w,
                       int64_t n_rows, int64_t n_nodes, int64_t* scratch, int64_t* ekey, double* ew, int64_t* count, void* stream) {
    if (!count) return n2v::fail(N2V_ERR_INVALID, "eccsplit_pairs: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_sel == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int64_t), s) != hipSuccess) return n2v::fail(N2V_ERR_HIP, "eccsplit_pairs: memset failed");
        return N2V_OK;
    }
    if (!small(n_sel) || n_sel > n_rows || 2 * n_sel > LIMIT || !small(n_rows) || !small(n_nodes))
        return n2v::fail(N2V_ERR_INVALID, "eccsplit_pairs: n_sel=%lld (2 n_sel < 2^31) n_rows=%lld n_nodes=%lld", (long long)n_sel,
                         (long long)n_rows, (long long)n_nodes);
    if (!key_sorted || !perm || !w || !scratch || !ekey || !ew) return n2v::fail(N2V_ERR_INVALID, "eccsplit_pairs: null pointer");
    compact(PairP{key_sorted, perm, rows, reinterpret_cast<const int64_t*>(w), n_sel, n_rows, n_nodes, ekey,
                  reinterpret_cast<int64_t*>(ew)}, n_sel, scratch, count, s);
    return n2v::check_launch("eccsplit_pairs");
}

int n2v_eccsplit_fill(const int64_t* ekey_sorted, const int64_t* perm, int64_t nnz, const double* ew, int64_t n_nodes,
                      int64_t* row_ptr, int32_t* col, double* w, void* stream) {
    if (nnz == 0) return N2V_OK;
    if (!small(nnz) || !small(n_nodes)) return n2v::fail(N2V_ERR_INVALID, "eccsplit_fill: nnz=%lld n_nodes=%lld", (long long)nnz, (long long)n_nodes);
    if (!ekey_sorted || !perm || !ew || !row_ptr || !col || !w) return n2v::fail(N2V_ERR_INVALID, "eccsplit_fill: null pointer");
    fill_kernel<<<n2v::grid_for(nnz, 256), 256, 0, (hipStream_t)stream>>>(ekey_sorted, perm, nnz, reinterpret_cast<const int64_t*>(ew),
                                                                        n_nodes, row_ptr, col, reinterpret_cast<int64_t*>(w));
    return n2v::check_launch("eccsplit_fill");
}

}  // extern "C"
