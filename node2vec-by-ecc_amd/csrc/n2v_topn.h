// Top-N lists of the rating predictors (n2v_eccknn.hip, n2v_svd.hip, n2v_slopeone.hip) — gfx950 (MI355X).  C-ABI:
// include/n2v_sim.h.
//
// What the top-N kernels share (eccknn_topn_kernel in its four centring modes, svd_topn_kernel, which NMF uses too, and
// slope_topn_kernel): the fallback-and-clip of a prediction (also predict_kernel's), the cursor over the
// items an owner has rated, the owner's best-N list in LDS under the one order of n2v_rank.h with the item id as the
// position, and the merge of the S segment lists of an owner.  One wavefront (a 64-thread workgroup) per
// (owner, segment of candidates); every value that steers control flow is the same in all 64 lanes.
#pragma once
#include "n2v_common.h"
#include "n2v_rank.h"
#include "n2v_sim.h"

namespace n2v {

constexpr int TOPN_MAX_SEG = 64;  // segments per owner: one lane each in the merge

// surprise's AlgoBase.predict on one estimate: the training mean where the estimate is impossible, then
// min(higher_bound, est) and max(lower_bound, est).  A NaN becomes hi.
__device__ __forceinline__ double predict_value(double est, bool impossible, double global_mean, double lo, double hi) {
    double e = impossible ? global_mean : est;
    e = (e < hi) ? e : hi;
    e = (e > lo) ? e : lo;
    return e;
}

// The owner-major CSR of the rated items: seen_ptr int64[n_rows + 1], seen_i int32[n] strictly ascending inside a row.
struct Seen {
    const int64_t* ptr; const int32_t* item; int64_t n_rows; int64_t n;
};

// Walks one owner's rated items beside an ascending run of candidates.  Row ranges are clamped to [0, n], so a CSR that
// n2v_eccknn_csr_check would refuse gives wrong lists, never a read outside seen_i[0 .. n).
struct SeenCursor {
    const int32_t* item; int64_t pos, end;
    // owner outside [0, n_rows): nothing is seen.  Positioned at the first entry >= first (one binary search).
    __device__ __forceinline__ void open(const Seen& s, int64_t owner, int64_t first) {
        item = s.item; pos = 0; end = 0;
        if (owner < 0 || owner >= s.n_rows) return;
        const int64_t n = s.n > 0 ? s.n : 0;
        int64_t pb = s.ptr[owner], pe = s.ptr[owner + 1];
        pb = pb < 0 ? 0 : (pb > n ? n : pb);
        pe = pe < pb ? pb : (pe > n ? n : pe);
        int64_t lo = pb, hi = pe;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (item[mid] < first) lo = mid + 1; else hi = mid;
        }
        pos = lo; end = pe;
    }
    // candidates must be asked in ascending order
    __device__ __forceinline__ bool has(int64_t candidate) {
        while (pos < end && item[pos] < candidate) ++pos;
        return pos < end && item[pos] == candidate;
    }
};

// The owner's best-N list in LDS.  It starts as N entries (NaN, POS_NONE): below any real entry, so it is always "full".
struct TopList {
    double* ls; int32_t* lp; int n; uint64_t tk; int tp;
    __device__ __forceinline__ void init(double* s, int32_t* p, int n_, int lane) {
        ls = s; lp = p; n = n_; tk = 0ull; tp = POS_NONE;
        for (int i = lane; i < n; i += 64) { ls[i] = __builtin_nan(""); lp[i] = POS_NONE; }
        __syncthreads();
    }
    // every lane passes the same (score, item)
    __device__ __forceinline__ void offer(double score, int item, int lane) {
        const uint64_t key = order_key(score);
        if (beats(key, item, tk, tp)) list_insert(ls, lp, n, score, item, key, lane, tk, tp);
    }
    __device__ __forceinline__ void store(double* __restrict__ out_s, int32_t* __restrict__ out_p, int lane) const {
        __syncthreads();
        for (int i = lane; i < n; i += 64) { out_s[i] = ls[i]; out_p[i] = lp[i]; }
    }
};

// The candidates [c0, c1) of segment seg of S over n_items.
__device__ __forceinline__ void segment_range(int64_t n_items, int seg, int S, int64_t& c0, int64_t& c1) {
    c0 = n_items * seg / S;
    c1 = n_items * (seg + 1) / S;
}

// One wavefront per owner merges its S segment lists; a missing entry is (-1, NaN).
static __global__ void __launch_bounds__(256)
topn_merge_kernel(const double* __restrict__ part_score, const int32_t* __restrict__ part_pos, int64_t n_owners, int S, int N,
                  int32_t* __restrict__ items, double* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= n_owners) return;
    merge_lists(part_score + o * S * N, part_pos + o * S * N, S, N, lane, items + o * N, score + o * N, -1);
}

// The argument checks every top-N call shares; 0 or the error.
inline int topn_args(const char* who, int64_t n_owners, int64_t n_items, int32_t top_n, int32_t segments,
                     const void* seen_ptr, const void* seen_i, int64_t n_seen, const void* owners, const void* part_score,
                     const void* part_pos, const void* items, const void* score) {
    if (n_owners < 1 || n_owners > 0x7fffffffLL) return fail(N2V_ERR_INVALID, "%s: n_owners %lld outside [1, 2^31)", who, (long long)n_owners);
    if (n_items < 1 || n_items >= (int64_t)POS_NONE) return fail(N2V_ERR_INVALID, "%s: n_items %lld outside [1, 2^31 - 1)", who, (long long)n_items);
    if (top_n < 1 || top_n > N2V_TOPN_MAX_N) return fail(N2V_ERR_INVALID, "%s: top_n %d outside [1, %d]", who, (int)top_n, N2V_TOPN_MAX_N);
    if (segments < 0 || segments > TOPN_MAX_SEG) return fail(N2V_ERR_INVALID, "%s: segments %d outside [0, %d]", who, (int)segments, TOPN_MAX_SEG);
    if (n_seen < 0) return fail(N2V_ERR_INVALID, "%s: n_seen %lld < 0", who, (long long)n_seen);
    if (!seen_ptr || (n_seen > 0 && !seen_i) || !owners || !part_score || !part_pos || !items || !score)
        return fail(N2V_ERR_INVALID, "%s: null pointer", who);
    return N2V_OK;
}

inline int topn_merge(const char* who, const double* part_score, const int32_t* part_pos, int64_t n_owners, int S, int N,
                      int32_t* items, double* score, hipStream_t stream) {
    topn_merge_kernel<<<(unsigned)((n_owners + 3) / 4), 256, 0, stream>>>(part_score, part_pos, n_owners, S, N, items, score);
    return check_launch(who);
}

}  // namespace n2v
