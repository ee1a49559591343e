// Ranking helpers shared by the top-k kernels (n2v_rec.hip, n2v_eccknn.hip, n2v_sim.hip) — gfx950 (MI355X).
//
// The order is ONE total order on (score, position): higher score first, among equal scores the lower position
// (Python's stable sort on the caller's list); -0.0 ties +0.0, NaN is below everything.  Every list comparison is
// beats() on that order, so neither a tile size, a segment count nor the place where a tie group meets a border can
// change a result.
#pragma once
#include <hip/hip_runtime.h>

namespace n2v {

constexpr int POS_NONE = 0x7fffffff;   // position of an empty list entry: (NaN, POS_NONE) is below any real entry

// order-preserving key: larger value <=> larger key; NaN lowest; -0.0 and +0.0 compare equal and share a key
__device__ __forceinline__ uint64_t order_key(double v) {
    if (v != v) return 0ull;
    if (v == 0.0) return 0x8000000000000000ull;
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ uint32_t order_key(float v) {
    if (v != v) return 0u;
    if (v == 0.f) return 0x80000000u;
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// (ka, pa) comes before (kb, pb) in the ranking
__device__ __forceinline__ bool beats(uint64_t ka, int pa, uint64_t kb, int pb) {
    return ka > kb || (ka == kb && pa < pb);
}

// Insert (cs, cp) into the sorted list ls/lp of k entries (the last one falls out), all 64 lanes together: entry i takes
// the candidate or entry i - 1 when it does not come before the candidate.  Chunks of 64 entries from the top down, so an
// entry is read before the chunk below it is written.  tk/tp receive the new last entry.
// S / K: double scores with uint64_t keys (n2v_rec.hip, n2v_eccknn.hip) or float scores with uint32_t keys (n2v_knn.hip).
template <typename S, typename K>
__device__ __forceinline__ void list_insert(S* ls, int32_t* lp, int k, S cs, int cp, K ck, int lane, K& tk, int& tp) {
    const int top = ((k - 1) >> 6) << 6;
    for (int base = top; base >= 0; base -= 64) {
        const int i = base + lane;
        S si = (S)__builtin_nan(""), sm = si;
        int pi = POS_NONE, pm = POS_NONE;
        if (i < k) {
            si = ls[i]; pi = lp[i];
            if (i > 0) { sm = ls[i - 1]; pm = lp[i - 1]; }
        }
        const bool keep = beats(order_key(si), pi, ck, cp);
        const bool prev_before = i == 0 || beats(order_key(sm), pm, ck, cp);
        const S ns = keep ? si : (prev_before ? cs : sm);
        const int np = keep ? pi : (prev_before ? cp : pm);
        if (i < k && !keep) { ls[i] = ns; lp[i] = np; }
        if (base == top) {
            const int last = (k - 1) & 63;
            tk = order_key(__shfl(ns, last, 64));
            tp = __shfl(np, last, 64);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // the stores are seen by this wavefront's next loads
}

// Merge S sorted lists of k entries each (list s at part_score / part_pos + s * k, S <= 64) into the k best of all of
// them, one wavefront: lane s holds the head of list s, and k times the best head leaves.  Entry i goes to ranked[i] /
// score[i]; an empty entry (NaN, POS_NONE) that reaches the result has its position written as `none`.
__device__ __forceinline__ void merge_lists(const double* __restrict__ part_score, const int32_t* __restrict__ part_pos,
                                            int S, int k, int lane, int32_t* __restrict__ ranked,
                                            double* __restrict__ score, int none) {
    const int64_t base = (int64_t)lane * k;
    int h = 0;
    double s = __builtin_nan("");
    int p = POS_NONE;
    if (lane < S) { s = part_score[base]; p = part_pos[base]; }
    for (int i = 0; i < k; ++i) {
        uint64_t bk = order_key(s);
        int bp = p, bl = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t ok = __shfl_xor((unsigned long long)bk, o, 64);
            const int op = __shfl_xor(bp, o, 64), ol = __shfl_xor(bl, o, 64);
            if (beats(ok, op, bk, bp)) { bk = ok; bp = op; bl = ol; }
        }
        bl = __shfl(bl, 0, 64);
        const double ws = __shfl(s, bl, 64);
        const int wp = __shfl(p, bl, 64);
        if (lane == 0) { ranked[i] = wp == POS_NONE ? none : wp; score[i] = ws; }
        if (lane == bl) {
            ++h;
            s = __builtin_nan(""); p = POS_NONE;
            if (h < k) { s = part_score[base + h]; p = part_pos[base + h]; }
        }
    }
}

}  // namespace n2v
