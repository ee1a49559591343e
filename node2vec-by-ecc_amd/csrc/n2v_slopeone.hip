// SlopeOne rating prediction from the item-deviation table — gfx950 (MI355X).  C-ABI: include/n2v_sim.h.
//
// surprise 1.0.6's SlopeOne, restated (tests/slopeone_reference.py is the definition; parity with surprise itself is
// unpinned).  The table dev / freq is a method of the tile kernels of n2v_eccknn.hip; this file holds its two readers.
//   slope_estimate_kernel  one wavefront per query (u, i): the lanes fetch freq[i][j] and dev[i][j] for 64 entries j of
//                    ur[u] at a time, and the usable ones (freq > 0) are added one after the other in list order, the
//                    pattern of baselines_kernel.  est = mu[u] + s / n, or mu[u] where n is 0.
//   slope_topn_kernel  one wavefront per (owner, segment of the items), 64 neighbouring candidates at a time, one a lane.
//                    The owner's rated items pass through LDS in chunks, in training order; for each of them, j, the lanes
//                    read freq[j][c0 + lane] and dev[j][c0 + lane], two contiguous pieces of row j, and every lane adds
//                    -dev[j][c], which has the bits of dev[c][j] (the table's lower half is the negation of its upper
//                    half), to its own sum: the estimate kernel's order for every candidate at once, with no gather and
//                    no selection list.  Rated candidates are masked by a search of the seen CSR per lane; the others go
//                    through predict_value and are offered to the segment's best-N list in ascending item order, each
//                    offer wave-uniform (a ballot of the lanes that would enter, then one broadcast per set bit).
//                    Nothing of size owners x items is stored; the S segment lists merge as in the other top-N kernels.
// Every value that steers a loop or reaches a barrier is the same in all 64 lanes.
#include "n2v_common.h"
#include "n2v_sim.h"
#include "n2v_rank.h"
#include "n2v_topn.h"

namespace {

using n2v::beats, n2v::order_key, n2v::predict_value, n2v::Seen, n2v::TopList, n2v::uni;

constexpr int64_t MAX_TABLE = (int64_t)1 << 31;   // elements of dev: 16 GiB of fp64
constexpr int UC = 1024;                          // entries of ur[u] staged in LDS at a time

struct SlopeModel {
    const double* dev; const int32_t* freq; int64_t n_items;
    const int64_t* ur_ptr; const int32_t* ur_i; int64_t n_users; int64_t n; const double* mu;
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The list of user u inside [0, n]; an unknown user has none.
__device__ __forceinline__ void user_range(const SlopeModel& m, int64_t u, int64_t& pb, int64_t& pe) {
    pb = 0; pe = 0;
    if (u < 0 || u >= m.n_users) return;
    pb = clamp64(m.ur_ptr[u], 0, m.n);
    pe = clamp64(m.ur_ptr[u + 1], pb, m.n);
}

__device__ __forceinline__ double slope_finish(double mu, double s, int n) { return n == 0 ? mu : mu + s / (double)n; }

// ---- estimate ---------------------------------------------------------------------------------------------------------

struct SlopeEstArgs {
    SlopeModel m; const int32_t* qu; const int32_t* qi; double* est; int32_t* n_dev; uint8_t* impossible;
};

__global__ void __launch_bounds__(64) slope_estimate_kernel(SlopeEstArgs a) {
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t u = a.qu[q], i = a.qi[q];
    if (u < 0 || u >= a.m.n_users || i < 0 || i >= a.m.n_items) {    // 'User and/or item is unkown.'
        if (lane == 0) { a.est[q] = 0.0; a.n_dev[q] = 0; a.impossible[q] = 1; }
        return;
    }
    int64_t pb, pe;
    user_range(a.m, u, pb, pe);
    const double* drow = a.m.dev + i * a.m.n_items;
    const int32_t* frow = a.m.freq + i * a.m.n_items;
    double sum = 0.0;
    int cnt = 0;
    for (int64_t base = pb; base < pe; base += 64) {
        const int64_t p = base + lane;
        double term = 0.0;
        bool in = false;
        if (p < pe) {
            const int64_t j = a.m.ur_i[p];
            if (j >= 0 && j < a.m.n_items && frow[j] > 0) { in = true; term = drow[j]; }
        }
        unsigned long long have = __ballot(in);
        cnt += __popcll(have);
        while (have) {                                            // in list order; wave-uniform
            const int src = __ffsll((long long)have) - 1;
            have &= have - 1;
            sum = sum + __shfl(term, src, 64);
        }
    }
    if (lane == 0) { a.est[q] = slope_finish(a.m.mu[u], sum, cnt); a.n_dev[q] = cnt; a.impossible[q] = 0; }
}

// ---- top-N ------------------------------------------------------------------------------------------------------------

struct SlopeTopnArgs {
    SlopeModel m; Seen seen; const int32_t* owners; int N; int S;
    double global_mean, lo, hi;
    double* part_score; int32_t* part_pos;
};

// Is item c among the rated items [sb, se) of the owner (ascending)?
__device__ __forceinline__ bool seen_has(const int32_t* __restrict__ item, int64_t sb, int64_t se, int64_t c) {
    int64_t lo = sb, hi = se;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (item[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo < se && item[lo] == c;
}

// freq[j][c] and dev[j][c] of the lane's candidate; a lane outside the segment and an entry that is no item read nothing.
__device__ __forceinline__ void slope_fetch(const SlopeModel& m, int64_t j, int64_t c, bool inside, int32_t& f, double& d) {
    f = 0; d = 0.0;
    if (inside && j >= 0) { f = m.freq[j * m.n_items + c]; d = m.dev[j * m.n_items + c]; }
}
// One term of the estimate of (u, c): dev[c][j] is +0.0 on the diagonal and -dev[j][c] elsewhere.
__device__ __forceinline__ void slope_add(int64_t j, int64_t c, int32_t f, double d, double& s, int& n) {
    const double t = j == c ? 0.0 : -d;
    n += f > 0 ? 1 : 0;
    s = f > 0 ? s + t : s;
}

__global__ void __launch_bounds__(64) slope_topn_kernel(SlopeTopnArgs a) {
    __shared__ int32_t uj[UC];                                    // a chunk of ur[u]; -1: an id outside [0, n_items)
    __shared__ double ts[N2V_TOPN_MAX_N];
    __shared__ int32_t tp[N2V_TOPN_MAX_N];
    const int64_t o = blockIdx.x;
    const int seg = blockIdx.y, lane = threadIdx.x;
    const int64_t u = a.owners[o];
    const int64_t n_items = a.m.n_items;
    const bool known = u >= 0 && u < a.m.n_users;
    int64_t c0, c1;
    n2v::segment_range(n_items, seg, a.S, c0, c1);
    int64_t pb, pe;
    user_range(a.m, u, pb, pe);
    int64_t sb = 0, se = 0;                                       // the owner's row of the seen CSR, inside [0, n_seen]
    if (u >= 0 && u < a.seen.n_rows) {
        const int64_t ns = a.seen.n > 0 ? a.seen.n : 0;
        sb = clamp64(a.seen.ptr[u], 0, ns);
        se = clamp64(a.seen.ptr[u + 1], sb, ns);
    }
    const double mu = known ? a.m.mu[u] : 0.0;
    TopList top;
    top.init(ts, tp, a.N, lane);
    const bool one_chunk = pe - pb <= UC;                         // then the list is staged once for every block
    int64_t staged = -1;                                          // the list position uj[0] holds
    for (int64_t cb = c0; cb < c1; cb += 64) {
        const int64_t c = cb + lane;
        const bool inside = c < c1;
        double s = 0.0;
        int n = 0;
        for (int64_t base = pb; base < pe; base += UC) {
            const int len = pe - base < UC ? (int)(pe - base) : UC;
            if (!(one_chunk && staged == base)) {
                __syncthreads();                                  // the previous chunk has been read
                for (int e = lane; e < len; e += 64) {
                    const int32_t j = a.m.ur_i[base + e];
                    uj[e] = (j >= 0 && j < n_items) ? j : -1;
                }
                __syncthreads();
                staged = base;
            }
            int e = 0;
            for (; e + 4 <= len; e += 4) {                        // four rows' loads in flight, then their adds in order
                int64_t j[4];
                int32_t f[4];
                double d[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { j[k] = uni(uj[e + k]); slope_fetch(a.m, j[k], c, inside, f[k], d[k]); }
#pragma unroll
                for (int k = 0; k < 4; ++k) slope_add(j[k], c, f[k], d[k], s, n);
            }
            for (; e < len; ++e) {                                // training order: the order of every lane's sum
                const int64_t j = uni(uj[e]);
                int32_t f;
                double d;
                slope_fetch(a.m, j, c, inside, f, d);
                slope_add(j, c, f, d, s, n);
            }
        }
        const bool cand = inside && !seen_has(a.seen.item, sb, se, c);
        const double score = predict_value(slope_finish(mu, s, n), !known, a.global_mean, a.lo, a.hi);
        unsigned long long offer = __ballot(cand && beats(order_key(score), (int)c, top.tk, top.tp));
        while (offer) {                                           // ascending item id; wave-uniform
            const int src = __ffsll((long long)offer) - 1;
            offer &= offer - 1;
            top.offer(__shfl(score, src, 64), (int)(cb + src), lane);
        }
    }
    const int64_t out = (o * a.S + seg) * a.N;
    top.store(a.part_score + out, a.part_pos + out, lane);
}

// The checks the two calls share; 0 or the error.
int model_args(const char* who, const double* dev, const int32_t* freq, int64_t n_items, const int64_t* ur_ptr,
               const int32_t* ur_i, int64_t n_users, int64_t n, const double* user_mean) {
    if (n_items < 1 || n_users < 1 || n_users > 0x7fffffff || n < 0)
        return n2v::fail(N2V_ERR_INVALID, "%s: n_items=%lld n_users=%lld n=%lld", who, (long long)n_items, (long long)n_users, (long long)n);
    if (n_items > 65535 || n_items * n_items > MAX_TABLE)
        return n2v::fail(N2V_ERR_INVALID, "%s: n_items^2 = %lld^2 exceeds the table limit of %lld elements", who,
                         (long long)n_items, (long long)MAX_TABLE);
    if (!dev || !freq || !ur_ptr || !user_mean || (n > 0 && !ur_i)) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer", who);
    return N2V_OK;
}

}  // namespace

extern "C" {

int n2v_slopeone_estimate(const double* dev, const int32_t* freq, int64_t n_items, const int64_t* ur_ptr, const int32_t* ur_i,
                          int64_t n_users, int64_t n, const double* user_mean, const int32_t* q_u, const int32_t* q_i,
                          int64_t n_q, double* est, int32_t* n_dev, uint8_t* impossible, void* stream) {
    if (n_q < 1 || n_q > 0x7fffffff) return n2v::fail(N2V_ERR_INVALID, "slopeone_estimate: n_q %lld outside [1, 2^31)", (long long)n_q);
    if (const int rc = model_args("slopeone_estimate", dev, freq, n_items, ur_ptr, ur_i, n_users, n, user_mean)) return rc;
    if (!q_u || !q_i || !est || !n_dev || !impossible) return n2v::fail(N2V_ERR_INVALID, "slopeone_estimate: null pointer");
    SlopeEstArgs a{SlopeModel{dev, freq, n_items, ur_ptr, ur_i, n_users, n, user_mean}, q_u, q_i, est, n_dev, impossible};
    slope_estimate_kernel<<<(unsigned)n_q, 64, 0, (hipStream_t)stream>>>(a);
    return n2v::check_launch("slopeone_estimate");
}

int n2v_slopeone_topn(const double* dev, const int32_t* freq, int64_t n_items, const int64_t* ur_ptr, const int32_t* ur_i,
                      int64_t n_users, int64_t n, const double* user_mean, const int64_t* seen_ptr, const int32_t* seen_i,
                      int64_t n_seen, const int32_t* owners, int64_t n_owners, double global_mean, double lo, double hi,
                      int32_t top_n, int32_t segments, double* part_score, int32_t* part_pos, int32_t* items, double* score,
                      void* stream) {
    if (const int rc = model_args("slopeone_topn", dev, freq, n_items, ur_ptr, ur_i, n_users, n, user_mean)) return rc;
    if (const int rc = n2v::topn_args("slopeone_topn", n_owners, n_items, top_n, segments, seen_ptr, seen_i, n_seen, owners,
                                      part_score, part_pos, items, score))
        return rc;
    const int S = segments > 0 ? segments : n2v_topn_segments(n_owners, n_items);
    SlopeTopnArgs a{SlopeModel{dev, freq, n_items, ur_ptr, ur_i, n_users, n, user_mean}, Seen{seen_ptr, seen_i, n_users, n_seen},
                    owners, top_n, S, global_mean, lo, hi, part_score, part_pos};
    slope_topn_kernel<<<dim3((unsigned)n_owners, (unsigned)S), 64, 0, (hipStream_t)stream>>>(a);
    if (const int rc = n2v::check_launch("slopeone_topn")) return rc;
    return n2v::topn_merge("slopeone_topn (merge)", part_score, part_pos, n_owners, S, top_n, items, score, (hipStream_t)stream);
}

}  // extern "C"
