// Matrix factorisation on the device: surprise's SVD (biases + factors, plain SGD) under a deterministic stratified
// schedule.  C-ABI and the full definition: include/n2v_sim.h ("Matrix factorisation"); the restatement the kernels
// equal bit for bit: tests/svd_reference.py.  Parity with surprise itself is UNPINNED (it is not a dependency).
//
//   blocks_check_kernel  integers only: one lane per entry of blk_ptr and per rating, names a malformed block list.
//   epoch_kernel<NS>     one launch per stratum, one wavefront per block (a 64-thread workgroup).  Lane l owns the
//                        factors l + 64 * k, k < NS, of both rows, so a rating is two row reads, one 64-lane xor
//                        butterfly for the dot and two row writes.  The blocks of a stratum share no user and no item:
//                        the wavefronts of one launch touch disjoint rows, and the next stratum is the next launch.
//                        Inside a block the ratings of one user are consecutive, so pu[u] and bu[u] stay in registers
//                        until the user changes, and the next rating's (u, i, r), qi row and bi are fetched before the
//                        current rating's arithmetic; where the next item is the current one, the registers just
//                        computed are handed over instead.  Neither changes an operation or its order.
//   estimate_kernel<NS>  one wavefront per query, the same lane_dot.
//   svd_topn_kernel<NS>  one wavefront per (owner, segment of the items): the best-N unseen items of the owner through
//                        the same lane_dot and estimate_value, without storing the owners x items predictions.
// load_row / store_row / lane_dot are shared with the NMF kernels (n2v_mf_device.h).
// fp64 throughout; -ffp-contract=off (csrc/Makefile) keeps every multiply and add separately rounded.
#include "n2v_common.h"
#include "n2v_mf_device.h"
#include "n2v_sim.h"
#include "n2v_topn.h"

namespace {

constexpr int MAX_FACTORS = n2v::MF_MAX_FACTORS;
constexpr int MAX_STRATA = 32768;

using n2v::clamp64;
using n2v::lane_dot;                                              // n2v_mf_device.h: the rows and the dot
using n2v::load_row;
using n2v::store_row;

// ---- the block list ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) blocks_check_kernel(const int64_t* __restrict__ blk_ptr, const int32_t* __restrict__ blk_u,
                                                           const int32_t* __restrict__ blk_i, int64_t P, int64_t n_users,
                                                           int64_t n_items, int64_t n, int32_t* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n_blk = P * P;
    int32_t bits = 0;
    if (t < n_blk) {
        const int64_t pb = blk_ptr[t], pe = blk_ptr[t + 1];
        if (pb < 0 || pb > n || pe < 0 || pe > n || pe < pb || (t == 0 && pb != 0)) bits |= N2V_SVD_BAD_PTR;
        if (t == n_blk - 1 && pe != n) bits |= N2V_SVD_BAD_END;
    }
    if (t < n) {
        const int64_t u = blk_u[t], i = blk_i[t];
        if (u < 0 || u >= n_users || i < 0 || i >= n_items) {
            bits |= N2V_SVD_BAD_ID;
        } else {
            const int64_t ub = (u * P) / n_users, ib = (i * P) / n_items;
            const int64_t k = ((ib - ub + P) % P) * P + ub;       // < P * P
            const int64_t pb = blk_ptr[k];
            if (t < pb || t >= blk_ptr[k + 1]) bits |= N2V_SVD_WRONG_BLOCK;
            else if (t > pb && t > 0 && blk_u[t - 1] > u) bits |= N2V_SVD_UNSORTED;
        }
    }
    if (bits) atomicOr(status, bits);
}

// ---- one stratum ------------------------------------------------------------------------------------------------------

struct EpochArgs {
    const int64_t* blk_ptr; const int32_t* blk_u; const int32_t* blk_i; const double* blk_r;
    int64_t P, s, n_users, n_items, n;
    int nf, biased;
    double mu, lr_bu, lr_bi, lr_pu, lr_qi, reg_bu, reg_bi, reg_pu, reg_qi;
    double* bu; double* bi; double* pu; double* qi;
};

template <int NS>
__global__ void __launch_bounds__(64) epoch_kernel(EpochArgs a) {
    const int lane = threadIdx.x;
    const int nf = a.nf;
    const int64_t blk = a.s * a.P + blockIdx.x;
    const int64_t pb = clamp64(a.blk_ptr[blk], 0, a.n), pe = clamp64(a.blk_ptr[blk + 1], pb, a.n);
    if (pb >= pe) return;

    int64_t cu = -1;                                              // the user whose row is in p / b_u
    double p[NS], b_u = 0.0;
    // the next rating, fetched one rating ahead
    int64_t u_n = a.blk_u[pb], i_n = a.blk_i[pb];
    double r_n = a.blk_r[pb], q_n[NS], b_in = 0.0;
    bool ok_n = u_n >= 0 && u_n < a.n_users && i_n >= 0 && i_n < a.n_items;
    if (ok_n) {
        load_row<NS>(a.qi + i_n * nf, nf, lane, q_n);
        if (a.biased) b_in = a.bi[i_n];
    }
    for (int64_t pos = pb; pos < pe; ++pos) {
        const int64_t u = u_n, i = i_n;
        const double r = r_n;
        const bool ok = ok_n, more = pos + 1 < pe;
        double q[NS], b_i = b_in;
#pragma unroll
        for (int k = 0; k < NS; ++k) q[k] = q_n[k];
        if (ok && u != cu) {                                      // the user changes: write the old row, read the new one
            if (cu >= 0) {
                store_row<NS>(a.pu + cu * nf, nf, lane, p);
                if (a.biased && lane == 0) a.bu[cu] = b_u;
            }
            load_row<NS>(a.pu + u * nf, nf, lane, p);
            if (a.biased) b_u = a.bu[u];
            cu = u;
        }
        if (more) {
            u_n = a.blk_u[pos + 1]; i_n = a.blk_i[pos + 1]; r_n = a.blk_r[pos + 1];
            ok_n = u_n >= 0 && u_n < a.n_users && i_n >= 0 && i_n < a.n_items;
            if (ok_n && !(ok && i_n == i)) {                      // the same item: handed over below
                load_row<NS>(a.qi + i_n * nf, nf, lane, q_n);
                if (a.biased) b_in = a.bi[i_n];
            }
        }
        if (!ok) continue;                                        // only a list that fails blocks_check has one

        const double dot = lane_dot<NS>(q, p, nf, lane);
        const double err = a.biased ? r - (((a.mu + b_u) + b_i) + dot) : r - dot;
        if (a.biased) {
            b_u = b_u + a.lr_bu * (err - a.reg_bu * b_u);
            b_i = b_i + a.lr_bi * (err - a.reg_bi * b_i);
            if (lane == 0) a.bi[i] = b_i;
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const double puf = p[k], qif = q[k];
            p[k] = puf + a.lr_pu * (err * qif - a.reg_pu * puf);
            q[k] = qif + a.lr_qi * (err * puf - a.reg_qi * qif);
        }
        store_row<NS>(a.qi + i * nf, nf, lane, q);
        if (more && ok_n && i_n == i) {
#pragma unroll
            for (int k = 0; k < NS; ++k) q_n[k] = q[k];
            b_in = b_i;
        }
    }
    if (cu >= 0) {
        store_row<NS>(a.pu + cu * nf, nf, lane, p);
        if (a.biased && lane == 0) a.bu[cu] = b_u;
    }
}

// ---- estimate ---------------------------------------------------------------------------------------------------------

struct Model {
    const double* bu; const double* bi; const double* pu; const double* qi;
    int64_t n_users, n_items;
    int nf, biased;
    double mu;
};

// The estimate from the dot, the one copy behind estimate_kernel and svd_topn_kernel: ku / ki say whether u / i are
// inside their tables, dot is lane_dot of the two rows when both are.  Returns true where the estimate is impossible.
__device__ __forceinline__ bool estimate_value(const Model& m, bool ku, bool ki, int64_t u, int64_t i, double dot, double& est) {
    bool imp = false;
    if (m.biased) {
        est = m.mu;
        if (ku) est = est + m.bu[u];
        if (ki) est = est + m.bi[i];
        if (ku && ki) est = est + dot;
    } else {
        imp = !(ku && ki);                                        // 'User and item are unknown.'
        est = imp ? 0.0 : dot;
    }
    return imp;
}

struct EstArgs {
    Model m; int64_t n_q;
    const int32_t* q_u; const int32_t* q_i;
    double* est; uint8_t* impossible;
};

template <int NS>
__global__ void __launch_bounds__(64) estimate_kernel(EstArgs a) {
    const int lane = threadIdx.x;
    const int64_t qn = blockIdx.x;
    const int64_t u = a.q_u[qn], i = a.q_i[qn];
    const bool ku = u >= 0 && u < a.m.n_users, ki = i >= 0 && i < a.m.n_items;
    double dot = 0.0;
    if (ku && ki) {                                               // wave-uniform
        double p[NS], q[NS];
        load_row<NS>(a.m.pu + u * a.m.nf, a.m.nf, lane, p);
        load_row<NS>(a.m.qi + i * a.m.nf, a.m.nf, lane, q);
        dot = lane_dot<NS>(q, p, a.m.nf, lane);
    }
    if (lane != 0) return;
    double est;
    const bool imp = estimate_value(a.m, ku, ki, u, i, dot, est);
    a.est[qn] = est;
    a.impossible[qn] = imp ? 1 : 0;
}

// ---- top-N ------------------------------------------------------------------------------------------------------------

struct TopnArgs {
    Model m; n2v::Seen seen;
    const int32_t* owners; int N; int S;
    double global_mean, lo, hi;
    double* part_score; int32_t* part_pos;
};

// One wavefront per (owner, segment of the items), the frame of eccknn_topn_kernel (n2v_topn.h): the owner's p row is
// loaded once, every unseen item of the segment is one q row, the same lane_dot and estimate_value as estimate_kernel,
// the fallback and clip of predict_value, and a fold into the segment's best-N list.
template <int NS>
__global__ void __launch_bounds__(64) svd_topn_kernel(TopnArgs a) {
    __shared__ double ts[N2V_TOPN_MAX_N];
    __shared__ int32_t tp[N2V_TOPN_MAX_N];
    const int64_t o = blockIdx.x;
    const int seg = blockIdx.y, lane = threadIdx.x;
    const int64_t u = a.owners[o];
    const bool ku = u >= 0 && u < a.m.n_users;
    int64_t c0, c1;
    n2v::segment_range(a.m.n_items, seg, a.S, c0, c1);
    n2v::SeenCursor cur;
    cur.open(a.seen, u, c0);
    n2v::TopList top;
    top.init(ts, tp, a.N, lane);
    double p[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) p[k] = 0.0;
    if (ku) load_row<NS>(a.m.pu + u * a.m.nf, a.m.nf, lane, p);
    for (int64_t i = c0; i < c1; ++i) {
        if (cur.has(i)) continue;
        double dot = 0.0;
        if (ku) {
            double q[NS];
            load_row<NS>(a.m.qi + i * a.m.nf, a.m.nf, lane, q);
            dot = lane_dot<NS>(q, p, a.m.nf, lane);
        }
        double est;
        const bool imp = estimate_value(a.m, ku, true, u, i, dot, est);
        top.offer(n2v::predict_value(est, imp, a.global_mean, a.lo, a.hi), (int)i, lane);
    }
    const int64_t base = (o * a.S + seg) * a.N;
    top.store(a.part_score + base, a.part_pos + base, lane);
}

}  // namespace

extern "C" {

int32_t n2v_svd_max_factors(void) { return MAX_FACTORS; }
int32_t n2v_svd_max_strata(void) { return MAX_STRATA; }

int n2v_svd_blocks_check(const int64_t* blk_ptr, const int32_t* blk_u, const int32_t* blk_i, int64_t n_strata,
                         int64_t n_users, int64_t n_items, int64_t n, int32_t* status, void* stream) {
    if (n_strata < 1 || n_strata > MAX_STRATA || n_users < 1 || n_items < 1 || n < 1 || n_users > 0x7fffffffLL ||
        n_items > 0x7fffffffLL)
        return n2v::fail(N2V_ERR_INVALID, "svd_blocks_check: n_strata=%lld n_users=%lld n_items=%lld n=%lld", (long long)n_strata,
                         (long long)n_users, (long long)n_items, (long long)n);
    if (!blk_ptr || !blk_u || !blk_i || !status) return n2v::fail(N2V_ERR_INVALID, "svd_blocks_check: null pointer");
    const int64_t lanes = n_strata * n_strata > n ? n_strata * n_strata : n;
    if (lanes > (int64_t)0x7fffffff * 256) return n2v::fail(N2V_ERR_INVALID, "svd_blocks_check: too many blocks or ratings");
    blocks_check_kernel<<<n2v::grid_for(lanes, 256), 256, 0, (hipStream_t)stream>>>(blk_ptr, blk_u, blk_i, n_strata, n_users,
                                                                                   n_items, n, status);
    return n2v::check_launch("svd_blocks_check");
}

int n2v_svd_epoch(const int64_t* blk_ptr, const int32_t* blk_u, const int32_t* blk_i, const double* blk_r,
                  int64_t n_strata, int64_t n_users, int64_t n_items, int64_t n, int32_t n_factors, double mu,
                  int32_t biased, double lr_bu, double lr_bi, double lr_pu, double lr_qi, double reg_bu, double reg_bi,
                  double reg_pu, double reg_qi, double* bu, double* bi, double* pu, double* qi, void* stream) {
    if (n_strata < 1 || n_strata > MAX_STRATA || n_users < 1 || n_items < 1 || n < 1 || n_users > 0x7fffffffLL ||
        n_items > 0x7fffffffLL)
        return n2v::fail(N2V_ERR_INVALID, "svd_epoch: n_strata=%lld n_users=%lld n_items=%lld n=%lld", (long long)n_strata,
                         (long long)n_users, (long long)n_items, (long long)n);
    if (n_factors < 1 || n_factors > MAX_FACTORS)
        return n2v::fail(N2V_ERR_INVALID, "svd_epoch: n_factors %d outside [1, %d]", n_factors, MAX_FACTORS);
    if (!blk_ptr || !blk_u || !blk_i || !blk_r || !pu || !qi || (biased && (!bu || !bi)))
        return n2v::fail(N2V_ERR_INVALID, "svd_epoch: null pointer");
    EpochArgs a{blk_ptr, blk_u, blk_i, blk_r, n_strata, 0, n_users, n_items, n, n_factors, biased ? 1 : 0, mu,
                lr_bu, lr_bi, lr_pu, lr_qi, reg_bu, reg_bi, reg_pu, reg_qi, bu, bi, pu, qi};
    for (int64_t s = 0; s < n_strata; ++s) {                      // stream order is the barrier between strata
        a.s = s;
        N2V_MF_DISPATCH(epoch_kernel, n_factors, <<<(unsigned)n_strata, 64, 0, (hipStream_t)stream>>>(a));
    }
    return n2v::check_launch("svd_epoch");
}

int n2v_svd_estimate(const double* bu, const double* bi, const double* pu, const double* qi, int64_t n_users,
                     int64_t n_items, int32_t n_factors, double mu, int32_t biased, const int32_t* q_u, const int32_t* q_i,
                     int64_t n_q, double* est, uint8_t* impossible, void* stream) {
    if (n_users < 1 || n_items < 1 || n_q < 1 || n_q > 0x7fffffffLL)
        return n2v::fail(N2V_ERR_INVALID, "svd_estimate: n_users=%lld n_items=%lld n_q=%lld", (long long)n_users,
                         (long long)n_items, (long long)n_q);
    if (n_factors < 1 || n_factors > MAX_FACTORS)
        return n2v::fail(N2V_ERR_INVALID, "svd_estimate: n_factors %d outside [1, %d]", n_factors, MAX_FACTORS);
    if (!pu || !qi || !q_u || !q_i || !est || !impossible || (biased && (!bu || !bi)))
        return n2v::fail(N2V_ERR_INVALID, "svd_estimate: null pointer");
    EstArgs a{Model{bu, bi, pu, qi, n_users, n_items, n_factors, biased ? 1 : 0, mu}, n_q, q_u, q_i, est, impossible};
    N2V_MF_DISPATCH(estimate_kernel, n_factors, <<<(unsigned)n_q, 64, 0, (hipStream_t)stream>>>(a));
    return n2v::check_launch("svd_estimate");
}

int n2v_svd_topn(const double* bu, const double* bi, const double* pu, const double* qi, int64_t n_users, int64_t n_items,
                 int32_t n_factors, double mu, int32_t biased, const int64_t* seen_ptr, const int32_t* seen_i, int64_t n_seen,
                 const int32_t* owners, int64_t n_owners, double global_mean, double lo, double hi, int32_t top_n,
                 int32_t segments, double* part_score, int32_t* part_pos, int32_t* items, double* score, void* stream) {
    if (n_users < 1 || n_items < 1) return n2v::fail(N2V_ERR_INVALID, "svd_topn: n_users=%lld n_items=%lld", (long long)n_users, (long long)n_items);
    if (n_factors < 1 || n_factors > MAX_FACTORS)
        return n2v::fail(N2V_ERR_INVALID, "svd_topn: n_factors %d outside [1, %d]", n_factors, MAX_FACTORS);
    if (const int rc = n2v::topn_args("svd_topn", n_owners, n_items, top_n, segments, seen_ptr, seen_i, n_seen, owners,
                                      part_score, part_pos, items, score))
        return rc;
    if (!pu || !qi || (biased && (!bu || !bi))) return n2v::fail(N2V_ERR_INVALID, "svd_topn: null pointer");
    const int S = segments > 0 ? segments : n2v_topn_segments(n_owners, n_items);
    TopnArgs a{Model{bu, bi, pu, qi, n_users, n_items, n_factors, biased ? 1 : 0, mu}, n2v::Seen{seen_ptr, seen_i, n_users, n_seen},
               owners, top_n, S, global_mean, lo, hi, part_score, part_pos};
    N2V_MF_DISPATCH(svd_topn_kernel, n_factors, <<<dim3((unsigned)n_owners, (unsigned)S), 64, 0, (hipStream_t)stream>>>(a));
    if (const int rc = n2v::check_launch("svd_topn")) return rc;
    return n2v::topn_merge("svd_topn (merge)", part_score, part_pos, n_owners, S, top_n, items, score, (hipStream_t)stream);
}

}  // extern "C"
