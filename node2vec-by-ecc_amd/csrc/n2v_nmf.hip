// Non-negative matrix factorisation on the device: surprise's NMF (Luo et al. 2014, unbiased), whose multiplicative
// update freezes both factor tables for an epoch, so it trains in surprise's own order, one wavefront per row.  C-ABI and
// the full definition: include/n2v_sim.h ("Non-negative matrix factorisation"); the restatement the kernels equal bit
// for bit: tests/nmf_reference.py.  Parity with surprise itself is UNPINNED (it is not a dependency).
//
//   lists_check_kernel   integers only: one lane per row and per entry of one row-major list; names a malformed list and
//                        counts every id of the list, lists_count_kernel then holds the counts against the row lengths of
//                        the transposed list.
//   nmf_pass_kernel<NS>  one wavefront per row (a 64-thread workgroup) of either side: the first n_users workgroups are
//                        the user pass, the others the item pass; both read the old tables only and write pu_out /
//                        qi_out.  Lane l owns the factors l + 64 * k, k < NS, of the own row and of the two accumulators,
//                        all in registers.  The list's ids and ratings arrive 64 entries a load (lane j holds entry j of
//                        the chunk, the next chunk is in flight) and are broadcast from there, so an entry's row of the
//                        other table needs one memory round trip, and it is fetched DEPTH entries ahead of its use: the
//                        chain of adds into num / den never waits for a load it could have issued earlier.  An entry is
//                        one row read, one lane_dot (n2v_mf_device.h, the SVD kernels' own) and two multiply-adds per
//                        owned factor.  A row is never split: the order of the sum is the definition.
// fp64 throughout; -ffp-contract=off (csrc/Makefile) keeps every multiply and add separately rounded.
#include "n2v_common.h"
#include "n2v_mf_device.h"
#include "n2v_sim.h"

namespace {

constexpr int MAX_FACTORS = n2v::MF_MAX_FACTORS;
constexpr int DEPTH = 4;                                          // rows of the other table in flight; divides 64

using n2v::clamp64;
using n2v::lane_dot;
using n2v::load_row;
using n2v::store_row;

// ---- the lists --------------------------------------------------------------------------------------------------------

// One lane per row and per entry of the list (ptr int64[n_rows + 1], other int32[n]); count[id] += 1 per in-range id.
__global__ void __launch_bounds__(256) lists_check_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ other,
                                                          int64_t n_rows, int64_t n_other, int64_t n, int ascending,
                                                          int32_t* __restrict__ count, int32_t* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t bits = 0;
    if (t < n_rows) {
        const int64_t pb = ptr[t], pe = ptr[t + 1];
        if (pb < 0 || pb > n || pe < 0 || pe > n || pe < pb || (t == 0 && pb != 0)) bits |= N2V_NMF_BAD_PTR;
        if (t == n_rows - 1 && pe != n) bits |= N2V_NMF_BAD_END;
    }
    if (t < n) {
        const int64_t id = other[t];
        if (id < 0 || id >= n_other) bits |= N2V_NMF_BAD_ID;
        else atomicAdd(count + id, 1);
        if (ascending && t > 0 && other[t - 1] >= id) {           // legal only where a row starts at t
            int64_t lo = 0, hi = n_rows + 1;                      // first k in [0, n_rows] with ptr[k] >= t
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (ptr[mid] < t) lo = mid + 1; else hi = mid;
            }
            if (lo > n_rows || ptr[lo] != t) bits |= N2V_NMF_UNSORTED;
        }
    }
    if (bits) atomicOr(status, bits);
}

// count[row] of one list's ids against the row lengths of the transposed list.
__global__ void __launch_bounds__(256) lists_count_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ count,
                                                          int64_t n_rows, int32_t* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_rows && ptr[t + 1] - ptr[t] != (int64_t)count[t]) atomicOr(status, N2V_NMF_BAD_COUNT);
}

// ---- one pass ---------------------------------------------------------------------------------------------------------

struct PassArgs {
    const int64_t* ptr; const int32_t* other; const double* r; const int32_t* order;
    int64_t n_rows, n_other, n;
    double reg;
    const double* own; const double* oth; double* out;
};

// Lane `j` of a wave-uniform index: the value of that lane in every lane.
__device__ __forceinline__ int bcast(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ double bcast(double v, int j) {
    return __hiloint2double(bcast(__double2hiint(v), j), bcast(__double2loint(v), j));
}

template <int NS>
__device__ __forceinline__ void nmf_row(const PassArgs& a, int64_t slot, int nf, int lane) {
    const int64_t row = a.order ? (int64_t)a.order[slot] : slot;
    if (row < 0 || row >= a.n_rows) return;                       // only an order table that is no permutation has one
    const int64_t pb = clamp64(a.ptr[row], 0, a.n), pe = clamp64(a.ptr[row + 1], pb, a.n);

    double p[NS], num[NS], den[NS];
    load_row<NS>(a.own + row * nf, nf, lane, p);
#pragma unroll
    for (int k = 0; k < NS; ++k) num[k] = den[k] = 0.0;

    // entry base + lane of the list: id -1 (skipped) past the end
    auto load_chunk = [&](int64_t base, int& id, double& r) {
        const bool in = base + lane < pe;
        id = in ? a.other[base + lane] : -1;
        r = in ? a.r[base + lane] : 0.0;
    };
    int id_c, id_n;
    double r_c, r_n;
    load_chunk(pb, id_c, r_c);
    load_chunk(pb + 64, id_n, r_n);
    double qn[DEPTH][NS];                                         // slot d: the row of the chunk's entries d, d + DEPTH, ...
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
        const int64_t id = bcast(id_c, d);
#pragma unroll
        for (int k = 0; k < NS; ++k) qn[d][k] = 0.0;
        if (id >= 0 && id < a.n_other) load_row<NS>(a.oth + id * nf, nf, lane, qn[d]);
    }
    for (int64_t base = pb; base < pe; base += 64) {
        const int cnt = pe - base < 64 ? (int)(pe - base) : 64;
        for (int j0 = 0; j0 < cnt; j0 += DEPTH) {
            if (j0 + DEPTH <= cnt) {
                // A full group, without a branch between its entries: the DEPTH dots depend on neither each other nor
                // num / den, so their butterflies overlap; only the adds below are a chain.  The same operations on the
                // same values as the loop after it, in the same order per accumulator.
                double q[DEPTH][NS], r[DEPTH], est[DEPTH];
                bool ok[DEPTH];
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) {
                    const int64_t id = bcast(id_c, j0 + d);
                    r[d] = bcast(r_c, j0 + d);
                    ok[d] = id >= 0 && id < a.n_other;
#pragma unroll
                    for (int k = 0; k < NS; ++k) q[d][k] = qn[d][k];
                    const int jn = j0 + d + DEPTH;
                    const int64_t idn = jn < 64 ? bcast(id_c, jn) : bcast(id_n, jn - 64);
                    if (idn >= 0 && idn < a.n_other) load_row<NS>(a.oth + idn * nf, nf, lane, qn[d]);
                }
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) est[d] = lane_dot<NS>(q[d], p, nf, lane);
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) {
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        num[k] = ok[d] ? num[k] + q[d][k] * r[d] : num[k];
                        den[k] = ok[d] ? den[k] + q[d][k] * est[d] : den[k];
                    }
                }
                continue;
            }
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {                     // the last, short group of the list
                const int j = j0 + d;
                if (j >= cnt) break;
                const int64_t id = bcast(id_c, j);
                const double r = bcast(r_c, j);
                double q[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) q[k] = qn[d][k];
                const int jn = j + DEPTH;                         // the entry DEPTH ahead takes the slot over
                const int64_t idn = jn < 64 ? bcast(id_c, jn) : bcast(id_n, jn - 64);
                if (idn >= 0 && idn < a.n_other) load_row<NS>(a.oth + idn * nf, nf, lane, qn[d]);
                if (id < 0 || id >= a.n_other) continue;          // only a list that fails the check has one
                const double est = lane_dot<NS>(q, p, nf, lane);
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    num[k] = num[k] + q[k] * r;
                    den[k] = den[k] + q[k] * est;
                }
            }
        }
        id_c = id_n; r_c = r_n;
        load_chunk(base + 128, id_n, r_n);
    }
    const double nreg = (double)(pe - pb) * a.reg;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        den[k] = den[k] + nreg * p[k];
        p[k] = p[k] * (num[k] / den[k]);
    }
    store_row<NS>(a.out + row * nf, nf, lane, p);
}

template <int NS>
__global__ void __launch_bounds__(64) nmf_pass_kernel(PassArgs users, PassArgs items, int nf) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (b < users.n_rows) nmf_row<NS>(users, b, nf, lane);
    else nmf_row<NS>(items, b - users.n_rows, nf, lane);
}

bool overlap(const double* a, int64_t na, const double* b, int64_t nb) { return a < b + nb && b < a + na; }

}  // namespace

extern "C" {

int32_t n2v_nmf_depth(void) { return DEPTH; }

int n2v_nmf_lists_check(const int64_t* u_ptr, const int32_t* u_i, const int64_t* i_ptr, const int32_t* i_u, int64_t n_users,
                        int64_t n_items, int64_t n, int32_t* scratch, int32_t* status, void* stream) {
    if (n_users < 1 || n_items < 1 || n < 1 || n_users > 0x7fffffffLL || n_items > 0x7fffffffLL || n > (int64_t)0x7fffffff * 256)
        return n2v::fail(N2V_ERR_INVALID, "nmf_lists_check: n_users=%lld n_items=%lld n=%lld", (long long)n_users,
                         (long long)n_items, (long long)n);
    if (!u_ptr || !u_i || !i_ptr || !i_u || !scratch || !status) return n2v::fail(N2V_ERR_INVALID, "nmf_lists_check: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(scratch, 0, sizeof(int32_t) * (size_t)(n_users + n_items), st) != hipSuccess)
        return n2v::fail(N2V_ERR_HIP, "nmf_lists_check: memset failed");
    int32_t* by_item = scratch;                                   // the user-major list's ids are items
    int32_t* by_user = scratch + n_items;
    lists_check_kernel<<<n2v::grid_for(n_users > n ? n_users : n, 256), 256, 0, st>>>(u_ptr, u_i, n_users, n_items, n, 0, by_item, status);
    lists_check_kernel<<<n2v::grid_for(n_items > n ? n_items : n, 256), 256, 0, st>>>(i_ptr, i_u, n_items, n_users, n, 1, by_user, status);
    lists_count_kernel<<<n2v::grid_for(n_items, 256), 256, 0, st>>>(i_ptr, by_item, n_items, status);
    lists_count_kernel<<<n2v::grid_for(n_users, 256), 256, 0, st>>>(u_ptr, by_user, n_users, status);
    return n2v::check_launch("nmf_lists_check");
}

int n2v_nmf_epoch(const int64_t* u_ptr, const int32_t* u_i, const double* u_r, const int64_t* i_ptr, const int32_t* i_u,
                  const double* i_r, const int32_t* u_order, const int32_t* i_order, int64_t n_users, int64_t n_items,
                  int64_t n, int32_t n_factors, double reg_pu, double reg_qi, const double* pu, const double* qi,
                  double* pu_out, double* qi_out, void* stream) {
    if (n_users < 1 || n_items < 1 || n < 1 || n_users > 0x7fffffffLL || n_items > 0x7fffffffLL ||
        n_users + n_items > 0x7fffffffLL)
        return n2v::fail(N2V_ERR_INVALID, "nmf_epoch: n_users=%lld n_items=%lld n=%lld", (long long)n_users, (long long)n_items,
                         (long long)n);
    if (n_factors < 1 || n_factors > MAX_FACTORS)
        return n2v::fail(N2V_ERR_INVALID, "nmf_epoch: n_factors %d outside [1, %d]", n_factors, MAX_FACTORS);
    if (!u_ptr || !u_i || !u_r || !i_ptr || !i_u || !i_r || !pu || !qi || !pu_out || !qi_out)
        return n2v::fail(N2V_ERR_INVALID, "nmf_epoch: null pointer");
    const int64_t su = n_users * n_factors, si = n_items * n_factors;
    if (overlap(pu_out, su, pu, su) || overlap(pu_out, su, qi, si) || overlap(qi_out, si, pu, su) || overlap(qi_out, si, qi, si) ||
        overlap(pu_out, su, qi_out, si))
        return n2v::fail(N2V_ERR_INVALID, "nmf_epoch: an output table overlaps an input table or the other output");
    const PassArgs users{u_ptr, u_i, u_r, u_order, n_users, n_items, n, reg_pu, pu, qi, pu_out};
    const PassArgs items{i_ptr, i_u, i_r, i_order, n_items, n_users, n, reg_qi, qi, pu, qi_out};
    N2V_MF_DISPATCH(nmf_pass_kernel, n_factors, <<<(unsigned)(n_users + n_items), 64, 0, (hipStream_t)stream>>>(users, items, n_factors));
    return n2v::check_launch("nmf_epoch");
}

}  // extern "C"
