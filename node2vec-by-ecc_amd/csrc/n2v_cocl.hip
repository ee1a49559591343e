// Co-clustering rating prediction on the device: surprise's CoClustering (George and Merugu 2005), whose every step
// reads only tables fixed when the step began, so it trains in surprise's own order with every row in parallel.  C-ABI and
// the full definition: include/n2v_sim.h ("Co-clustering"); the restatement the kernels equal bit for bit:
// tests/coclustering_reference.py.  Parity with surprise itself is UNPINNED (it is not a dependency).
//
//   cocl_partial_kernel   one wavefront per user, 16 to a workgroup: lane ic adds the ratings of the user's items in item
//                         cluster ic, in list order, and every lane the row's total; the co-cluster counts are integer
//                         atomics, into the workgroup's table in LDS and from there once per cell into memory (one atomic
//                         per user and cell put 6 040 users onto nine addresses at 3 x 3 clusters: 90 us of the call).
//   cocl_chain_kernel     one workgroup per sum table row: the co-cluster row of user cluster uc (lane = ic, over the users of
//                         uc ascending), the item-cluster sums (lane = ic, over all users) and the user-cluster sums (lane =
//                         uc).  The chain of adds is wavefront 0's alone; what one wavefront cannot do is keep enough loads
//                         in flight to feed it (the partials come from memory, a microsecond away), so all 16 wavefronts
//                         compact the users the row takes, SEL at a time, and stage their partials in LDS, STAGE at a time,
//                         and wavefront 0 adds them from there in order.  It then finishes its own averages.
//   cocl_assign_kernel<U> one wavefront per row of one side, four to a workgroup that shares the co-cluster table in LDS
//                         (laid out so that lane c reads the candidate cluster c's entry of one row of it: no bank conflict
//                         on either side).  Lane c carries errors[c].  The list arrives 64 entries a load, lane j holding
//                         entry j, its cluster and the other side's mean, fetched one chunk ahead, and is broadcast from
//                         there.  d does not depend on errors, so only the add of d * d is a chain.  A row is never split:
//                         the order of the sum is the definition.  With at most 32 candidates the idle lanes take further
//                         entries of the same row: P lanes an entry (P the power of two that holds the candidates), 64 / P
//                         entries a step, their squares through LDS to every lane's own ordered sum.  The longest row
//                         bounds a pass, so it is the row that is made faster, not several rows that share a wavefront.
//                         numpy's argmin over the lanes: the first NaN, else the first minimum.
//   cocl_estimate_kernel  one query per lane.
//   cocl_topn_kernel      one wavefront per (owner, segment), 64 neighbouring candidates at a time, one a lane, the frame of
//                         slope_topn_kernel (n2v_topn.h): cocl_value, the estimate kernel's own function, then predict_value.
// fp64 throughout; -ffp-contract=off (csrc/Makefile) keeps every multiply and add separately rounded.
// Every value that steers a loop or reaches a barrier is the same in all 64 lanes.
#include "n2v_common.h"
#include "n2v_sim.h"
#include "n2v_rank.h"
#include "n2v_topn.h"

namespace {

constexpr int MAXC = 64;                                          // clusters per side: one lane each
constexpr int PART_WAVES = 16;                                    // users per workgroup of the partial sums: they share one count table
constexpr int CHAIN_THREADS = 1024;                               // a chain's workgroup: wavefront 0 adds, all of them fetch
constexpr int SEL = CHAIN_THREADS;                                // users a chain looks at at a time, one a thread
constexpr int AHEAD = 16;                                         // staged partials wavefront 0 reads ahead of its adds
constexpr int STAGE = 6144;                                       // partials a chain stages in LDS per round (48 KB)
constexpr int ASSIGN_WAVES = 4;                                   // rows in flight per workgroup of the assign kernel
constexpr int ASSIGN_MAX_BLOCKS = 2048;

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Lane `j` (wave-uniform) of a value: that lane's value in every lane.
__device__ __forceinline__ int bcast(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ double bcast(double v, int j) {
    return __hiloint2double(bcast(__double2hiint(v), j), bcast(__double2loint(v), j));
}

// The one expression of the model, as written: a = avg_cocltr[uc][ic], um = user_mean[u], au = avg_cltr_u[uc],
// im = item_mean[i], ai = avg_cltr_i[ic].
__device__ __forceinline__ double cocl_expr(double a, double um, double au, double im, double ai) {
    return (((a + um) - au) + im) - ai;
}

// ---- the averages -----------------------------------------------------------------------------------------------------

struct SumArgs {
    const int64_t* ptr; const int32_t* ids; const double* r;
    int64_t n_users, n_items, n;
    const int32_t* cltr_u; const int32_t* cltr_i; int n_cu, n_ci;
    double global_mean;
    double* part;                                                 // fp64[n_users][n_ci + 1]; column n_ci: the row's total
    double* avg_u; double* avg_i; double* avg_cc; unsigned long long* count_cc;
};

__global__ void __launch_bounds__(64 * PART_WAVES) cocl_partial_kernel(SumArgs a) {
    __shared__ int32_t hist[MAXC * MAXC];                         // the workgroup's counts, [uc][ic]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cells = a.n_cu * a.n_ci;
    for (int k = threadIdx.x; k < cells; k += 64 * PART_WAVES) hist[k] = 0;
    __syncthreads();
    const int64_t u = (int64_t)blockIdx.x * PART_WAVES + wave;
    if (u < a.n_users) {                                          // wave-uniform
        const int64_t pb = clamp64(a.ptr[u], 0, a.n), pe = clamp64(a.ptr[u + 1], pb, a.n);
        const int uc = a.cltr_u[u];
        const bool own = uc >= 0 && uc < a.n_cu;                  // a user in no cluster adds nothing
        double s = 0.0, t = 0.0;
        int c = 0;
        for (int64_t base = pb; own && base < pe; base += 64) {
            const int64_t p = base + lane;
            int ic = -1;
            double rv = 0.0;
            if (p < pe) {
                const int64_t id = a.ids[p];
                if (id >= 0 && id < a.n_items) {
                    const int k = a.cltr_i[id];
                    if (k >= 0 && k < a.n_ci) { ic = k; rv = a.r[p]; }
                }
            }
            const int cnt = pe - base < 64 ? (int)(pe - base) : 64;
            for (int j = 0; j < cnt; ++j) {                       // list order: the order of both sums
                const int icj = bcast(ic, j);
                const double rj = bcast(rv, j);
                if (icj < 0) continue;                            // wave-uniform
                t = t + rj;
                s = lane == icj ? s + rj : s;
                c += lane == icj ? 1 : 0;
            }
        }
        const int W = a.n_ci + 1;
        if (lane < a.n_ci) {
            a.part[u * W + lane] = s;
            if (c > 0) atomicAdd(hist + uc * a.n_ci + lane, c);
        }
        if (lane == 0) a.part[u * W + a.n_ci] = t;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += 64 * PART_WAVES) {  // one global atomic per cell and workgroup, not per user
        const int v = hist[k];
        if (v > 0) atomicAdd(a.count_cc + k, (unsigned long long)v);
    }
}

__device__ __forceinline__ double cocl_average(double sum, unsigned long long count, double global_mean) {
    return count ? sum / (double)(int64_t)count : global_mean;
}

__global__ void __launch_bounds__(CHAIN_THREADS) cocl_chain_kernel(SumArgs a) {
    __shared__ double stage[STAGE];
    __shared__ int32_t sel[SEL];
    __shared__ int32_t wcount[CHAIN_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.n_ci + 1;
    double acc = 0.0;                                             // the sum of wavefront 0's lane
    if (b == a.n_cu + 1) {                                        // the user-cluster sums: lane = uc, over all users
        for (int64_t w0 = 0; w0 < a.n_users; w0 += SEL) {
            const int64_t u = w0 + tid;
            if (u < a.n_users) { sel[tid] = a.cltr_u[u]; stage[tid] = a.part[u * W + a.n_ci]; }
            __syncthreads();
            if (wave == 0) {
                const int cnt = a.n_users - w0 < SEL ? (int)(a.n_users - w0) : SEL;
                int k = 0;
                for (; k + AHEAD <= cnt; k += AHEAD) {            // AHEAD LDS reads in flight, then their adds in order
                    int cu[AHEAD];
                    double t[AHEAD];
#pragma unroll
                    for (int j = 0; j < AHEAD; ++j) { cu[j] = sel[k + j]; t[j] = stage[k + j]; }
#pragma unroll
                    for (int j = 0; j < AHEAD; ++j) acc = cu[j] == lane ? acc + t[j] : acc;
                }
                for (; k < cnt; ++k) acc = sel[k] == lane ? acc + stage[k] : acc;
            }
            __syncthreads();                                      // the window is rewritten
        }
        if (wave == 0 && lane < a.n_cu) {
            unsigned long long count = 0;
            for (int ic = 0; ic < a.n_ci; ++ic) count += a.count_cc[(int64_t)lane * a.n_ci + ic];
            a.avg_u[lane] = cocl_average(acc, count, a.global_mean);
        }
        return;
    }
    const bool all = b == a.n_cu;                                 // the item-cluster sums; else the co-cluster row of uc = b
    const int cap = STAGE / a.n_ci;                               // users a round stages
    for (int64_t w0 = 0; w0 < a.n_users; w0 += SEL) {
        const int64_t u = w0 + tid;                               // the users this row takes, ascending
        const bool mine = u < a.n_users && (all || a.cltr_u[u] == b);
        const unsigned long long mask = __ballot(mine);
        if (lane == 0) wcount[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < CHAIN_THREADS / 64; ++w) {
            const int c = wcount[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (mine) sel[before + __popcll(mask & ((1ull << lane) - 1ull))] = tid;
        __syncthreads();
        for (int k0 = 0; k0 < total; k0 += cap) {
            const int m = total - k0 < cap ? total - k0 : cap;
            for (int idx = tid; idx < m * a.n_ci; idx += CHAIN_THREADS) {
                const int k = idx / a.n_ci, c = idx - k * a.n_ci;
                stage[idx] = a.part[(w0 + sel[k0 + k]) * W + c];
            }
            __syncthreads();
            if (wave == 0 && lane < a.n_ci) {
                int k = 0;
                for (; k + AHEAD <= m; k += AHEAD) {
                    double v[AHEAD];
#pragma unroll
                    for (int j = 0; j < AHEAD; ++j) v[j] = stage[(k + j) * a.n_ci + lane];
#pragma unroll
                    for (int j = 0; j < AHEAD; ++j) acc = acc + v[j];
                }
                for (; k < m; ++k) acc = acc + stage[k * a.n_ci + lane];
            }
            __syncthreads();                                      // stage, and after the last round sel and wcount, are rewritten
        }
    }
    if (wave != 0 || lane >= a.n_ci) return;
    if (all) {
        unsigned long long count = 0;
        for (int uc = 0; uc < a.n_cu; ++uc) count += a.count_cc[(int64_t)uc * a.n_ci + lane];
        a.avg_i[lane] = cocl_average(acc, count, a.global_mean);
    } else {
        a.avg_cc[(int64_t)b * a.n_ci + lane] = cocl_average(acc, a.count_cc[(int64_t)b * a.n_ci + lane], a.global_mean);
    }
}

// ---- one assignment pass ----------------------------------------------------------------------------------------------

struct AssignArgs {
    const int64_t* ptr; const int32_t* other; const double* r; const int32_t* order;
    int64_t n_rows, n_other, n;
    int n_own_c, n_oth_c, n_ci;
    const double* own_mean; const double* oth_mean; const double* avg_own; const double* avg_oth; const double* avg_cc;
    const int32_t* cltr_oth; int32_t* cltr_own;
};

// numpy's argmin of the lanes' values below n: the first NaN if there is one, else the first minimum.
__device__ __forceinline__ int lane_argmin(double v, int n, int lane) {
    const bool in = lane < n;
    const unsigned long long nan = __ballot(in && v != v);
    if (nan) return __ffsll((long long)nan) - 1;
    double m = in ? v : __builtin_inf();
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(m, off, 64);
        m = o < m ? o : m;
    }
    return __ffsll((long long)__ballot(in && v == m)) - 1;
}

// P: the lanes one entry takes, the power of two that holds the candidate clusters.  P = 64: the list's entries one after the
// other, each broadcast from its lane.  P <= 32: E = 64 / P entries at once, lane e * P + c forming d * d of entry e for
// candidate c; the squares then pass through LDS and every lane adds those of its candidate in list order, so the chain is
// one add per entry and the rest of an entry costs a 1 / E share of an instruction stream.
template <bool USER, int P>
__global__ void __launch_bounds__(64 * ASSIGN_WAVES) cocl_assign_kernel(AssignArgs a) {
    __shared__ double table[MAXC * MAXC];                         // [other cluster][candidate]
    __shared__ double avg_oth[MAXC];
    __shared__ double dsq[ASSIGN_WAVES][64];
    constexpr int E = 64 / P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & (P - 1), e = lane / P;                   // the lane's candidate and its entry of a step
    for (int idx = threadIdx.x; idx < a.n_oth_c * MAXC; idx += 64 * ASSIGN_WAVES) {
        const int oc = idx >> 6, k = idx & 63;
        table[idx] = k < a.n_own_c ? (USER ? a.avg_cc[(int64_t)k * a.n_ci + oc] : a.avg_cc[(int64_t)oc * a.n_ci + k]) : 0.0;
    }
    if ((int)threadIdx.x < a.n_oth_c) avg_oth[threadIdx.x] = a.avg_oth[threadIdx.x];
    __syncthreads();
    const double a_own = c < a.n_own_c ? a.avg_own[c] : 0.0;

    for (int64_t slot = (int64_t)blockIdx.x * ASSIGN_WAVES + wave; slot < a.n_rows; slot += (int64_t)gridDim.x * ASSIGN_WAVES) {
        const int64_t row = a.order ? (int64_t)a.order[slot] : slot;
        if (row < 0 || row >= a.n_rows) continue;                 // only an order table that is no permutation has one
        const int64_t pb = clamp64(a.ptr[row], 0, a.n), pe = clamp64(a.ptr[row + 1], pb, a.n);
        const double own_m = a.own_mean[row];

        // entry base + lane of the list: id -1 past the end or outside [0, n_other)
        auto load_ids = [&](int64_t base, int& id, double& r) {
            id = -1; r = 0.0;
            if (base + lane < pe) {
                const int32_t v = a.other[base + lane];
                r = a.r[base + lane];
                if (v >= 0 && v < a.n_other) id = v;
            }
        };
        // the entry's cluster on the other side (-1: the entry adds nothing) and the other side's mean
        auto gather = [&](int id, int& oc, double& om) {
            oc = -1; om = 0.0;
            if (id >= 0) {
                const int32_t k = a.cltr_oth[id];
                om = a.oth_mean[id];
                if (k >= 0 && k < a.n_oth_c) oc = k;
            }
        };
        // d * d of one entry for the lane's candidate
        auto square = [&](int oc, double r, double om, double ao) {
            const double t = table[(oc < 0 ? 0 : oc) * MAXC + c];
            const double est = USER ? cocl_expr(t, own_m, a_own, om, ao) : cocl_expr(t, om, ao, own_m, a_own);
            const double d = r - est;
            return d * d;
        };
        int id_n, id_nn, oc_c, oc_n;
        double r_c, r_n, r_nn, om_c, om_n;
        load_ids(pb, id_n, r_c);
        gather(id_n, oc_c, om_c);
        load_ids(pb + 64, id_n, r_n);
        double err = 0.0;
        for (int64_t base = pb; base < pe; base += 64) {
            gather(id_n, oc_n, om_n);                             // the next chunk's, in flight during this one
            load_ids(base + 128, id_nn, r_nn);
            const double ao_c = avg_oth[oc_c < 0 ? 0 : oc_c];
            const int cnt = pe - base < 64 ? (int)(pe - base) : 64;   // a lane past the end of the list holds cluster -1
            if constexpr (P == 64) {
                for (int j0 = 0; j0 < cnt; j0 += 4) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = j0 + k;
                        const int oc = bcast(oc_c, j);
                        const double sq = square(oc, bcast(r_c, j), bcast(om_c, j), bcast(ao_c, j));
                        err = oc < 0 ? err : err + sq;
                    }
                }
            } else {
                for (int j0 = 0; j0 < cnt; j0 += E) {             // entries j0 .. j0 + E - 1, one per group of P lanes
                    const int j = j0 + e;
                    const int oc = __shfl(oc_c, j, 64);
                    dsq[wave][lane] = square(oc, __shfl(r_c, j, 64), __shfl(om_c, j, 64), __shfl(ao_c, j, 64));
                    const unsigned long long valid = __ballot(oc >= 0);
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");    // the squares are seen by this wavefront's loads
#pragma unroll
                    for (int k = 0; k < E; ++k) {                 // list order: the order of the sum
                        const double sq = dsq[wave][k * P + c];
                        err = (valid >> (k * P)) & 1ull ? err + sq : err;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");    // ... and read before the next step's stores
                }
            }
            oc_c = oc_n; om_c = om_n; r_c = r_n;
            id_n = id_nn; r_n = r_nn;
        }
        const int best = lane_argmin(err, a.n_own_c, lane);       // lanes 0 .. n_own_c - 1 are the candidates of group 0
        if (lane == 0) a.cltr_own[row] = best;
    }
}

template <bool USER>
void launch_assign(const AssignArgs& a, unsigned blocks, hipStream_t st) {
    const dim3 grid(blocks), block(64 * ASSIGN_WAVES);
    if (a.n_own_c > 32) cocl_assign_kernel<USER, 64><<<grid, block, 0, st>>>(a);
    else if (a.n_own_c > 16) cocl_assign_kernel<USER, 32><<<grid, block, 0, st>>>(a);
    else if (a.n_own_c > 8) cocl_assign_kernel<USER, 16><<<grid, block, 0, st>>>(a);
    else if (a.n_own_c > 4) cocl_assign_kernel<USER, 8><<<grid, block, 0, st>>>(a);
    else if (a.n_own_c > 2) cocl_assign_kernel<USER, 4><<<grid, block, 0, st>>>(a);
    else if (a.n_own_c > 1) cocl_assign_kernel<USER, 2><<<grid, block, 0, st>>>(a);
    else cocl_assign_kernel<USER, 1><<<grid, block, 0, st>>>(a);
}

// ---- estimate ---------------------------------------------------------------------------------------------------------

struct Model {
    const int32_t* cltr_u; const int32_t* cltr_i; const double* avg_u; const double* avg_i; const double* avg_cc;
    const double* user_mean; const double* item_mean;
    int64_t n_users, n_items; int n_cu, n_ci;
    double global_mean;
};

// The estimate of (u, i), the one copy behind cocl_estimate_kernel and cocl_topn_kernel; an id outside its range is
// unknown.  A cluster id outside its range (no fitted model has one) is never an index: the estimate is the training mean.
__device__ __forceinline__ double cocl_value(const Model& m, int64_t u, int64_t i) {
    const bool ku = u >= 0 && u < m.n_users, ki = i >= 0 && i < m.n_items;
    if (ku && ki) {
        const int uc = m.cltr_u[u], ic = m.cltr_i[i];
        if (uc < 0 || uc >= m.n_cu || ic < 0 || ic >= m.n_ci) return m.global_mean;
        return cocl_expr(m.avg_cc[(int64_t)uc * m.n_ci + ic], m.user_mean[u], m.avg_u[uc], m.item_mean[i], m.avg_i[ic]);
    }
    if (ku) return m.user_mean[u];
    if (ki) return m.item_mean[i];
    return m.global_mean;
}

__global__ void __launch_bounds__(256) cocl_estimate_kernel(Model m, const int32_t* __restrict__ q_u, const int32_t* __restrict__ q_i,
                                                            int64_t n_q, double* __restrict__ est, uint8_t* __restrict__ impossible) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_q) return;
    est[q] = cocl_value(m, q_u[q], q_i[q]);
    impossible[q] = 0;
}

// ---- top-N ------------------------------------------------------------------------------------------------------------

struct TopnArgs {
    Model m; n2v::Seen seen; const int32_t* owners; int N; int S;
    double lo, hi;
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

__global__ void __launch_bounds__(64) cocl_topn_kernel(TopnArgs a) {
    __shared__ double ts[N2V_TOPN_MAX_N];
    __shared__ int32_t tp[N2V_TOPN_MAX_N];
    const int64_t o = blockIdx.x;
    const int seg = blockIdx.y, lane = threadIdx.x;
    const int64_t u = a.owners[o];
    int64_t c0, c1;
    n2v::segment_range(a.m.n_items, seg, a.S, c0, c1);
    int64_t sb = 0, se = 0;                                       // the owner's row of the seen CSR, inside [0, n_seen]
    if (u >= 0 && u < a.seen.n_rows) {
        const int64_t ns = a.seen.n > 0 ? a.seen.n : 0;
        sb = clamp64(a.seen.ptr[u], 0, ns);
        se = clamp64(a.seen.ptr[u + 1], sb, ns);
    }
    n2v::TopList top;
    top.init(ts, tp, a.N, lane);
    for (int64_t cb = c0; cb < c1; cb += 64) {
        const int64_t c = cb + lane;
        const bool inside = c < c1;
        const bool cand = inside && !seen_has(a.seen.item, sb, se, c);
        const double score = n2v::predict_value(inside ? cocl_value(a.m, u, c) : 0.0, false, a.m.global_mean, a.lo, a.hi);
        unsigned long long offer = __ballot(cand && n2v::beats(n2v::order_key(score), (int)c, top.tk, top.tp));
        while (offer) {                                           // ascending item id; wave-uniform
            const int src = __ffsll((long long)offer) - 1;
            offer &= offer - 1;
            top.offer(__shfl(score, src, 64), (int)(cb + src), lane);
        }
    }
    const int64_t out = (o * a.S + seg) * a.N;
    top.store(a.part_score + out, a.part_pos + out, lane);
}

bool clusters_ok(int32_t n_cu, int32_t n_ci) { return n_cu >= 1 && n_cu <= MAXC && n_ci >= 1 && n_ci <= MAXC; }

// The checks the two readers of a fitted model share; 0 or the error.
int model_args(const char* who, const Model& m) {
    if (m.n_users < 1 || m.n_items < 1 || m.n_users > 0x7fffffffLL || m.n_items > 0x7fffffffLL)
        return n2v::fail(N2V_ERR_INVALID, "%s: n_users=%lld n_items=%lld", who, (long long)m.n_users, (long long)m.n_items);
    if (!clusters_ok(m.n_cu, m.n_ci))
        return n2v::fail(N2V_ERR_INVALID, "%s: n_cltr_u=%d n_cltr_i=%d outside [1, %d]", who, m.n_cu, m.n_ci, MAXC);
    if (!m.cltr_u || !m.cltr_i || !m.avg_u || !m.avg_i || !m.avg_cc || !m.user_mean || !m.item_mean)
        return n2v::fail(N2V_ERR_INVALID, "%s: null pointer", who);
    return N2V_OK;
}

}  // namespace

extern "C" {

int32_t n2v_cocl_max_clusters(void) { return MAXC; }

int n2v_cocl_averages(const int64_t* ur_ptr, const int32_t* ur_i, const double* ur_r, int64_t n_users, int64_t n_items, int64_t n,
                      const int32_t* cltr_u, const int32_t* cltr_i, int32_t n_cltr_u, int32_t n_cltr_i, double global_mean,
                      double* part, double* avg_cltr_u, double* avg_cltr_i, double* avg_cocltr, int64_t* count_cocltr,
                      void* stream) {
    if (n_users < 1 || n_items < 1 || n < 0 || n_users > 0x7fffffffLL || n_items > 0x7fffffffLL)
        return n2v::fail(N2V_ERR_INVALID, "cocl_averages: n_users=%lld n_items=%lld n=%lld", (long long)n_users, (long long)n_items,
                         (long long)n);
    if (!clusters_ok(n_cltr_u, n_cltr_i))
        return n2v::fail(N2V_ERR_INVALID, "cocl_averages: n_cltr_u=%d n_cltr_i=%d outside [1, %d]", n_cltr_u, n_cltr_i, MAXC);
    if (!ur_ptr || (n > 0 && (!ur_i || !ur_r)) || !cltr_u || !cltr_i || !part || !avg_cltr_u || !avg_cltr_i || !avg_cocltr ||
        !count_cocltr)
        return n2v::fail(N2V_ERR_INVALID, "cocl_averages: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(count_cocltr, 0, sizeof(int64_t) * (size_t)n_cltr_u * (size_t)n_cltr_i, st) != hipSuccess)
        return n2v::fail(N2V_ERR_HIP, "cocl_averages: memset failed");
    const SumArgs a{ur_ptr, ur_i, ur_r, n_users, n_items, n, cltr_u, cltr_i, n_cltr_u, n_cltr_i, global_mean, part,
                    avg_cltr_u, avg_cltr_i, avg_cocltr, (unsigned long long*)count_cocltr};
    cocl_partial_kernel<<<(unsigned)((n_users + PART_WAVES - 1) / PART_WAVES), 64 * PART_WAVES, 0, st>>>(a);
    cocl_chain_kernel<<<(unsigned)n_cltr_u + 2, CHAIN_THREADS, 0, st>>>(a);
    return n2v::check_launch("cocl_averages");
}

int n2v_cocl_assign(const int64_t* ptr, const int32_t* other, const double* r, const int32_t* order, int64_t n_users,
                    int64_t n_items, int64_t n, int32_t user_side, int32_t n_cltr_u, int32_t n_cltr_i, const double* user_mean,
                    const double* item_mean, const double* avg_cltr_u, const double* avg_cltr_i, const double* avg_cocltr,
                    int32_t* cltr_u, int32_t* cltr_i, void* stream) {
    if (n_users < 1 || n_items < 1 || n < 0 || n_users > 0x7fffffffLL || n_items > 0x7fffffffLL)
        return n2v::fail(N2V_ERR_INVALID, "cocl_assign: n_users=%lld n_items=%lld n=%lld", (long long)n_users, (long long)n_items,
                         (long long)n);
    if (!clusters_ok(n_cltr_u, n_cltr_i))
        return n2v::fail(N2V_ERR_INVALID, "cocl_assign: n_cltr_u=%d n_cltr_i=%d outside [1, %d]", n_cltr_u, n_cltr_i, MAXC);
    if (!ptr || (n > 0 && (!other || !r)) || !user_mean || !item_mean || !avg_cltr_u || !avg_cltr_i || !avg_cocltr || !cltr_u ||
        !cltr_i)
        return n2v::fail(N2V_ERR_INVALID, "cocl_assign: null pointer");
    if (cltr_u < cltr_i + n_items && cltr_i < cltr_u + n_users)
        return n2v::fail(N2V_ERR_INVALID, "cocl_assign: cltr_u and cltr_i overlap: one side is read while the other is written");
    const int64_t n_rows = user_side ? n_users : n_items;
    const unsigned blocks = (unsigned)((n_rows + ASSIGN_WAVES - 1) / ASSIGN_WAVES < ASSIGN_MAX_BLOCKS
                                           ? (n_rows + ASSIGN_WAVES - 1) / ASSIGN_WAVES : ASSIGN_MAX_BLOCKS);
    if (user_side) {
        launch_assign<true>(AssignArgs{ptr, other, r, order, n_users, n_items, n, n_cltr_u, n_cltr_i, n_cltr_i, user_mean, item_mean,
                                       avg_cltr_u, avg_cltr_i, avg_cocltr, cltr_i, cltr_u}, blocks, (hipStream_t)stream);
    } else {
        launch_assign<false>(AssignArgs{ptr, other, r, order, n_items, n_users, n, n_cltr_i, n_cltr_u, n_cltr_i, item_mean, user_mean,
                                        avg_cltr_i, avg_cltr_u, avg_cocltr, cltr_u, cltr_i}, blocks, (hipStream_t)stream);
    }
    return n2v::check_launch("cocl_assign");
}

int n2v_cocl_estimate(const int32_t* cltr_u, const int32_t* cltr_i, const double* avg_cltr_u, const double* avg_cltr_i,
                      const double* avg_cocltr, const double* user_mean, const double* item_mean, int64_t n_users,
                      int64_t n_items, int32_t n_cltr_u, int32_t n_cltr_i, double global_mean, const int32_t* q_u,
                      const int32_t* q_i, int64_t n_q, double* est, uint8_t* impossible, void* stream) {
    const Model m{cltr_u, cltr_i, avg_cltr_u, avg_cltr_i, avg_cocltr, user_mean, item_mean, n_users, n_items, n_cltr_u, n_cltr_i,
                  global_mean};
    if (const int rc = model_args("cocl_estimate", m)) return rc;
    if (n_q < 1 || n_q > (int64_t)0x7fffffff * 256) return n2v::fail(N2V_ERR_INVALID, "cocl_estimate: n_q %lld", (long long)n_q);
    if (!q_u || !q_i || !est || !impossible) return n2v::fail(N2V_ERR_INVALID, "cocl_estimate: null pointer");
    cocl_estimate_kernel<<<n2v::grid_for(n_q, 256), 256, 0, (hipStream_t)stream>>>(m, q_u, q_i, n_q, est, impossible);
    return n2v::check_launch("cocl_estimate");
}

int n2v_cocl_topn(const int32_t* cltr_u, const int32_t* cltr_i, const double* avg_cltr_u, const double* avg_cltr_i,
                  const double* avg_cocltr, const double* user_mean, const double* item_mean, int64_t n_users, int64_t n_items,
                  int32_t n_cltr_u, int32_t n_cltr_i, const int64_t* seen_ptr, const int32_t* seen_i, int64_t n_seen,
                  const int32_t* owners, int64_t n_owners, double global_mean, double lo, double hi, int32_t top_n,
                  int32_t segments, double* part_score, int32_t* part_pos, int32_t* items, double* score, void* stream) {
    const Model m{cltr_u, cltr_i, avg_cltr_u, avg_cltr_i, avg_cocltr, user_mean, item_mean, n_users, n_items, n_cltr_u, n_cltr_i,
                  global_mean};
    if (const int rc = model_args("cocl_topn", m)) return rc;
    if (const int rc = n2v::topn_args("cocl_topn", n_owners, n_items, top_n, segments, seen_ptr, seen_i, n_seen, owners,
                                      part_score, part_pos, items, score))
        return rc;
    const int S = segments > 0 ? segments : n2v_topn_segments(n_owners, n_items);
    const TopnArgs a{m, n2v::Seen{seen_ptr, seen_i, n_users, n_seen}, owners, top_n, S, lo, hi, part_score, part_pos};
    cocl_topn_kernel<<<dim3((unsigned)n_owners, (unsigned)S), 64, 0, (hipStream_t)stream>>>(a);
    if (const int rc = n2v::check_launch("cocl_topn")) return rc;
    return n2v::topn_merge("cocl_topn (merge)", part_score, part_pos, n_owners, S, top_n, items, score, (hipStream_t)stream);
}

}  // extern "C"
