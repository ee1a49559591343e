// EccenKNN: eccentricity-weighted k-NN rating prediction — gfx950 (MI355X).  C-ABI: include/n2v_sim.h.
//
// Reference: src/main_rec.py:73-151 (cosine_eccen / msd_eccen: `for y: for xi: for xj` over five dense n_x x n_x
// arrays) and :305-329 (estimate: heapq.nlargest over the raters of y, then a weighted mean in rank order).
//   densify_kernel   one lane per rating: the y-major dense rating matrix and its presence mask (0 is a legal rating);
//   sim_kernel       one workgroup per 64x64 tile of the upper triangle, 4x4 pairs per thread with their accumulators in
//                    registers; the two 64-column panels of the dense matrix and the mask pass through LDS in chunks of
//                    YC values of y.  Every pair walks y ascending and performs the reference's separately rounded
//                    multiplies and adds (the library is built with -ffp-contract=off), so the accumulators and sim are
//                    the reference's bits.  A y that one side did not rate leaves the accumulators untouched (a select,
//                    not a multiply by zero: ratings may be anything).  No float atomics (their order is undefined) and
//                    no v_mfma_f64 (its four products are not added one after the other).  The mirror is written from
//                    the same tile: prods and sq_diff are symmetric bit for bit, sqi and sqj swap.
//   sim_sparse_kernel the same frame and the same outputs from the x-major CSR of the ratings: nothing of size n_x x n_y
//                    exists.  The tile's 128 rows pass through LDS in rounds of up to SC entries (y, r) a row, each row
//                    from its own cursor.  A round's bound is the smallest last-staged y among the rows that have entries
//                    beyond their staged ones: up to it every row's staged segment is complete, so every thread merges
//                    its 16 pairs of segments two-pointer fashion in y order, and the cursors advance by what was ready.
//                    The row that set the bound consumes its whole chunk, so every round makes progress.  pair_step
//                    and finish_tile are shared with sim_kernel.  csr_check_kernel (integers only) names a malformed CSR; the similarity
//                    kernel itself clamps every row range to [0, n] and never indexes w with a y outside [0, n_y).
//                    The two Pearson similarities of surprise's KNNBasic (n2v_eccknn_pearson, n2v_eccknn_pearson_sparse)
//                    are two more METHODs of the same two kernels: pearson carries prods, sqi, sqj, si, sj; the
//                    baseline form carries prods, sq_diff_i, sq_diff_j of the ratings' deviations from
//                    global_mean + by[y] + bx[x], with the thread's 4 + 4 bx in registers and global_mean + by[y]
//                    staged beside w[y].  w may be absent there: the factor is 1.0, which changes no bit.
//                    SlopeOne's deviation table (n2v_slopeone_dev, n2v_slopeone_dev_sparse) is a fifth METHOD with the
//                    lightest accumulator, one count and one sum of ri - rj a pair, and a finishing step of its own
//                    (finish_tile_slope): the lower half is the upper value with its sign bit flipped, also inside a
//                    diagonal tile.  The estimate and the top-N kernel that read the table are in n2v_slopeone.hip.
//   baselines_kernel one half-epoch of surprise's baseline_als: one wavefront per row gathers the other side's
//                    baselines 64 at a time and adds the terms (r - mean) - b in list order.
//   estimate_kernel  one wavefront per query: gathers sim[x, x2] over the raters of y, keeps the best k of them in a
//                    sorted LDS list under the one order of n2v_rank.h (higher sim first, equal sims by list position,
//                    -0.0 ties +0.0, NaN below everything) and sums in rank order.  A template over the centring mode of
//                    knn_estimate: none (EccenKNN, KNNBasic: n2v_eccknn_estimate), or the row mean, the z-score or the
//                    baseline of surprise's KNNWithMeans / KNNWithZScore / KNNBaseline (n2v_eccknn_estimate_centered):
//                    the same selection, three more fp64 gathers per kept neighbour, no more LDS.
//   estimate_sweep_kernel one wavefront per query: every (k, min_k) cell of a grid from one selection at the largest k.
//                    The list's order is total, so the selection for k is its first k entries and the rank-order sums for
//                    k are a prefix of the sums for the largest k; knn_estimate is split into knn_unknown, knn_select,
//                    knn_sums and knn_finish, and the sweep runs the selection once, the sums from one k of the grid to
//                    the next, and the finish per min_k.  The grid travels in the kernel's arguments.
//   row_moments_kernel one wavefront per row: the mean and the population sigma of a row's ratings, each sum in list order.
//   predict_kernel   one workgroup: global-mean fallback, clip to the rating scale, and the squared errors added one
//                    after the other in query order (rmse).
//   errors_kernel    one workgroup per column of predictions: rmse and mae, both sums in query order as predict_kernel's.
//   eccknn_topn_kernel one wavefront per (owner, segment of the items): the owner's unseen items ascending, each through
//                    the same knn_estimate and predict_value as the two kernels above, folded into a best-N list in LDS;
//                    nothing of size owners x items is stored.  The S segment lists of an owner are merged under the
//                    same order (n2v_topn.h), so the result does not depend on S.
#include <type_traits>

#include "n2v_common.h"
#include "n2v_sim.h"
#include "n2v_rank.h"
#include "n2v_topn.h"

namespace {

constexpr int TB = 64;            // rows / columns of a tile
constexpr int YC = 32;            // values of y staged per barrier
constexpr int64_t MAX_DENSE = (int64_t)1 << 31;   // elements of the dense matrix (16 GiB of fp64)

// ---- densify ----------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) densify_kernel(const int32_t* __restrict__ x, const int32_t* __restrict__ y,
                                                      const double* __restrict__ r, int64_t n, int64_t n_x, int64_t n_y,
                                                      double* __restrict__ dense, uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t xi = x[i], yi = y[i];
    if (xi < 0 || xi >= n_x || yi < 0 || yi >= n_y) return;      // the host wrapper's contract; never out of bounds
    dense[yi * n_x + xi] = r[i];
    mask[yi * n_x + xi] = 1;
}

// ---- similarity -------------------------------------------------------------------------------------------------------

constexpr int M_PEARSON = 2;      // METHOD values after N2V_ECCKNN_COSINE / N2V_ECCKNN_MSD; the C-ABI reaches them only
constexpr int M_PBASE = 3;        // through n2v_eccknn_pearson[_sparse] (kind 0 / 1), never through the old method enum
constexpr int M_SLOPE = 4;        // SlopeOne's deviations, through n2v_slopeone_dev[_sparse] only: p0 the sum of ri - rj

struct SimOut {
    int64_t n_x; int min_support;
    double* sim; int32_t* freq; double* prods; double* sqi; double* sqj; double* sq_diff;
    double* si; double* sj; double shrinkage;                     // pearson's sums; pearson_baseline's shrinkage
};
// What pearson_baseline reads beside the ratings.
struct Baselines {
    const double* bx; const double* by; double global_mean;
};
struct SimArgs {                                                  // w may be NULL for the two Pearson methods
    const double* dense; const uint8_t* mask; int64_t n_y; const double* w; SimOut o; Baselines b;
};

// The finishing step of a tile, the one copy behind the dense and the sparse kernel: thread (ty, tx) holds the
// accumulators of pairs (i0 + 4 ty + u, j0 + 4 tx + v).  i == j -> 1, freq < min_support -> 0, else the method's formula;
// the mirror is written from the same values with the per-side accumulators (p1 / p2 and p3 / p4) swapped.
//   cosine    p0 prods, p1 sqi, p2 sqj                  msd               p0 sq_diff
//   pearson   p0 prods, p1 sqi, p2 sqj, p3 si, p4 sj    pearson_baseline  p0 prods, p1 sq_diff_i, p2 sq_diff_j
template <int METHOD>
__device__ __forceinline__ double finish_pair(const SimOut& o, int32_t fr, double p0, double p1, double p2, double p3,
                                              double p4) {
    if (fr < o.min_support) return 0.0;
    if (METHOD == N2V_ECCKNN_COSINE) return p0 / sqrt(p1 * p2);
    if (METHOD == N2V_ECCKNN_MSD) return 1.0 / (p0 / (double)fr + 1.0);
    if (METHOD == M_PEARSON) {
        const double n = (double)fr;
        const double num = n * p0 - p3 * p4;
        const double denum = sqrt((n * p1 - p3 * p3) * (n * p2 - p4 * p4));   // a negative product: NaN, and it is kept
        return denum == 0 ? 0.0 : num / denum;
    }
    const double f1 = (double)(fr - 1);                           // min_support is at least 2 here
    return (p0 / sqrt(p1 * p2)) * (f1 / (f1 + o.shrinkage));      // no zero test in the source: 0/0 and x/0 stay
}

template <int METHOD>
__device__ __forceinline__ void finish_tile(const SimOut& o, int64_t i0, int64_t j0, int ty, int tx, bool diag_tile,
                                            const int32_t (&fr)[4][4], const double (&p0)[4][4], const double (&p1)[4][4],
                                            const double (&p2)[4][4], const double (&p3)[4][4], const double (&p4)[4][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + 4 * ty + u;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t j = j0 + 4 * tx + v;
            if (i >= o.n_x || j >= o.n_x) continue;
            const double s = i == j ? 1.0 : finish_pair<METHOD>(o, fr[u][v], p0[u][v], p1[u][v], p2[u][v], p3[u][v], p4[u][v]);
            const int64_t k = i * o.n_x + j, m = j * o.n_x + i;
            o.sim[k] = s;
            if (o.freq) o.freq[k] = fr[u][v];
            if (METHOD == N2V_ECCKNN_MSD) {
                if (o.sq_diff) o.sq_diff[k] = p0[u][v];
            } else {
                if (o.prods) o.prods[k] = p0[u][v];
                if (o.sqi) o.sqi[k] = p1[u][v];
                if (o.sqj) o.sqj[k] = p2[u][v];
                if (METHOD == M_PEARSON) {
                    if (o.si) o.si[k] = p3[u][v];
                    if (o.sj) o.sj[k] = p4[u][v];
                }
            }
            if (diag_tile) continue;                              // a diagonal tile computed its own lower half
            o.sim[m] = s;
            if (o.freq) o.freq[m] = fr[u][v];
            if (METHOD == N2V_ECCKNN_MSD) {
                if (o.sq_diff) o.sq_diff[m] = p0[u][v];
            } else {
                if (o.prods) o.prods[m] = p0[u][v];
                if (o.sqi) o.sqi[m] = p2[u][v];
                if (o.sqj) o.sqj[m] = p1[u][v];
                if (METHOD == M_PEARSON) {
                    if (o.si) o.si[m] = p4[u][v];
                    if (o.sj) o.sj[m] = p3[u][v];
                }
            }
        }
    }
}

// One co-rated y of one pair, the one copy behind the dense and the sparse kernel: a and b are the two ratings (under
// pearson_baseline their deviations), qa and qb their squares, wy the weight of y.  co is a select, never a multiply: a
// y that one side did not rate leaves every accumulator untouched, whatever the staged values are; the sparse kernel
// meets only co-rated y and passes true.  Every product and sum is rounded on its own, left to right as the reference
// writes them (`ri * rj * i_dict[y]`).  finish_tile names p0 .. p4 per method.
template <int METHOD>
__device__ __forceinline__ void pair_step(bool co, double a, double b, double qa, double qb, double wy, int32_t& fr,
                                          double& p0, double& p1, double& p2, double& p3, double& p4) {
    fr += co ? 1 : 0;
    if (METHOD == N2V_ECCKNN_COSINE || METHOD == M_PEARSON || METHOD == M_PBASE) {
        const double pr = (a * b) * wy;
        p0 = co ? p0 + pr : p0;
        p1 = co ? p1 + qa : p1;
        p2 = co ? p2 + qb : p2;
        if (METHOD == M_PEARSON) {
            p3 = co ? p3 + a : p3;
            p4 = co ? p4 + b : p4;
        }
    } else if (METHOD == M_SLOPE) {
        p0 = co ? p0 + (a - b) : p0;
    } else {
        const double d = (a - b) * wy;
        p0 = co ? p0 + d * d : p0;
    }
}

// SlopeOne's finishing step: o.sim is dev, o.prods the optional raw sums.  The pair i < j writes both of its entries:
// dev[i][j] = p0 / fr (no rater in common: 0.0 / 0 = NaN) and dev[j][i] = -dev[i][j], the negation of the stored value,
// so two items every co-rater rated alike get +0.0 above the diagonal and -0.0 below it.  A pair i > j of a diagonal tile
// writes nothing: its entries are its mirror pair's.  The raw sum of the pair (j, i) is the sum of the negated terms from
// +0.0: -p0, and +0.0 where p0 is a zero (x + -x and 0.0 + -0.0 are +0.0).
__device__ __forceinline__ void finish_tile_slope(const SimOut& o, int64_t i0, int64_t j0, int ty, int tx,
                                                  const int32_t (&fr)[4][4], const double (&p0)[4][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + 4 * ty + u;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t j = j0 + 4 * tx + v;
            if (i >= o.n_x || j >= o.n_x || i > j) continue;
            const int64_t k = i * o.n_x + j, m = j * o.n_x + i;
            const double d = i == j ? 0.0 : p0[u][v] / (double)fr[u][v];
            o.sim[k] = d;
            o.freq[k] = fr[u][v];
            if (o.prods) o.prods[k] = p0[u][v];
            if (i == j) continue;
            o.sim[m] = -d;
            o.freq[m] = fr[u][v];
            if (o.prods) o.prods[m] = p0[u][v] == 0.0 ? 0.0 : -p0[u][v];
        }
    }
}

// The thread's 4 + 4 bx (rows 4 ty + u of the tile, columns 4 tx + v), read only for x < n_x.
__device__ __forceinline__ void load_bx(const Baselines& b, int64_t n_x, int64_t i0, int64_t j0, int ty, int tx,
                                        double (&bxi)[4], double (&bxj)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + 4 * ty + u, j = j0 + 4 * tx + u;
        bxi[u] = i < n_x ? b.bx[i] : 0.0;
        bxj[u] = j < n_x ? b.bx[j] : 0.0;
    }
}

template <int METHOD>
__global__ void __launch_bounds__(256) sim_kernel(SimArgs a) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;                                          // upper triangle of tiles; the mirror comes from it
    __shared__ __attribute__((aligned(16))) double ra[YC][TB];    // ratings of the tile's rows    [y][row]
    __shared__ __attribute__((aligned(16))) double rb[YC][TB];    // ratings of the tile's columns [y][col]
    __shared__ __attribute__((aligned(4))) uint8_t ma[YC][TB];
    __shared__ __attribute__((aligned(4))) uint8_t mb[YC][TB];
    __shared__ double wl[YC];
    __shared__ double pbl[METHOD == M_PBASE ? YC : 1];            // global_mean + by[y] of the staged y

    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t i0 = (int64_t)ti * TB, j0 = (int64_t)tj * TB;

    int32_t fr[4][4];
    double p0[4][4], p1[4][4], p2[4][4], p3[4][4], p4[4][4];      // finish_tile names them per method
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) { fr[u][v] = 0; p0[u][v] = 0.0; p1[u][v] = 0.0; p2[u][v] = 0.0; p3[u][v] = 0.0; p4[u][v] = 0.0; }
    double bxi[4] = {0.0, 0.0, 0.0, 0.0}, bxj[4] = {0.0, 0.0, 0.0, 0.0};
    if (METHOD == M_PBASE) load_bx(a.b, a.o.n_x, i0, j0, ty, tx, bxi, bxj);

    for (int64_t y0 = 0; y0 < a.n_y; y0 += YC) {
        __syncthreads();                                          // the previous chunk has been consumed
        for (int e = t; e < YC * TB; e += 256) {
            const int yy = e >> 6, c = e & 63;
            const int64_t y = y0 + yy;
            double va = 0.0, vb = 0.0;
            uint8_t qa = 0, qb = 0;
            if (y < a.n_y) {
                if (i0 + c < a.o.n_x) { va = a.dense[y * a.o.n_x + i0 + c]; qa = a.mask[y * a.o.n_x + i0 + c]; }
                if (j0 + c < a.o.n_x) { vb = a.dense[y * a.o.n_x + j0 + c]; qb = a.mask[y * a.o.n_x + j0 + c]; }
            }
            ra[yy][c] = va; rb[yy][c] = vb; ma[yy][c] = qa; mb[yy][c] = qb;
        }
        if (t < YC) wl[t] = (y0 + t < a.n_y) ? (a.w ? a.w[y0 + t] : 1.0) : 0.0;
        if (METHOD == M_PBASE && t < YC) pbl[t] = (y0 + t < a.n_y) ? a.b.global_mean + a.b.by[y0 + t] : 0.0;
        __syncthreads();
#pragma unroll 2
        for (int yy = 0; yy < YC; ++yy) {                         // y ascending: the order of every accumulator
            const uint32_t mi = *reinterpret_cast<const uint32_t*>(&ma[yy][4 * ty]);
            const uint32_t mj = *reinterpret_cast<const uint32_t*>(&mb[yy][4 * tx]);
            if (mi == 0 || mj == 0) continue;                     // none of this thread's 16 pairs is co-rated at y
            const double wy = wl[yy];
            double ri[4], rj[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { ri[u] = ra[yy][4 * ty + u]; rj[u] = rb[yy][4 * tx + u]; }
            const double pb = METHOD == M_PBASE ? pbl[yy] : 0.0;
            double si[4], sj[4];                                  // the 4 + 4 squares, once for the 16 pairs
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (METHOD == M_PBASE) { ri[u] = ri[u] - (pb + bxi[u]); rj[u] = rj[u] - (pb + bxj[u]); }   // the deviations
                si[u] = ri[u] * ri[u]; sj[u] = rj[u] * rj[u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const bool co = ((mi >> (8 * u)) & 0xff) && ((mj >> (8 * v)) & 0xff);
                    pair_step<METHOD>(co, ri[u], rj[v], si[u], sj[v], wy, fr[u][v], p0[u][v], p1[u][v], p2[u][v], p3[u][v],
                                      p4[u][v]);
                }
        }
    }

    if (METHOD == M_SLOPE) finish_tile_slope(a.o, i0, j0, ty, tx, fr, p0);
    else finish_tile<METHOD>(a.o, i0, j0, ty, tx, ti == tj, fr, p0, p1, p2, p3, p4);
}

// ---- similarity, sparse -----------------------------------------------------------------------------------------------

constexpr int SC = 16;            // entries of one row staged per round
constexpr int SP = SC + 1;        // padded row length in LDS: the 16 column rows of a wavefront fall on distinct banks
constexpr int Y_MAX = 0x7fffffff;

struct SparseArgs {
    const int64_t* xr_ptr; const int32_t* xr_y; const double* xr_r; int64_t n_y; int64_t n; const double* w; int64_t tiles;
    SimOut o; Baselines b;
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int METHOD>
__global__ void __launch_bounds__(256) sim_sparse_kernel(SparseArgs a) {
    __shared__ int32_t sy[2 * TB][SP];                            // rows 0..63: the tile's rows, 64..127: its columns
    __shared__ double sr[2 * TB][SP];
    __shared__ double sw[METHOD == M_SLOPE ? 1 : TB][SP];         // w[y] of the staged entries of the tile's rows
    __shared__ double sp[METHOD == M_PBASE ? TB : 1][SP];         // global_mean + by[y] of the same entries
    __shared__ int64_t pos[2 * TB], end[2 * TB];                  // cursor and end of every row, inside [0, n]
    __shared__ int32_t ready[2 * TB];
    __shared__ int32_t bound[2];

    // blockIdx.x counts the tiles of the upper triangle row by row: row ti starts at ti * T - ti (ti - 1) / 2
    const int64_t T = a.tiles, b = blockIdx.x;
    const double td = (double)(2 * T + 1);
    int64_t ti = clamp64((int64_t)((td - sqrt(td * td - 8.0 * (double)b)) * 0.5), 0, T - 1);
    while (ti + 1 < T && (ti + 1) * T - (ti + 1) * ti / 2 <= b) ++ti;
    while (ti > 0 && ti * T - ti * (ti - 1) / 2 > b) --ti;
    const int64_t tj = ti + (b - (ti * T - ti * (ti - 1) / 2));

    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t i0 = ti * TB, j0 = tj * TB;

    int32_t fr[4][4];
    double p0[4][4], p1[4][4], p2[4][4], p3[4][4], p4[4][4];      // finish_tile names them per method
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) { fr[u][v] = 0; p0[u][v] = 0.0; p1[u][v] = 0.0; p2[u][v] = 0.0; p3[u][v] = 0.0; p4[u][v] = 0.0; }
    double bxi[4] = {0.0, 0.0, 0.0, 0.0}, bxj[4] = {0.0, 0.0, 0.0, 0.0};
    if (METHOD == M_PBASE) load_bx(a.b, a.o.n_x, i0, j0, ty, tx, bxi, bxj);

    int live_a = 0, live_b = 0;
    if (t < 2 * TB) {
        const int64_t row = t < TB ? i0 + t : j0 + (t - TB);
        int64_t pb = 0, pe = 0;
        if (row < a.o.n_x) {
            pb = clamp64(a.xr_ptr[row], 0, a.n);
            pe = clamp64(a.xr_ptr[row + 1], pb, a.n);
        }
        pos[t] = pb; end[t] = pe;
        live_a = t < TB && pb < pe; live_b = t >= TB && pb < pe;
    }
    if (t < 2) bound[t] = Y_MAX;
    int n_a = __syncthreads_count(live_a), n_b = __syncthreads_count(live_b);
    int par = 0;
    while (n_a && n_b) {                                          // a tile ends when either side is exhausted
        for (int e = t; e < 2 * TB * SC; e += 256) {
            const int row = e / SC, k = e % SC;
            const int64_t p = pos[row] + k;
            if (p < end[row]) {
                const int32_t y = a.xr_y[p];
                sy[row][k] = y;
                sr[row][k] = a.xr_r[p];
                if (METHOD != M_SLOPE && row < TB) {
                    const bool in = y >= 0 && y < a.n_y;
                    sw[row][k] = in ? (a.w ? a.w[y] : 1.0) : __builtin_nan("");
                    if (METHOD == M_PBASE) sp[row][k] = in ? a.b.global_mean + a.b.by[y] : __builtin_nan("");
                }
            }
        }
        // the bound: the smallest last-staged y among rows with entries beyond their staged ones (none: everything)
        if (t < 2 * TB && end[t] - pos[t] > SC) atomicMin(&bound[par], a.xr_y[pos[t] + SC - 1]);
        if (t == 2 * TB) bound[par ^ 1] = Y_MAX;
        __syncthreads();
        live_a = 0; live_b = 0;
        if (t < 2 * TB) {
            const int32_t bd = bound[par];
            const int64_t rem = end[t] - pos[t];
            const int cnt = rem < SC ? (int)rem : SC;
            int rd = 0;
            if (cnt > 0) {
                if (sy[t][cnt - 1] <= bd) rd = cnt;               // also what makes the bound's own row advance
                else while (rd < cnt && sy[t][rd] <= bd) ++rd;
            }
            ready[t] = rd;
            pos[t] += rd;
            live_a = t < TB && pos[t] < end[t]; live_b = t >= TB && pos[t] < end[t];
        }
        n_a = __syncthreads_count(live_a);
        n_b = __syncthreads_count(live_b);
        int na[4], nb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { na[u] = ready[4 * ty + u]; nb[u] = ready[TB + 4 * tx + u]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ra = 4 * ty + u;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int rb = TB + 4 * tx + v;
                if (na[u] == 0 || nb[v] == 0) continue;
                if (sy[ra][na[u] - 1] < sy[rb][0] || sy[rb][nb[v] - 1] < sy[ra][0]) continue;   // disjoint y ranges
                int ka = 0, kb = 0;
                int32_t ya = sy[ra][0], yb = sy[rb][0];
                for (;;) {                                        // y ascending: the order of every accumulator
                    if (ya == yb) {
                        double ri = sr[ra][ka], rj = sr[rb][kb];
                        const double wy = METHOD == M_SLOPE ? 1.0 : sw[ra][ka];
                        if (METHOD == M_PBASE) {
                            const double pb = sp[ra][ka];
                            ri = ri - (pb + bxi[u]); rj = rj - (pb + bxj[v]);
                        }
                        pair_step<METHOD>(true, ri, rj, ri * ri, rj * rj, wy, fr[u][v], p0[u][v], p1[u][v], p2[u][v], p3[u][v],
                                          p4[u][v]);
                        if (++ka >= na[u] || ++kb >= nb[v]) break;
                        ya = sy[ra][ka]; yb = sy[rb][kb];
                    } else if (ya < yb) {
                        if (++ka >= na[u]) break;
                        ya = sy[ra][ka];
                    } else {
                        if (++kb >= nb[v]) break;
                        yb = sy[rb][kb];
                    }
                }
            }
        }
        par ^= 1;
        __syncthreads();                                          // the staged segments have been consumed
    }
    if (METHOD == M_SLOPE) finish_tile_slope(a.o, i0, j0, ty, tx, fr, p0);
    else finish_tile<METHOD>(a.o, i0, j0, ty, tx, ti == tj, fr, p0, p1, p2, p3, p4);
}

// One lane per row and per entry; integers only.
__global__ void __launch_bounds__(256) csr_check_kernel(const int64_t* __restrict__ xr_ptr, const int32_t* __restrict__ xr_y,
                                                        int64_t n_x, int64_t n_y, int64_t n, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t bits = 0;
    if (i < n_x) {
        const int64_t pb = xr_ptr[i], pe = xr_ptr[i + 1];
        if (pb < 0 || pb > n || pe < 0 || pe > n || pe < pb) bits |= N2V_ECCKNN_CSR_BAD_PTR;
    }
    if (i < n) {
        const int32_t y = xr_y[i];
        if (y < 0 || y >= n_y) bits |= N2V_ECCKNN_CSR_BAD_Y;
        if (i > 0 && xr_y[i - 1] >= y) {                          // legal only where a row starts at i
            int64_t lo = 0, hi = n_x + 1;                         // first k in [0, n_x] with xr_ptr[k] >= i
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (xr_ptr[mid] < i) lo = mid + 1; else hi = mid;
            }
            if (lo > n_x || xr_ptr[lo] != i) bits |= N2V_ECCKNN_CSR_UNSORTED;
        }
    }
    if (bits) atomicOr(status, bits);
}

// ---- baselines --------------------------------------------------------------------------------------------------------

// One half-epoch of baseline_als, one wavefront per row: b_out[row] = (sum over the row's list, in list order, of
// (r - mean) - b_other[id]) / (reg + entries).  The lanes gather 64 terms at a time; every lane then adds them one after
// the other.  An id outside [0, n_other) is no entry: it adds nothing and is not counted.  Row ranges are clamped to
// [0, ptr[n_rows]].
__global__ void __launch_bounds__(64) baselines_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ ids,
                                                       const double* __restrict__ r, int64_t n_rows, int64_t n_other,
                                                       double mean, double reg, const double* __restrict__ b_other,
                                                       double* __restrict__ b_out) {
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t n = ptr[n_rows] > 0 ? ptr[n_rows] : 0;
    const int64_t pb = clamp64(ptr[row], 0, n), pe = clamp64(ptr[row + 1], pb, n);
    double sum = 0.0;
    int64_t cnt = 0;
    for (int64_t base = pb; base < pe; base += 64) {
        const int64_t p = base + lane;
        double term = 0.0;
        bool in = false;
        if (p < pe) {
            const int64_t id = ids[p];
            in = id >= 0 && id < n_other;
            if (in) term = (r[p] - mean) - b_other[id];           // `r - global_mean - bu[u]`: left to right
        }
        unsigned long long have = __ballot(in);
        cnt += __popcll(have);
        while (have) {                                            // in list order; wave-uniform
            const int src = __ffsll((long long)have) - 1;
            have &= have - 1;
            sum = sum + __shfl(term, src, 64);
        }
    }
    if (lane == 0) b_out[row] = sum / (reg + (double)cnt);
}

// ---- row moments ------------------------------------------------------------------------------------------------------

// mu[row] and sd[row] of the ratings r[ptr[row] .. ptr[row + 1]), one wavefront per row, two passes: the sum from 0.0 in
// list order over the count, then sqrt of the sum of (r - mu) * (r - mu) in list order over the count.  The lanes gather
// 64 terms at a time; every lane then adds them one after the other.  Row ranges are clamped to [0, n]; an empty row is
// 0 / 0.  A sigma equal to 0.0 becomes zero_sigma unless that is NaN.
__global__ void __launch_bounds__(64) row_moments_kernel(const int64_t* __restrict__ ptr, const double* __restrict__ r,
                                                         int64_t n, double zero_sigma, double* __restrict__ mu,
                                                         double* __restrict__ sd) {
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t pb = clamp64(ptr[row], 0, n), pe = clamp64(ptr[row + 1], pb, n);
    const double cnt = (double)(pe - pb);
    double sum = 0.0;
    for (int64_t base = pb; base < pe; base += 64) {
        const int64_t p = base + lane;
        const double v = p < pe ? r[p] : 0.0;
        const int m = pe - base < 64 ? (int)(pe - base) : 64;
        for (int j = 0; j < m; ++j) sum = sum + __shfl(v, j, 64);  // in list order; wave-uniform
    }
    const double mean = sum / cnt;
    double ss = 0.0;
    for (int64_t base = pb; base < pe; base += 64) {
        const int64_t p = base + lane;
        double v = 0.0;
        if (p < pe) { const double d = r[p] - mean; v = d * d; }
        const int m = pe - base < 64 ? (int)(pe - base) : 64;
        for (int j = 0; j < m; ++j) ss = ss + __shfl(v, j, 64);
    }
    double sigma = sqrt(ss / cnt);
    if (sigma == 0.0 && zero_sigma == zero_sigma) sigma = zero_sigma;
    if (lane == 0) { mu[row] = mean; sd[row] = sigma; }
}

// ---- estimate ---------------------------------------------------------------------------------------------------------

using n2v::POS_NONE, n2v::order_key, n2v::beats, n2v::list_insert;   // n2v_rank.h

using n2v::predict_value, n2v::Seen, n2v::SeenCursor, n2v::TopList;   // n2v_topn.h

struct KnnModel {
    const double* sim; int64_t n_x; const int64_t* yr_ptr; const int32_t* yr_x; const double* yr_r; int64_t n_y;
    int k; int min_k;
};

// What a neighbour's rating is centred on, a compile-time mode of knn_estimate: nothing (EccenKNN, KNNBasic), the row
// mean of x2 (KNNWithMeans), the same over the row's sigma (KNNWithZScore), or the baseline of the pair (KNNBaseline).
constexpr int C_NONE = 0;         // then N2V_ECCKNN_CENTER_MEANS, _ZSCORE, _BASELINE
// tx: mu[n_x] (means, z-score) or bx[n_x] (baseline); sd: sigma[n_x] (z-score); by[n_y] (baseline).  Mode none reads none.
struct Centering {
    double gm; int user_based; const double* tx; const double* sd; const double* by;
};

// The estimate of (x, y), the one copy behind estimate_kernel and eccknn_topn_kernel: all 64 lanes of a 64-thread
// workgroup together, x and y the same in every lane, ls / lp the k-entry selection list in LDS.  Every lane leaves with
// the same est, actual_k and return value (true: the estimate is impossible, est = 0).
// The centred modes select the same neighbours and differ in the sums and the finish: a kept neighbour adds
// s * (r - mu[x2]), s * ((r - mu[x2]) / sd[x2]) or s * (r - ((gm + bx[x2]) + by[y])); fewer than min_k of them zero
// sum_ratings instead of making the estimate impossible; est = base [+ sum_ratings / sum_sim [* sd[x]]] with base mu[x] or
// (gm + bu[u]) + bi[i].  Under the baseline mode nothing is impossible: an unknown user or item drops its bias.
// The four steps of an estimate, each in one copy: knn_unknown, knn_select, knn_sums, knn_finish.  knn_estimate is the four
// in a row; knn_estimate_sweep runs the selection once at the largest k of a grid and the other steps per cell.

// True when x or y is unknown, which settles the estimate without a neighbour: est and imp are it.
template <int MODE>
__device__ __forceinline__ bool knn_unknown(const KnnModel& a, const Centering& c, int64_t x, int64_t y, double& est,
                                            bool& imp) {
    est = 0.0; imp = false;
    const bool kx = x >= 0 && x < a.n_x, ky = y >= 0 && y < a.n_y;
    if (kx && ky) return false;
    if (MODE == N2V_ECCKNN_CENTER_BASELINE) {                         // the user's bias first, whichever side x is
        double e = c.gm;
        if (c.user_based) { if (kx) e = e + c.tx[x]; if (ky) e = e + c.by[y]; }
        else { if (ky) e = e + c.by[y]; if (kx) e = e + c.tx[x]; }
        est = e;
    } else {
        imp = true;                                               // 'User and/or item is unkown.'
    }
    return true;
}

// The selection: the best k of the raters of y under the order of n2v_rank.h, in ls / lp in rank order.  Returns L, the
// length of y's list (beg: where it starts); the first min(L, k) entries of the list are real, the others fillers.  The
// order is total, so the first k2 < k entries are what a selection with k2 would have kept.
__device__ __forceinline__ int knn_select(const KnnModel& a, int k, int64_t x, int64_t y, double* ls, int32_t* lp, int lane,
                                          int64_t& beg) {
    __syncthreads();                                              // the previous estimate's list has been read
    // the list starts as k entries (NaN, POS_NONE): below any real entry, so it is always "full"
    for (int i = lane; i < k; i += 64) { ls[i] = __builtin_nan(""); lp[i] = POS_NONE; }
    __syncthreads();
    beg = a.yr_ptr[y];
    const int64_t len64 = a.yr_ptr[y + 1] - beg;
    const int L = (int)(len64 < POS_NONE ? len64 : POS_NONE - 1);
    const double* srow = a.sim + x * a.n_x;
    uint64_t tk = 0ull;
    int tp = POS_NONE;
    for (int base = 0; base < L; base += 64) {
        const int p = base + lane;
        double s = __builtin_nan("");
        if (p < L) {
            const int64_t x2 = a.yr_x[beg + p];
            if (x2 >= 0 && x2 < a.n_x) s = srow[x2];
        }
        unsigned long long cand = __ballot(p < L && beats(order_key(s), p, tk, tp));
        while (cand) {                                            // in list order; wave-uniform
            const int src = __ffsll((long long)cand) - 1;
            cand &= cand - 1;
            const double cs = __shfl(s, src, 64);
            const int cp = base + src;
            const uint64_t ck = order_key(cs);
            if (beats(ck, cp, tk, tp)) list_insert(ls, lp, k, cs, cp, ck, lane, tk, tp);
        }
    }
    return L;
}

// Ranks [from, to) of the selection added to the sums, to <= min(L, k): `for (sim, r) in k_neighbors: if sim > 0: ...`.
// Every lane runs the same sums, one add after the other in rank order, so the sums over [0, to) are the same bits in
// however many calls the range is walked.  pby: by[y] under the baseline mode.
template <int MODE>
__device__ __forceinline__ void knn_sums(const KnnModel& a, const Centering& c, int64_t beg, int L, double pby,
                                         const double* ls, const int32_t* lp, int lane, int from, int to, double& sum_sim,
                                         double& sum_ratings, int& actual_k) {
    for (int base = from; base < to; base += 64) {
        const int i = base + lane;
        double s = 0.0, sr = 0.0;
        if (i < to) {
            const int p = lp[i];
            if (p < L) {                                          // always: a filler is below every real entry
                if (MODE == C_NONE) {
                    s = ls[i];
                    sr = s * a.yr_r[beg + p];                     // sim * r, rounded before it is added
                } else {
                    // the neighbour's tables are read from the position the list kept, under the selection's own test:
                    // an id outside [0, n_x) is in the list only with a NaN score; it adds nothing and reads nothing
                    const int64_t x2 = a.yr_x[beg + p];
                    if (x2 >= 0 && x2 < a.n_x) {
                        s = ls[i];
                        const double r = a.yr_r[beg + p];
                        double d;
                        if (MODE == N2V_ECCKNN_CENTER_MEANS) d = r - c.tx[x2];
                        else if (MODE == N2V_ECCKNN_CENTER_ZSCORE) d = (r - c.tx[x2]) / c.sd[x2];
                        else d = r - ((c.gm + c.tx[x2]) + pby);
                        sr = s * d;
                    }
                }
            }
        }
        const int cnt = to - base < 64 ? to - base : 64;
        for (int j = 0; j < cnt; ++j) {
            const double sj = __shfl(s, j, 64), tj = __shfl(sr, j, 64);
            if (sj > 0) { sum_sim = sum_sim + sj; sum_ratings = sum_ratings + tj; ++actual_k; }
        }
    }
}

// The finish of the mode for one min_k; true: the estimate is impossible (est = 0).
template <int MODE>
__device__ __forceinline__ bool knn_finish(const Centering& c, int64_t x, double pby, int min_k, double sum_sim,
                                           double sum_ratings, int actual_k, double& est) {
    if (MODE == C_NONE) {
        const bool imp = actual_k < min_k;                        // 'Not enough neighbors.'
        est = imp ? 0.0 : sum_ratings / sum_sim;
        return imp;
    }
    if (actual_k < min_k) sum_ratings = 0.0;                      // too few neighbours: the base alone, not impossible
    double b;
    if (MODE == N2V_ECCKNN_CENTER_BASELINE) b = c.user_based ? (c.gm + c.tx[x]) + pby : (c.gm + pby) + c.tx[x];
    else b = c.tx[x];
    if (actual_k == 0) est = b;                                   // `except ZeroDivisionError: pass`
    else if (MODE == N2V_ECCKNN_CENTER_ZSCORE) est = b + (sum_ratings / sum_sim) * c.sd[x];
    else est = b + sum_ratings / sum_sim;
    return false;
}

template <int MODE>
__device__ __forceinline__ bool knn_estimate(const KnnModel& a, const Centering& c, int64_t x, int64_t y, double* ls,
                                             int32_t* lp, int lane, double& est, int& n_pos) {
    n_pos = 0;
    bool imp;
    if (knn_unknown<MODE>(a, c, x, y, est, imp)) return imp;
    int64_t beg;
    const int L = knn_select(a, a.k, x, y, ls, lp, lane, beg);
    double sum_sim = 0.0, sum_ratings = 0.0;
    int actual_k = 0;
    const double pby = MODE == N2V_ECCKNN_CENTER_BASELINE ? c.by[y] : 0.0;
    knn_sums<MODE>(a, c, beg, L, pby, ls, lp, lane, 0, L < a.k ? L : a.k, sum_sim, sum_ratings, actual_k);
    n_pos = actual_k;
    return knn_finish<MODE>(c, x, pby, a.min_k, sum_sim, sum_ratings, actual_k, est);
}

struct EstArgs {
    KnnModel m; const int32_t* qx; const int32_t* qy; int64_t n_q;
    double* est; int32_t* actual_k; uint8_t* impossible;
};

template <int MODE>
__global__ void __launch_bounds__(64) estimate_kernel(EstArgs a, Centering c) {
    __shared__ double ls[N2V_ECCKNN_MAX_K];
    __shared__ int32_t lp[N2V_ECCKNN_MAX_K];
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    double est;
    int actual_k;
    const bool imp = knn_estimate<MODE>(a.m, c, a.qx[q], a.qy[q], ls, lp, lane, est, actual_k);
    if (lane == 0) { a.est[q] = est; a.actual_k[q] = actual_k; a.impossible[q] = imp ? 1 : 0; }
}

// The grid of a sweep travels by value: ks and min_ks strictly ascending, m.k = ks[n_k - 1], m.min_k unused.
struct SweepArgs {
    KnnModel m; const int32_t* qx; const int32_t* qy; int64_t n_q;
    int n_k, n_m; int ks[N2V_ECCKNN_MAX_SWEEP], min_ks[N2V_ECCKNN_MAX_SWEEP];
    double* est; int32_t* actual_k; uint8_t* impossible;         // [n_k][n_m][n_q], [n_k][n_q], [n_k][n_m][n_q]
};

// Every (ks[j], min_ks[m]) cell of query q from one selection at the largest k: the list is walked once, rank
// min(L, ks[j - 1]) to min(L, ks[j]) for j = 0, 1, ..., and where the walk stands at min(L, ks[j]) the sums are those of
// knn_estimate with k = ks[j] (knn_select, knn_sums), so every min_k is finished from them and written; nothing is kept.
template <int MODE>
__device__ __forceinline__ void knn_estimate_sweep(const SweepArgs& a, const Centering& c, int64_t q, double* ls,
                                                   int32_t* lp, int lane) {
    const int64_t x = a.qx[q], y = a.qy[q];
    double est;
    bool imp;
    if (knn_unknown<MODE>(a.m, c, x, y, est, imp)) {
        if (lane == 0) {
            for (int j = 0; j < a.n_k; ++j) {
                a.actual_k[j * a.n_q + q] = 0;
                for (int m = 0; m < a.n_m; ++m) {
                    const int64_t o = ((int64_t)j * a.n_m + m) * a.n_q + q;
                    a.est[o] = est; a.impossible[o] = imp ? 1 : 0;
                }
            }
        }
        return;
    }
    int64_t beg;
    const int L = knn_select(a.m, a.m.k, x, y, ls, lp, lane, beg);
    double sum_sim = 0.0, sum_ratings = 0.0;
    int actual_k = 0, from = 0;
    const double pby = MODE == N2V_ECCKNN_CENTER_BASELINE ? c.by[y] : 0.0;
    for (int j = 0; j < a.n_k; ++j) {
        const int to = L < a.ks[j] ? L : a.ks[j];
        knn_sums<MODE>(a.m, c, beg, L, pby, ls, lp, lane, from, to, sum_sim, sum_ratings, actual_k);
        from = to;
        if (lane == 0) a.actual_k[j * a.n_q + q] = actual_k;
        for (int m = 0; m < a.n_m; ++m) {
            imp = knn_finish<MODE>(c, x, pby, a.min_ks[m], sum_sim, sum_ratings, actual_k, est);
            if (lane == 0) {
                const int64_t o = ((int64_t)j * a.n_m + m) * a.n_q + q;
                a.est[o] = est; a.impossible[o] = imp ? 1 : 0;
            }
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(64) estimate_sweep_kernel(SweepArgs a, Centering c) {
    __shared__ double ls[N2V_ECCKNN_MAX_K];
    __shared__ int32_t lp[N2V_ECCKNN_MAX_K];
    knn_estimate_sweep<MODE>(a, c, blockIdx.x, ls, lp, threadIdx.x);
}

// ---- top-N ------------------------------------------------------------------------------------------------------------

struct TopnArgs {
    KnnModel m; int user_based; Seen seen; int64_t n_items;
    const int32_t* owners; int N; int S;
    double global_mean, lo, hi;
    double* part_score; int32_t* part_pos;
};

// One wavefront per (owner, segment of candidates): the owner's unseen items of the segment, ascending, each estimated
// as (x, y) = (owner, item) when user_based and (item, owner) otherwise, clipped, and folded into the segment's best-N
// list under the order of n2v_rank.h with the item id as the position.  An owner outside the seen CSR's rows (-1) has
// seen nothing and every estimate of it is impossible (under the baseline mode: global_mean + bi[item]).
template <int MODE>
__global__ void __launch_bounds__(64) eccknn_topn_kernel(TopnArgs a, Centering c) {
    __shared__ double ls[N2V_ECCKNN_MAX_K];
    __shared__ int32_t lp[N2V_ECCKNN_MAX_K];
    __shared__ double ts[N2V_TOPN_MAX_N];
    __shared__ int32_t tp[N2V_TOPN_MAX_N];
    const int64_t o = blockIdx.x;
    const int seg = blockIdx.y, lane = threadIdx.x;
    const int64_t u = a.owners[o];
    int64_t c0, c1;
    n2v::segment_range(a.n_items, seg, a.S, c0, c1);
    SeenCursor cur;
    cur.open(a.seen, u, c0);
    TopList top;
    top.init(ts, tp, a.N, lane);
    for (int64_t i = c0; i < c1; ++i) {
        if (cur.has(i)) continue;
        double est;
        int actual_k;
        const bool imp = knn_estimate<MODE>(a.m, c, a.user_based ? u : i, a.user_based ? i : u, ls, lp, lane, est, actual_k);
        top.offer(predict_value(est, imp, a.global_mean, a.lo, a.hi), (int)i, lane);
    }
    const int64_t base = (o * a.S + seg) * a.N;
    top.store(a.part_score + base, a.part_pos + base, lane);
}

// ---- predict + rmse ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) predict_kernel(const double* __restrict__ est, const uint8_t* __restrict__ imp,
                                                      const double* __restrict__ r_true, int64_t n, double global_mean,
                                                      double lo, double hi, double* __restrict__ pred,
                                                      double* __restrict__ rmse) {
    __shared__ double sq[256];
    double acc = 0.0;                                             // thread 0's; test order
    for (int64_t base = 0; base < n; base += 256) {
        const int64_t i = base + threadIdx.x;
        if (i < n) {
            const double e = predict_value(est[i], imp[i] != 0, global_mean, lo, hi);
            pred[i] = e;
            if (r_true) { const double d = r_true[i] - e; sq[threadIdx.x] = d * d; }
        }
        if (r_true) {
            __syncthreads();
            if (threadIdx.x == 0) {
                const int cnt = n - base < 256 ? (int)(n - base) : 256;
                for (int j = 0; j < cnt; ++j) acc = acc + sq[j];
            }
            __syncthreads();
        }
    }
    if (r_true && threadIdx.x == 0) rmse[0] = sqrt(acc / (double)n);
}

// ---- rmse and mae of columns ------------------------------------------------------------------------------------------

// One workgroup per column of pred[n_cols][n]; the sums as predict_kernel takes its own, so rmse[c] is its value.
__global__ void __launch_bounds__(256) errors_kernel(const double* __restrict__ pred, const double* __restrict__ r_true,
                                                     int64_t n, double* __restrict__ rmse, double* __restrict__ mae) {
    __shared__ double sq[256];
    __shared__ double ab[256];
    const double* col = pred + (int64_t)blockIdx.x * n;
    double acc = 0.0, aab = 0.0;                                  // thread 0's; test order
    for (int64_t base = 0; base < n; base += 256) {
        const int64_t i = base + threadIdx.x;
        if (i < n) { const double d = r_true[i] - col[i]; sq[threadIdx.x] = d * d; ab[threadIdx.x] = fabs(d); }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = n - base < 256 ? (int)(n - base) : 256;
            for (int j = 0; j < cnt; ++j) { acc = acc + sq[j]; aab = aab + ab[j]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (rmse) rmse[blockIdx.x] = sqrt(acc / (double)n);
        if (mae) mae[blockIdx.x] = aab / (double)n;
    }
}

}  // namespace

// ---- the six tile calls: a frame check, the family's own checks, an args struct, a launch -----------------------------

// The checks every dense tile call makes, in the order its callers always made them: the shape, the dense limit, the
// family's own checks (extra: a callable, 0 or the error; SlopeOne's come before the dense limit, extra_first), the
// pointers every method reads, the tile count.  xs / ys name the two sides in the messages.  T, the tiles a side, or the
// (negative) error.
template <class Extra>
static int64_t dense_frame(const char* who, const char* xs, const char* ys, int64_t n_x, int64_t n_y, const double* dense,
                           const uint8_t* mask, const double* sim, bool extra_first, Extra extra) {
    if (n_x < 1 || n_y < 1) return n2v::fail(N2V_ERR_INVALID, "%s: %s=%lld %s=%lld", who, xs, (long long)n_x, ys, (long long)n_y);
    if (extra_first) if (const int rc = extra()) return rc;
    if (n_x > MAX_DENSE || n_y > MAX_DENSE || n_x * n_y > MAX_DENSE)
        return n2v::fail(N2V_ERR_INVALID, "%s: %s * %s = %lld x %lld exceeds the dense limit of %lld elements", who, xs, ys,
                         (long long)n_x, (long long)n_y, (long long)MAX_DENSE);
    if (!extra_first) if (const int rc = extra()) return rc;
    if (!dense || !mask || !sim) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer", who);
    const int64_t T = (n_x + TB - 1) / TB;
    if (T > 65535) return n2v::fail(N2V_ERR_INVALID, "%s: %s %lld needs more than 65535 tiles a side", who, xs, (long long)n_x);
    return T;
}

// The same for the sparse form, where every family's checks sit between the shape and the pointers.
template <class Extra>
static int64_t sparse_frame(const char* who, const char* xs, const char* ys, int64_t n_x, int64_t n_y, int64_t n,
                            const int64_t* xr_ptr, const int32_t* xr_y, const double* xr_r, const double* sim, Extra extra) {
    if (n_x < 1 || n_y < 1 || n_y > Y_MAX || n < 0)
        return n2v::fail(N2V_ERR_INVALID, "%s: %s=%lld %s=%lld n=%lld", who, xs, (long long)n_x, ys, (long long)n_y, (long long)n);
    if (const int rc = extra()) return rc;
    if (!xr_ptr || !sim || (n > 0 && (!xr_y || !xr_r))) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer", who);
    const int64_t T = (n_x + TB - 1) / TB;
    if (T > 65535) return n2v::fail(N2V_ERR_INVALID, "%s: %s %lld needs more than 65535 tiles a side", who, xs, (long long)n_x);
    return T;
}

// One workgroup per tile of the T x T grid (the lower triangle returns at once); method is one of the five METHODs.
static int launch_sim(const char* who, int method, int64_t T, const SimArgs& a, void* stream) {
    const dim3 grid((unsigned)T, (unsigned)T);
    hipStream_t s = (hipStream_t)stream;
    switch (method) {
        case N2V_ECCKNN_COSINE: sim_kernel<N2V_ECCKNN_COSINE><<<grid, 256, 0, s>>>(a); break;
        case N2V_ECCKNN_MSD: sim_kernel<N2V_ECCKNN_MSD><<<grid, 256, 0, s>>>(a); break;
        case M_PEARSON: sim_kernel<M_PEARSON><<<grid, 256, 0, s>>>(a); break;
        case M_PBASE: sim_kernel<M_PBASE><<<grid, 256, 0, s>>>(a); break;
        case M_SLOPE: sim_kernel<M_SLOPE><<<grid, 256, 0, s>>>(a); break;
        default: return n2v::fail(N2V_ERR_INVALID, "%s: no tile kernel for method %d", who, method);
    }
    return n2v::check_launch(who);
}

// One workgroup per tile of the upper triangle, a.tiles a side.
static int launch_sim_sparse(const char* who, int method, const SparseArgs& a, void* stream) {
    const unsigned grid = (unsigned)(a.tiles * (a.tiles + 1) / 2);   // < 2^31 for T <= 65535
    hipStream_t s = (hipStream_t)stream;
    switch (method) {
        case N2V_ECCKNN_COSINE: sim_sparse_kernel<N2V_ECCKNN_COSINE><<<grid, 256, 0, s>>>(a); break;
        case N2V_ECCKNN_MSD: sim_sparse_kernel<N2V_ECCKNN_MSD><<<grid, 256, 0, s>>>(a); break;
        case M_PEARSON: sim_sparse_kernel<M_PEARSON><<<grid, 256, 0, s>>>(a); break;
        case M_PBASE: sim_sparse_kernel<M_PBASE><<<grid, 256, 0, s>>>(a); break;
        case M_SLOPE: sim_sparse_kernel<M_SLOPE><<<grid, 256, 0, s>>>(a); break;
        default: return n2v::fail(N2V_ERR_INVALID, "%s: no tile kernel for method %d", who, method);
    }
    return n2v::check_launch(who);
}

// What cosine and msd check beside the frame: the method, and the weights they cannot do without; 0 or the error.
static int method_args(const char* who, int32_t method, const double* w) {
    if (method != N2V_ECCKNN_COSINE && method != N2V_ECCKNN_MSD) return n2v::fail(N2V_ERR_INVALID, "%s: method %d", who, method);
    if (!w) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer", who);
    return N2V_OK;
}

// What the two Pearson calls check beside the frame; 0 or the error.
static int pearson_args(const char* who, int32_t kind, const double* bx, const double* by) {
    if (kind != N2V_ECCKNN_PEARSON && kind != N2V_ECCKNN_PEARSON_BASELINE) return n2v::fail(N2V_ERR_INVALID, "%s: kind %d", who, kind);
    if (kind == N2V_ECCKNN_PEARSON_BASELINE && (!bx || !by)) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer (bx / by, required by kind 1)", who);
    return N2V_OK;
}

// kind 0: a1 .. a4 are sqi, sqj, si, sj; kind 1: a1, a2 are sq_diff_i, sq_diff_j and min_support is raised to 2.
static SimOut pearson_out(int32_t kind, int64_t n_x, int32_t min_support, double shrinkage, double* sim, int32_t* freq,
                          double* prods, double* a1, double* a2, double* a3, double* a4) {
    const bool base = kind == N2V_ECCKNN_PEARSON_BASELINE;
    return SimOut{n_x, base && min_support < 2 ? 2 : min_support, sim, freq, prods, a1, a2, nullptr,
                  base ? nullptr : a3, base ? nullptr : a4, shrinkage};
}

// What the two SlopeOne table calls check of their outputs; 0 or the error.
static int slope_args(const char* who, int64_t n_items, const double* dev, const int32_t* freq) {
    if (n_items > 65535 || n_items * n_items > MAX_DENSE)
        return n2v::fail(N2V_ERR_INVALID, "%s: n_items^2 = %lld^2 exceeds the table limit of %lld elements", who,
                         (long long)n_items, (long long)MAX_DENSE);
    if (!dev || !freq) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer", who);
    return N2V_OK;
}

static SimOut slope_out(int64_t n_items, double* dev, int32_t* freq, double* acc) {
    return SimOut{n_items, 0, dev, freq, acc, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0};
}

// ---- the plain and the centred k-NN calls: one body each for the estimate and for the top-N lists ---------------------

// What a centred call adds to the plain one: the caller's centring code as it came, and the tables.  The plain calls pass
// none (NULL): mode C_NONE, which reads no table.
struct Centred {
    int32_t code; Centering tables;
};

// The checks the two centred calls make of their own; 0 or the error.  A table the mode reads may not be NULL.
static int centering_args(const char* who, const Centred& c) {
    if (c.code != N2V_ECCKNN_CENTER_MEANS && c.code != N2V_ECCKNN_CENTER_ZSCORE && c.code != N2V_ECCKNN_CENTER_BASELINE)
        return n2v::fail(N2V_ERR_INVALID, "%s: centering %d (1 means, 2 z-score, 3 baseline)", who, c.code);
    if (!c.tables.tx) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer (tx, the mu or bx table over x)", who);
    if (c.code == N2V_ECCKNN_CENTER_ZSCORE && !c.tables.sd) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer (sd, required by centering 2)", who);
    if (c.code == N2V_ECCKNN_CENTER_BASELINE && !c.tables.by) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer (by, required by centering 3)", who);
    return N2V_OK;
}

static int knn_options(const char* who, int32_t k, int32_t min_k) {
    if (k < 1 || k > N2V_ECCKNN_MAX_K) return n2v::fail(N2V_ERR_INVALID, "%s: k %d outside [1, %d]", who, k, N2V_ECCKNN_MAX_K);
    if (min_k < 1) return n2v::fail(N2V_ERR_INVALID, "%s: min_k %d < 1 (an empty neighbourhood has no mean)", who, min_k);
    return N2V_OK;
}

// f(mode, tables) with the centring mode as a compile-time constant: what picks the instantiation of estimate_kernel and
// of eccknn_topn_kernel.  c NULL: C_NONE; otherwise a code centering_args let through.
template <class F>
static void with_centering(const Centred* c, F f) {
    if (!c) return f(std::integral_constant<int, C_NONE>{}, Centering{0.0, 1, nullptr, nullptr, nullptr});
    switch (c->code) {
        case N2V_ECCKNN_CENTER_MEANS: return f(std::integral_constant<int, N2V_ECCKNN_CENTER_MEANS>{}, c->tables);
        case N2V_ECCKNN_CENTER_ZSCORE: return f(std::integral_constant<int, N2V_ECCKNN_CENTER_ZSCORE>{}, c->tables);
        default: return f(std::integral_constant<int, N2V_ECCKNN_CENTER_BASELINE>{}, c->tables);
    }
}

// What the single-cell and the sweep estimate calls check after their k and min_k; 0 or the error.
static int estimate_args(const char* who, const KnnModel& m, const int32_t* qx, const int32_t* qy, int64_t n_q,
                         const Centred* c, const double* est, const int32_t* actual_k, const uint8_t* impossible) {
    if (n_q < 1 || n_q > 0x7fffffff) return n2v::fail(N2V_ERR_INVALID, "%s: n_q %lld outside [1, 2^31)", who, (long long)n_q);
    if (m.n_x < 1 || m.n_y < 1) return n2v::fail(N2V_ERR_INVALID, "%s: n_x=%lld n_y=%lld", who, (long long)m.n_x, (long long)m.n_y);
    if (c) if (const int rc = centering_args(who, *c)) return rc;
    if (!m.sim || !m.yr_ptr || !qx || !qy || !est || !actual_k || !impossible) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer", who);
    return N2V_OK;
}

// n2v_eccknn_estimate (c NULL) and n2v_eccknn_estimate_centered.
static int estimate_call(const char* who, const KnnModel& m, const int32_t* qx, const int32_t* qy, int64_t n_q,
                         const Centred* c, double* est, int32_t* actual_k, uint8_t* impossible, void* stream) {
    if (const int rc = knn_options(who, m.k, m.min_k)) return rc;
    if (const int rc = estimate_args(who, m, qx, qy, n_q, c, est, actual_k, impossible)) return rc;
    const EstArgs a{m, qx, qy, n_q, est, actual_k, impossible};
    with_centering(c, [&](auto mode, const Centering& t) {
        estimate_kernel<decltype(mode)::value><<<(unsigned)n_q, 64, 0, (hipStream_t)stream>>>(a, t);
    });
    return n2v::check_launch(who);
}

// n2v_eccknn_estimate_sweep (c NULL) and n2v_eccknn_estimate_sweep_centered.  ks and min_ks are host arrays.
static int sweep_call(const char* who, KnnModel m, const int32_t* qx, const int32_t* qy, int64_t n_q, const int32_t* ks,
                      int32_t n_k, const int32_t* min_ks, int32_t n_m, const Centred* c, double* est, int32_t* actual_k,
                      uint8_t* impossible, void* stream) {
    if (n_k < 1 || n_k > N2V_ECCKNN_MAX_SWEEP || n_m < 1 || n_m > N2V_ECCKNN_MAX_SWEEP)
        return n2v::fail(N2V_ERR_INVALID, "%s: n_k %d or n_m %d outside [1, %d]", who, n_k, n_m, N2V_ECCKNN_MAX_SWEEP);
    if (!ks || !min_ks) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer (ks, min_ks: host arrays)", who);
    SweepArgs a{};
    for (int j = 0; j < n_k; ++j) {
        if (const int rc = knn_options(who, ks[j], 1)) return rc;
        if (j && ks[j] <= ks[j - 1]) return n2v::fail(N2V_ERR_INVALID, "%s: ks not strictly ascending (%d after %d)", who, ks[j], ks[j - 1]);
        a.ks[j] = ks[j];
    }
    for (int j = 0; j < n_m; ++j) {
        if (const int rc = knn_options(who, 1, min_ks[j])) return rc;
        if (j && min_ks[j] <= min_ks[j - 1])
            return n2v::fail(N2V_ERR_INVALID, "%s: min_ks not strictly ascending (%d after %d)", who, min_ks[j], min_ks[j - 1]);
        a.min_ks[j] = min_ks[j];
    }
    if (const int rc = estimate_args(who, m, qx, qy, n_q, c, est, actual_k, impossible)) return rc;
    m.k = ks[n_k - 1]; m.min_k = min_ks[0];
    a.m = m; a.qx = qx; a.qy = qy; a.n_q = n_q; a.n_k = n_k; a.n_m = n_m;
    a.est = est; a.actual_k = actual_k; a.impossible = impossible;
    with_centering(c, [&](auto mode, const Centering& t) {
        estimate_sweep_kernel<decltype(mode)::value><<<(unsigned)n_q, 64, 0, (hipStream_t)stream>>>(a, t);
    });
    return n2v::check_launch(who);
}

// n2v_eccknn_topn (c NULL) and n2v_eccknn_topn_centered; merge_who names the merge launch in an error.
static int topn_call(const char* who, const char* merge_who, const KnnModel& m, int32_t user_based, const int64_t* seen_ptr,
                     const int32_t* seen_i, int64_t n_seen, const int32_t* owners, int64_t n_owners, double global_mean,
                     double lo, double hi, int32_t top_n, int32_t segments, const Centred* c,
                     double* part_score, int32_t* part_pos, int32_t* items, double* score, void* stream) {
    if (const int rc = knn_options(who, m.k, m.min_k)) return rc;
    if (m.n_x < 1 || m.n_y < 1) return n2v::fail(N2V_ERR_INVALID, "%s: n_x=%lld n_y=%lld", who, (long long)m.n_x, (long long)m.n_y);
    if (c) if (const int rc = centering_args(who, *c)) return rc;
    const int64_t n_users = user_based ? m.n_x : m.n_y, n_items = user_based ? m.n_y : m.n_x;
    if (const int rc = n2v::topn_args(who, n_owners, n_items, top_n, segments, seen_ptr, seen_i, n_seen, owners, part_score,
                                      part_pos, items, score))
        return rc;
    if (!m.sim || !m.yr_ptr) return n2v::fail(N2V_ERR_INVALID, "%s: null pointer", who);
    const int S = segments > 0 ? segments : n2v_topn_segments(n_owners, n_items);
    const TopnArgs a{m, user_based ? 1 : 0, Seen{seen_ptr, seen_i, n_users, n_seen}, n_items, owners, top_n, S, global_mean,
                     lo, hi, part_score, part_pos};
    hipStream_t s = (hipStream_t)stream;
    with_centering(c, [&](auto mode, const Centering& t) {
        eccknn_topn_kernel<decltype(mode)::value><<<dim3((unsigned)n_owners, (unsigned)S), 64, 0, s>>>(a, t);
    });
    if (const int rc = n2v::check_launch(who)) return rc;
    return n2v::topn_merge(merge_who, part_score, part_pos, n_owners, S, top_n, items, score, s);
}

extern "C" {

int32_t n2v_eccknn_max_k(void) { return N2V_ECCKNN_MAX_K; }
int64_t n2v_eccknn_max_dense(void) { return MAX_DENSE; }

int n2v_eccknn_densify(const int32_t* x, const int32_t* y, const double* r, int64_t n, int64_t n_x, int64_t n_y,
                       double* dense, uint8_t* mask, void* stream) {
    if (n < 0 || n_x < 1 || n_y < 1) return n2v::fail(N2V_ERR_INVALID, "eccknn_densify: n=%lld n_x=%lld n_y=%lld", (long long)n, (long long)n_x, (long long)n_y);
    if (n_x > MAX_DENSE || n_y > MAX_DENSE || n_x * n_y > MAX_DENSE)
        return n2v::fail(N2V_ERR_INVALID, "eccknn_densify: n_x * n_y = %lld x %lld exceeds the dense limit of %lld elements",
                         (long long)n_x, (long long)n_y, (long long)MAX_DENSE);
    if (!dense || !mask || (n > 0 && (!x || !y || !r))) return n2v::fail(N2V_ERR_INVALID, "eccknn_densify: null pointer");
    if (n > (int64_t)0x7fffffff * 256) return n2v::fail(N2V_ERR_INVALID, "eccknn_densify: too many ratings");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(dense, 0, (size_t)(n_x * n_y) * sizeof(double), s) != hipSuccess ||
        hipMemsetAsync(mask, 0, (size_t)(n_x * n_y), s) != hipSuccess)
        return n2v::fail(N2V_ERR_HIP, "eccknn_densify: memset failed");
    if (n == 0) return N2V_OK;
    densify_kernel<<<n2v::grid_for(n, 256), 256, 0, s>>>(x, y, r, n, n_x, n_y, dense, mask);
    return n2v::check_launch("eccknn_densify");
}

int n2v_eccknn_sim(const double* dense, const uint8_t* mask, int64_t n_x, int64_t n_y, const double* w, int32_t method,
                   int32_t min_support, double* sim, int32_t* freq, double* prods, double* sqi, double* sqj,
                   double* sq_diff, void* stream) {
    const char* who = "eccknn_sim";
    const int64_t T = dense_frame(who, "n_x", "n_y", n_x, n_y, dense, mask, sim, false, [&] { return method_args(who, method, w); });
    if (T < 0) return (int)T;
    const SimArgs a{dense, mask, n_y, w, SimOut{n_x, min_support, sim, freq, prods, sqi, sqj, sq_diff, nullptr, nullptr, 0.0},
                    Baselines{nullptr, nullptr, 0.0}};
    return launch_sim(who, method, T, a, stream);
}

int32_t n2v_eccknn_sparse_chunk(void) { return SC; }

int n2v_eccknn_csr_check(const int64_t* xr_ptr, const int32_t* xr_y, int64_t n_x, int64_t n_y, int64_t n, int32_t* status,
                         void* stream) {
    if (n_x < 1 || n_y < 1 || n < 0) return n2v::fail(N2V_ERR_INVALID, "eccknn_csr_check: n_x=%lld n_y=%lld n=%lld", (long long)n_x, (long long)n_y, (long long)n);
    if (!xr_ptr || !status || (n > 0 && !xr_y)) return n2v::fail(N2V_ERR_INVALID, "eccknn_csr_check: null pointer");
    const int64_t lanes = n_x > n ? n_x : n;
    if (lanes > (int64_t)0x7fffffff * 256) return n2v::fail(N2V_ERR_INVALID, "eccknn_csr_check: too many rows or entries");
    csr_check_kernel<<<n2v::grid_for(lanes, 256), 256, 0, (hipStream_t)stream>>>(xr_ptr, xr_y, n_x, n_y, n, status);
    return n2v::check_launch("eccknn_csr_check");
}

int n2v_eccknn_sim_sparse(const int64_t* xr_ptr, const int32_t* xr_y, const double* xr_r, int64_t n_x, int64_t n_y,
                          int64_t n, const double* w, int32_t method, int32_t min_support, double* sim, int32_t* freq,
                          double* prods, double* sqi, double* sqj, double* sq_diff, void* stream) {
    const char* who = "eccknn_sim_sparse";
    const int64_t T = sparse_frame(who, "n_x", "n_y", n_x, n_y, n, xr_ptr, xr_y, xr_r, sim, [&] { return method_args(who, method, w); });
    if (T < 0) return (int)T;
    const SparseArgs a{xr_ptr, xr_y, xr_r, n_y, n, w, T,
                       SimOut{n_x, min_support, sim, freq, prods, sqi, sqj, sq_diff, nullptr, nullptr, 0.0},
                       Baselines{nullptr, nullptr, 0.0}};
    return launch_sim_sparse(who, method, a, stream);
}

int n2v_eccknn_pearson(const double* dense, const uint8_t* mask, int64_t n_x, int64_t n_y, const double* w, int32_t kind,
                       int32_t min_support, double global_mean, const double* bx, const double* by, double shrinkage,
                       double* sim, int32_t* freq, double* prods, double* a1, double* a2, double* a3, double* a4,
                       void* stream) {
    const char* who = "eccknn_pearson";
    const int64_t T = dense_frame(who, "n_x", "n_y", n_x, n_y, dense, mask, sim, false, [&] { return pearson_args(who, kind, bx, by); });
    if (T < 0) return (int)T;
    const SimArgs a{dense, mask, n_y, w, pearson_out(kind, n_x, min_support, shrinkage, sim, freq, prods, a1, a2, a3, a4),
                    Baselines{bx, by, global_mean}};
    return launch_sim(who, kind == N2V_ECCKNN_PEARSON ? M_PEARSON : M_PBASE, T, a, stream);
}

int n2v_eccknn_pearson_sparse(const int64_t* xr_ptr, const int32_t* xr_y, const double* xr_r, int64_t n_x, int64_t n_y,
                              int64_t n, const double* w, int32_t kind, int32_t min_support, double global_mean,
                              const double* bx, const double* by, double shrinkage, double* sim, int32_t* freq,
                              double* prods, double* a1, double* a2, double* a3, double* a4, void* stream) {
    const char* who = "eccknn_pearson_sparse";
    const int64_t T = sparse_frame(who, "n_x", "n_y", n_x, n_y, n, xr_ptr, xr_y, xr_r, sim, [&] { return pearson_args(who, kind, bx, by); });
    if (T < 0) return (int)T;
    const SparseArgs a{xr_ptr, xr_y, xr_r, n_y, n, w, T,
                       pearson_out(kind, n_x, min_support, shrinkage, sim, freq, prods, a1, a2, a3, a4),
                       Baselines{bx, by, global_mean}};
    return launch_sim_sparse(who, kind == N2V_ECCKNN_PEARSON ? M_PEARSON : M_PBASE, a, stream);
}

int n2v_slopeone_dev(const double* dense, const uint8_t* mask, int64_t n_items, int64_t n_users, double* dev, int32_t* freq,
                     double* acc, void* stream) {
    const char* who = "slopeone_dev";
    const int64_t T = dense_frame(who, "n_items", "n_users", n_items, n_users, dense, mask, dev, true,
                                  [&] { return slope_args(who, n_items, dev, freq); });
    if (T < 0) return (int)T;
    const SimArgs a{dense, mask, n_users, nullptr, slope_out(n_items, dev, freq, acc), Baselines{nullptr, nullptr, 0.0}};
    return launch_sim(who, M_SLOPE, T, a, stream);
}

int n2v_slopeone_dev_sparse(const int64_t* xr_ptr, const int32_t* xr_y, const double* xr_r, int64_t n_items, int64_t n_users,
                            int64_t n, double* dev, int32_t* freq, double* acc, void* stream) {
    const char* who = "slopeone_dev_sparse";
    const int64_t T = sparse_frame(who, "n_items", "n_users", n_items, n_users, n, xr_ptr, xr_y, xr_r, dev,
                                   [&] { return slope_args(who, n_items, dev, freq); });
    if (T < 0) return (int)T;
    const SparseArgs a{xr_ptr, xr_y, xr_r, n_users, n, nullptr, T, slope_out(n_items, dev, freq, acc),
                       Baselines{nullptr, nullptr, 0.0}};
    return launch_sim_sparse(who, M_SLOPE, a, stream);
}

int n2v_eccknn_baselines(const int64_t* ur_ptr, const int32_t* ur_i, const double* ur_r, int64_t n_users,
                         const int64_t* ir_ptr, const int32_t* ir_u, const double* ir_r, int64_t n_items, double global_mean,
                         int32_t n_epochs, double reg_u, double reg_i, double* bu, double* bi, void* stream) {
    if (n_users < 1 || n_items < 1 || n_users > 0x7fffffff || n_items > 0x7fffffff)
        return n2v::fail(N2V_ERR_INVALID, "eccknn_baselines: n_users=%lld n_items=%lld outside [1, 2^31)", (long long)n_users, (long long)n_items);
    if (n_epochs < 0) return n2v::fail(N2V_ERR_INVALID, "eccknn_baselines: n_epochs %d < 0", n_epochs);
    if (!(reg_u >= 0)) return n2v::fail(N2V_ERR_INVALID, "eccknn_baselines: reg_u %g < 0", reg_u);
    if (!(reg_i >= 0)) return n2v::fail(N2V_ERR_INVALID, "eccknn_baselines: reg_i %g < 0", reg_i);
    if (!ur_ptr || !ur_i || !ur_r || !ir_ptr || !ir_u || !ir_r || !bu || !bi) return n2v::fail(N2V_ERR_INVALID, "eccknn_baselines: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(bu, 0, (size_t)n_users * sizeof(double), s) != hipSuccess ||
        hipMemsetAsync(bi, 0, (size_t)n_items * sizeof(double), s) != hipSuccess)
        return n2v::fail(N2V_ERR_HIP, "eccknn_baselines: memset failed");
    for (int32_t e = 0; e < n_epochs; ++e) {                      // every item from bu, then every user from the new bi
        baselines_kernel<<<(unsigned)n_items, 64, 0, s>>>(ir_ptr, ir_u, ir_r, n_items, n_users, global_mean, reg_i, bu, bi);
        baselines_kernel<<<(unsigned)n_users, 64, 0, s>>>(ur_ptr, ur_i, ur_r, n_users, n_items, global_mean, reg_u, bi, bu);
    }
    return n2v::check_launch("eccknn_baselines");
}

int n2v_eccknn_estimate(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x, const double* yr_r,
                        int64_t n_y, const int32_t* qx, const int32_t* qy, int64_t n_q, int32_t k, int32_t min_k,
                        double* est, int32_t* actual_k, uint8_t* impossible, void* stream) {
    return estimate_call("eccknn_estimate", KnnModel{sim, n_x, yr_ptr, yr_x, yr_r, n_y, k, min_k}, qx, qy, n_q, nullptr, est,
                         actual_k, impossible, stream);
}

int n2v_eccknn_estimate_centered(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x, const double* yr_r,
                                 int64_t n_y, const int32_t* qx, const int32_t* qy, int64_t n_q, int32_t k, int32_t min_k,
                                 int32_t centering, int32_t user_based, double global_mean, const double* tx, const double* sd,
                                 const double* by, double* est, int32_t* actual_k, uint8_t* impossible, void* stream) {
    const Centred c{centering, Centering{global_mean, user_based ? 1 : 0, tx, sd, by}};
    return estimate_call("eccknn_estimate_centered", KnnModel{sim, n_x, yr_ptr, yr_x, yr_r, n_y, k, min_k}, qx, qy, n_q, &c,
                         est, actual_k, impossible, stream);
}

int n2v_eccknn_estimate_sweep(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x, const double* yr_r,
                              int64_t n_y, const int32_t* qx, const int32_t* qy, int64_t n_q, const int32_t* ks, int32_t n_k,
                              const int32_t* min_ks, int32_t n_m, double* est, int32_t* actual_k, uint8_t* impossible,
                              void* stream) {
    return sweep_call("eccknn_estimate_sweep", KnnModel{sim, n_x, yr_ptr, yr_x, yr_r, n_y, 0, 0}, qx, qy, n_q, ks, n_k, min_ks,
                      n_m, nullptr, est, actual_k, impossible, stream);
}

int n2v_eccknn_estimate_sweep_centered(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x,
                                       const double* yr_r, int64_t n_y, const int32_t* qx, const int32_t* qy, int64_t n_q,
                                       const int32_t* ks, int32_t n_k, const int32_t* min_ks, int32_t n_m, int32_t centering,
                                       int32_t user_based, double global_mean, const double* tx, const double* sd,
                                       const double* by, double* est, int32_t* actual_k, uint8_t* impossible, void* stream) {
    const Centred c{centering, Centering{global_mean, user_based ? 1 : 0, tx, sd, by}};
    return sweep_call("eccknn_estimate_sweep_centered", KnnModel{sim, n_x, yr_ptr, yr_x, yr_r, n_y, 0, 0}, qx, qy, n_q, ks, n_k,
                      min_ks, n_m, &c, est, actual_k, impossible, stream);
}

int n2v_eccknn_row_moments(const int64_t* ptr, const double* r, int64_t n_rows, int64_t n, double zero_sigma, double* mu,
                           double* sd, void* stream) {
    if (n_rows < 1 || n_rows > 0x7fffffff || n < 0)
        return n2v::fail(N2V_ERR_INVALID, "eccknn_row_moments: n_rows=%lld outside [1, 2^31) or n=%lld < 0", (long long)n_rows, (long long)n);
    if (!ptr || !mu || !sd || (n > 0 && !r)) return n2v::fail(N2V_ERR_INVALID, "eccknn_row_moments: null pointer");
    row_moments_kernel<<<(unsigned)n_rows, 64, 0, (hipStream_t)stream>>>(ptr, r, n, zero_sigma, mu, sd);
    return n2v::check_launch("eccknn_row_moments");
}

int32_t n2v_topn_segments(int64_t n_owners, int64_t n_candidates) {
    if (n_owners < 1 || n_candidates < 1) return 1;
    int64_t s = (65536 + n_owners - 1) / n_owners;               // 256 one-wavefront workgroups per compute unit: the
                                                                  // candidates' costs differ widely, short segments even them out
    if (s > n_candidates) s = n_candidates;
    if (s > n2v::TOPN_MAX_SEG) s = n2v::TOPN_MAX_SEG;
    return (int32_t)(s < 1 ? 1 : s);
}

int n2v_eccknn_topn(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x, const double* yr_r,
                    int64_t n_y, int32_t user_based, const int64_t* seen_ptr, const int32_t* seen_i, int64_t n_seen,
                    const int32_t* owners, int64_t n_owners, int32_t k, int32_t min_k, double global_mean, double lo,
                    double hi, int32_t top_n, int32_t segments, double* part_score, int32_t* part_pos, int32_t* items,
                    double* score, void* stream) {
    return topn_call("eccknn_topn", "eccknn_topn (merge)", KnnModel{sim, n_x, yr_ptr, yr_x, yr_r, n_y, k, min_k}, user_based,
                     seen_ptr, seen_i, n_seen, owners, n_owners, global_mean, lo, hi, top_n, segments, nullptr,
                     part_score, part_pos, items, score, stream);
}

int n2v_eccknn_topn_centered(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x, const double* yr_r,
                             int64_t n_y, int32_t user_based, const int64_t* seen_ptr, const int32_t* seen_i, int64_t n_seen,
                             const int32_t* owners, int64_t n_owners, int32_t k, int32_t min_k, double global_mean, double lo,
                             double hi, int32_t top_n, int32_t segments, int32_t centering, const double* tx, const double* sd,
                             const double* by, double* part_score, int32_t* part_pos, int32_t* items, double* score,
                             void* stream) {
    const Centred c{centering, Centering{global_mean, user_based ? 1 : 0, tx, sd, by}};
    return topn_call("eccknn_topn_centered", "eccknn_topn_centered (merge)", KnnModel{sim, n_x, yr_ptr, yr_x, yr_r, n_y, k, min_k},
                     user_based, seen_ptr, seen_i, n_seen, owners, n_owners, global_mean, lo, hi, top_n, segments, &c,
                     part_score, part_pos, items, score, stream);
}

int n2v_eccknn_predict(const double* est, const uint8_t* impossible, const double* r_true, int64_t n_q, double global_mean,
                       double lo, double hi, double* pred, double* rmse, void* stream) {
    if (n_q < 1) return n2v::fail(N2V_ERR_INVALID, "eccknn_predict: n_q %lld < 1", (long long)n_q);
    if (!est || !impossible || !pred || (r_true && !rmse)) return n2v::fail(N2V_ERR_INVALID, "eccknn_predict: null pointer");
    predict_kernel<<<1, 256, 0, (hipStream_t)stream>>>(est, impossible, r_true, n_q, global_mean, lo, hi, pred, rmse);
    return n2v::check_launch("eccknn_predict");
}

int n2v_eccknn_errors(const double* pred, const double* r_true, int64_t n_q, int64_t n_cols, double* rmse, double* mae,
                      void* stream) {
    if (n_q < 1 || n_cols < 1 || n_cols > 0x7fffffff)
        return n2v::fail(N2V_ERR_INVALID, "eccknn_errors: n_q %lld < 1 or n_cols %lld outside [1, 2^31)", (long long)n_q, (long long)n_cols);
    if (!pred || !r_true || (!rmse && !mae)) return n2v::fail(N2V_ERR_INVALID, "eccknn_errors: null pointer");
    errors_kernel<<<(unsigned)n_cols, 256, 0, (hipStream_t)stream>>>(pred, r_true, n_q, rmse, mae);
    return n2v::check_launch("eccknn_errors");
}

}  // extern "C"
