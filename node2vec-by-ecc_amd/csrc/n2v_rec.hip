// Top-N recommendation of the BiNE path — gfx950 (MI355X).  C-ABI: include/n2v_bine.h.
//
// Reference: src/bine_train.py:311-359 (top_N: score every (test user, test item) pair by U.V, 0 for a vertex the
// model does not know, keep the top_n items per user) and :361-406 (precision / recall / AP / RR / nDCG per user).
// The reference fills a dict of dicts and sorts each; here nothing of size users x items is stored:
//   rec_topn_kernel   128 user rows x a segment of 64-item tiles per workgroup; the fp64 scores of a tile are formed on
//                     the matrix cores (v_mfma_f64_16x16x4_f64, operands staged through LDS in k-chunks of 16) and each
//                     wavefront folds the 32 rows it owns into their running best-k lists before the next tile;
//   rec_merge_kernel  one wavefront per user merges the S segment lists into the final one;
//   rec_metrics_kernel one lane per user, the five numbers of :361-406.
// Items are ranked by the one total order of n2v_rank.h on (score, item position in the caller's list); every
// comparison in this file is its beats().
#include "n2v_common.h"
#include "n2v_bine.h"
#include "n2v_rank.h"

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int RB = 2;            // 16-row MFMA blocks per wavefront
constexpr int BM = 64 * RB;      // user rows per workgroup (4 wavefronts x 16 RB)
constexpr int BN = 64;           // items per tile = one lane each in the selection
constexpr int CB = BN / 16;      // 16-column MFMA blocks per tile
constexpr int KC = 16;           // k-chunk staged per barrier
constexpr int LP = KC + 1;       // LDS pitch of a staged row (doubles): the 4 k-groups of an operand read spread over the banks
constexpr int SP = BN + 16;      // LDS pitch of a score row: the 4 rows one accumulator register writes land 32 banks apart
constexpr int MAX_SEG = 64;      // segments per user: one lane each in the merge

using n2v::POS_NONE, n2v::order_key, n2v::beats, n2v::list_insert, n2v::merge_lists;   // n2v_rank.h

struct RecArgs {
    const double* emb; int64_t n_rows; int dim; int stride;
    const int32_t* u_idx; int64_t n_users;
    const int32_t* v_idx; int64_t n_items;
    int k; int S;
    double* part_score; int32_t* part_pos;
};

__global__ void __launch_bounds__(256) rec_topn_kernel(RecArgs a) {
    __shared__ double As[BM][LP];
    __shared__ double Bs[BN][LP];
    __shared__ double Sc[4][16][SP];
    __shared__ uint64_t thr_key[BM];
    __shared__ int thr_pos[BM];
    __shared__ int arow[BM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * BM;
    const int seg = blockIdx.y;
    const int64_t n_tiles = (a.n_items + BN - 1) / BN;
    const int64_t t0 = n_tiles * seg / a.S, t1 = n_tiles * (seg + 1) / a.S;
    const int k = a.k;

    for (int r = tid; r < BM; r += 256) {
        const int64_t u = r0 + r;
        int idx = u < a.n_users ? a.u_idx[u] : -1;
        if (idx < 0 || idx >= a.n_rows) idx = -1;
        arow[r] = idx;
        thr_key[r] = 0ull;
        thr_pos[r] = POS_NONE;
    }
    // every list starts as k entries (NaN, POS_NONE): below any real entry, so a list is always "full"
    for (int rr = 0; rr < 16 * RB; ++rr) {
        const int64_t u = r0 + wave * 16 * RB + rr;
        if (u >= a.n_users) break;
        const int64_t base = (u * a.S + seg) * k;
        for (int i = lane; i < k; i += 64) { a.part_score[base + i] = __builtin_nan(""); a.part_pos[base + i] = POS_NONE; }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();

    // staging map: element e = tid + 256 j of a chunk is (row e / 16, k e % 16)
    const int sk = tid & 15, srow = tid >> 4;
    const double* ap[4 * RB];
#pragma unroll
    for (int j = 0; j < 4 * RB; ++j) {
        const int idx = arow[srow + 16 * j];
        ap[j] = idx < 0 ? nullptr : a.emb + (int64_t)idx * a.stride + sk;
    }
    const int kg = lane >> 4, m16 = lane & 15;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t c0 = t * BN;
        const double* bp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t c = c0 + srow + 16 * j;
            int idx = c < a.n_items ? a.v_idx[c] : -1;
            if (idx < 0 || idx >= a.n_rows) idx = -1;
            bp[j] = idx < 0 ? nullptr : a.emb + (int64_t)idx * a.stride + sk;
        }
        doublex4 acc[RB][CB];
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < CB; ++j) acc[i][j] = doublex4{0.0, 0.0, 0.0, 0.0};
        double av[4 * RB], bv[4];
        {
            const bool kin = sk < a.dim;        // columns [dim, stride) are never read
#pragma unroll
            for (int j = 0; j < 4 * RB; ++j) av[j] = (ap[j] && kin) ? ap[j][0] : 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = (bp[j] && kin) ? bp[j][0] : 0.0;
        }
        for (int k0 = 0; k0 < a.dim; k0 += KC) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4 * RB; ++j) As[srow + 16 * j][sk] = av[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) Bs[srow + 16 * j][sk] = bv[j];
            __syncthreads();
            if (k0 + KC < a.dim) {              // the next chunk travels while this one is multiplied
                const int kn = k0 + KC;
                const bool kin = kn + sk < a.dim;
#pragma unroll
                for (int j = 0; j < 4 * RB; ++j) av[j] = (ap[j] && kin) ? ap[j][kn] : 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = (bp[j] && kin) ? bp[j][kn] : 0.0;
            }
            // operand map of the instruction: lane l supplies A[row l % 16][k l / 16] and B[k l / 16][col l % 16]
#pragma unroll
            for (int kk = 0; kk < KC; kk += 4) {
                double fa[RB], fb[CB];
#pragma unroll
                for (int i = 0; i < RB; ++i) fa[i] = As[wave * 16 * RB + i * 16 + m16][kk + kg];
#pragma unroll
                for (int j = 0; j < CB; ++j) fb[j] = Bs[j * 16 + m16][kk + kg];
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int j = 0; j < CB; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
        }

        // ---- selection: this wavefront's 16 RB rows x the tile's 64 items, one lane per item
        const int64_t pc = c0 + lane;
        int vi = -2;                                            // -2: past the end of the item list
        if (pc < a.n_items) { vi = a.v_idx[pc]; if (vi < 0 || vi >= a.n_rows) vi = -1; }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            // result map of the f64 instruction: register v of lane l holds D[row l / 16 + 4 v][col l % 16]
#pragma unroll
            for (int j = 0; j < CB; ++j)
#pragma unroll
                for (int v = 0; v < 4; ++v) Sc[wave][kg + 4 * v][j * 16 + m16] = acc[rb][j][v];
            __builtin_amdgcn_wave_barrier();
            for (int r = 0; r < 16; ++r) {
                const int lr = wave * 16 * RB + rb * 16 + r;
                const int64_t u = r0 + lr;
                if (u >= a.n_users) break;
                double s = Sc[wave][r][lane];
                if (arow[lr] < 0 || vi < 0) s = 0.0;            // an unknown end scores exactly 0 (pre = 0, :316-322)
                uint64_t tk = thr_key[lr];
                int tp = thr_pos[lr];
                unsigned long long cand = __ballot(vi != -2 && beats(order_key(s), (int)pc, tk, tp));
                if (cand == 0ull) continue;
                const int64_t base = (u * a.S + seg) * k;
                while (cand) {
                    const int src = __builtin_ctzll(cand);
                    cand &= cand - 1ull;
                    const double cs = __shfl(s, src, 64);
                    const int cp = (int)(c0 + src);
                    const uint64_t ck = order_key(cs);
                    if (beats(ck, cp, tk, tp)) list_insert(a.part_score + base, a.part_pos + base, k, cs, cp, ck, lane, tk, tp);
                }
                if (lane == 0) { thr_key[lr] = tk; thr_pos[lr] = tp; }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// One wavefront per user merges the user's S segment lists (merge_lists, n2v_rank.h).
__global__ void __launch_bounds__(256)
rec_merge_kernel(const double* __restrict__ part_score, const int32_t* __restrict__ part_pos, int64_t n_users, int S, int k,
                 int32_t* __restrict__ ranked, double* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_users) return;
    merge_lists(part_score + u * S * k, part_pos + u * S * k, S, k, lane, ranked + u * k, score + u * k, POS_NONE);
}

// precision_and_racall, AP, RR, nDCG (src/bine_train.py:361-406) of one user: additions in index order and divisions only.
__global__ void __launch_bounds__(256)
rec_metrics_kernel(const int32_t* __restrict__ ranked, int64_t n_users, int k, const int64_t* __restrict__ truth_ptr,
                   const int32_t* __restrict__ truth_pos, const int32_t* __restrict__ truth_len,
                   const double* __restrict__ discount, const double* __restrict__ idcg, double* __restrict__ out) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_users) return;
    const int64_t tb = truth_ptr[u], te = truth_ptr[u + 1];
    const int32_t* rk = ranked + u * k;
    int hits = 0;
    double sum_precs = 0.0, rr = 0.0, dcg = 0.0;
    for (int i = 0; i < k; ++i) {
        const int item = rk[i];
        int64_t lo = tb, hi = te;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (truth_pos[mid] < item) lo = mid + 1; else hi = mid;
        }
        if (lo >= te || truth_pos[lo] != item) continue;
        ++hits;
        sum_precs += (double)hits / ((double)i + 1.0);
        if (hits == 1) rr = 1.0 / ((double)i + 1.0);
        dcg += discount[i];
    }
    const double glen = (double)truth_len[u];
    double* o = out + u * 5;
    o[0] = (double)hits / (1.0 * (double)k);
    o[1] = (double)hits / (1.0 * glen);
    o[2] = hits > 0 ? sum_precs / glen : 0.0;
    o[3] = rr;
    o[4] = dcg / idcg[u];
}

}  // namespace

// ================================================================================================== C-ABI
extern "C" int32_t n2v_bine_rec_segments(int64_t n_users, int64_t n_items) {
    if (n_users < 1 || n_items < 1) return 1;
    const int64_t row_blocks = (n_users + BM - 1) / BM, tiles = (n_items + BN - 1) / BN;
    int64_t s = (1024 + row_blocks - 1) / row_blocks;           // about four workgroups per compute unit
    if (s > tiles) s = tiles;
    if (s > MAX_SEG) s = MAX_SEG;
    return (int32_t)(s < 1 ? 1 : s);
}

extern "C" int n2v_bine_rec_topn(const double* emb, int64_t n_rows, int32_t dim, int32_t stride, const int32_t* u_idx,
                                 int64_t n_users, const int32_t* v_idx, int64_t n_items, int32_t top_n, int32_t segments,
                                 double* part_score, int32_t* part_pos, int32_t* ranked, double* score, void* stream) {
    if (n_users < 1 || n_items < 1)
        return n2v::fail(N2V_ERR_INVALID, "n2v_bine_rec_topn: %lld users x %lld items: nothing to rank", (long long)n_users,
                         (long long)n_items);
    if (top_n < 1 || top_n > N2V_REC_MAX_TOPN)
        return n2v::fail(N2V_ERR_INVALID, "n2v_bine_rec_topn: top_n %d outside [1, %d]", (int)top_n, N2V_REC_MAX_TOPN);
    if (segments < 0 || segments > MAX_SEG)
        return n2v::fail(N2V_ERR_INVALID, "n2v_bine_rec_topn: segments %d outside [0, %d]", (int)segments, MAX_SEG);
    if (n_rows < 1 || dim < 1 || stride < dim)
        return n2v::fail(N2V_ERR_INVALID, "n2v_bine_rec_topn: bad table (rows %lld dim %d stride %d)", (long long)n_rows, (int)dim,
                         (int)stride);
    if (n_items >= (int64_t)POS_NONE || n_users > (int64_t)0x7fffffff)
        return n2v::fail(N2V_ERR_INVALID, "n2v_bine_rec_topn: too many users or items");
    if (!emb || !u_idx || !v_idx || !part_score || !part_pos || !ranked || !score)
        return n2v::fail(N2V_ERR_INVALID, "n2v_bine_rec_topn: null pointer");
    const int S = segments > 0 ? segments : n2v_bine_rec_segments(n_users, n_items);
    const int k = (int)(n_items < top_n ? n_items : top_n);
    RecArgs a{};
    a.emb = emb; a.n_rows = n_rows; a.dim = dim; a.stride = stride;
    a.u_idx = u_idx; a.n_users = n_users; a.v_idx = v_idx; a.n_items = n_items;
    a.k = k; a.S = S; a.part_score = part_score; a.part_pos = part_pos;
    const dim3 grid((unsigned)((n_users + BM - 1) / BM), (unsigned)S);
    hipLaunchKernelGGL(rec_topn_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    int rc = n2v::check_launch("n2v_bine_rec_topn");
    if (rc != N2V_OK) return rc;
    hipLaunchKernelGGL(rec_merge_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, (hipStream_t)stream, part_score,
                       part_pos, n_users, S, k, ranked, score);
    return n2v::check_launch("n2v_bine_rec_topn (merge)");
}

extern "C" int n2v_bine_rec_metrics(const int32_t* ranked, int64_t n_users, int32_t k, const int64_t* truth_ptr,
                                    const int32_t* truth_pos, const int32_t* truth_len, const double* discount,
                                    const double* idcg, double* out, void* stream) {
    if (n_users < 1 || k < 1) return n2v::fail(N2V_ERR_INVALID, "n2v_bine_rec_metrics: %lld users, k %d", (long long)n_users, (int)k);
    if (!ranked || !truth_ptr || !truth_len || !discount || !idcg || !out)
        return n2v::fail(N2V_ERR_INVALID, "n2v_bine_rec_metrics: null pointer");
    hipLaunchKernelGGL(rec_metrics_kernel, dim3(n2v::grid_for(n_users, 256)), dim3(256), 0, (hipStream_t)stream, ranked, n_users,
                       (int)k, truth_ptr, truth_pos, truth_len, discount, idcg, out);
    return n2v::check_launch("n2v_bine_rec_metrics");
}
