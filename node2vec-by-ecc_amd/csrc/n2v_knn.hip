// Fused k nearest neighbours of prepared rows — gfx950 (MI355X).  C-ABI: include/n2v_sim.h (n2v_sim_knn*).
//
// gensim's most_similar and the reference's find_similar_users (src/utils.py:428-442) rank every row of a matrix against a
// query by cosine.  Through n2v_sim_block + n2v_sim_rows_topk that stores n_q x n_cols scores to keep n_q x k of them; here
// nothing of that size exists:
//   knn_tile_kernel   128 query rows x a segment of 128-column tiles per workgroup.  A tile's scores are formed by
//                     sim_mfma_tile (n2v_sim_tile.h), the function sim_mfma_kernel runs, so a pair has the bits
//                     n2v_sim_block writes for it.  Each wavefront then passes its 64x64 quarter through LDS in two
//                     32-row blocks and folds every row into that row's running best-k list, one lane per column: one
//                     ballot against the list's last entry, and only the columns that beat it are inserted.
//   knn_merge_kernel  one wavefront per query merges the partial lists into the final one.
// The two column halves of a tile belong to different wavefronts, so a (segment, half) pair owns a list: 2 * n_seg partial
// lists a query, in caller-owned scratch.  Columns are ranked by the one total order of n2v_rank.h on (score, column); every
// comparison in this file is its beats(), so neither the segment count nor a tile border can change a result.
#include "n2v_common.h"
#include "n2v_sim.h"
#include "n2v_rank.h"
#include "n2v_sim_tile.h"

namespace {

using n2v::POS_NONE, n2v::order_key, n2v::beats, n2v::list_insert, n2v::floatx16;
constexpr int MT = n2v::SIM_MT;
constexpr int SB = 32;             // rows of one accumulator block = rows of a wavefront's LDS score block
constexpr int MAX_SEG = 32;        // 2 * MAX_SEG partial lists: one lane each in the merge
constexpr int KC = 32;             // dpad granule of n2v_sim_prepare

struct KnnArgs {
    const float* Q; int64_t n_q;
    const float* B; int64_t n_cols;
    int dpad;
    const int32_t* exclude;
    int k; int S;
    float* part_score; int32_t* part_pos;
};

__global__ void __launch_bounds__(256) knn_tile_kernel(KnnArgs a) {
    __shared__ __attribute__((aligned(16))) float As[n2v::SIM_MKC][n2v::SIM_MLD];
    __shared__ __attribute__((aligned(16))) float Bs[n2v::SIM_MKC][n2v::SIM_MLD];
    __shared__ float Sc[4][SB][64];            // per wavefront: 32 rows x its 64 columns; stores and loads are both row-contiguous
    __shared__ uint32_t thr_key[4][64];        // per wavefront: the last entry of each of its 64 rows' lists
    __shared__ int thr_pos[4][64];
    __shared__ int excl[MT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int64_t r0 = (int64_t)blockIdx.x * MT;
    const int seg = blockIdx.y, L = 2 * a.S, list = 2 * seg + wc, k = a.k;
    const int64_t n_tiles = (a.n_cols + MT - 1) / MT;
    const int64_t t0 = n_tiles * seg / a.S, t1 = n_tiles * (seg + 1) / a.S;

    for (int r = tid; r < MT; r += 256) {
        const int64_t q = r0 + r;
        excl[r] = (a.exclude && q < a.n_q) ? a.exclude[q] : -1;
    }
    thr_key[wave][lane] = 0u;
    thr_pos[wave][lane] = POS_NONE;
    // every list starts as k entries (NaN, POS_NONE): below any real entry, so a list is always "full"
    for (int rr = 0; rr < 64; ++rr) {
        const int64_t q = r0 + wr * 64 + rr;
        if (q >= a.n_q) break;
        const int64_t base = (q * L + list) * k;
        for (int i = lane; i < k; i += 64) { a.part_score[base + i] = __builtin_nanf(""); a.part_pos[base + i] = POS_NONE; }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();

    const int lrow = tid >> 1, kq = (tid & 1) * 8;
    const int64_t ar = r0 + lrow;
    const float* ap = a.Q + ar * a.dpad + kq;
    const bool a_ok = ar < a.n_q;
    const int kh = lane >> 5, m = lane & 31;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t c0 = t * MT, br = c0 + lrow;
        floatx16 acc[2][2];
        n2v::sim_mfma_tile(ap, a.B + br * a.dpad + kq, a_ok, br < a.n_cols, a.dpad, As, Bs, acc, wr, wc, lrow, kq, kh, m);

        // ---- selection: this wavefront's 64 rows x 64 columns, one lane per column
        const int64_t pc = c0 + wc * 64 + lane;
        const bool col_ok = pc < a.n_cols;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int v = 0; v < 16; ++v) Sc[wave][8 * (v >> 2) + 4 * kh + (v & 3)][bj * 32 + m] = acc[bi][bj][v];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
            for (int r = 0; r < SB; ++r) {
                const int wrow = bi * SB + r, lr = wr * 64 + wrow;
                const int64_t q = r0 + lr;
                if (q >= a.n_q) break;
                const float s = Sc[wave][r][lane];
                uint32_t tk = thr_key[wave][wrow];
                int tp = thr_pos[wave][wrow];
                unsigned long long cand = __ballot(col_ok && (int)pc != excl[lr] && beats(order_key(s), (int)pc, tk, tp));
                if (cand == 0ull) continue;
                const int64_t base = (q * L + list) * k;
                while (cand) {
                    const int src = __builtin_ctzll(cand);
                    cand &= cand - 1ull;
                    const float cs = __shfl(s, src, 64);
                    const int cp = (int)(c0 + wc * 64 + src);
                    const uint32_t ck = order_key(cs);
                    if (beats(ck, cp, tk, tp)) list_insert(a.part_score + base, a.part_pos + base, k, cs, cp, ck, lane, tk, tp);
                }
                if (lane == 0) { thr_key[wave][wrow] = tk; thr_pos[wave][wrow] = tp; }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// One wavefront per query, lane l holds the head of partial list l; k times the best head leaves.  An entry that was never
// filled leaves as (-1, NaN).
__global__ void __launch_bounds__(256)
knn_merge_kernel(const float* __restrict__ part_score, const int32_t* __restrict__ part_pos, int64_t n_q, int L, int k,
                 int32_t* __restrict__ cols, float* __restrict__ vals) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_q) return;
    const int64_t base = (q * L + lane) * k;
    int h = 0;
    float s = __builtin_nanf("");
    int p = POS_NONE;
    if (lane < L) { s = part_score[base]; p = part_pos[base]; }
    for (int i = 0; i < k; ++i) {
        uint32_t bk = order_key(s);
        int bp = p, bl = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t ok = __shfl_xor(bk, o, 64);
            const int op = __shfl_xor(bp, o, 64), ol = __shfl_xor(bl, o, 64);
            if (beats(ok, op, bk, bp)) { bk = ok; bp = op; bl = ol; }
        }
        bl = __shfl(bl, 0, 64);
        const float ws = __shfl(s, bl, 64);
        const int wp = __shfl(p, bl, 64);
        if (lane == 0) { cols[q * k + i] = wp == POS_NONE ? -1 : wp; vals[q * k + i] = wp == POS_NONE ? __builtin_nanf("") : ws; }
        if (lane == bl) {
            ++h;
            s = __builtin_nanf(""); p = POS_NONE;
            if (h < k) { s = part_score[base + h]; p = part_pos[base + h]; }
        }
    }
}

// CUs of the device that is current at the call (MI355X: 256); 256 where no device answers.  Asked every time, so
// n2v_sim_knn_scratch and n2v_sim_knn agree as long as the caller keeps one device current across the two.
int64_t cu_count() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        n > 0)
        return n;
    return 256;
}

// 0 = auto: about three workgroups per compute unit, whatever n_cols is (a segment without tiles is legal)
int resolve_seg(int64_t n_q, int32_t n_seg) {
    if (n_seg > 0) return n_seg;
    const int64_t row_blocks = n_q > 0 ? (n_q + MT - 1) / MT : 1;
    int64_t s = (3 * cu_count() + row_blocks - 1) / row_blocks;
    if (s > MAX_SEG) s = MAX_SEG;
    return (int)(s < 1 ? 1 : s);
}

}  // namespace

// ================================================================================================== C-ABI
extern "C" int32_t n2v_sim_knn_max_k(void) { return N2V_SIM_KNN_MAX_K; }
extern "C" int32_t n2v_sim_knn_max_seg(void) { return MAX_SEG; }

extern "C" int64_t n2v_sim_knn_scratch(int64_t n_q, int32_t k, int32_t n_seg) {
    if (n_q < 0 || k < 1 || k > N2V_SIM_KNN_MAX_K || n_seg < 0 || n_seg > MAX_SEG) return -1;
    return n_q * 2 * resolve_seg(n_q, n_seg) * (int64_t)k * (int64_t)(sizeof(float) + sizeof(int32_t));
}

extern "C" int n2v_sim_knn(const float* Q, int64_t n_q, const float* B, int64_t n_cols, int32_t dpad, int32_t method,
                           const int32_t* exclude, int32_t k, int32_t n_seg, void* scratch, int32_t* cols, float* vals,
                           void* stream) {
    if (method != N2V_SIM_COS && method != N2V_SIM_PEARSON)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sim_knn: method %d is not a dot product (cos, pearson)", (int)method);
    if (n_q < 0 || n_cols < 0 || dpad < KC || (dpad % KC) != 0) return n2v::fail(N2V_ERR_INVALID, "n2v_sim_knn: bad sizes");
    if (k < 1 || k > N2V_SIM_KNN_MAX_K)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sim_knn: k %d outside [1, %d]", (int)k, N2V_SIM_KNN_MAX_K);
    if (n_seg < 0 || n_seg > MAX_SEG) return n2v::fail(N2V_ERR_INVALID, "n2v_sim_knn: n_seg %d outside [0, %d]", (int)n_seg, MAX_SEG);
    if (n_cols > (int64_t)POS_NONE) return n2v::fail(N2V_ERR_INVALID, "n2v_sim_knn: too many columns");
    if ((n_q + MT - 1) / MT > (int64_t)0x7fffffff) return n2v::fail(N2V_ERR_INVALID, "n2v_sim_knn: too many queries in one call");
    if ((((uintptr_t)Q | (uintptr_t)B) & 15) != 0) return n2v::fail(N2V_ERR_INVALID, "n2v_sim_knn: operands not 16-byte aligned");
    if (n_q == 0) return N2V_OK;
    if (n_cols > 0 && (!Q || !B)) return n2v::fail(N2V_ERR_INVALID, "n2v_sim_knn: null pointer");
    if (!scratch || !cols || !vals) return n2v::fail(N2V_ERR_INVALID, "n2v_sim_knn: null pointer");
    if ((uintptr_t)scratch & 3) return n2v::fail(N2V_ERR_INVALID, "n2v_sim_knn: scratch not 4-byte aligned");
    KnnArgs a{};
    a.Q = Q; a.n_q = n_q; a.B = B; a.n_cols = n_cols; a.dpad = dpad; a.exclude = exclude; a.k = k;
    a.S = resolve_seg(n_q, n_seg);
    const int64_t entries = n_q * 2 * a.S * (int64_t)k;
    a.part_score = (float*)scratch;
    a.part_pos = (int32_t*)scratch + entries;
    const dim3 grid((unsigned)((n_q + MT - 1) / MT), (unsigned)a.S);
    hipLaunchKernelGGL(knn_tile_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    const int rc = n2v::check_launch("n2v_sim_knn");
    if (rc != N2V_OK) return rc;
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((n_q + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a.part_score,
                       a.part_pos, n_q, 2 * a.S, (int)k, cols, vals);
    return n2v::check_launch("n2v_sim_knn (merge)");
}
