/* n2v_sim.h — C-ABI of the all-pairs similarity + selection kernels (gfx950), SURVEY.md 8(f-1) and 8(f-3).
 *
 * Replaces, in the reference (paths relative to its root):
 *   src/main_link.py:62-170   precision_at_k / make_links_and_score / links_score / link_prediction:
 *                             score every (user, item) — or every unordered node — pair that is not a
 *                             training edge, keep the k best for k in {1,10,50,100,500,1000}
 *   src/main_link.py:351-453  js / get_similarity / build_user_sim_matrx / get_add_edge_by_*:
 *                             N_user x N_user similarity ("cos", "pearson", "jsd") and a per-user
 *                             threshold or top-int(N*ratio) selection
 * Both are O(N^2 d) Python loops over gensim's `similarity` there.  Here a 64x64-tile kernel forms the
 * scores of a row block against all columns (fp32 FMA over rows prepared so that the similarity is a dot
 * product; the Jensen-Shannon form evaluates the reference's rel_entr sum per element) and either
 *   (a) streams candidates above a running threshold into a small buffer (global top-k; nothing of size
 *       N^2 is stored, training edges are dropped by a binary search of their sorted keys — only for the
 *       few candidates that pass the threshold), or
 *   (b) writes the row block [rows x n_cols] once, from which one workgroup per row selects by threshold
 *       (count + ordered fill) or by exact radix select of the k-th largest score (ordered fill), in list
 *       order — the order the reference's per-user loops emit.
 * Conventions as in n2v_hip.h: device pointers, caller-owned memory, asynchronous on `stream`,
 * int return codes + n2v_last_error().
 */
#ifndef N2V_SIM_H
#define N2V_SIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define N2V_SIM_COS 0      /* emb.similarity: dot of unit vectors            (src/main_link.py:359-360) */
#define N2V_SIM_PEARSON 1  /* scipy pearsonr(x, y)[0]: dot of centred units   (src/main_link.py:361-362) */
#define N2V_SIM_JSD 2      /* js(p, q): (KL(p|m) + KL(q|m)) / 2, p = x/sum(x) (src/main_link.py:351-356,363-364) */

/* Rows -> the form the tile kernel multiplies.  vec: fp32[n_src][stride]; rows (may be NULL = 0..n_rows-1):
 * int64[n_rows] gather index into vec; out: fp32[n_rows][dpad], dpad a multiple of 32 >= dim, padding 0.
 *   COS     x / sqrt(sum x^2)          (gensim matutils.unitvec)
 *   PEARSON (x - mean) / |x - mean|    (scipy.stats.pearsonr's own normalisation)
 *   JSD     x / sum(x)                 (the reference's p_norm; negative entries are kept — they make the
 *                                       reference's rel_entr infinite and so they do here)                  */
int n2v_sim_prepare(const float* vec, int32_t stride, int32_t dim, const int64_t* rows, int64_t n_rows,
                    int32_t method, float* out, int32_t dpad, void* stream);

/* Scores of rows [row_begin, row_begin + n_rows) of A against all n_cols rows of B (both prepared, row
 * length dpad): out[(r - row_begin) * ld + c].  method: N2V_SIM_JSD evaluates the rel_entr sum, anything
 * else the dot product.  zero_diag_off >= 0: the score of (r, c == r + zero_diag_off) is set to 0
 * (`user_user_sim_list[i] = 0`, src/main_link.py:386,404,421,438,451); < 0: off.                          */
int n2v_sim_block(const float* A, int64_t row_begin, int64_t n_rows, const float* B, int64_t n_cols,
                  int32_t dpad, int32_t method, int64_t zero_diag_off, float* out, int64_t ld, void* stream);

/* Global top-k scan (src/main_link.py:69-105): every score of rows [row_begin, row_end) x [0, n_cols) that
 * is > *tau (device float), whose pair is not in excl_keys (sorted int64 row * n_cols + col; NULL/0 = none)
 * and — if upper_triangle — has col > row (`for j in range(i+1, len(nodes))`, :72), is appended to the
 * candidate arrays at an index taken from *counter (int64, device; keeps counting past `capacity`, entries
 * beyond it are dropped — the caller raises tau and rescans).                                              */
int n2v_sim_topk_scan(const float* A, int64_t row_begin, int64_t row_end, const float* B, int64_t n_cols,
                      int32_t dpad, int32_t method, int32_t upper_triangle, const float* tau,
                      const int64_t* excl_keys, int64_t n_excl, float* cand_score, int32_t* cand_row,
                      int32_t* cand_col, int64_t capacity, int64_t* counter, void* stream);

/* Per-row selection from a score block (scores: fp32[n_rows][ld], n_cols valid columns), one workgroup per
 * row, results in COLUMN order inside a row:
 *   n2v_sim_rows_count: counts[r] = #{c : score > thre}                       (:396-424)
 *   n2v_sim_rows_fill : cols/vals at out_off[r] .. (out_off: int64[n_rows], exclusive prefix of counts)
 *   n2v_sim_rows_topk : the k largest of every row — all scores above the k-th largest value plus the first
 *                       ties of it in column order, i.e. exactly sorted(..., key=-score)[:k] as a SET
 *                       (:379-394,426-440); cols/vals: [n_rows][k].  NaN ranks lowest.  k <= n_cols.
 *                       -0.0 and +0.0 tie, as they do for Python's sort (column order decides between them);
 *                       a selected -0.0 is returned as -0.0.                                                */
int n2v_sim_rows_count(const float* scores, int64_t n_rows, int64_t n_cols, int64_t ld, float thre,
                       int64_t* counts, void* stream);
int n2v_sim_rows_fill(const float* scores, int64_t n_rows, int64_t n_cols, int64_t ld, float thre,
                      const int64_t* out_off, int32_t* cols, float* vals, void* stream);
int n2v_sim_rows_topk(const float* scores, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t k,
                      int32_t* cols, float* vals, void* stream);

/* ---- Fused k nearest neighbours (csrc/n2v_knn.hip): gensim's most_similar, src/utils.py:428-442 find_similar_users ----
 * Q: fp32[n_q][dpad], B: fp32[n_cols][dpad], both as n2v_sim_prepare writes them (16-byte aligned, dpad a multiple of 32).
 * method: N2V_SIM_COS or N2V_SIM_PEARSON (one kernel, the preparation differs); N2V_SIM_JSD is N2V_ERR_INVALID.  The scores
 * are always formed on the matrix cores, by the device function n2v_sim_block's MFMA kernel runs (N2V_SIM_VECTOR is
 * ignored): the score of (q, c) is bit for bit what n2v_sim_block writes for that pair.
 * The candidates of query q are the columns c < n_cols except c == exclude[q] (exclude: int32[n_q] or NULL; an entry < 0
 * or >= n_cols excludes nothing), ranked by csrc/n2v_rank.h: higher score first, equal scores by lower column, NaN below
 * everything, -0.0 ties +0.0.  cols[q][i] / vals[q][i], i < k, are the first k IN RANK ORDER; where fewer than k candidates
 * exist the rest is (-1, NaN).  n_seg splits the 128-column tiles into segments that run as separate workgroups (0: chosen
 * from the CU count of the device current at the call, the same for n2v_sim_knn_scratch and n2v_sim_knn; segments beyond
 * the number of tiles are empty and legal); a merge pass joins their partial lists.  THE
 * RESULT DOES NOT DEPEND ON n_seg.  Nothing of size n_q * n_cols is written: scratch holds 2 * n_seg lists of k entries a
 * query, n2v_sim_knn_scratch bytes for the n_seg the call will use, 4-byte aligned, and need not be initialised.
 * 1 <= k <= N2V_SIM_KNN_MAX_K, 0 <= n_seg <= n2v_sim_knn_max_seg(), n_q >= 0, 0 <= n_cols < 2^31 (n_cols == 0: every
 * entry is empty).  Bad arguments return N2V_ERR_INVALID before any launch (n2v_sim_knn_scratch: -1).                   */
#define N2V_SIM_KNN_MAX_K 256
int32_t n2v_sim_knn_max_k(void);
int32_t n2v_sim_knn_max_seg(void);
int64_t n2v_sim_knn_scratch(int64_t n_q, int32_t k, int32_t n_seg);
int n2v_sim_knn(const float* Q, int64_t n_q, const float* B, int64_t n_cols, int32_t dpad, int32_t method,
                const int32_t* exclude, int32_t k, int32_t n_seg, void* scratch, int32_t* cols, float* vals, void* stream);

/* ---- EccenKNN: eccentricity-weighted k-NN rating prediction (csrc/n2v_eccknn.hip) --------------------------------
 * Replaces src/main_rec.py:73-151 (cosine_eccen / msd_eccen, a triple Python loop over five dense n_x x n_x arrays)
 * and :305-329 (estimate).  x is the side similarities are formed over, y the other one; ids are inner ids (first
 * appearance in the training data).  Everything is fp64 and equals the reference's arithmetic bit for bit: every pair
 * (xi, xj) walks the y both rated in ascending order, and every += is one rounded multiply chain and one rounded add.
 * A NaN's sign and payload are not part of that contract (IEEE 754 leaves them to the implementation).             */
#define N2V_ECCKNN_COSINE 0   /* prods += (ri*rj)*w[y]; sqi += ri*ri; sqj += rj*rj;  sim = prods / sqrt(sqi*sqj)     */
#define N2V_ECCKNN_MSD 1      /* sq_diff += ((ri-rj)*w[y])^2;                        sim = 1 / (sq_diff/freq + 1)    */
#define N2V_ECCKNN_MAX_K 256  /* largest neighbourhood n2v_eccknn_estimate keeps                                     */
int32_t n2v_eccknn_max_k(void);
int64_t n2v_eccknn_max_dense(void); /* largest n_x * n_y (elements) the dense form accepts: 2^31; beyond it an error */

/* Ratings (x[i], y[i], r[i]), i < n, no duplicate (x, y) -> the y-major dense form the similarity kernel reads:
 * dense: fp64[n_y][n_x], mask: uint8[n_y][n_x] (1 = rated; 0.0 is a legal rating).  Both are cleared first.        */
int n2v_eccknn_densify(const int32_t* x, const int32_t* y, const double* r, int64_t n, int64_t n_x, int64_t n_y,
                       double* dense, uint8_t* mask, void* stream);

/* sim: fp64[n_x][n_x], symmetric, diagonal 1; 0 where freq < min_support; w: fp64[n_y].  freq (int32), prods, sqi,
 * sqj (cosine) and sq_diff (msd) are the reference's accumulators [n_x][n_x], the diagonal included; each may be
 * NULL.  One workgroup per 64x64 tile of the upper triangle, the mirror written from the same tile.               */
int n2v_eccknn_sim(const double* dense, const uint8_t* mask, int64_t n_x, int64_t n_y, const double* w, int32_t method,
                   int32_t min_support, double* sim, int32_t* freq, double* prods, double* sqi, double* sqj,
                   double* sq_diff, void* stream);

/* The sparse form of n2v_eccknn_sim: the same outputs, byte for byte, from the x-major CSR of the ratings instead of the
 * dense matrix, so nothing of size n_x * n_y exists and there is no bound on that product.  xr_ptr: int64[n_x + 1];
 * xr_y: int32[n], strictly ascending inside a row; xr_r: fp64[n]; row x is [xr_ptr[x], xr_ptr[x + 1]).  An empty row is
 * legal (freq 0, sim 0 off the diagonal); xr_y and xr_r may be NULL when n == 0.  One workgroup per 64x64 tile of the
 * upper triangle: the tile's rows pass through LDS in rounds of up to n2v_eccknn_sparse_chunk() entries a row, and every
 * pair merges the two staged segments in y order, so each pair still visits its co-rated y ascending.
 * n_x >= 1, 1 <= n_y < 2^31, n >= 0, n_x <= 65535 * 64.
 * The kernel reads nothing outside xr_y[0..n), xr_r[0..n) and w[0..n_y) whatever the arrays hold: row ranges are clamped
 * to [0, n] and an entry whose y is outside [0, n_y) takes w = NaN.  Malformed arrays give garbage values, not a fault;
 * n2v_eccknn_csr_check (integers only) names what is wrong by bits of *status (int32, device, cleared by the caller):    */
#define N2V_ECCKNN_CSR_BAD_PTR 1    /* xr_ptr not monotone, or an entry of it outside [0, n]                            */
#define N2V_ECCKNN_CSR_BAD_Y 2      /* an xr_y outside [0, n_y)                                                         */
#define N2V_ECCKNN_CSR_UNSORTED 4   /* two neighbouring entries of one row not strictly ascending                       */
int32_t n2v_eccknn_sparse_chunk(void);   /* entries of one row staged per round                                         */
int n2v_eccknn_csr_check(const int64_t* xr_ptr, const int32_t* xr_y, int64_t n_x, int64_t n_y, int64_t n, int32_t* status,
                         void* stream);
int n2v_eccknn_sim_sparse(const int64_t* xr_ptr, const int32_t* xr_y, const double* xr_r, int64_t n_x, int64_t n_y,
                          int64_t n, const double* w, int32_t method, int32_t min_support, double* sim, int32_t* freq,
                          double* prods, double* sqi, double* sqj, double* sq_diff, void* stream);

/* ---- KNNBasic's Pearson similarities and the ALS baselines (the plain k-NN that EccenKNN is compared against) -------
 * src/main_rec.py:166-169 hands 'pearson' and 'pearson_baseline' to surprise's own functions, :181-189 feeds the second
 * one compute_baselines(), global_mean and shrinkage, and :197 passes the per-item dictionary to all of them.  surprise
 * (scikit-surprise 1.0.6, requirements.txt:42) is not a dependency: what follows is its arithmetic restated, parity with
 * surprise itself is UNPINNED, and tests/eccknn_pearson_reference.py is the definition the kernels equal bit for bit.
 * The optional w[y] is the factor the reference meant to apply (surprise would have rejected the keyword).
 *
 * One half-epoch per launch, 2 * n_epochs launches: bu = bi = 0, then per epoch
 *   bi[i] = (sum over ir[i], in list order, of (r - global_mean) - bu[u]) / (reg_i + len(ir[i]))     for every item,
 *   bu[u] = (sum over ur[u], in list order, of (r - global_mean) - bi[i]) / (reg_u + len(ur[u]))     from the new bi.
 * ur_ptr: int64[n_users + 1], ur_i: int32, ur_r: fp64 (the ratings of every user in training order; ur_ptr[n_users] is
 * their number), ir_* the same per item.  An id outside the other side's range is no entry: it adds nothing and does
 * not count in len.  An empty row gives 0.0 / (reg + 0).  n_epochs >= 0 (0: zeros), reg_u, reg_i >= 0.
 * surprise's defaults are n_epochs 10, reg_u 15, reg_i 10.  (baseline_als; the sgd method is sequential and not built.) */
int n2v_eccknn_baselines(const int64_t* ur_ptr, const int32_t* ur_i, const double* ur_r, int64_t n_users,
                         const int64_t* ir_ptr, const int32_t* ir_u, const double* ir_r, int64_t n_items, double global_mean,
                         int32_t n_epochs, double reg_u, double reg_i, double* bu, double* bi, void* stream);

/* The frame, the inputs and the error rules of n2v_eccknn_sim / n2v_eccknn_sim_sparse; w may be NULL (no factor, the
 * bits of w = 1.0).  Per co-rated y ascending, freq += 1 and
 *   PEARSON           prods += (ri*rj)*w[y]; sqi += ri*ri; sqj += rj*rj; si += ri; sj += rj;  n = (double)freq
 *                     sim = 0 if freq < min_support, else with denum = sqrt((n*sqi - si*si) * (n*sqj - sj*sj)):
 *                     0 if denum == 0, else (n*prods - si*sj) / denum.  A difference that cancellation makes negative
 *                     gives sqrt of a negative number: the NaN is kept.            a1 .. a4 = sqi, sqj, si, sj
 *   PEARSON_BASELINE  pb = global_mean + by[y]; di = ri - (pb + bx[xi]); dj = rj - (pb + bx[xj]);
 *                     prods += (di*dj)*w[y]; sq_diff_i += di*di; sq_diff_j += dj*dj
 *                     sim = 0 if freq < max(2, min_support), else
 *                     (prods / sqrt(sq_diff_i*sq_diff_j)) * ((double)(freq-1) / ((double)(freq-1) + shrinkage)); no
 *                     zero test: 0/0 and x/0 stay NaN / inf.      a1, a2 = sq_diff_i, sq_diff_j; a3, a4 are ignored
 * The diagonal of sim is 1.  freq, prods and a1 .. a4 are [n_x][n_x], the diagonal included, each may be NULL; the
 * mirror swaps a1 / a2 and a3 / a4.  bx: fp64[n_x], by: fp64[n_y], required for PEARSON_BASELINE, ignored for PEARSON,
 * as are global_mean and shrinkage (surprise's default: 100).                                                        */
#define N2V_ECCKNN_PEARSON 0
#define N2V_ECCKNN_PEARSON_BASELINE 1
int n2v_eccknn_pearson(const double* dense, const uint8_t* mask, int64_t n_x, int64_t n_y, const double* w, int32_t kind,
                       int32_t min_support, double global_mean, const double* bx, const double* by, double shrinkage,
                       double* sim, int32_t* freq, double* prods, double* a1, double* a2, double* a3, double* a4,
                       void* stream);
int n2v_eccknn_pearson_sparse(const int64_t* xr_ptr, const int32_t* xr_y, const double* xr_r, int64_t n_x, int64_t n_y,
                              int64_t n, const double* w, int32_t kind, int32_t min_support, double global_mean,
                              const double* bx, const double* by, double shrinkage, double* sim, int32_t* freq,
                              double* prods, double* a1, double* a2, double* a3, double* a4, void* stream);

/* One wavefront per query (qx[q], qy[q]); -1 = unknown.  yr_ptr: int64[n_y + 1], yr_x: int32, yr_r: fp64 — the raters
 * of every y in training order.  Candidates are (sim[x, x2], r) in list order; the k largest by sim are kept, equal
 * sims in list order (heapq.nlargest with a key = a stable descending sort), -0.0 ties +0.0.  DEVIATION: a NaN sim
 * ranks below everything — Python's result with NaN keys depends on the order of its comparisons.  The selection is
 * walked in rank order: sim > 0 adds sim to sum_sim and sim*r to sum_ratings.  actual_k < min_k, or an unknown x or
 * y: impossible[q] = 1 and est[q] = 0; otherwise est[q] = sum_ratings / sum_sim (before any fallback or clipping).
 * 1 <= k <= N2V_ECCKNN_MAX_K, min_k >= 1, n_q >= 1.                                                                 */
int n2v_eccknn_estimate(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x, const double* yr_r,
                        int64_t n_y, const int32_t* qx, const int32_t* qy, int64_t n_q, int32_t k, int32_t min_k,
                        double* est, int32_t* actual_k, uint8_t* impossible, void* stream);

/* ---- Centred k-NN: surprise's KNNWithMeans, KNNWithZScore and KNNBaseline (csrc/n2v_eccknn.hip) ------------------------
 * The other three k-NN predictors of surprise 1.0.6, restated from memory of its source: parity with surprise itself is
 * UNPINNED, and tests/knn_centered_reference.py is the definition the kernels equal bit for bit (fp64, no fused
 * multiply-add, every parenthesis below one rounding).  The neighbours are selected exactly as by n2v_eccknn_estimate, by
 * the same device function; the modes differ in what a kept neighbour (x2, s = sim[x, x2] > 0, r) adds and in the finish:
 *   sum_sim += s; actual_k += 1; sum_ratings += t with
 *     MEANS     t = s * (r - mu[x2])
 *     ZSCORE    t = s * ((r - mu[x2]) / sd[x2])
 *     BASELINE  t = s * (r - ((global_mean + bx[x2]) + by[y]))
 *   actual_k < min_k: sum_ratings = 0 (NOT impossible, unlike n2v_eccknn_estimate);
 *   base = mu[x] (MEANS, ZSCORE) or (global_mean + bu[u]) + bi[i] (BASELINE: the user's bias first, whichever side x is);
 *   est = base if actual_k == 0, else base + sum_ratings / sum_sim (ZSCORE: base + (sum_ratings / sum_sim) * sd[x]).
 * MEANS / ZSCORE: an unknown x or y is impossible (est 0, actual_k 0) and nothing else is.  BASELINE: nothing is; an
 * unknown user drops bu[u], an unknown item drops bi[i] (both: est = global_mean), the neighbours are not visited and
 * actual_k = 0.  tx: fp64[n_x], mu (MEANS, ZSCORE) or bx (BASELINE); sd: fp64[n_x], read by ZSCORE only; by: fp64[n_y],
 * read by BASELINE only; (bx, by) = (bu, bi) when user_based, (bi, bu) otherwise.  A table the mode reads may not be
 * NULL; a centering other than the three below is N2V_ERR_INVALID.  An entry of yr_x outside [0, n_x) is never used as
 * an index: its similarity is NaN, it adds nothing and no table is read for it.
 *
 * n2v_eccknn_row_moments, one wavefront per row of the CSR (ptr int64[n_rows + 1], r fp64[n]; row ranges clamped to [0, n]):
 *   mu[row] = (sum of the row's r, from 0.0, in list order) / count
 *   sd[row] = sqrt((sum of (r - mu[row]) * (r - mu[row]), in list order) / count)
 * An empty row gives 0 / 0.  A sd equal to 0.0 is replaced by zero_sigma unless zero_sigma is NaN (no replacement).
 * surprise's overall sigma is the same call on one row that holds every rating.  DEVIATION: numpy's mean / std add
 * pairwise above 8 elements; these sums are sequential.                                                               */
#define N2V_ECCKNN_CENTER_MEANS 1
#define N2V_ECCKNN_CENTER_ZSCORE 2
#define N2V_ECCKNN_CENTER_BASELINE 3
int n2v_eccknn_row_moments(const int64_t* ptr, const double* r, int64_t n_rows, int64_t n, double zero_sigma, double* mu,
                           double* sd, void* stream);
int n2v_eccknn_estimate_centered(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x, const double* yr_r,
                                 int64_t n_y, const int32_t* qx, const int32_t* qy, int64_t n_q, int32_t k, int32_t min_k,
                                 int32_t centering, int32_t user_based, double global_mean, const double* tx, const double* sd,
                                 const double* by, double* est, int32_t* actual_k, uint8_t* impossible, void* stream);

/* surprise's AlgoBase.predict, restated from its documented behaviour: pred = global_mean where impossible, then
 * min(hi, .) and max(lo, .) (a NaN becomes hi).  r_true (may be NULL): *rmse = sqrt(sum((r_true - pred)^2) / n_q),
 * the sum taken in query order by one workgroup.                                                                   */
int n2v_eccknn_predict(const double* est, const uint8_t* impossible, const double* r_true, int64_t n_q, double global_mean,
                       double lo, double hi, double* pred, double* rmse, void* stream);

/* ---- k-NN sweep: every (k, min_k) of a grid from one neighbour selection (csrc/n2v_eccknn.hip) --------------------------
 * The reference's experiment varies -k and -mink over the same similarities and the same queries.  The prefix argument:
 * the selection list is kept in a total order (sim descending, list position ascending, NaN last), so the selection for k
 * is the first k entries of the selection for any larger k; the sums that follow are sequential in rank order, so the sums
 * for k are a prefix of the sums for the largest k, the same adds in the same order; and min_k enters only in the finish.
 * Hence one selection at ks[n_k - 1] and one walk down it give every cell, and cell (j, m) holds exactly what
 * n2v_eccknn_estimate (n2v_eccknn_estimate_centered) gives for k = ks[j], min_k = min_ks[m], bit for bit.
 * ks: int32[n_k], min_ks: int32[n_m]: HOST arrays, read during the call and passed to the kernel by value; both strictly
 * ascending, 1 <= n_k, n_m <= N2V_ECCKNN_MAX_SWEEP, 1 <= ks[j] <= N2V_ECCKNN_MAX_K, min_ks[m] >= 1.  The outputs are
 * cell-major, a cell being a contiguous column over the queries:
 *   est: fp64[n_k][n_m][n_q], impossible: uint8[n_k][n_m][n_q], actual_k: int32[n_k][n_q] (it does not depend on min_k).
 * One wavefront per query; everything else as the single-cell calls, whose argument rules hold.  A bad grid, a NULL
 * output or a bad table of the centred call is N2V_ERR_INVALID before any launch.                                      */
#define N2V_ECCKNN_MAX_SWEEP 16   /* values a side of the grid                                                           */
int n2v_eccknn_estimate_sweep(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x, const double* yr_r,
                              int64_t n_y, const int32_t* qx, const int32_t* qy, int64_t n_q, const int32_t* ks, int32_t n_k,
                              const int32_t* min_ks, int32_t n_m, double* est, int32_t* actual_k, uint8_t* impossible,
                              void* stream);
int n2v_eccknn_estimate_sweep_centered(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x,
                                       const double* yr_r, int64_t n_y, const int32_t* qx, const int32_t* qy, int64_t n_q,
                                       const int32_t* ks, int32_t n_k, const int32_t* min_ks, int32_t n_m, int32_t centering,
                                       int32_t user_based, double global_mean, const double* tx, const double* sd,
                                       const double* by, double* est, int32_t* actual_k, uint8_t* impossible, void* stream);

/* The two error measures of surprise's cross_validate over the columns of pred: fp64[n_cols][n_q] against r_true: fp64[n_q],
 * one workgroup per column, both sums taken in query order by one thread:
 *   rmse[c] = sqrt(sum((r_true - pred)^2) / n_q), the bits n2v_eccknn_predict gives for that column;
 *   mae[c]  = sum(|r_true - pred|) / n_q.
 * rmse, mae: fp64[n_cols]; either may be NULL, not both.  n_q >= 1, 1 <= n_cols < 2^31.                                   */
int n2v_eccknn_errors(const double* pred, const double* r_true, int64_t n_q, int64_t n_cols, double* rmse, double* mae,
                      void* stream);

/* ---- Matrix factorisation: surprise's SVD under a deterministic stratified schedule (csrc/n2v_svd.hip) --------------
 * The third algorithm of src/main_rec.py:341-348 (`-algo svd`, surprise 1.0.6's SVD).  surprise is not a dependency: the
 * model and the update below are its arithmetic restated from memory, parity with surprise itself is UNPINNED, and
 * tests/svd_reference.py is the definition the kernels equal bit for bit.  Everything is fp64 without fused
 * multiply-add, every expression evaluated as written, left to right.  Per rating (u, i, r), with puf / qif the values
 * before the rating:
 *   dot = sum over f of qi[i][f] * pu[u][f]                      (the order: below)
 *   err = r - (((mu + bu[u]) + bi[i]) + dot)                     biased;   err = r - dot   otherwise
 *   bu[u] = bu[u] + lr_bu * (err - reg_bu * bu[u]);  bi[i] = bi[i] + lr_bi * (err - reg_bi * bi[i])      biased only
 *   pu[u][f] = puf + lr_pu * (err * qif - reg_pu * puf);  qi[i][f] = qif + lr_qi * (err * puf - reg_qi * qif)
 * The dot: lane l of a wavefront starts from +0.0 and adds the products of the factors l, l + 64, l + 128, l + 192 that
 * exist, ascending; then v = v + v[lane ^ m] for m = 32, 16, 8, 4, 2, 1.  Addition commutes, so all 64 lanes end with
 * the same value and err needs no broadcast.  (A NaN's sign and payload are not part of the contract.)
 *
 * The schedule, P = n_strata: user u is in block ub = (u * P) / n_users, item i in ib = (i * P) / n_items (64-bit
 * integers), a rating in stratum s = (ib - ub) mod P and there in block ub.  One epoch applies the blocks in the order
 * `for s: for ub:`, and inside a block the ratings in the order given (ascending u, then training order).  Two blocks
 * of one stratum share no user and no item, so one wavefront per block and one launch per stratum — stream order is
 * the only barrier, there are no atomics on the model — give exactly the result of that sequential loop.  P = 1 is
 * surprise's own order.  Blocks may be empty.
 * blk_ptr: int64[P * P + 1], block (s, ub) is [blk_ptr[s * P + ub], blk_ptr[s * P + ub + 1]); blk_u, blk_i: int32[n];
 * blk_r: fp64[n].  n2v_svd_blocks_check (integers only; reads nothing outside blk_ptr[0 .. P * P] and the n entries)
 * names what is wrong by bits of *status (int32, device, cleared by the caller).  n2v_svd_epoch is only defined on lists
 * that pass it: it clamps every range to [0, n] and skips a rating whose ids are out of range, so a malformed list is no
 * out-of-bounds access, but two blocks of a stratum that share a row would race.                                       */
#define N2V_SVD_BAD_PTR 1       /* blk_ptr does not start at 0, is not monotone, or leaves [0, n]                     */
#define N2V_SVD_BAD_END 2       /* blk_ptr[P * P] != n                                                                 */
#define N2V_SVD_BAD_ID 4        /* a blk_u outside [0, n_users) or a blk_i outside [0, n_items)                        */
#define N2V_SVD_WRONG_BLOCK 8   /* a rating outside the range of the block (s, ub) its ids put it in                   */
#define N2V_SVD_UNSORTED 16     /* inside a block, a blk_u below its predecessor                                       */
int32_t n2v_svd_max_factors(void);   /* 256: four factors a lane                                                       */
int32_t n2v_svd_max_strata(void);    /* 32768                                                                          */
int n2v_svd_blocks_check(const int64_t* blk_ptr, const int32_t* blk_u, const int32_t* blk_i, int64_t n_strata,
                         int64_t n_users, int64_t n_items, int64_t n, int32_t* status, void* stream);
/* One epoch: n_strata launches.  bu: fp64[n_users], bi: fp64[n_items], pu: fp64[n_users][n_factors],
 * qi: fp64[n_items][n_factors], updated in place; bu and bi are neither read nor written when biased == 0.
 * 1 <= n_factors <= 256, 1 <= n_strata <= 32768, n >= 1.                                                              */
int n2v_svd_epoch(const int64_t* blk_ptr, const int32_t* blk_u, const int32_t* blk_i, const double* blk_r,
                  int64_t n_strata, int64_t n_users, int64_t n_items, int64_t n, int32_t n_factors, double mu,
                  int32_t biased, double lr_bu, double lr_bi, double lr_pu, double lr_qi, double reg_bu, double reg_bi,
                  double reg_pu, double reg_qi, double* bu, double* bi, double* pu, double* qi, void* stream);
/* One wavefront per query (q_u[q], q_i[q]); an id outside its range (-1) is unknown.  The same dot, through the same
 * device function.  biased: est = mu, + bu[u] if the user is known, + bi[i] if the item is, + dot if both are, in that
 * order; impossible = 0.  Otherwise est = dot if both are known, else est = 0 and impossible = 1 ('User and item are
 * unknown.').  Before any fallback or clipping: n2v_eccknn_predict does those.  n_q >= 1.                             */
int n2v_svd_estimate(const double* bu, const double* bi, const double* pu, const double* qi, int64_t n_users,
                     int64_t n_items, int32_t n_factors, double mu, int32_t biased, const int32_t* q_u, const int32_t* q_i,
                     int64_t n_q, double* est, uint8_t* impossible, void* stream);

/* ---- Non-negative matrix factorisation: surprise's NMF in surprise's own order (csrc/n2v_nmf.hip) ---------------------
 * surprise 1.0.6's NMF with biased = False (Luo et al. 2014).  surprise is not a dependency: the update below is its
 * arithmetic restated from memory, parity with surprise itself is UNPINNED, and tests/nmf_reference.py is the definition
 * the kernels equal bit for bit.  The model is the unbiased one above (est = dot, the same dot), so n2v_svd_estimate and
 * n2v_svd_topn serve it with biased = 0.  Everything is fp64 without fused multiply-add, as written, left to right.
 * One epoch reads pu and qi as they were when it began and writes pu_out and qi_out.  For every user u, over its
 * ratings (i, r) in the order of the user-major list, num and den starting from +0.0 per factor:
 *   est = dot(qi[i], pu[u]);  num[f] = num[f] + qi[i][f] * r;  den[f] = den[f] + qi[i][f] * est
 * and after the list, with len its length as a double:
 *   den[f] = den[f] + (len * reg_pu) * pu[u][f];  pu_out[u][f] = pu[u][f] * (num[f] / den[f])
 * For every item i the same with the roles swapped (rows pu[u] of its raters, reg_qi, qi_out), over the item-major list,
 * which holds each item's raters ascending in u: surprise's all_ratings() order.  There is no special case: a zero
 * denominator gives the NaN or infinity of the arithmetic (an empty list: 0 / 0), and they propagate.  (A NaN's sign and
 * payload are not part of the contract.)
 * A list is (ptr int64[n_rows + 1], other int32[n], r fp64[n]), row k being [ptr[k], ptr[k + 1]).  n2v_nmf_lists_check
 * (integers only; scratch: int32[n_users + n_items], cleared by the call; *status: int32, device, cleared by the caller)
 * names what is wrong with the pair of lists by bits of *status.  n2v_nmf_epoch is only defined on lists that pass it:
 * it clamps every row range to [0, n] and skips an entry whose id is out of range, so a malformed list is no
 * out-of-bounds access.                                                                                                */
#define N2V_NMF_BAD_PTR 1       /* a ptr does not start at 0, is not monotone, or leaves [0, n]                       */
#define N2V_NMF_BAD_END 2       /* a ptr does not end at n                                                             */
#define N2V_NMF_BAD_ID 4        /* an item id outside [0, n_items) or a user id outside [0, n_users)                   */
#define N2V_NMF_UNSORTED 8      /* a row of the item-major list not strictly ascending in u                            */
#define N2V_NMF_BAD_COUNT 16    /* an id occurs in one list another number of times than its row of the other is long  */
int32_t n2v_nmf_depth(void);         /* rows of the other table a wavefront fetches ahead of the entry it works on     */
int n2v_nmf_lists_check(const int64_t* u_ptr, const int32_t* u_i, const int64_t* i_ptr, const int32_t* i_u, int64_t n_users,
                        int64_t n_items, int64_t n, int32_t* scratch, int32_t* status, void* stream);
/* One epoch, one launch: one wavefront per user and per item.  u_order int32[n_users] / i_order int32[n_items]: the row
 * the k-th wavefront of a side takes (a permutation; longest lists first is the fast one; NULL: the identity); it changes
 * no bit.  pu, qi: the tables read; pu_out, qi_out: the tables written, each disjoint from both inputs and from the other
 * output, else N2V_ERR_INVALID before any launch.  1 <= n_factors <= 256, n >= 1.                                      */
int n2v_nmf_epoch(const int64_t* u_ptr, const int32_t* u_i, const double* u_r, const int64_t* i_ptr, const int32_t* i_u,
                  const double* i_r, const int32_t* u_order, const int32_t* i_order, int64_t n_users, int64_t n_items,
                  int64_t n, int32_t n_factors, double reg_pu, double reg_qi, const double* pu, const double* qi,
                  double* pu_out, double* qi_out, void* stream);

/* ---- Top-N lists of the rating predictors (csrc/n2v_eccknn.hip, n2v_svd.hip, n2v_topn.h) ------------------------------
 * What src/recsys.py sketches ("Get the top songs" per user) and surprise's recipe algo.test(build_anti_testset()) +
 * get_top_n compute, without storing the n_users x n_items predictions.  tests/topn_reference.py is the definition.
 * An owner is an inner user id (owners: int32[n_owners]; an id outside [0, n_users), such as -1, is an unknown user who
 * has seen nothing).  Its candidates are the inner items 0 .. n_items - 1 it has not rated: seen_ptr int64[n_users + 1],
 * seen_i int32[n_seen], the rated items of every user strictly ascending (a CSR that passes n2v_eccknn_csr_check; the
 * kernels clamp every row range to [0, n_seen], so a malformed one gives wrong lists, never a fault).  A candidate's
 * score is n2v_eccknn_estimate's (n2v_svd_estimate's) value through n2v_eccknn_predict's fallback and clip, by the same
 * device functions: the same bits.  Ranking is the one total order of csrc/n2v_rank.h with the item id as the position:
 * higher score first, equal scores by lower item id, -0.0 ties +0.0 (Python's stable sort(key=est, reverse=True) over the
 * anti-testset in inner-id order).  items: int32[n_owners][top_n], score: fp64[n_owners][top_n]; an owner with fewer than
 * top_n candidates ends in (-1, NaN) entries.  One wavefront per (owner, segment of the items), `segments` of them per
 * owner (0: n2v_topn_segments), each with its best-top_n list in LDS; part_score fp64 / part_pos int32
 * [n_owners][segments][top_n] are the caller's scratch, and a second kernel merges them under the same order, so the
 * result does not depend on `segments`.  1 <= top_n <= N2V_TOPN_MAX_N, 0 <= segments <= 64, n_owners >= 1,
 * n_items < 2^31 - 1.  n2v_eccknn_topn: (x, y) = (owner, item) when user_based, (item, owner) otherwise, so n_users is
 * n_x or n_y; sim, yr_*, k and min_k as n2v_eccknn_estimate.  n2v_svd_topn: the tables of n2v_svd_estimate; global_mean
 * is the fallback of an impossible estimate (the training mean), which mu is not when biased == 0.                   */
#define N2V_TOPN_MAX_N 256
int32_t n2v_topn_segments(int64_t n_owners, int64_t n_candidates);
int n2v_eccknn_topn(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x, const double* yr_r,
                    int64_t n_y, int32_t user_based, const int64_t* seen_ptr, const int32_t* seen_i, int64_t n_seen,
                    const int32_t* owners, int64_t n_owners, int32_t k, int32_t min_k, double global_mean, double lo,
                    double hi, int32_t top_n, int32_t segments, double* part_score, int32_t* part_pos, int32_t* items,
                    double* score, void* stream);
/* n2v_eccknn_topn with the estimates of n2v_eccknn_estimate_centered (centering, tx, sd, by as there; global_mean is both
 * the centring's and the fallback's).  Under BASELINE an unknown owner's candidates score global_mean + bi[item], clipped. */
int n2v_eccknn_topn_centered(const double* sim, int64_t n_x, const int64_t* yr_ptr, const int32_t* yr_x, const double* yr_r,
                             int64_t n_y, int32_t user_based, const int64_t* seen_ptr, const int32_t* seen_i, int64_t n_seen,
                             const int32_t* owners, int64_t n_owners, int32_t k, int32_t min_k, double global_mean, double lo,
                             double hi, int32_t top_n, int32_t segments, int32_t centering, const double* tx, const double* sd,
                             const double* by, double* part_score, int32_t* part_pos, int32_t* items, double* score,
                             void* stream);
int n2v_svd_topn(const double* bu, const double* bi, const double* pu, const double* qi, int64_t n_users, int64_t n_items,
                 int32_t n_factors, double mu, int32_t biased, const int64_t* seen_ptr, const int32_t* seen_i, int64_t n_seen,
                 const int32_t* owners, int64_t n_owners, double global_mean, double lo, double hi, int32_t top_n,
                 int32_t segments, double* part_score, int32_t* part_pos, int32_t* items, double* score, void* stream);

/* ---- SlopeOne: surprise's parameter-free item-deviation predictor (csrc/n2v_eccknn.hip, csrc/n2v_slopeone.hip) -------
 * surprise 1.0.6's SlopeOne (Lemire and Maclachlan 2005), restated from memory of its source: parity with surprise itself
 * is UNPINNED, and tests/slopeone_reference.py is the definition the kernels equal bit for bit (fp64, every operation
 * below one rounding; a NaN's sign and payload are not part of the contract).  x = items, y = users.
 * The table: for every pair of items i < j, over the users u who rated both, ascending in u,
 *   freq[i][j] += 1;  acc[i][j] = acc[i][j] + (r[u][i] - r[u][j])                  (from 0 and +0.0)
 *   dev[i][j] = acc[i][j] / (double)freq[i][j]      (freq 0: 0.0 / 0 = NaN; n2v_slopeone_estimate never reads it)
 *   dev[j][i] = -dev[i][j]                          (the stored value with its sign bit flipped, a zero included)
 *   dev[i][i] = 0.0;  freq[j][i] = freq[i][j];  freq[i][i] = the raters of i
 * dev: fp64[n_items][n_items]; freq: int32[n_items][n_items]; acc (may be NULL): fp64[n_items][n_items], the raw sums of
 * surprise's loop over every ordered pair, acc[j][i] being the sum of (r[u][j] - r[u][i]): -acc[i][j], and +0.0 where
 * that is a zero.  They are one more method of the two tile kernels behind n2v_eccknn_sim / n2v_eccknn_sim_sparse, whose
 * inputs (dense, mask of n2v_eccknn_densify; the x-major CSR), frame, clamping and error rules they share; there is no
 * w and no min_support.  n_items * n_items <= 2^31 (16 GiB of dev and 8 GiB of freq at the limit), and for the dense
 * form n_items * n_users <= n2v_eccknn_max_dense().                                                                    */
int n2v_slopeone_dev(const double* dense, const uint8_t* mask, int64_t n_items, int64_t n_users, double* dev, int32_t* freq,
                     double* acc, void* stream);
int n2v_slopeone_dev_sparse(const int64_t* xr_ptr, const int32_t* xr_y, const double* xr_r, int64_t n_items, int64_t n_users,
                            int64_t n, double* dev, int32_t* freq, double* acc, void* stream);
/* One wavefront per query (q_u[q], q_i[q]).  ur_ptr: int64[n_users + 1], ur_i: int32[n] — the items every user rated, in
 * training order; user_mean: fp64[n_users] (n2v_eccknn_row_moments over the same lists).  Over the entries j of ur[u] in
 * list order with freq[i][j] > 0 (the item itself included, when u rated it): s = s + dev[i][j] from +0.0, n_dev += 1;
 *   est = user_mean[u] if n_dev == 0, else user_mean[u] + s / (double)n_dev       (before any fallback or clipping)
 * A u or i outside its range (-1) is unknown: impossible = 1, est = 0, n_dev = 0; nothing else is impossible.  Row ranges
 * are clamped to [0, n] and an entry of ur_i outside [0, n_items) is no entry, so a malformed list is no out-of-bounds
 * access.  n_q >= 1.                                                                                                   */
int n2v_slopeone_estimate(const double* dev, const int32_t* freq, int64_t n_items, const int64_t* ur_ptr, const int32_t* ur_i,
                          int64_t n_users, int64_t n, const double* user_mean, const int32_t* q_u, const int32_t* q_i,
                          int64_t n_q, double* est, int32_t* n_dev, uint8_t* impossible, void* stream);
/* The top-N lists of the section above with n2v_slopeone_estimate's value as the score, by the bits: one wavefront per
 * (owner, segment), 64 neighbouring candidates at a time, one a lane; every rated j adds -dev[j][c], which has the bits of
 * dev[c][j], to the lane's own sum in list order, so a candidate's reads are two contiguous pieces of row j.  Owners,
 * seen_*, top_n, segments, the scratch and the outputs as n2v_eccknn_topn.                                             */
int n2v_slopeone_topn(const double* dev, const int32_t* freq, int64_t n_items, const int64_t* ur_ptr, const int32_t* ur_i,
                      int64_t n_users, int64_t n, const double* user_mean, const int64_t* seen_ptr, const int32_t* seen_i,
                      int64_t n_seen, const int32_t* owners, int64_t n_owners, double global_mean, double lo, double hi,
                      int32_t top_n, int32_t segments, double* part_score, int32_t* part_pos, int32_t* items, double* score,
                      void* stream);

/* ---- Co-clustering: surprise's CoClustering in surprise's own order (csrc/n2v_cocl.hip) ---------------------------------
 * surprise 1.0.6's CoClustering (George and Merugu 2005).  surprise is not a dependency: the algorithm below is restated
 * from memory, parity with surprise itself is UNPINNED, and tests/coclustering_reference.py is the definition the kernels
 * equal bit for bit.  Everything is fp64 without fused multiply-add, as written, left to right.  (A NaN's sign and payload
 * are not part of the contract.)  Every user is in one of n_cltr_u clusters (cltr_u int32[n_users]), every item in one of
 * n_cltr_i (cltr_i int32[n_items]), 1 <= n_cltr_u, n_cltr_i <= n2v_cocl_max_clusters() = 64: one lane holds one cluster.
 * A list is (ptr int64[n_rows + 1], other int32[n], r fp64[n]), row k being [ptr[k], ptr[k + 1]), in training order
 * (Trainset.ur / Trainset.ir).  user_mean fp64[n_users] / item_mean fp64[n_items]: n2v_eccknn_row_moments over them.
 * The averages: int64 counts and fp64 sums per user cluster, item cluster and co-cluster; an empty one's average is
 * global_mean, any other sum / (double)count.  DEVIATION from surprise, deliberate: surprise adds each sum as one chain
 * over all ratings; here the sums are grouped by user row.  For user u over ur[u] in list order, from +0.0:
 *   t_u = t_u + r;  s_u[ic] = s_u[ic] + r  with ic = cltr_i[i]
 * then over the users in ascending inner id, for every ic (an s_u[ic] nothing was added to is +0.0):
 *   sum_cltr_u[cltr_u[u]] += t_u;  sum_cltr_i[ic] += s_u[ic];  sum_cocltr[cltr_u[u]][ic] += s_u[ic]
 * so a chain is n_users long, not n long; where every sum is exact (ratings that are multiples of 1/2) the two orders
 * give the same bytes.  One assignment pass, for every row of one side and every candidate cluster c of that side, over
 * the row's list in list order from +0.0 (user side: row u, c = uc, ic = cltr_i[i]; item side: row i, c = ic,
 * uc = cltr_u[u]):
 *   est = (((avg_cocltr[uc][ic] + user_mean[u]) - avg_cltr_u[uc]) + item_mean[i]) - avg_cltr_i[ic]
 *   d = r - est;  errors[c] = errors[c] + d * d
 * and the row takes numpy's argmin of errors: the first index holding a NaN if there is one, else the first index of the
 * minimum; an empty list leaves cluster 0.  An epoch is the averages, the user pass, then the item pass over the
 * assignment the user pass wrote and the SAME averages.
 * No kernel indexes with a value it has not checked: a row range is clamped to [0, n]; an entry whose id is outside its
 * range, or whose cluster (its own, or in n2v_cocl_averages its user's) is outside [0, n_cltr), adds nothing, so a
 * malformed list or assignment is no out-of-bounds access.                                                              */
int32_t n2v_cocl_max_clusters(void);
/* The three average tables of an assignment, a clear and two launches: one wavefront per user writes part (the caller's scratch,
 * fp64[n_users][n_cltr_i + 1]: s_u, then t_u) and adds its counts to count_cocltr (int64[n_cltr_u][n_cltr_i], cleared by
 * the call; integer atomics); then one wavefront per table row runs the chains over the users and writes its averages:
 * avg_cltr_u fp64[n_cltr_u], avg_cltr_i fp64[n_cltr_i], avg_cocltr fp64[n_cltr_u][n_cltr_i].  n >= 0.                  */
int n2v_cocl_averages(const int64_t* ur_ptr, const int32_t* ur_i, const double* ur_r, int64_t n_users, int64_t n_items, int64_t n,
                      const int32_t* cltr_u, const int32_t* cltr_i, int32_t n_cltr_u, int32_t n_cltr_i, double global_mean,
                      double* part, double* avg_cltr_u, double* avg_cltr_i, double* avg_cocltr, int64_t* count_cocltr,
                      void* stream);
/* One assignment pass of one side, one launch, one wavefront per row.  user_side != 0: the list is the user-major one
 * (other = items), cltr_i is read and cltr_u written; user_side == 0: the item-major one, cltr_u read and cltr_i written.
 * order int32[n_rows]: the row the k-th wavefront takes (a permutation; longest lists first is the fast one; NULL: the
 * identity); it changes no bit.  cltr_u and cltr_i must not overlap, else N2V_ERR_INVALID before any launch.  n >= 0.  */
int n2v_cocl_assign(const int64_t* ptr, const int32_t* other, const double* r, const int32_t* order, int64_t n_users,
                    int64_t n_items, int64_t n, int32_t user_side, int32_t n_cltr_u, int32_t n_cltr_i, const double* user_mean,
                    const double* item_mean, const double* avg_cltr_u, const double* avg_cltr_i, const double* avg_cocltr,
                    int32_t* cltr_u, int32_t* cltr_i, void* stream);
/* One query per lane (q_u[q], q_i[q]); an id outside its range (-1) is unknown.  Both known: the expression above with the
 * fitted clusters; only the user: user_mean[u]; only the item: item_mean[i]; neither: global_mean.  impossible = 0 always.
 * Before any clipping: n2v_eccknn_predict does that.  n_q >= 1.                                                        */
int n2v_cocl_estimate(const int32_t* cltr_u, const int32_t* cltr_i, const double* avg_cltr_u, const double* avg_cltr_i,
                      const double* avg_cocltr, const double* user_mean, const double* item_mean, int64_t n_users,
                      int64_t n_items, int32_t n_cltr_u, int32_t n_cltr_i, double global_mean, const int32_t* q_u,
                      const int32_t* q_i, int64_t n_q, double* est, uint8_t* impossible, void* stream);
/* The top-N lists of the section above with n2v_cocl_estimate's value as the score, by the same device function and so by
 * the same bits: one wavefront per (owner, segment), 64 neighbouring candidates at a time, one a lane.  An unknown owner
 * scores every item at its clipped item_mean.  Owners, seen_*, top_n, segments, the scratch and the outputs as
 * n2v_eccknn_topn.                                                                                                      */
int n2v_cocl_topn(const int32_t* cltr_u, const int32_t* cltr_i, const double* avg_cltr_u, const double* avg_cltr_i,
                  const double* avg_cocltr, const double* user_mean, const double* item_mean, int64_t n_users, int64_t n_items,
                  int32_t n_cltr_u, int32_t n_cltr_i, const int64_t* seen_ptr, const int32_t* seen_i, int64_t n_seen,
                  const int32_t* owners, int64_t n_owners, double global_mean, double lo, double hi, int32_t top_n,
                  int32_t segments, double* part_score, int32_t* part_pos, int32_t* items, double* score, void* stream);

/* ---- Eccentricity statistics: the ir / ie / ire / ier item weights and the per-user ue (csrc/n2v_eccstats.hip) -----
 * Replaces src/utils.py:53-153 (pandas group-bys and merges).  Rows are (user, item, feedback, timewindow) with inner
 * ids; a group is a distinct (item, timewindow) pair, numbered in ascending (item, timewindow) order.  Everything is
 * fp64 / int32 / int64 on the caller's stream with caller-owned buffers.  Every rounded sum has one stated order
 * (tests/eccstats_reference.py) and the result equals that restatement bit for bit; a NaN's sign and payload are not
 * part of the contract.  Segment sums run left to right in segment order; global sums add consecutive chunks of
 * N2V_ECCSTATS_CHUNK elements left to right, then the chunk sums left to right.                                    */
#define N2V_ECCSTATS_CHUNK 4096
#define N2V_ECCSTATS_Z 0         /* out = a - (mean / std)            stats of a; the reference's precedence        */
#define N2V_ECCSTATS_ZERO_ONE 1  /* out = (a - min) / (max - min)     stats of a                                     */
#define N2V_ECCSTATS_MUL 2       /* out = a * b                                                                      */
#define N2V_ECCSTATS_DIV 3       /* out = a / b                                                                      */
#define N2V_ECCSTATS_DIV_INF0 4  /* out = a / b, +-inf replaced by 0.0                                               */

/* HOST: table[c] = -log((double)c) for 1 <= c < len by the host's libm (what Python's math.log calls), table[0] NaN.
 * The device's log is not promised to equal libm's, so irg is resolved through this table.                         */
int n2v_eccstats_log_table(int64_t len, double* table);

/* key_sorted: int64[n] ascending, key = item * n_tw + rank of the timewindow (a stable sort); perm: int64[n], the row
 * that sorted position k holds.  Writes row_group: int32[n] BY ROW, group_begin: int64[n + 1] (entries 0 .. n_groups),
 * unum: int64[n] (entries < n_groups), item_gptr: int64[n_items + 1] (the groups of item i are item_gptr[i] ..
 * item_gptr[i + 1]), counts: int64[2] = {n_groups, largest unum}.  scratch: int64[n2v_eccstats_groups_scratch(n)].
 * 1 <= n < 2^31.                                                                                                    */
int64_t n2v_eccstats_groups_scratch(int64_t n);
int n2v_eccstats_groups(const int64_t* key_sorted, const int64_t* perm, int64_t n, int64_t n_tw, int64_t n_items,
                        int64_t* scratch, int32_t* row_group, int64_t* group_begin, int64_t* unum, int64_t* item_gptr,
                        int64_t* counts, void* stream);
/* irg[g] = log_table[unum[g]] (a DEVICE copy of the table).  A count outside [1, table_len) gives NaN and sets bit 0
 * of *status (int32, device, cleared by the caller).                                                                */
int n2v_eccstats_irg(const int64_t* unum, int64_t n_groups, const double* log_table, int64_t table_len, double* irg,
                     int32_t* status, void* stream);

/* Segments s = [seg_ptr[s], seg_ptr[s + 1]) of positions k; p = perm[k] (perm NULL: p = k):
 *   out_sum[s]  = sum a[p]                  (mean != 0: divided by the segment's length)
 *   out_wsum[s] = sum a[p] * g[idx[p]]      (idx NULL: g[p]); each product rounded before it is added
 * both from +0.0, left to right.  A p outside [0, n_a) or an index outside [0, n_g) contributes NaN.  Segments shorter
 * than 64 take one lane each, longer ones a wavefront each.  out_sum or out_wsum may be NULL.
 * scratch: int32[n_seg + 1].  1 <= n_seg < 2^31.                                                                    */
int n2v_eccstats_segsum(const int64_t* seg_ptr, int64_t n_seg, const int64_t* perm, const double* a, int64_t n_a,
                        const int32_t* idx, const double* g, int64_t n_g, int32_t mean, int32_t* scratch, double* out_sum,
                        double* out_wsum, void* stream);

/* stats: fp64[8] = {sum, mean = sum / n, ssd = sum (x - mean) * (x - mean), var = ssd / n, std = sqrt(var), min, max,
 * n}.  min / max: NaN if any x is NaN; -0.0 is below +0.0.  scratch: fp64[n2v_eccstats_moments_scratch(n)].        */
int64_t n2v_eccstats_moments_scratch(int64_t n);
int n2v_eccstats_moments(const double* x, int64_t n, double* scratch, double* stats, void* stream);

/* Elementwise, op one of N2V_ECCSTATS_*; b is read by MUL / DIV / DIV_INF0, stats by Z / ZERO_ONE.                  */
int n2v_eccstats_finish(int32_t op, const double* a, const double* b, const double* stats, int64_t n, double* out,
                        void* stream);

/* ---- Eccentricity split: ue -> n bins of users -> one bipartite user-item CSR graph per bin (csrc/n2v_eccsplit.hip) -----
 * Replaces src/utils.py:305-312 (mark_n), :382-405 (split_and_save_edgelist, save_edgelist) and the read-back of each
 * file by src/main.py:66-80.  Rows are (user, item, weight) with inner ids (int64) in file order; the graph of a set of
 * rows is the one csr.from_edges(user name, item name, weight, directed=False) builds on the host: a repeated (user,
 * item) row keeps its last weight, every surviving pair gives the entries u -> i and i -> u, the dense id of a node is
 * the rank of its name among the graph's names, start_order is first appearance (user before item on a row).  Integer
 * arithmetic only: weights are moved by their bytes (NaN payloads, inf and -0.0 included), never added.  The sorts are the
 * caller's (stable, ascending, int64 keys).  Workgroups meet only at launch boundaries: no result depends on dispatch
 * order.  Limits: every size (n_rows, n_users + n_items, n_bins, 2 * selected rows) is at most 2^31 - 1, so the keys
 * dense_u * N + dense_i stay below 2^62; beyond them N2V_ERR_INVALID.  A size of 0 launches nothing.  Indices are the
 * caller's promise (check them before the call); the kernels skip or clamp what is outside its range.             */
#define N2V_ECCSPLIT_TILE 2048                       /* elements per workgroup of the compaction passes             */
#define N2V_ECCSPLIT_NONE 0x7fffffffffffffffLL       /* first[] of a node that no selected row names                */
int32_t n2v_eccsplit_tile(void);
/* int64 words of scratch for a compaction over n elements (select: n_rows, nodes: n_users + n_items, pairs: n_sel). */
int64_t n2v_eccsplit_scratch(int64_t n);

/* key[i] orders as the split orders ue: ascending, -0.0 and +0.0 equal, every NaN (any sign or payload) after +inf. */
int n2v_eccsplit_sort_key(const double* ue, int64_t n, int64_t* key, void* stream);
/* order[r]: the user at rank r of the stable sort by (key, tie rank), a permutation of 0 .. n_users - 1.  Writes
 * bin[order[r]] = n_bins if n_users / n_bins == 0, else min(r / (n_users / n_bins) + 1, n_bins): int32 in 1 .. n_bins. */
int n2v_eccsplit_mark(const int64_t* order, int64_t n_users, int64_t n_bins, int32_t* bin, void* stream);

/* rows[0 .. *count): the row numbers k with bin[user[k]] == which (which == 0: every row), ascending; rows holds n_rows
 * words, count is one device word.  Flag and compaction are one pass over user (ballots per tile, a scan of the tile
 * counts, a scatter).  scratch: int64[n2v_eccsplit_scratch(n_rows)].                                                 */
int n2v_eccsplit_select(const int64_t* user, int64_t n_rows, const int32_t* bin, int64_t n_users, int32_t which, int64_t* scratch,
                        int64_t* rows, int64_t* count, void* stream);
/* first: int64[n_users + n_items], set to N2V_ECCSPLIT_NONE by the caller.  Over t < min(*n_sel, cap), k = rows[t]:
 * first[user[k]] = min(.., 2 k), first[n_users + item[k]] = min(.., 2 k + 1), by 64-bit integer atomic minima (any order
 * gives the same words).  rows NULL: k = t; n_sel NULL: cap rows.  cap <= n_rows.                                  */
int n2v_eccsplit_first(const int64_t* rows, const int64_t* n_sel, int64_t cap, const int64_t* user, const int64_t* item,
                       int64_t n_rows, int64_t n_users, int64_t n_items, int64_t* first, void* stream);
/* The nodes j (users, then items) with first[j] != NONE, in that order, numbered 0 .. *count - 1 ("slots"):
 * node_name[slot] = user_names[j] or item_names[j - n_users], node_first[slot] = first[j], slot_of[j] = slot, and
 * slot_of[j] = -1 for the others.  node_name / node_first: int64[n_users + n_items]; slot_of: int32[n_users + n_items];
 * scratch: int64[n2v_eccsplit_scratch(n_users + n_items)].                                                          */
int n2v_eccsplit_nodes(const int64_t* first, int64_t n_users, int64_t n_items, const int64_t* user_names, const int64_t* item_names,
                       int64_t* scratch, int64_t* node_name, int64_t* node_first, int32_t* slot_of, int64_t* count, void* stream);
/* perm_name / perm_first: the slot at position r of the sort of node_name / node_first (n_nodes entries each).
 * rank[perm_name[r]] = r (the dense id of a slot); start_order[j] = rank[perm_first[j]].  int32[n_nodes] each.       */
int n2v_eccsplit_ranks(const int64_t* perm_name, const int64_t* perm_first, int64_t n_nodes, int32_t* rank, int32_t* start_order,
                       void* stream);
/* key[t] = rank[slot_of[user[k]]] * n_nodes + rank[slot_of[n_users + item[k]]], k = rows[t] (rows NULL: t), t < n_sel. */
int n2v_eccsplit_keys(const int64_t* rows, int64_t n_sel, const int64_t* user, const int64_t* item, int64_t n_rows, int64_t n_users,
                      int64_t n_items, const int32_t* slot_of, const int32_t* rank, int64_t n_nodes, int64_t* key, void* stream);
/* key_sorted / perm: the stable sort of key (perm[t]: the position in key that sorted position t holds).  The last
 * element of every run of equal keys survives, numbered p = 0 .. *count - 1 in key order, and gives two entries:
 * ekey[2 p] = key, ekey[2 p + 1] = its mirror (i * n_nodes + u), ew[2 p] = ew[2 p + 1] = w[rows[perm[t]]] by its bytes.
 * ekey: int64[2 n_sel]; ew: fp64[2 n_sel]; scratch: int64[n2v_eccsplit_scratch(n_sel)].  2 n_sel < 2^31.            */
int n2v_eccsplit_pairs(const int64_t* key_sorted, const int64_t* perm, int64_t n_sel, const int64_t* rows, const double* w,
                       int64_t n_rows, int64_t n_nodes, int64_t* scratch, int64_t* ekey, double* ew, int64_t* count, void* stream);
/* ekey_sorted / perm: the sort of the nnz = 2 * pairs entries.  row_ptr: int64[n_nodes + 1] (rows without entries are
 * empty), col[e] = ekey_sorted[e] % n_nodes: int32[nnz], w[e] = ew[perm[e]]: fp64[nnz] by its bytes.                */
int n2v_eccsplit_fill(const int64_t* ekey_sorted, const int64_t* perm, int64_t nnz, const double* ew, int64_t n_nodes,
                      int64_t* row_ptr, int32_t* col, double* w, void* stream);

/* ---- Eccentricity consistency: two-period join, n x n transition table, per-user ie profile, feature rows
 * (csrc/n2v_ecccons.hip) -----
 * Replaces the joins and group-bys of src/utils.py:163-226 (septile_for_plot) and :326-379 (calculate_uie_dist,
 * calculate_uvec, make_data).  Integers are counted exactly and fp64 values are moved by their bytes; the only rounded
 * operations are the final divisions and, in the weighted profile, sums whose order is stated below.  Workgroups meet
 * only through 64-bit integer atomic adds (which commute) and at launch boundaries: every result is the same on every
 * run.  Every size is at most 2^31 - 1 and a bin count at most N2V_ECCCONS_MAX_BINS; beyond them N2V_ERR_INVALID.  The
 * kernels skip an index outside its range; the check functions below tell the caller that there was one.  Compactions
 * are the stable one of n2v_eccsplit_select: scratch is int64[n2v_eccsplit_scratch(n)].                            */
#define N2V_ECCCONS_MAX_BINS 256
#define N2V_ECCCONS_CELLS 4096                       /* int32 counters of the crosstab's LDS histogram: 16 KiB      */
#define N2V_ECCCONS_CHUNK 16384                      /* elements per workgroup of the crosstab                      */
#define N2V_ECCCONS_BAD_RANGE 1                      /* status bits of the check functions                          */
#define N2V_ECCCONS_BAD_PTR 2

/* *status |= N2V_ECCCONS_BAD_RANGE if some a[k], k < n, lies outside lo .. hi.  status: one int32 device word.     */
int n2v_ecccons_check_i32(const int32_t* a, int64_t n, int32_t lo, int32_t hi, int32_t* status, void* stream);
int n2v_ecccons_check_i64(const int64_t* a, int64_t n, int64_t lo, int64_t hi, int32_t* status, void* stream);
/* *status |= N2V_ECCCONS_BAD_PTR unless ptr[0] == 0, ptr[n_seg] == total and ptr never descends.                   */
int n2v_ecccons_check_ptr(const int64_t* ptr, int64_t n_seg, int64_t total, int32_t* status, void* stream);

/* Entities e < n of one index space with the values v1 / v2 and the row counts c1 / c2 of two periods (a count of 0:
 * absent).  ids[0 .. *count): the e with c1[e] > min_count and c2[e] > min_count (and both > 0), ascending; o1 / o2 their
 * values.  ids / o1 / o2 hold n words and are untouched past *count.                                               */
int n2v_ecccons_join(const double* v1, const double* v2, const int64_t* c1, const int64_t* c2, int64_t n, int64_t min_count,
                     int64_t* scratch, int64_t* ids, double* o1, double* o2, int64_t* count, void* stream);

/* bins1 / bins2: int32[m] in 1 .. n_bins.  count[a - 1][b - 1] = elements with bins1 == a and bins2 == b (int64[n][n]),
 * count_sum[a - 1] = the sum of row a - 1, ratio = count * 1.0 / count_sum (fp64[n][n]; the row of a bin that bins1
 * never names is NaN).  A histogram of at most N2V_ECCCONS_CELLS int32 counters per workgroup in LDS: all n x n cells
 * when n <= 64, otherwise stripes of N2V_ECCCONS_CELLS / n values of bins1, one sweep of the workgroup's
 * N2V_ECCCONS_CHUNK elements per stripe.  m may be 0.                                                              */
int n2v_ecccons_crosstab(const int32_t* bins1, const int32_t* bins2, int64_t m, int32_t n_bins, int64_t* count,
                         int64_t* count_sum, double* ratio, void* stream);

/* The rows of user u are perm[user_ptr[u] .. user_ptr[u + 1]) (file order inside a user: the stable sort by user).
 * item_bin[item]: 1 .. n_bins, or 0 for an item without a bin, whose rows are skipped.  One wavefront per user.
 *   weighted == 0:  profile[u][b - 1] = (rows of u in bin b) / (rows of u in any bin), integers counted exactly and
 *                   divided in fp64
 *   weighted != 0:  profile[u][b - 1] = (sum of feedback over those rows) / (sum of feedback over the rows of u in
 *                   any bin), each sum from +0.0 in the order of the user's rows
 * A user without a row in any bin gets 0 / 0 = NaN.  profile: fp64[n_users][n_bins].                                */
int n2v_ecccons_profile(const int64_t* user_ptr, const int64_t* perm, int64_t n_users, const int64_t* item,
                        const double* feedback, int64_t n_rows, const int32_t* item_bin, int64_t n_items, int32_t n_bins,
                        int32_t weighted, double* profile, void* stream);

/* rows[0 .. *count): the rows k whose item has a vector (vec_slot[item[k]] in 0 .. n_vec - 1; vec_slot NULL: every row),
 * ascending; y[slot] = feedback[k].  rows / y hold n_rows words.                                                    */
int n2v_ecccons_feature_rows(const int64_t* item, const double* feedback, int64_t n_rows, int64_t n_items,
                             const int32_t* vec_slot, int64_t n_vec, int64_t* scratch, int64_t* rows, double* y,
                             int64_t* count, void* stream);
/* X[t] = profile[user[k]] ++ vec[vec_slot[item[k]]] widened to fp64 (row length n_bins + d), or, with vec NULL,
 * profile[user[k]] ++ [item_value[item[k]]] (row length n_bins + 1), k = rows[t], t < n_kept.  One wavefront per row;
 * 16-byte accesses when n_bins, the row length and the pointers allow.                                             */
int n2v_ecccons_features(const int64_t* rows, int64_t n_kept, const int64_t* user, const int64_t* item, int64_t n_rows,
                         int64_t n_users, int64_t n_items, const double* profile, int32_t n_bins, const int32_t* vec_slot,
                         const float* vec, int64_t n_vec, int32_t d, const double* item_value, double* X, void* stream);

/* ---- Random forests on binned features (csrc/n2v_forest.hip) -----
 * The regressor and the entropy classifier of src/main_ecc.py:160-202 on the rows n2v_ecccons_features writes.  The
 * definition is tests/forest_reference.py: fp64 features go to uint8 bins, a tree grows level by level
 * from per-(node, feature) histograms whose channels are integers (draw counts, counts times round(y * 2^y_bits), class
 * counts), and the score of a split is computed from those integers in a stated fp64 order.  Workgroups meet only through
 * integer atomic adds and at launch boundaries, so two fits give the same bytes.  Samples stay partitioned by node:
 * order[p] is the sample at position p and the frontier node m of a level owns the positions seg[m] .. seg[m + 1); no
 * segment is empty.  Node ids are breadth first inside a tree; left[v] is -1 at a leaf and the right child is left[v] + 1.
 * Limits, refused with N2V_ERR_INVALID before anything is launched: n < 2^31, features <= N2V_FOREST_MAX_FEATURES, bins
 * 2 .. N2V_FOREST_MAX_BINS, classes 2 .. N2V_FOREST_MAX_CLASSES (0: the regressor), depth <= N2V_FOREST_MAX_DEPTH.  The
 * kernels trust bins < n_bins, classes < n_classes and the tree tables: the check functions below tell the caller, through
 * the bits of one int32 device word, that a value is outside its range, and the caller runs them first.               */
#define N2V_FOREST_MAX_FEATURES 4096
#define N2V_FOREST_MAX_BINS 256
#define N2V_FOREST_MAX_CLASSES 32
#define N2V_FOREST_MAX_DEPTH 32
#define N2V_FOREST_PIECE 2048                        /* positions per workgroup of the histogram kernel             */
#define N2V_FOREST_HIST_LDS 65536                    /* bytes of LDS a histogram workgroup may take                 */
#define N2V_FOREST_STREAM_BOOT 0                     /* last Philox counter word: bootstrap draws / feature keys    */
#define N2V_FOREST_STREAM_FEAT 1
#define N2V_FOREST_BAD_NAN 1                         /* status bits                                                 */
#define N2V_FOREST_BAD_BIN 2
#define N2V_FOREST_BAD_CLASS 4
#define N2V_FOREST_BAD_FEATURE 8
#define N2V_FOREST_BAD_CHILD 16
#define N2V_FOREST_BAD_TARGET 32

/* Features per histogram workgroup: the largest power of two <= 64 whose tile x n_bins cells fit N2V_FOREST_HIST_LDS
 * (a cell: int32 count + int64 sum, or n_classes int32 counts).  0 for an argument outside its range.               */
int32_t n2v_forest_feature_tile(int32_t n_bins, int32_t n_classes);
/* HOST: table[a] = a * log(a) by the host's libm, table[0] = 0, a < len.                                             */
int n2v_forest_glog_table(int64_t len, double* table);
/* *status |= BAD_NAN for a NaN in x[count]; BAD_BIN for a bin >= n_bins; BAD_CLASS for a class outside 0 .. n_classes - 1. */
int n2v_forest_check_x(const double* x, int64_t count, int32_t* status, void* stream);
int n2v_forest_check_bins(const uint8_t* bins, int64_t count, int32_t n_bins, int32_t* status, void* stream);
int n2v_forest_check_classes(const int32_t* cls, int64_t count, int32_t n_classes, int32_t* status, void* stream);
/* The tables of n_trees trees, tree t at tree_ptr[t] .. tree_ptr[t + 1) (the caller has checked tree_ptr on the host).  At
 * every node with left != -1: BAD_CHILD unless node < left and left + 1 < the tree's size, BAD_FEATURE unless feature is in
 * 0 .. n_features - 1, BAD_BIN unless threshold is in 0 .. n_bins - 1.                                                */
int n2v_forest_check_tree(const int32_t* feature, const int32_t* threshold, const int32_t* left, const int64_t* tree_ptr,
                          int32_t n_trees, int64_t n_nodes, int32_t n_features, int32_t n_bins, int32_t* status, void* stream);
/* xs: fp64[n_features][n], every row sorted ascending, no NaN.  edges: fp64[n_features][n_bins - 1], the first
 * n_edges[f] of row f ascending: the distinct values but the first when there are at most n_bins, else the distinct ones
 * among xs[(b * n) / n_bins], b = 1 .. n_bins - 1.                                                                    */
int n2v_forest_edges(const double* xs, int64_t n, int32_t n_features, int32_t n_bins, double* edges, int32_t* n_edges, void* stream);
/* bins[i][f] = the number of edges of f that are <= x[i][f] (uint8[n][n_features]); a NaN sets BAD_NAN and bin 0.      */
int n2v_forest_bin(const double* x, int64_t n, int32_t n_features, int32_t n_bins, const double* edges, const int32_t* n_edges,
                   uint8_t* bins, int32_t* status, void* stream);
/* w[i] = the draws k < n of tree `tree` with (philox4x32_10(seed; k lo, k hi, tree, STREAM_BOOT)[0] * n) >> 32 == i.    */
int n2v_forest_bootstrap(uint64_t seed, int32_t tree, int64_t n, int32_t* w, void* stream);
/* yq[i] = (int64) rint(y[i] * 2^y_bits), *max_abs = the largest |yq| (one int64 device word); BAD_TARGET for a y that
 * is not finite or whose yq reaches 2^53.                                                                            */
int n2v_forest_quantise(const double* y, int64_t n, int32_t y_bits, int64_t* yq, int64_t* max_abs, int32_t* status, void* stream);
/* keys[m][j] = (philox4x32_10(seed; node_id0 + m, j, tree, STREAM_FEAT)[0] << 12) | j, int64[nodes][n_features]: sorted
 * along a row, the max_features-th smallest is the key_limit of n2v_forest_split.                                     */
int n2v_forest_feature_keys(uint64_t seed, int32_t tree, int32_t node_id0, int32_t nodes, int32_t n_features, int64_t* keys,
                            void* stream);
/* The histograms of the frontier nodes node0 .. node1 - 1 over the features 0 .. f_count - 1 (zeroed first):
 * regressor (n_classes == 0) int64[node][feature][bin][2] = (sum of w, sum of w * yq); classifier
 * int32[node][feature][bin][class] = sum of w.  bins: uint8[n][n_features]; n_positions = seg[node1] - seg[node0].     */
int n2v_forest_hist(const uint8_t* bins, int64_t n, int32_t n_features, int32_t f_count, int32_t n_bins, int32_t n_classes,
                    const int32_t* order, const int32_t* seg, int32_t node0, int32_t node1, int64_t n_positions, const int32_t* w,
                    const int64_t* yq, const int32_t* cls, void* hist, void* stream);
/* The best split of each of `nodes` nodes from their histograms, node m having the id node_id0 + m: writes feature /
 * threshold (-1 at a leaf), left = -1, value (fp64[id] or fp64[id][n_classes]) and split[m] = 1 where the node splits.
 * key_limit: NULL for every feature, else int64[nodes].  leaf_only: every node is a leaf (f_count may then be 1).
 * best_score / best_thr: scratch [nodes][f_count]; node_count / node_parent: scratch [nodes].                         */
int n2v_forest_split(const void* hist, int32_t nodes, int32_t f_count, int32_t n_bins, int32_t n_classes, int32_t min_samples_split,
                     int32_t min_samples_leaf, int32_t leaf_only, const double* gtab, int64_t gtab_len, uint64_t seed, int32_t tree,
                     int32_t node_id0, const int64_t* key_limit, int32_t y_bits, double* best_score, int32_t* best_thr,
                     int64_t* node_count, double* node_parent, int32_t* feature, int32_t* threshold, int32_t* left, double* value,
                     int32_t* split, void* stream);
/* flags: int32[2][n_positions]: flags[0][p] = 1 where position p belongs to a splitting node and goes left,
 * flags[1][p] = 1 where it goes right.                                                                                */
int n2v_forest_route_flags(const uint8_t* bins, int64_t n, int32_t n_features, const int32_t* order, const int32_t* seg, int32_t n_seg,
                           int64_t n_positions, const int32_t* split, const int32_t* feature, const int32_t* threshold,
                           int32_t node_id0, int32_t* flags, void* stream);
/* sums: the inclusive scan of flags along each row; rank: the inclusive scan of split; n_split its total, n_next the
 * number of flagged positions.  Writes the stable partition of every splitting node's segment to new_order, the children's
 * segments to new_seg[2 * n_split + 1] and left[node_id0 + m] = next_id0 + 2 * (rank[m] - 1).                         */
int n2v_forest_route_scatter(const int32_t* order, const int32_t* seg, int32_t n_seg, int64_t n_positions, const int32_t* split,
                             const int32_t* rank, const int32_t* flags, const int32_t* sums, int32_t node_id0, int32_t next_id0,
                             int32_t n_split, int64_t n_next, int32_t* left, int32_t* new_order, int32_t* new_seg, void* stream);
/* out[i][c] = (the sum over the trees, in ascending order from +0.0, of value[leaf of i][c]) / n_trees; width: 1 or the
 * number of classes; a walk takes at most max_depth steps.  The tables have passed n2v_forest_check_tree.             */
int n2v_forest_predict(const uint8_t* bins, int64_t n, int32_t n_features, const int32_t* feature, const int32_t* threshold,
                       const int32_t* left, const double* value, const int64_t* tree_ptr, int32_t n_trees, int32_t width,
                       int32_t max_depth, double* out, void* stream);
/* out[i] = the first maximum of proba[i][0 .. n_classes).                                                             */
int n2v_forest_argmax(const double* proba, int64_t n, int32_t n_classes, int32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
