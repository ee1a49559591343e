// Eccentricity consistency: two-period join -> n x n transition table; per-user ie profile -> feature rows — gfx950 (MI355X).
// C-ABI: include/n2v_sim.h.
//
// Reference: src/utils.py:163-226 (septile_for_plot: the merges on id / uid, the support filter unum > 4, the group-by
// of the two septile columns and its row sums) and :326-379 (calculate_uie_dist, calculate_uvec, make_data).
//   check     integer inputs: a range check and a CSR pointer check that set bits of a status word.
//   join      the stable compaction of n2v_compact.h over the entities present in both periods above the support.
//   crosstab  per-workgroup int32 histogram in LDS (16 KiB, all n x n cells up to n = 64, stripes of bins1 above),
//             flushed by 64-bit integer atomic adds: integer adds commute, the table is exact and the same on every run.
//             count_sum and ratio come from a one-workgroup kernel after the counts are complete.
//   profile   one wavefront per user: per-bin counts by LDS integer atomics; the weighted form adds the feedback of the
//             user's rows one after the other, lane b % 64 owning bin b, so every sum runs in row order.
//   features  one wavefront per kept row: profile[user] ++ item vector (fp32 widened) or ++ the item's number.
// Every kernel checks the indices it follows and skips what is outside: a malformed input never leaves its buffers.
#include "n2v_common.h"
#include "n2v_compact.h"
#include "n2v_sim.h"

namespace {

constexpr int64_t LIMIT = 0x7fffffff;                    // every size is below 2^31
constexpr int MAX_BINS = N2V_ECCCONS_MAX_BINS;
constexpr int CELLS = N2V_ECCCONS_CELLS;
constexpr int CHUNK = N2V_ECCCONS_CHUNK;

bool small(int64_t v) { return v >= 1 && v <= LIMIT; }

// ---- checks -----------------------------------------------------------------------------------------------------------

template <class T>
__global__ void __launch_bounds__(256) range_kernel(const T* __restrict__ a, int64_t n, T lo, T hi, int32_t* status) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = k < n && (a[k] < lo || a[k] > hi);
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, N2V_ECCCONS_BAD_RANGE);
}

__global__ void __launch_bounds__(256) ptr_kernel(const int64_t* __restrict__ ptr, int64_t n_seg, int64_t total, int32_t* status) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (k < n_seg) bad = ptr[k] > ptr[k + 1];
    if (k == 0) bad = bad || ptr[0] != 0 || ptr[n_seg] != total;
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, N2V_ECCCONS_BAD_PTR);
}

// ---- join ---------------------------------------------------------------------------------------------------------------

struct JoinP {
    const int64_t* v1; const int64_t* v2; const int64_t* c1; const int64_t* c2; int64_t min_count;
    int64_t* ids; int64_t* o1; int64_t* o2;
    __device__ bool test(int64_t e) const {
        const int64_t a = c1[e], b = c2[e];
        return a > 0 && b > 0 && a > min_count && b > min_count;
    }
    __device__ void emit(int64_t e, int64_t slot) const { ids[slot] = e; o1[slot] = v1[e]; o2[slot] = v2[e]; }
    __device__ void skip(int64_t) const {}
};

// ---- crosstab -----------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) crosstab_kernel(const int32_t* __restrict__ bins1, const int32_t* __restrict__ bins2, int64_t m,
                                                       int n, int stripe, unsigned long long* __restrict__ count) {
    __shared__ int cell[CELLS];
    const int t = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * CHUNK, hi = lo + CHUNK < m ? lo + CHUNK : m;
    for (int r0 = 0; r0 < n; r0 += stripe) {                             // values r0 + 1 .. r0 + rows of bins1
        const int rows = stripe < n - r0 ? stripe : n - r0, used = rows * n;
        for (int c = t; c < used; c += 256) cell[c] = 0;
        __syncthreads();
        for (int64_t k = lo + t; k < hi; k += 256) {
            const int a = bins1[k], b = bins2[k];
            if (a > r0 && a <= r0 + rows && b >= 1 && b <= n) atomicAdd(&cell[(a - 1 - r0) * n + (b - 1)], 1);
        }
        __syncthreads();
        for (int c = t; c < used; c += 256) {
            const int v = cell[c];
            if (v) atomicAdd(count + (int64_t)r0 * n + c, (unsigned long long)v);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) ratio_kernel(const int64_t* __restrict__ count, int n, int64_t* __restrict__ count_sum,
                                                    double* __restrict__ ratio) {
    __shared__ int64_t sum[MAX_BINS];
    const int t = threadIdx.x;
    if (t < n) {
        int64_t s = 0;
        for (int c = 0; c < n; ++c) s += count[t * n + c];
        sum[t] = s;
        count_sum[t] = s;
    }
    __syncthreads();
    for (int c = t; c < n * n; c += 256) ratio[c] = (double)count[c] * 1.0 / (double)sum[c / n];     // 0 / 0: NaN
}

// ---- profile ------------------------------------------------------------------------------------------------------------

struct ProfileArgs {
    const int64_t* user_ptr; const int64_t* perm; int64_t n_users; const int64_t* item; const double* feedback; int64_t n_rows;
    const int32_t* item_bin; int64_t n_items; int n_bins; int weighted; double* profile;
};

__global__ void __launch_bounds__(256) profile_kernel(ProfileArgs a) {
    __shared__ int cnt[4][MAX_BINS];
    __shared__ double sum[4][MAX_BINS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t u = (int64_t)blockIdx.x * 4 + wave;
    const bool live = u < a.n_users;
    int64_t lo = 0, hi = 0;
    if (live) {
        lo = a.user_ptr[u]; hi = a.user_ptr[u + 1];
        lo = lo < 0 ? 0 : (lo < a.n_rows ? lo : a.n_rows);
        hi = hi < lo ? lo : (hi < a.n_rows ? hi : a.n_rows);
    }
    for (int b = lane; b < a.n_bins; b += 64) { cnt[wave][b] = 0; sum[wave][b] = 0.0; }
    __syncthreads();
    int kept = 0;
    double total = 0.0;                                                  // the same in every lane
    for (int64_t base = lo; base < hi; base += 64) {
        const int64_t k = base + lane;
        int b = 0;
        double f = 0.0;
        if (k < hi) {
            const int64_t row = a.perm[k];
            if (row >= 0 && row < a.n_rows) {
                const int64_t it = a.item[row];
                if (it >= 0 && it < a.n_items) {
                    const int x = a.item_bin[it];
                    if (x >= 1 && x <= a.n_bins) { b = x; f = a.feedback[row]; }
                }
            }
        }
        if (b) { atomicAdd(&cnt[wave][b - 1], 1); ++kept; }
        if (a.weighted) {
            const int len = hi - base < 64 ? (int)(hi - base) : 64;
            for (int j = 0; j < len; ++j) {                              // the user's rows one after the other
                const int bj = __shfl(b, j);
                const double fj = __shfl(f, j);
                if (bj) {
                    total = total + fj;
                    if (((bj - 1) & 63) == lane) sum[wave][bj - 1] = sum[wave][bj - 1] + fj;
                }
            }
        }
    }
    for (int o = 32; o; o >>= 1) kept += __shfl_xor(kept, o);
    __syncthreads();
    if (!live) return;
    double* out = a.profile + u * a.n_bins;
    for (int b = lane; b < a.n_bins; b += 64)
        out[b] = a.weighted ? sum[wave][b] / total : (double)cnt[wave][b] / (double)kept;            // 0 / 0: NaN
}

// ---- features -----------------------------------------------------------------------------------------------------------

struct RowsP {
    const int64_t* item; const int64_t* fb; int64_t n_items; const int32_t* vec_slot; int64_t n_vec; int64_t* rows; int64_t* y;
    __device__ bool test(int64_t k) const {
        const int64_t it = item[k];
        if (it < 0 || it >= n_items) return false;
        if (!vec_slot) return true;
        const int64_t s = vec_slot[it];
        return s >= 0 && s < n_vec;
    }
    __device__ void emit(int64_t k, int64_t slot) const { rows[slot] = k; y[slot] = fb[k]; }
    __device__ void skip(int64_t) const {}
};

struct FeatArgs {
    const int64_t* rows; int64_t n_kept; const int64_t* user; const int64_t* item; int64_t n_rows; int64_t n_users; int64_t n_items;
    const double* profile; int n_bins; const int32_t* vec_slot; const float* vec; int64_t n_vec; int d; const double* item_value;
    double* X; int wide;
};

__global__ void __launch_bounds__(256) features_kernel(FeatArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.n_kept) return;
    const int64_t k = a.rows[t];
    if (k < 0 || k >= a.n_rows) return;
    const int64_t u = a.user[k], it = a.item[k];
    if (u < 0 || u >= a.n_users || it < 0 || it >= a.n_items) return;
    const int tail = a.vec ? a.d : 1;
    const double* src = a.profile + u * a.n_bins;
    double* dst = a.X + t * (a.n_bins + tail);
    if (!a.vec) {
        for (int j = lane; j < a.n_bins; j += 64) dst[j] = src[j];
        if (lane == 0) dst[a.n_bins] = a.item_value[it];
        return;
    }
    const int64_t s = a.vec_slot[it];
    if (s < 0 || s >= a.n_vec) return;
    const float* v = a.vec + s * a.d;
    if (a.wide) {                                                        // n_bins and d even, every base 16-byte aligned
        const double2* src2 = reinterpret_cast<const double2*>(src);
        double2* dst2 = reinterpret_cast<double2*>(dst);
        const float2* v2 = reinterpret_cast<const float2*>(v);
        const int h = a.n_bins / 2;
        for (int j = lane; j < h; j += 64) dst2[j] = src2[j];
        for (int j = lane; j < a.d / 2; j += 64) { const float2 x = v2[j]; dst2[h + j] = make_double2((double)x.x, (double)x.y); }
    } else {
        for (int j = lane; j < a.n_bins; j += 64) dst[j] = src[j];
        for (int j = lane; j < a.d; j += 64) dst[a.n_bins + j] = (double)v[j];
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int n2v_ecccons_check_i32(const int32_t* a, int64_t n, int32_t lo, int32_t hi, int32_t* status, void* stream) {
    if (n == 0) return N2V_OK;
    if (!small(n)) return n2v::fail(N2V_ERR_INVALID, "ecccons_check_i32: n=%lld (0 .. 2^31-1)", (long long)n);
    if (!a || !status) return n2v::fail(N2V_ERR_INVALID, "ecccons_check_i32: null pointer");
    range_kernel<int32_t><<<n2v::grid_for(n, 256), 256, 0, (hipStream_t)stream>>>(a, n, lo, hi, status);
    return n2v::check_launch("ecccons_check_i32");
}

int n2v_ecccons_check_i64(const int64_t* a, int64_t n, int64_t lo, int64_t hi, int32_t* status, void* stream) {
    if (n == 0) return N2V_OK;
    if (!small(n)) return n2v::fail(N2V_ERR_INVALID, "ecccons_check_i64: n=%lld (0 .. 2^31-1)", (long long)n);
    if (!a || !status) return n2v::fail(N2V_ERR_INVALID, "ecccons_check_i64: null pointer");
    range_kernel<int64_t><<<n2v::grid_for(n, 256), 256, 0, (hipStream_t)stream>>>(a, n, lo, hi, status);
    return n2v::check_launch("ecccons_check_i64");
}

int n2v_ecccons_check_ptr(const int64_t* ptr, int64_t n_seg, int64_t total, int32_t* status, void* stream) {
    if (!small(n_seg) || total < 0 || total > LIMIT)
        return n2v::fail(N2V_ERR_INVALID, "ecccons_check_ptr: n_seg=%lld total=%lld", (long long)n_seg, (long long)total);
    if (!ptr || !status) return n2v::fail(N2V_ERR_INVALID, "ecccons_check_ptr: null pointer");
    ptr_kernel<<<n2v::grid_for(n_seg, 256), 256, 0, (hipStream_t)stream>>>(ptr, n_seg, total, status);
    return n2v::check_launch("ecccons_check_ptr");
}

int n2v_ecccons_join(const double* v1, const double* v2, const int64_t* c1, const int64_t* c2, int64_t n, int64_t min_count,
                     int64_t* scratch, int64_t* ids, double* o1, double* o2, int64_t* count, void* stream) {
    if (!count) return n2v::fail(N2V_ERR_INVALID, "ecccons_join: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int64_t), s) != hipSuccess) return n2v::fail(N2V_ERR_HIP, "ecccons_join: memset failed");
        return N2V_OK;
    }
    if (!small(n) || min_count < 0) return n2v::fail(N2V_ERR_INVALID, "ecccons_join: n=%lld min_count=%lld", (long long)n, (long long)min_count);
    if (!v1 || !v2 || !c1 || !c2 || !scratch || !ids || !o1 || !o2) return n2v::fail(N2V_ERR_INVALID, "ecccons_join: null pointer");
    n2v::compact(JoinP{reinterpret_cast<const int64_t*>(v1), reinterpret_cast<const int64_t*>(v2), c1, c2, min_count, ids,
                       reinterpret_cast<int64_t*>(o1), reinterpret_cast<int64_t*>(o2)}, n, scratch, count, s);
    return n2v::check_launch("ecccons_join");
}

int n2v_ecccons_crosstab(const int32_t* bins1, const int32_t* bins2, int64_t m, int32_t n_bins, int64_t* count,
                         int64_t* count_sum, double* ratio, void* stream) {
    if (m < 0 || m > LIMIT || n_bins < 1 || n_bins > MAX_BINS)
        return n2v::fail(N2V_ERR_INVALID, "ecccons_crosstab: m=%lld n_bins=%d (1 .. %d)", (long long)m, n_bins, MAX_BINS);
    if (!count || !count_sum || !ratio || (m && (!bins1 || !bins2))) return n2v::fail(N2V_ERR_INVALID, "ecccons_crosstab: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, sizeof(int64_t) * n_bins * n_bins, s) != hipSuccess)
        return n2v::fail(N2V_ERR_HIP, "ecccons_crosstab: memset failed");
    const int stripe = n_bins <= 64 ? n_bins : CELLS / n_bins;           // stripe * n_bins <= CELLS
    if (m)
        crosstab_kernel<<<n2v::grid_for(m, CHUNK), 256, 0, s>>>(bins1, bins2, m, n_bins, stripe, reinterpret_cast<unsigned long long*>(count));
    ratio_kernel<<<1, 256, 0, s>>>(count, n_bins, count_sum, ratio);
    return n2v::check_launch("ecccons_crosstab");
}

int n2v_ecccons_profile(const int64_t* user_ptr, const int64_t* perm, int64_t n_users, const int64_t* item,
                        const double* feedback, int64_t n_rows, const int32_t* item_bin, int64_t n_items, int32_t n_bins,
                        int32_t weighted, double* profile, void* stream) {
    if (n_users == 0) return N2V_OK;
    if (!small(n_users) || n_rows < 0 || n_rows > LIMIT || !small(n_items) || n_bins < 1 || n_bins > MAX_BINS)
        return n2v::fail(N2V_ERR_INVALID, "ecccons_profile: n_users=%lld n_rows=%lld n_items=%lld n_bins=%d (1 .. %d)",
                         (long long)n_users, (long long)n_rows, (long long)n_items, n_bins, MAX_BINS);
    if (!user_ptr || !item_bin || !profile || (n_rows && (!perm || !item || !feedback)))
        return n2v::fail(N2V_ERR_INVALID, "ecccons_profile: null pointer");
    ProfileArgs a{user_ptr, perm, n_users, item, feedback, n_rows, item_bin, n_items, n_bins, weighted != 0, profile};
    profile_kernel<<<n2v::grid_for(n_users, 4), 256, 0, (hipStream_t)stream>>>(a);
    return n2v::check_launch("ecccons_profile");
}

int n2v_ecccons_feature_rows(const int64_t* item, const double* feedback, int64_t n_rows, int64_t n_items,
                             const int32_t* vec_slot, int64_t n_vec, int64_t* scratch, int64_t* rows, double* y,
                             int64_t* count, void* stream) {
    if (!count) return n2v::fail(N2V_ERR_INVALID, "ecccons_feature_rows: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int64_t), s) != hipSuccess) return n2v::fail(N2V_ERR_HIP, "ecccons_feature_rows: memset failed");
        return N2V_OK;
    }
    if (!small(n_rows) || !small(n_items) || n_vec < 0 || n_vec > LIMIT)
        return n2v::fail(N2V_ERR_INVALID, "ecccons_feature_rows: n_rows=%lld n_items=%lld n_vec=%lld", (long long)n_rows,
                         (long long)n_items, (long long)n_vec);
    if (!item || !feedback || !scratch || !rows || !y) return n2v::fail(N2V_ERR_INVALID, "ecccons_feature_rows: null pointer");
    n2v::compact(RowsP{item, reinterpret_cast<const int64_t*>(feedback), n_items, vec_slot, n_vec, rows, reinterpret_cast<int64_t*>(y)},
                 n_rows, scratch, count, s);
    return n2v::check_launch("ecccons_feature_rows");
}

int n2v_ecccons_features(const int64_t* rows, int64_t n_kept, const int64_t* user, const int64_t* item, int64_t n_rows,
                         int64_t n_users, int64_t n_items, const double* profile, int32_t n_bins, const int32_t* vec_slot,
                         const float* vec, int64_t n_vec, int32_t d, const double* item_value, double* X, void* stream) {
    if (n_kept == 0) return N2V_OK;
    if (!small(n_kept) || n_kept > n_rows || !small(n_rows) || !small(n_users) || !small(n_items) || n_bins < 1 || n_bins > MAX_BINS)
        return n2v::fail(N2V_ERR_INVALID, "ecccons_features: n_kept=%lld n_rows=%lld n_users=%lld n_items=%lld n_bins=%d",
                         (long long)n_kept, (long long)n_rows, (long long)n_users, (long long)n_items, n_bins);
    if (!rows || !user || !item || !profile || !X) return n2v::fail(N2V_ERR_INVALID, "ecccons_features: null pointer");
    if (vec ? (!vec_slot || d < 1 || d > 65536 || n_vec < 1 || n_vec > LIMIT) : !item_value)
        return n2v::fail(N2V_ERR_INVALID, "ecccons_features: item vectors need vec_slot, 1 <= d <= 65536 and n_vec >= 1; without them item_value");
    const int len = n_bins + (vec ? d : 1);
    if (n_kept * len > (int64_t)1 << 40) return n2v::fail(N2V_ERR_INVALID, "ecccons_features: %lld x %d values", (long long)n_kept, len);
    const int wide = vec && n_bins % 2 == 0 && d % 2 == 0 && aligned16(profile) && aligned16(vec) && aligned16(X);
    FeatArgs a{rows, n_kept, user, item, n_rows, n_users, n_items, profile, n_bins, vec_slot, vec, n_vec, vec ? d : 0, item_value, X, wide};
    features_kernel<<<n2v::grid_for(n_kept, 4), 256, 0, (hipStream_t)stream>>>(a);
    return n2v::check_launch("ecccons_features");
}

}  // extern "C"
