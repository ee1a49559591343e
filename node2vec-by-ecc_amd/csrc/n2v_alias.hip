// Alias-table construction — gfx950 (MI355X) kernels.
//
// Replaces alias_setup and the node tables of preprocess_transition_probs of the reference
// (src/node2vec.py:240-269, :184-188).  Results are bit-identical to the
// reference: fp64 throughout, the neighbourhood sum is the plain left-to-right sum of
// Python's sum() (:149,:186), probabilities are divide-then-multiply (:150,:253), and
// Vose's pairing pops both stacks from their most recently pushed end (:259-268).  That
// pairing is serial per table, so one lane builds one table (node tables and caller-given
// tables; the edge tables are built one wavefront per table, n2v_tables.hip).
// The two stacks live in the `aux` word of the table's own slots (smaller grows up from
// slot 0, larger grows down from slot K-1; together they never hold more than K indices),
// so construction needs no scratch memory beyond the output.
//
// Compile with -ffp-contract=off: no fused multiply-add may replace the reference's
// separately rounded operations.
#include "n2v_common.h"
#include "n2v_vose.h"

namespace {

// On entry T[k].q holds the normalised probability of slot k (src/node2vec.py:150/187).
// The pairing itself (register-carried, reference-exact) is in n2v_vose.h.
__device__ __forceinline__ void vose_inplace(n2v_alias_slot* __restrict__ T, int64_t K) {
    n2v::vose_pair<n2v::kProb>(T, K);
}

__global__ void __launch_bounds__(256)
setup_tables_kernel(int64_t n_tables, const int64_t* __restrict__ tab_off, n2v_alias_slot* __restrict__ slots) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tables) return;
    vose_inplace(slots + tab_off[i], tab_off[i + 1] - tab_off[i]);
}

__global__ void __launch_bounds__(256)
node_tables_kernel(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const double* __restrict__ w,
                   n2v_alias_slot* __restrict__ slots, int32_t* __restrict__ status) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_nodes) return;
    const int64_t b = row_ptr[v], K = row_ptr[v + 1] - b;
    if (K == 0) return;
    n2v_alias_slot* T = slots + b;
    double norm = 0.0;
    for (int64_t k = 0; k < K; ++k) norm = norm + (w ? w[b + k] : 1.0);  // sum(), :186
    if (norm == 0.0) {
        atomicOr(status, N2V_STATUS_ZERO_NORM);
        return;
    }
    for (int64_t k = 0; k < K; ++k) T[k].q = (w ? w[b + k] : 1.0);
    n2v::vose_pair<n2v::kWeight>(T, K, norm);  // prob = u / norm (:187), q = K * prob (:253), pairing
}

// The pop node tables of preprocess_transition_probs_popularity / get_alias_nodes_cur with popwalk == "pop"
// (src/node2vec.py:13-25, :213-221): weight * 1.0 / len(G[nbr]) — or the plain weight when plain[v] is set (a node whose
// label starts with 9999999, :18, :215; the test looks at v, not at the neighbour).  Nodes [v_begin, v_end); the table of v
// lands at slots[row_ptr[v] - row_ptr[v_begin]], so the same kernel serves all nodes (v_begin = 0) and one table on demand.
__global__ void __launch_bounds__(256)
node_tables_pop_kernel(int64_t v_begin, int64_t v_end, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                       const double* __restrict__ w, const uint8_t* __restrict__ plain, n2v_alias_slot* __restrict__ slots,
                       int32_t* __restrict__ status) {
    const int64_t v = v_begin + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= v_end) return;
    const int64_t b = row_ptr[v], K = row_ptr[v + 1] - b;
    if (K == 0) return;
    n2v_alias_slot* T = slots + (b - row_ptr[v_begin]);
    const bool exempt = plain[v] != 0;
    double norm = 0.0;
    for (int64_t k = 0; k < K; ++k) {
        double u = w ? w[b + k] : 1.0;
        if (!exempt) {
            const int32_t nb = col[b + k];
            const int64_t pop = row_ptr[nb + 1] - row_ptr[nb];
            if (pop == 0) {                      // ZeroDivisionError in the reference (:21, :218)
                atomicOr(status, N2V_STATUS_ZERO_POP);
                return;
            }
            u = u / (double)pop;                 // w * 1.0 is w
        }
        T[k].q = u;
        norm = norm + u;                         // sum(), :22 / :219
    }
    if (norm == 0.0 || norm != norm) {
        atomicOr(status, N2V_STATUS_ZERO_NORM);
        return;
    }
    n2v::vose_pair<n2v::kWeight>(T, K, norm);
}

}  // namespace

extern "C" int n2v_alias_setup_tables(int64_t n_tables, const int64_t* tab_off, n2v_alias_slot* slots, void* stream) {
    if (n_tables < 0) return n2v::fail(N2V_ERR_INVALID, "n2v_alias_setup_tables: negative count");
    if (n_tables == 0) return N2V_OK;
    if (!tab_off || !slots) return n2v::fail(N2V_ERR_INVALID, "n2v_alias_setup_tables: null pointer");
    hipLaunchKernelGGL(setup_tables_kernel, dim3(n2v::grid_for(n_tables, 256)), dim3(256), 0, (hipStream_t)stream,
                       n_tables, tab_off, slots);
    return n2v::check_launch("n2v_alias_setup_tables");
}

extern "C" int n2v_build_node_tables(int64_t n_nodes, const int64_t* row_ptr, const int32_t* col, const double* w,
                                     n2v_alias_slot* slots, int32_t* status, void* stream) {
    (void)col;
    if (n_nodes < 0 || !row_ptr || !status)
        return n2v::fail(N2V_ERR_INVALID, "n2v_build_node_tables: null pointer or negative size");
    if (n_nodes == 0) return N2V_OK;
    if (!slots) return n2v::fail(N2V_ERR_INVALID, "n2v_build_node_tables: null slots");
    hipLaunchKernelGGL(node_tables_kernel, dim3(n2v::grid_for(n_nodes, 256)), dim3(256), 0, (hipStream_t)stream,
                       n_nodes, row_ptr, w, slots, status);
    return n2v::check_launch("n2v_build_node_tables");
}

extern "C" int n2v_build_node_tables_pop(int64_t v_begin, int64_t v_end, const int64_t* row_ptr, const int32_t* col,
                                         const double* w, const uint8_t* plain, n2v_alias_slot* slots, int32_t* status,
                                         void* stream) {
    if (v_begin < 0 || v_end < v_begin || !row_ptr || !status)
        return n2v::fail(N2V_ERR_INVALID, "n2v_build_node_tables_pop: null pointer or bad node range");
    if (v_end == v_begin) return N2V_OK;
    if (!slots || !col || !plain) return n2v::fail(N2V_ERR_INVALID, "n2v_build_node_tables_pop: null pointer");
    hipLaunchKernelGGL(node_tables_pop_kernel, dim3(n2v::grid_for(v_end - v_begin, 256)), dim3(256), 0, (hipStream_t)stream,
                       v_begin, v_end, row_ptr, col, w, plain, slots, status);
    return n2v::check_launch("n2v_build_node_tables_pop");
}

extern "C" int n2v_abi_version(void) { return N2V_ABI_VERSION; }
extern "C" const char* n2v_last_error(void) { return n2v::err_buf(); }
