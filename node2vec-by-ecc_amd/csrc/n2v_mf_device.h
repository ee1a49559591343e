// Device steps shared by the factor-model kernels (n2v_svd.hip, n2v_nmf.hip): a factor row spread over the 64 lanes of a
// wavefront, lane l owning the factors l + 64 * k, k < NS, and the dot of the definition (include/n2v_sim.h, "Matrix
// factorisation").  One copy, so that every kernel that estimates a rating rounds the same way.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace n2v {

constexpr int MF_MAX_FACTORS = 256;                               // four factors a lane

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int NS>
__device__ __forceinline__ void load_row(const double* row, int nf, int lane, double (&x)[NS]) {
#pragma unroll
    for (int k = 0; k < NS; ++k) x[k] = lane + 64 * k < nf ? row[lane + 64 * k] : 0.0;
}

template <int NS>
__device__ __forceinline__ void store_row(double* row, int nf, int lane, const double (&x)[NS]) {
#pragma unroll
    for (int k = 0; k < NS; ++k)
        if (lane + 64 * k < nf) row[lane + 64 * k] = x[k];
}

// The dot of the definition; every lane returns the same value.
template <int NS>
__device__ __forceinline__ double lane_dot(const double (&q)[NS], const double (&p)[NS], int nf, int lane) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < NS; ++k)
        if (lane + 64 * k < nf) v = v + q[k] * p[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

}  // namespace n2v

// KERNEL<NS> for the number of 64-lane slots that n_factors needs
#define N2V_MF_DISPATCH(KERNEL, nf, ...)                                      \
    do {                                                                      \
        if ((nf) <= 64) KERNEL<1> __VA_ARGS__;                                \
        else if ((nf) <= 128) KERNEL<2> __VA_ARGS__;                          \
        else if ((nf) <= 192) KERNEL<3> __VA_ARGS__;                          \
        else KERNEL<4> __VA_ARGS__;                                           \
    } while (0)
