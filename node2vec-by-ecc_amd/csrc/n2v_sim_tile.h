// The 128x128 fp32 MFMA score tile shared by sim_mfma_kernel (n2v_sim.hip) and knn_tile_kernel (n2v_knn.hip) — gfx950.
//
// 128x128 scores per workgroup of 256 threads, 64x64 per wavefront as 2x2 blocks of v_mfma_f32_32x32x2_f32 (fp32 in, fp32
// accumulate: the reference's float32 dot, no reduced precision).  Operands staged k-major through LDS; per k-pair a wave
// issues 4 LDS reads for 4 MFMAs (8 192 FMAs).  Operand layout of the instruction: lane l supplies A[m = l % 32][k = l / 32]
// and B[k = l / 32][n = l % 32]; accumulator register v of lane l holds D[8 * (v / 4) + 4 * (l / 32) + (v % 4)][l % 32].
//
// A score is a function of its two rows and dpad alone: the accumulator starts at +0.0 and k runs 0 .. dpad - 1 in one fixed
// order, whatever the tile's position, the grid or the rows next to it.  Every kernel that calls sim_mfma_tile therefore
// gives a pair the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace n2v {

typedef float floatx16 __attribute__((ext_vector_type(16)));
constexpr int SIM_MT = 128;    // tile edge
constexpr int SIM_MKC = 16;    // k-chunk per barrier
constexpr int SIM_MLD = 132;   // LDS pitch: the two k-halves of a wave's store land 32 banks apart

// All 256 threads of the workgroup together.  ap / bp: this thread's staging source, row lrow = tid >> 1 of the tile's A / B
// rows at k offset kq = (tid & 1) * 8; a_ok / b_ok: that row exists (a missing row is staged as zeros).  acc[bi][bj] receives
// the 32x32 block (bi, bj) of the wavefront's 64x64 quarter (wr = wave >> 1, wc = wave & 1); kh = lane >> 5, m = lane & 31.
// The caller computes those six indices (its epilogue needs them too) and hands them in: with the function deriving its own
// copies the compiler gave sim_mfma_kernel<false> 123 VGPRs instead of 92.  The first barrier of the loop is also what
// separates a previous use of As / Bs from the stores of this one.
__device__ __forceinline__ void sim_mfma_tile(const float* ap, const float* bp, bool a_ok, bool b_ok, int dpad,
                                              float (*As)[SIM_MLD], float (*Bs)[SIM_MLD], floatx16 (&acc)[2][2],
                                              int wr, int wc, int lrow, int kq, int kh, int m) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;
    const float4 z4 = {0, 0, 0, 0};
    float4 a0 = z4, a1 = z4, b0 = z4, b1 = z4;
    if (a_ok) { a0 = *reinterpret_cast<const float4*>(ap); a1 = *reinterpret_cast<const float4*>(ap + 4); }
    if (b_ok) { b0 = *reinterpret_cast<const float4*>(bp); b1 = *reinterpret_cast<const float4*>(bp + 4); }
    for (int k0 = 0; k0 < dpad; k0 += SIM_MKC) {
        __syncthreads();
        As[kq + 0][lrow] = a0.x; As[kq + 1][lrow] = a0.y; As[kq + 2][lrow] = a0.z; As[kq + 3][lrow] = a0.w;
        As[kq + 4][lrow] = a1.x; As[kq + 5][lrow] = a1.y; As[kq + 6][lrow] = a1.z; As[kq + 7][lrow] = a1.w;
        Bs[kq + 0][lrow] = b0.x; Bs[kq + 1][lrow] = b0.y; Bs[kq + 2][lrow] = b0.z; Bs[kq + 3][lrow] = b0.w;
        Bs[kq + 4][lrow] = b1.x; Bs[kq + 5][lrow] = b1.y; Bs[kq + 6][lrow] = b1.z; Bs[kq + 7][lrow] = b1.w;
        __syncthreads();
        if (k0 + SIM_MKC < dpad) {      // next chunk's rows travel while this one is multiplied
            a0 = a1 = b0 = b1 = z4;
            if (a_ok) { a0 = *reinterpret_cast<const float4*>(ap + k0 + SIM_MKC); a1 = *reinterpret_cast<const float4*>(ap + k0 + SIM_MKC + 4); }
            if (b_ok) { b0 = *reinterpret_cast<const float4*>(bp + k0 + SIM_MKC); b1 = *reinterpret_cast<const float4*>(bp + k0 + SIM_MKC + 4); }
        }
#pragma unroll
        for (int kk = 0; kk < SIM_MKC; kk += 2) {
            const float av0 = As[kk + kh][wr * 64 + m], av1 = As[kk + kh][wr * 64 + 32 + m];
            const float bv0 = Bs[kk + kh][wc * 64 + m], bv1 = Bs[kk + kh][wc * 64 + 32 + m];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv1, acc[1][1], 0, 0, 0);
        }
    }
}

}  // namespace n2v
