// Device helpers and the sigmoid table of the word2vec kernels (n2v_sgns.hip, n2v_cbow.hip): the per-sentence LCG and
// hashes, the 8-at-a-time wave reduction, the negative draw over the cum-table + LUT, the lane layouts of a row and the
// in-order hand-out of sentences.  Everything sits in an unnamed namespace: each including file gets its own copy, its own
// c_exp_table and its own record of which devices hold it.  Include after `#pragma clang fp contract(fast)`.
#pragma once
#include <cmath>
#include <mutex>

#include "n2v_common.h"

namespace {

constexpr int kExpTableSize = 1000;  // gensim EXP_TABLE_SIZE
constexpr float kMaxExp = 6.0f;      // gensim MAX_EXP
__constant__ float c_exp_table[kExpTableSize];

constexpr uint64_t kLcgA = 25214903917ULL, kLcgC = 11ULL, kLcgMask = (1ULL << 48) - 1;

// x -> x advanced by k steps of the sentence's 48-bit LCG (composition of the affine map by squaring)
__device__ __forceinline__ uint64_t lcg_skip(uint64_t x, uint64_t k) {
    uint64_t cur_m = kLcgA, cur_c = kLcgC, acc_m = 1, acc_c = 0;
    while (k) {
        if (k & 1) { acc_m = (acc_m * cur_m) & kLcgMask; acc_c = (acc_c * cur_m + cur_c) & kLcgMask; }
        cur_c = ((cur_m + 1) * cur_c) & kLcgMask;
        cur_m = (cur_m * cur_m) & kLcgMask;
        k >>= 1;
    }
    return (acc_m * x + acc_c) & kLcgMask;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}
__device__ __forceinline__ uint32_t hash32(uint64_t seed, uint64_t walk, uint32_t pos, uint32_t salt) {
    return (uint32_t)(mix64(seed ^ mix64(walk * 0x9E3779B97F4A7C15ULL + (((uint64_t)salt << 32) | pos))) >> 32);
}

__device__ __forceinline__ float xor_dpp1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));
}
__device__ __forceinline__ float xor_dpp2(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));
}
template <int M>
__device__ __forceinline__ float xor_swz(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (M << 10) | 0x1f));
}

// Reduce 8 per-lane partial sums over the wave at once.  On return lane l holds the total
// of value index 4*(l&1) + 2*((l>>1)&1) + ((l>>2)&1), i.e. value k sits in lane bitrev3(k)
// (and in every lane congruent to it mod 8).
__device__ __forceinline__ float reduce8(const float (&p)[8], int lane) {
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
    float q[4], r[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float send = b0 ? p[k] : p[k + 4];
        const float keep = b0 ? p[k + 4] : p[k];
        q[k] = keep + xor_dpp1(send);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float send = b1 ? q[k] : q[k + 2];
        const float keep = b1 ? q[k + 2] : q[k];
        r[k] = keep + xor_dpp2(send);
    }
    float s = (b2 ? r[1] : r[0]) + xor_swz<4>(b2 ? r[0] : r[1]);
    s += xor_swz<8>(s);
    s += xor_swz<16>(s);
    s += __shfl_xor(s, 32);
    return s;
}

__device__ __forceinline__ constexpr int bitrev3(int k) { return ((k & 1) << 2) | (k & 2) | ((k >> 2) & 1); }

// bisect_left(cum_table, r) narrowed by a bucket table: lut[b] = bisect_left(cum_table, b << shift)
__device__ __forceinline__ int32_t draw_target(const uint32_t* __restrict__ cum, const uint32_t* __restrict__ lut,
                                               int shift, uint32_t r) {
    const uint32_t b = r >> shift;
    uint32_t lo = lut[b], hi = lut[b + 1];
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cum[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return (int32_t)lo;
}

template <int VPL>
struct Row {
    float v[VPL];
};

// How rows are shared between wavefronts (all of them race, as gensim's Hogwild threads do):
//  kPlain  : plain loads and stores.  Lines live in the issuing XCD's write-back L2, which is
//            not coherent with the other seven: an XCD keeps training on its own copy of a hot
//            row and whole-row write-backs overwrite each other.  Fastest; loses updates.
//  kAgent  : agent-scope (sc1) loads and stores — every access goes to the memory side
//            (Infinity Cache / HBM), so all wavefronts see one copy; a read-modify-write can
//            still lose a concurrent update.
//  kAtomic : agent-scope loads, and every update applied as a float atomic add at the memory
//            side (global_atomic_add_f32, 256 contiguous bytes per wave-instruction): no
//            update is ever lost.  Default.
enum : int { kPlain = 0, kAgent = 1, kAtomic = 2 };

template <int MODE>
__device__ __forceinline__ float2 ld2(const float* p) {
    if constexpr (MODE == kPlain) {
        return *reinterpret_cast<const float2*>(p);
    } else {
        const uint64_t b = __hip_atomic_load(reinterpret_cast<const uint64_t*>(p), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        return make_float2(__builtin_bit_cast(float, (uint32_t)b), __builtin_bit_cast(float, (uint32_t)(b >> 32)));
    }
}
template <int MODE>
__device__ __forceinline__ void st2(float* p, float x, float y) {
    if constexpr (MODE == kPlain) {
        *reinterpret_cast<float2*>(p) = make_float2(x, y);
    } else {
        const uint64_t b = (uint64_t)__builtin_bit_cast(uint32_t, x) | ((uint64_t)__builtin_bit_cast(uint32_t, y) << 32);
        __hip_atomic_store(reinterpret_cast<uint64_t*>(p), b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Lane layout of a row: VPL <= 2: lane owns VPL consecutive floats; VPL >= 4: 1-KiB chunks of
// the row, 4 floats per lane in each (every wave-instruction touches contiguous bytes).
template <int VPL>
__device__ __forceinline__ int lane_off(int lane) { return VPL <= 2 ? lane * VPL : lane * 4; }

template <int VPL, int MODE>
__device__ __forceinline__ Row<VPL> load_row(const float* base, int64_t row, int stride, int lane) {
    Row<VPL> r;
    if constexpr (MODE == kAtomic) {
        // element i of the lane = float i*64 + lane: each wave-instruction covers 256 contiguous
        // bytes, the shape the memory-side float atomics (add_row) run at full rate for
        const float* q = base + row * stride + lane;
#pragma unroll
        for (int i = 0; i < VPL; ++i) r.v[i] = __hip_atomic_load(q + i * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return r;
    }
    const float* p = base + row * stride + lane_off<VPL>(lane);
    if constexpr (VPL == 1) {
        if constexpr (MODE == kPlain) r.v[0] = *p;
        else r.v[0] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if constexpr (VPL == 2) {
        const float2 t = ld2<MODE>(p);
        r.v[0] = t.x; r.v[1] = t.y;
    } else {
#pragma unroll
        for (int i = 0; i < VPL; i += 4) {
            if constexpr (MODE == kPlain) {
                const float4 t = *reinterpret_cast<const float4*>(p + i * 64);
                r.v[i] = t.x; r.v[i + 1] = t.y; r.v[i + 2] = t.z; r.v[i + 3] = t.w;
            } else {
                const float2 t0 = ld2<MODE>(p + i * 64), t1 = ld2<MODE>(p + i * 64 + 2);
                r.v[i] = t0.x; r.v[i + 1] = t0.y; r.v[i + 2] = t1.x; r.v[i + 3] = t1.y;
            }
        }
    }
    return r;
}

template <int VPL, int MODE>
__device__ __forceinline__ void store_row(float* base, int64_t row, int stride, int lane, const Row<VPL>& r) {
    float* p = base + row * stride + lane_off<VPL>(lane);
    if constexpr (VPL == 1) {
        if constexpr (MODE == kPlain) *p = r.v[0];
        else __hip_atomic_store(p, r.v[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if constexpr (VPL == 2) {
        st2<MODE>(p, r.v[0], r.v[1]);
    } else {
#pragma unroll
        for (int i = 0; i < VPL; i += 4) {
            if constexpr (MODE == kPlain) {
                *reinterpret_cast<float4*>(p + i * 64) = make_float4(r.v[i], r.v[i + 1], r.v[i + 2], r.v[i + 3]);
            } else {
                st2<MODE>(p + i * 64, r.v[i], r.v[i + 1]);
                st2<MODE>(p + i * 64 + 2, r.v[i + 2], r.v[i + 3]);
            }
        }
    }
}

// row += delta, one float atomic per element, at the memory side
template <int VPL>
__device__ __forceinline__ void add_row(float* base, int64_t row, int stride, int lane, const Row<VPL>& d) {
    float* q = base + row * stride + lane;  // same lane layout as load_row<VPL, kAtomic>
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        __hip_atomic_fetch_add(q + i * 64, d.v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// row += delta in load_row<VPL, kAgent>'s lane layout (the lane's own floats): the centre row of kAgent, see sgns_kernel
template <int VPL>
__device__ __forceinline__ void add_row_packed(float* base, int64_t row, int stride, int lane, const Row<VPL>& d) {
    float* p = base + row * stride + lane_off<VPL>(lane);
    if constexpr (VPL <= 2) {
#pragma unroll
        for (int v = 0; v < VPL; ++v) __hip_atomic_fetch_add(p + v, d.v[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
#pragma unroll
        for (int i = 0; i < VPL; i += 4)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                __hip_atomic_fetch_add(p + i * 64 + v, d.v[i + v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// g of a negative target (label 0) whose row is n: the whole-wave dot product, the sigmoid table, the learning rate —
// for a slot of sgns_kernel whose row an earlier slot of its group has already updated.
template <int VPL>
__device__ __forceinline__ float negative_gradient(const Row<VPL>& h, const Row<VPL>& n, float alpha) {
    float acc = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) acc = fmaf(h.v[v], n.v[v], acc);
    // the butterflies of reduce8 (an address per __shfl_xor step would be held in VGPRs across the whole kernel)
    acc += xor_dpp1(acc);
    acc += xor_dpp2(acc);
    acc += xor_swz<4>(acc);
    acc += xor_swz<8>(acc);
    acc += xor_swz<16>(acc);
    acc += __shfl_xor(acc, 32);
    const float f = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, acc)));
    if (!(f > -kMaxExp && f < kMaxExp)) return 0.f;
    return (0.f - c_exp_table[(int)((f + kMaxExp) * (float)(kExpTableSize / (int)kMaxExp / 2))]) * alpha;
}

// G = target slots in use per group of 8 (6 when negative == 5: the centre + 5 draws)
// Sentences (items) are handed to the wavefronts IN ORDER by a device counter: every wave then works inside one narrow,
// moving window of the corpus, like the threads of the sequential algorithm's job queue.  With the static grid stride
// (item = wave, wave + n_waves, ...) the waves drift apart — a wave on a fuller CU falls behind by whole percents of the
// corpus — and the link-prediction AUC moved away from the sequential comparator with the grid (399 846
// rows, lossless rows: -0.0023 at 3072 workgroups, -0.0035 at 1561; in order: -0.00003 at every grid).
__device__ __forceinline__ int64_t next_item(unsigned long long* counter, int lane) {
    unsigned long long v = 0;
    if (lane == 0) v = atomicAdd(counter, 1ull);
    const int lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

float host_exp_table[kExpTableSize];
bool host_exp_ready = false;

void fill_exp_table() {
    if (host_exp_ready) return;
    for (int i = 0; i < kExpTableSize; ++i) {
        // gensim word2vec_inner.pyx init(): EXP_TABLE[i] = exp((i / 1000 * 2 - 1) * 6); e / (e + 1), float32
        const float x = ((float)i / (float)kExpTableSize * 2.0f - 1.0f) * kMaxExp;
        const float e = (float)std::exp((double)x);
        host_exp_table[i] = (float)(e / (e + 1.0f));
    }
    host_exp_ready = true;
}

// The sigmoid table reaches each device's constant memory once per process (a blocking copy the first time a device
// trains): re-uploading it with every launch cost a 4-KB copy kernel and ~20 us of host time per launch, which the
// thousands of short launches of the tiered merges pay in full.
std::mutex exp_upload_mutex;
bool exp_uploaded[64] = {};

int upload_exp_table() {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= 64) return n2v::fail(N2V_ERR_HIP, "n2v_sgns_train: hipGetDevice: %s", hipGetErrorString(e));
    std::lock_guard<std::mutex> lock(exp_upload_mutex);
    if (exp_uploaded[dev]) return N2V_OK;
    fill_exp_table();
    e = hipMemcpyToSymbol(HIP_SYMBOL(c_exp_table), host_exp_table, sizeof(host_exp_table), 0, hipMemcpyHostToDevice);
    if (e != hipSuccess) return n2v::fail(N2V_ERR_HIP, "n2v_sgns_train: exp table upload: %s", hipGetErrorString(e));
    exp_uploaded[dev] = true;
    return N2V_OK;
}

}  // namespace
