// Device steps, host helpers and the sigmoid table of the word2vec kernels (n2v_sgns.hip, n2v_cbow.hip, n2v_sgns_csr.hip),
// each defined once: the argument fields the kernels share, the per-sentence LCG and hashes, staging a sentence in LDS, its
// learning rate and shrunk windows, the 8-at-a-time wave reduction, the negative draw over the cum-table + LUT, the steps of
// a target group, the lane layouts of a row, the skip-gram centre step (sg_centre_step) and the in-order hand-out of
// sentences; on the host the refusals, argument fill and grid of a launch.  Everything sits in an unnamed namespace: each
// including file gets its own copy, its own c_exp_table and its own record of which devices hold it.  Include after
// `#pragma clang fp contract(fast)`.
#pragma once
#include <cmath>
#include <cstdlib>
#include <mutex>

#include "n2v_common.h"

namespace {

constexpr int kExpTableSize = 1000;  // gensim EXP_TABLE_SIZE
constexpr float kMaxExp = 6.0f;      // gensim MAX_EXP
__constant__ float c_exp_table[kExpTableSize];

constexpr int kSlotTokens = 4096;  // tokens of one wave's LDS slot: 4 waves x 4096 x 4 B = the 64 KB of LDS a workgroup may ask for

// What every word2vec kernel is told alike: SgnsArgs, CbowArgs and SgCsrArgs each embed it as `w` (w2v_args fills it)
struct W2vArgs {
    float* syn0;
    float* syn1neg;
    int64_t n_words;
    int32_t row_stride;
    int32_t window, negative;
    const uint32_t* sample_int;
    const uint32_t* cum_table;
    const uint32_t* lut;
    int32_t lut_shift;  // 31 - lut_bits
    float alpha0, min_alpha;
    int64_t sent_base, sent_step, sent_total, alpha_batch;
    uint64_t seed, id_base;      // id_base + index = the sentence's (walk's) id, which keys its hashes and its LCG
    unsigned long long* count;   // NULL, or where the trained pairs (CBOW: centres) are added
    unsigned long long* work;    // NULL: static grid stride; else the in-order item counter (reset by the launch)
    int32_t lpad;                // tokens of a wave's LDS slot, a multiple of 64
    int32_t predraw;  // 1: all negatives of a centre are drawn by the lanes in parallel before its pairs (short launches)
};

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

// ---- effective sentence: drop padding (tokens < 0; BOUNDED: and tokens >= n_words) and sub-sampled words, keep order.
// One ballot pass over the raw tokens raw[0, len): returns the number of kept tokens and stores those whose effective
// index e lies in [w_lo, w_hi) at sent[e - w_lo] (w_hi - w_lo <= the slot; a whole sentence: 0, the slot).  stop: end at
// the first block that reaches w_hi (the count returned is then not the sentence's).  slot_staged() follows the last pass.
template <bool BOUNDED>
__device__ __forceinline__ int stage_sentence(const W2vArgs a, const int32_t* raw, int len, uint64_t sid, int lane,
                                              int32_t* sent, int w_lo, int w_hi, bool stop) {
    int n_eff = 0;
    for (int base = 0; base < len; base += 64) {
        const int pos = base + lane;
        bool keep = false;
        int32_t tok = -1;
        if (pos < len) {
            tok = raw[pos];
            keep = tok >= 0;
            if constexpr (BOUNDED) keep = keep && (int64_t)tok < a.n_words;
            if (keep && a.sample_int) keep = !(a.sample_int[tok] < hash32(a.seed, sid, (uint32_t)pos, 0x5AB));
        }
        const unsigned long long m = __ballot(keep);
        const int e = n_eff + __popcll(m & ((1ULL << lane) - 1ULL));
        if (keep && e >= w_lo && e < w_hi) sent[e - w_lo] = tok;
        n_eff += __popcll(m);
        if (stop && n_eff >= w_hi) break;
    }
    return n_eff;
}

// the wave's stores to its LDS slot are visible to all of its lanes from here on
__device__ __forceinline__ void slot_staged() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// learning rate of sentence number si of the launch (gensim: linear decay, stepped per job)
__device__ __forceinline__ float sentence_alpha(const W2vArgs a, int64_t si) {
    const int64_t pushed = a.sent_base + (si / a.alpha_batch) * a.alpha_batch * a.sent_step;
    const float alpha = a.alpha0 - (a.alpha0 - a.min_alpha) * (float)((double)pushed / (double)a.sent_total);
    return fmaxf(alpha, a.min_alpha);
}

// first state of the LCG that draws the sentence's negatives
__device__ __forceinline__ uint64_t sentence_lcg(uint64_t seed, uint64_t sid) {
    return mix64(seed ^ mix64(sid + 0x632BE59BD9B4E019ULL)) & kLcgMask;
}

// the shrunk window [lo, hi) of centre i of an effective sentence of n_eff tokens (word2vec's `reduced_window`)
struct Window {
    int lo, hi;
};
__device__ __forceinline__ Window shrunk_window(const W2vArgs a, uint64_t sid, int i, int n_eff) {
    const int rb = (int)(hash32(a.seed, sid, (uint32_t)i, 0xB17) % (uint32_t)a.window);
    return {max(0, i - a.window + rb), min(n_eff, i + a.window + 1 - rb)};
}

// The sentence's LCG advanced past the draws of the centres before i_begin (`negative` per (centre, context) pair), in
// closed form: where a wave that trains only the centres from i_begin on starts drawing.
__device__ __forceinline__ uint64_t lcg_skip_to_centre(const W2vArgs a, uint64_t sid, int n_eff, int i_begin, uint64_t lcg,
                                                       int lane) {
    int pairs_before = 0;
    for (int base = 0; base < i_begin; base += 64) {
        const int i = base + lane;
        int np = 0;
        if (i < i_begin) {
            const Window w = shrunk_window(a, sid, i, n_eff);
            np = w.hi - w.lo > 1 ? w.hi - w.lo - 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) np += __shfl_xor(np, o, 64);
        pairs_before += np;
    }
    return lcg_skip(lcg, (uint64_t)pairs_before * (uint64_t)a.negative);
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

// ---- steps of a target group.  The targets of a centre (skip-gram: of a pair) are numbered 0 = the centre word (label 1)
// and d >= 1 = its d-th negative draw; they are processed 8 at a time, the group of slot 0 = target t0.

// Lane k (k < 8) draws the target of slot k of the group: its row, or -1 for no target (slot 0 of the first group is the
// centre, which the caller fills in; a draw equal to the centre ci is skipped).  lcg: state of the group's first draw.
__device__ __forceinline__ int32_t draw_group_target(const W2vArgs a, uint64_t lcg, int t0, int32_t ci, int lane) {
    int32_t my_t = -1;
    const int tk = t0 + lane;  // target number: 0 = positive, d >= 1 = d-th negative
    if (lane < 8 && tk >= 1 && tk <= a.negative) {
        uint64_t s = lcg;
        for (int d = max(t0, 1); d < tk; ++d) s = (s * kLcgA + kLcgC) & kLcgMask;
        const uint32_t r = (uint32_t)((s >> 16) % 2147483647ULL);
        my_t = draw_target(a.cum_table, a.lut, a.lut_shift, r);
        if (my_t == ci) my_t = -1;  // `if target_index == word_index: continue`
    }
    return my_t;
}

// advance the sentence's LCG past the group's negatives
__device__ __forceinline__ uint64_t lcg_past_group(uint64_t lcg, int negative, int t0) {
    const int used = min(negative, t0 + 7) - max(t0, 1) + 1;
    for (int d = 0; d < used; ++d) lcg = (lcg * kLcgA + kLcgC) & kLcgMask;
    return lcg;
}

// A row drawn by two slots of the group (common where a few hubs hold most of the unigram^0.75 mass): the sequential rule
// lets the later slot see the row the earlier one updated.  The targets are scalar, so a few scalar compares find such a
// slot (bit k of the mask); it sits out the group's parallel pass and is trained after it, from the row as this wave has
// updated it (in memory by then).  Only the order among slots of ONE row matters (another row's update changes neither h
// nor this row), and the late slot's registers are free again by then: carrying the updated row over in registers keeps
// all rows of the group live and spills at d = 128.
template <int G>
__device__ __forceinline__ uint32_t late_slots(const int32_t (&tgt)[G]) {
    uint32_t late = 0;
#pragma unroll
    for (int k = 1; k < G; ++k)
#pragma unroll
        for (int k1 = 0; k1 < k; ++k1)
            if (tgt[k] >= 0 && tgt[k] == tgt[k1]) late |= 1u << k;
    return late;
}

// g of a target whose dot product with the input is f: (label - sigmoid_table[f]) * alpha; |f| >= MAX_EXP: 0, no update
__device__ __forceinline__ float target_gradient(float f, float label, float alpha) {
    if (!(f > -kMaxExp && f < kMaxExp)) return 0.f;
    return (label - c_exp_table[(int)((f + kMaxExp) * (float)(kExpTableSize / (int)kMaxExp / 2))]) * alpha;
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

// row += delta in load_row<VPL, kAgent>'s lane layout (the lane's own floats): the centre row of kAgent, see sg_centre_step
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
    return target_gradient(f, 0.f, alpha);
}

// The skip-gram step of one centre: centre i of the effective sentence sent[0, n_eff) against every position of its shrunk
// window, sequential per (pair, target) as one wavefront sees it.  sgns_kernel and sgns_csr_kernel both train through it;
// a caller that staged only the effective indices from w_lo on passes its slot pointer less w_lo.  lcg is the sentence's
// LCG at the centre's first draw and is left at the next centre's; pairs_done counts the pairs.  my_k = bitrev3(lane & 7),
// which of the 8 reduced values the lane ends up holding: the kernel computes it once (computed here, the register
// allocation of the spilling instantiations moves).
// G = target slots in use per group of 8 (6 when negative <= 5: the centre + 5 draws).
template <int VPL, int G, int MODE>
__device__ __forceinline__ void sg_centre_step(const W2vArgs a, const int32_t* sent, int n_eff, int i, uint64_t sid,
                                               float alpha, int lane, int my_k, uint64_t& lcg, unsigned long long& pairs_done) {
    const int32_t ci = __builtin_amdgcn_readfirstlane(sent[i]);
    const Window w = shrunk_window(a, sid, i, n_eff);
    const int lo = w.lo, hi = w.hi;
    if (hi - lo <= 1) return;
    Row<VPL> c = load_row<VPL, MODE>(a.syn1neg, ci, a.row_stride, lane);
    Row<VPL> cd;  // kAtomic, kAgent: this wave's accumulated change of the centre row
#pragma unroll
    for (int v = 0; v < VPL; ++v) cd.v[v] = 0.f;
    // A wave's pairs are a chain of dependent loads, and the look-up of the negatives (bucket index, then a
    // bisect of the cumulative table) is two to three links of it per pair — visible even in full-size launches
    // at 7 waves per SIMD.  With predraw the lanes make ALL draws of the centre at once — draw number d
    // of the centre uses the sentence's LCG advanced d times, exactly the state the pair-by-pair path reaches —
    // and a pair fetches its targets from the lanes that hold them.
    const int nd = (hi - lo - 1) * a.negative;
    const bool pre = a.predraw && nd <= 128;
    int32_t drawn0 = -1, drawn1 = -1;   // draws 0..63 and 64..127 of this centre, one per lane
    if (pre) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int d = half * 64 + lane;
            int32_t t = -1;
            if (d < nd) {
                const uint64_t s = lcg_skip(lcg, (uint64_t)d);
                t = draw_target(a.cum_table, a.lut, a.lut_shift, (uint32_t)((s >> 16) % 2147483647ULL));
                if (t == ci) t = -1;  // `if target_index == word_index: continue`
            }
            if (half == 0) drawn0 = t;
            else drawn1 = t;
        }
    }
    int pidx = 0;  // number of this pair among the centre's pairs
    for (int j = lo; j < hi; ++j) {
        if (j == i) continue;
        const int32_t xj = __builtin_amdgcn_readfirstlane(sent[j]);
        Row<VPL> h = load_row<VPL, MODE>(a.syn0, xj, a.row_stride, lane);
        Row<VPL> work;
#pragma unroll
        for (int v = 0; v < VPL; ++v) work.v[v] = 0.f;
        // targets are processed 8 at a time: slot 0 of the first group is the centre word
        for (int t0 = 0; t0 < a.negative + 1; t0 += 8) {
            // lane k (k < 8) holds the target of slot k of this group
            int32_t my_t = -1;
            if (pre) {   // negative <= 7: one group, lane k in [1, negative] holds target k
                const int d = min(max(pidx * a.negative + lane - 1, 0), 127);
                const int v0 = __builtin_amdgcn_ds_bpermute((d & 63) << 2, drawn0);
                const int v1 = __builtin_amdgcn_ds_bpermute((d & 63) << 2, drawn1);
                if (lane >= 1 && lane <= a.negative) my_t = d < 64 ? v0 : v1;
            } else {
                my_t = draw_group_target(a, lcg, t0, ci, lane);
            }
            int32_t tgt[G];
            Row<VPL> n[G];
            float p[8];
#pragma unroll
            for (int k = 0; k < G; ++k) {
                tgt[k] = __builtin_amdgcn_readlane(my_t, k);
                if (k == 0 && t0 == 0) tgt[k] = ci;
            }
            // the mask of late_slots, written out: through the call the allocator places the spills of the d >= 256
            // instantiations of sgns_kernel otherwise (up to 36 bytes of scratch more per lane, up to 16 % of their pass)
            uint32_t late = 0;
#pragma unroll
            for (int k = 1; k < G; ++k)
#pragma unroll
                for (int k1 = 0; k1 < k; ++k1)
                    if (tgt[k] >= 0 && tgt[k] == tgt[k1]) late |= 1u << k;
#pragma unroll
            for (int k = 0; k < G; ++k) {
                if (k == 0 && t0 == 0) {
                    n[k] = c;
                } else if (tgt[k] >= 0 && !(late >> k & 1)) {
                    n[k] = load_row<VPL, MODE>(a.syn1neg, tgt[k], a.row_stride, lane);
                } else {
#pragma unroll
                    for (int v = 0; v < VPL; ++v) n[k].v[v] = 0.f;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float acc = 0.f;
                if (k < G) {
#pragma unroll
                    for (int v = 0; v < VPL; ++v) acc = fmaf(h.v[v], n[k].v[v], acc);
                }
                p[k] = acc;
            }
            const float f = reduce8(p, lane);
            // this lane's own target: sigmoid table, gradient
            const float g = target_gradient(f, (my_k == 0 && t0 == 0) ? 1.f : 0.f, alpha);
#pragma unroll
            for (int k = 0; k < G; ++k) {
                if (tgt[k] < 0 || (late >> k & 1)) continue;
                const float gk = __builtin_bit_cast(
                    float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g), bitrev3(k)));
                if (gk == 0.f) continue;  // |f| >= MAX_EXP: no update at all
                Row<VPL> dn;
#pragma unroll
                for (int v = 0; v < VPL; ++v) {
                    work.v[v] = fmaf(gk, n[k].v[v], work.v[v]);
                    dn.v[v] = gk * h.v[v];
                    n[k].v[v] += dn.v[v];
                }
                if (k == 0 && t0 == 0) {
                    c = n[k];
#pragma unroll
                    for (int v = 0; v < VPL; ++v) cd.v[v] += dn.v[v];
                } else if constexpr (MODE == kAtomic) {
                    add_row<VPL>(a.syn1neg, tgt[k], a.row_stride, lane, dn);
                } else {
                    store_row<VPL, MODE>(a.syn1neg, tgt[k], a.row_stride, lane, n[k]);
                }
            }
            if (late) {
                // the repeated slots, in slot order: a negative each (a draw equal to the centre is skipped)
#pragma unroll
                for (int k = 1; k < G; ++k) {
                    if (!(late >> k & 1)) continue;
                    Row<VPL> r = load_row<VPL, MODE>(a.syn1neg, tgt[k], a.row_stride, lane);
                    const float gk = negative_gradient<VPL>(h, r, alpha);
                    if (gk == 0.f) continue;
                    Row<VPL> dn;
#pragma unroll
                    for (int v = 0; v < VPL; ++v) {
                        work.v[v] = fmaf(gk, r.v[v], work.v[v]);
                        dn.v[v] = gk * h.v[v];
                        r.v[v] += dn.v[v];
                    }
                    if constexpr (MODE == kAtomic) add_row<VPL>(a.syn1neg, tgt[k], a.row_stride, lane, dn);
                    else store_row<VPL, MODE>(a.syn1neg, tgt[k], a.row_stride, lane, r);
                }
            }
            lcg = lcg_past_group(lcg, a.negative, t0);
        }
        if constexpr (MODE == kAtomic) {
            add_row<VPL>(a.syn0, xj, a.row_stride, lane, work);
        } else {
#pragma unroll
            for (int v = 0; v < VPL; ++v) h.v[v] += work.v[v];
            store_row<VPL, MODE>(a.syn0, xj, a.row_stride, lane, h);
        }
        ++pidx;
        ++pairs_done;
    }
    // The centre row sits in registers for the whole window (~20 pairs, tens of microseconds): written back whole it
    // would erase every update other waves made to it meanwhile — by far the longest exposure of any row.  kAgent
    // therefore ADDS this wave's accumulated change, like kAtomic (one atomic row per centre: < 1 % of the row
    // updates); the context and negative rows, held for one pair, keep their whole-row stores.
    if constexpr (MODE == kAtomic) add_row<VPL>(a.syn1neg, ci, a.row_stride, lane, cd);
    else if constexpr (MODE == kAgent) add_row_packed<VPL>(a.syn1neg, ci, a.row_stride, lane, cd);
    else store_row<VPL, MODE>(a.syn1neg, ci, a.row_stride, lane, c);
}

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

int upload_exp_table(const char* who) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= 64) return n2v::fail(N2V_ERR_HIP, "%s: hipGetDevice: %s", who, hipGetErrorString(e));
    std::lock_guard<std::mutex> lock(exp_upload_mutex);
    if (exp_uploaded[dev]) return N2V_OK;
    fill_exp_table();
    e = hipMemcpyToSymbol(HIP_SYMBOL(c_exp_table), host_exp_table, sizeof(host_exp_table), 0, hipMemcpyHostToDevice);
    if (e != hipSuccess) return n2v::fail(N2V_ERR_HIP, "%s: exp table upload: %s", who, hipGetErrorString(e));
    exp_uploaded[dev] = true;
    return N2V_OK;
}

// predraw (parallel draws of a centre's negatives): on whenever negative <= 7 (one target group).  Measured on C3's
// walks: full-size launches 7.98e8 -> 8.85e8 pairs/s, one wavefront per walk (latency-bound) 3.49 -> 2.67 us per pair,
// the 83-walk launches of the tiered merges 145 -> 128 us.  N2V_SGNS_PREDRAW=0 switches it off (A/B timing, and the
// test that both paths train the same bits).
inline int predraw_mode(int negative) {
    if (negative < 1 || negative > 7) return 0;
    const char* e = getenv("N2V_SGNS_PREDRAW");
    return (e && e[0] == '0') ? 0 : 1;
}

// the shared argument fields, from a training entry point's arguments of the same names
inline W2vArgs w2v_args(float* syn0, float* syn1neg, int64_t n_words, int32_t row_stride, int32_t window, int32_t negative,
                 const uint32_t* sample_int, const uint32_t* cum_table, const uint32_t* lut, int32_t lut_bits, float alpha,
                 float min_alpha, int64_t sentences_base, int64_t sentences_step, int64_t sentences_total,
                 int64_t alpha_batch, uint64_t seed, uint64_t id_base, unsigned long long* count,
                 unsigned long long* work_counter, int32_t lpad) {
    W2vArgs w;
    w.syn0 = syn0; w.syn1neg = syn1neg; w.n_words = n_words; w.row_stride = row_stride;
    w.window = window; w.negative = negative; w.sample_int = sample_int;
    w.cum_table = cum_table; w.lut = lut; w.lut_shift = 31 - lut_bits;
    w.alpha0 = alpha; w.min_alpha = min_alpha;
    w.sent_base = sentences_base; w.sent_step = sentences_step; w.sent_total = sentences_total;
    w.alpha_batch = alpha_batch;
    w.seed = seed; w.id_base = id_base; w.count = count;
    w.work = work_counter;
    w.lpad = lpad;
    w.predraw = predraw_mode(negative);
    return w;
}

// The grid of a launch over n_items work items, one per wavefront at a time: workgroups of 4 waves, at most `cap`.
// A launch in which no wave gets a second item needs no hand-out (the replicas' short launches: thousands per pass, and
// 6 640 waves asking one address for "nothing left" cost 90 us each time); otherwise the work counter is reset.
inline int w2v_grid(const char* who, int64_t n_items, int64_t cap, W2vArgs& w, hipStream_t st, dim3* grid) {
    int64_t blocks = (n_items + 3) / 4;
    if (blocks > cap) blocks = cap;
    *grid = dim3((unsigned)blocks);
    if (n_items <= blocks * 4) w.work = nullptr;
    if (w.work && hipMemsetAsync(w.work, 0, sizeof(unsigned long long), st) != hipSuccess)
        return n2v::fail(N2V_ERR_HIP, "%s: resetting the work counter failed", who);
    return N2V_OK;
}

// ---- what the ragged entry points (`who`: n2v_cbow_train, n2v_sgns_csr_train) refuse alike.
// Sizes to schedule, in the order they are reported.  size_ok, size_tail: the caller's own part of the size check and of its
// message.  chunk: 0 where sentences are not chunked.  *slot: tokens of a wave's LDS slot.
inline int refuse_ragged(const char* who, bool size_ok, const char* size_tail, int64_t n_sentences, int64_t n_tokens,
                  int64_t n_words, int32_t dim, int32_t window, int32_t negative, int32_t max_len, int32_t chunk,
                  int32_t update_mode, int32_t row_stride, int32_t lut_bits, int64_t sentences_base, int64_t sentences_step,
                  int64_t sentences_total, int64_t alpha_batch, int32_t* slot) {
    if (n_sentences < 0 || n_tokens < 0 || n_words < 1 || n_words > 0x7fffffffLL || dim < 1 || window < 1 || negative < 0 ||
        negative > 64 || !size_ok)
        return n2v::fail(N2V_ERR_INVALID, "%s: bad size (sentences %lld, tokens %lld, words %lld, dim %d, window %d, negative %d%s)",
                         who, (long long)n_sentences, (long long)n_tokens, (long long)n_words, (int)dim, (int)window,
                         (int)negative, size_tail);
    if (max_len < 1 || max_len > kSlotTokens)
        return n2v::fail(N2V_ERR_INVALID, "%s: max_len %d outside [1, %d]", who, (int)max_len, kSlotTokens);
    if (chunk < 0) return n2v::fail(N2V_ERR_INVALID, "%s: chunk %d is negative", who, (int)chunk);
    const int64_t s = ((chunk > 0 ? (int64_t)chunk + 2 * (int64_t)window : (int64_t)max_len) + 63) & ~(int64_t)63;
    if (s > kSlotTokens)
        return n2v::fail(N2V_ERR_INVALID, "%s: slot of %lld tokens (chunk %d + 2 x window %d) above %d", who, (long long)s,
                         (int)chunk, (int)window, kSlotTokens);
    *slot = (int32_t)s;
    if (update_mode != N2V_SGNS_ATOMIC)
        return n2v::fail(N2V_ERR_INVALID, "%s: update_mode %d: only N2V_SGNS_ATOMIC (lossless rows) is offered", who,
                         (int)update_mode);
    if (row_stride < dim || (row_stride != 64 && row_stride != 128 && row_stride != 256 && row_stride != 512))
        return n2v::fail(N2V_ERR_INVALID, "%s: row_stride %d must be 64, 128, 256 or 512 and >= dim %d", who, (int)row_stride,
                         (int)dim);
    if (lut_bits < 1 || lut_bits > 24) return n2v::fail(N2V_ERR_INVALID, "%s: lut_bits %d", who, (int)lut_bits);
    if (sentences_total < 1 || alpha_batch < 1 || sentences_step < 1 || sentences_base < 0)
        return n2v::fail(N2V_ERR_INVALID, "%s: bad schedule", who);
    return N2V_OK;
}

// ... and, once there is something to train, the pointers
inline int refuse_ragged_null(const char* who, const int32_t* tokens, const int64_t* offsets, const float* syn0,
                       const float* syn1neg, int32_t negative, const uint32_t* cum_table, const uint32_t* lut) {
    if (!tokens || !offsets || !syn0 || !syn1neg || (negative > 0 && (!cum_table || !lut)))
        return n2v::fail(N2V_ERR_INVALID, "%s: null pointer", who);
    return N2V_OK;
}

}  // namespace
