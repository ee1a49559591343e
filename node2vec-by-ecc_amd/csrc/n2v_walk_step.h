// What every walk kernel shares (n2v_walk.hip, n2v_walk_fat.hip, n2v_walk_otf.hip) — gfx950 (MI355X): which walk a lane
// owns, where its uniforms are, the walk record and the fat slot, a row's buffered output.  The kernels add the table fetch.
#pragma once
#include <type_traits>
#include "n2v_common.h"

namespace n2v {


// A call's share of simulate_walks (src/node2vec.py:97-111): start positions [pos_begin, pos_begin + pos_count) of
// rounds [round_begin, ...), n_local walks in all.  Local walk lw is position lw % pos_count of round lw / pos_count.
struct WalkShard {
    const int32_t* starts;
    int64_t n_starts, pos_begin, pos_count, round_begin, n_local;
    int32_t L;
};
struct WalkId {
    int64_t rl, pl;   // round and position inside the shard
    uint64_t gw;      // global walk index: the Philox counter
    int32_t start;    // first node
};
// A lane without a walk (mine == false) gets walk 0 of the shard and start node 0, and reads nothing.
__device__ __forceinline__ WalkId walk_id(const WalkShard& s, int64_t lw, bool mine = true) {
    WalkId w{0, 0, 0, 0};
    if (mine) {
        w.rl = lw / s.pos_count;
        w.pl = lw - w.rl * s.pos_count;
        w.start = s.starts[s.pos_begin + w.pl];
    }
    w.gw = (uint64_t)((s.round_begin + w.rl) * s.n_starts + s.pos_begin + w.pl);
    return w;
}


// Walk lw's 2 (L - 1) uniforms in the buffer: one walk after the other; or at walk_uoff[lw]; or, with a round stride, at
// walk_uoff[position] + round * stride (one offset list serves every round).
__device__ __forceinline__ const double* uniform_base(const double* uniforms, const WalkShard& s, const WalkId& w,
                                                      int64_t lw, const int64_t* walk_uoff,
                                                      int64_t uoff_round_stride = 0) {
    return uniforms + (!walk_uoff ? (int64_t)2 * (s.L - 1) * lw
                       : uoff_round_stride > 0 ? walk_uoff[w.pl] + w.rl * uoff_round_stride : walk_uoff[lw]);
}
// N2V_RNG_UNIFORMS_TILED (n2v_mt19937_fill_tiled): the walk with linear offset `off` is active walk off / (2 (L - 1));
// 64 walks form a group stored step-major, so a walk's consecutive steps are kTiledStride doubles apart.
constexpr int kTiledStride = 128;
__device__ __forceinline__ const double* uniform_base_tiled(const double* uniforms, int64_t off, int32_t L) {
    const uint64_t slot = (uint64_t)off / (uint64_t)(2 * (L - 1));
    return uniforms + 2 * ((slot >> 6) * (uint64_t)(L - 1) * 64 + (slot & 63));
}

// The two uniforms of 0-based step t: from the walk's segment of the buffer (rng == N2V_RNG_UNIFORMS, up 16-byte aligned)
// or from Philox.  They play the role of the two np.random.rand() calls of alias_draw (:277-278).
__device__ __forceinline__ void step_uniforms(int rng, const double* up, uint64_t seed, uint64_t gw, uint32_t t,
                                              double& u1, double& u2) {
    if (rng == N2V_RNG_UNIFORMS) {
        const double2 u = *reinterpret_cast<const double2*>(up + 2 * (int64_t)t);
        u1 = u.x; u2 = u.y;
    } else {
        philox_uniforms(seed, gw, t, u1, u2);
    }
}


// Walk record of a CSR entry (n2v_edge_rec): {slot_lo, base, dst, deg_hi} — everything the step after moving to `dst`
// needs.  The 40-bit index of the entry's alias table is split: low 32 bits in slot_lo, high 8 in the top byte of
// deg_hi, whose low 24 bits are deg(dst); base = row_ptr[dst].  Index N2V_NO_TABLE: the table is not stored.
// Fat slot (n2v_fat_slot) {q, rec_k, rec_J}: q[k] and the records of both outcomes of the draw, neighbour k and
// neighbour J[k], without their row bases, as two 16-byte halves
//     lo = {q.lo, q.hi, k.slot_lo, k.deg_hi}      hi = {k.dst, J.slot_lo, J.deg_hi, J.dst}
struct WalkRec {
    uint64_t tbl;    // index of the next step's table
    uint32_t K;      // deg(dst)
    uint32_t base;   // row_ptr[dst]; 0 from a fat slot
    int32_t dst;
};
__device__ __forceinline__ uint4 pack_rec(uint64_t tbl, uint32_t base, int32_t dst, uint32_t deg) {
    return make_uint4((uint32_t)tbl, base, (uint32_t)dst, deg | ((uint32_t)(tbl >> 32) << 24));
}
__device__ __forceinline__ WalkRec decode_rec(uint4 r) {
    return WalkRec{((uint64_t)(r.w >> 24) << 32) | r.x, r.w & 0xFFFFFFu, r.y, (int32_t)r.z};
}
__device__ __forceinline__ void write_fat_slot(n2v_fat_slot* out, double q, const n2v_edge_rec* rec_k,
                                               const n2v_edge_rec* rec_J) {
    const uint4 ra = *reinterpret_cast<const uint4*>(rec_k);
    const uint4 rb = *reinterpret_cast<const uint4*>(rec_J);
    uint4 lo, hi;
    lo.x = (uint32_t)__double2loint(q); lo.y = (uint32_t)__double2hiint(q);
    lo.z = ra.x; lo.w = ra.w;
    hi.x = ra.z; hi.y = rb.x; hi.z = rb.w; hi.w = rb.z;
    uint4* o = reinterpret_cast<uint4*>(out);
    o[0] = lo;
    o[1] = hi;
}
// the record alias_draw picks from a fat slot: neighbour k when u2 < q, else neighbour J[k] (:278-281)
__device__ __forceinline__ uint4 fat_pick(uint4 lo, uint4 hi, double u2) {
    const bool keep = u2 < __hiloint2double((int)lo.y, (int)lo.x);
    return keep ? make_uint4(lo.z, 0u, hi.x, lo.w) : make_uint4(hi.y, 0u, hi.w, hi.z);
}
__device__ __forceinline__ WalkRec decode_fat(uint4 lo, uint4 hi, double u2) { return decode_rec(fat_pick(lo, hi, u2)); }


// Writes a walk's row: `first`, then step() for every later node, BURST ids buffered in registers per store — whole
// 64-B lines (16), 16-B pieces (4) or single ids (1); L is a multiple of BURST and the row aligned to it.  A lane with
// mine == false takes the same steps (its wave's other lanes may need it) and writes nothing.
// step captures its invariants by value: the optimiser meets it inside this function before that is inlined into the
// kernel, where a by-reference capture is a load it will not hoist (Philox would recompute its round keys every step).
template <int BURST, typename Step>
__device__ __forceinline__ void emit_walk(int32_t* out, int32_t L, bool mine, int32_t first, Step&& step) {
    int32_t buf[BURST];
    buf[0] = first;
#pragma unroll
    for (int i = 1; i < BURST; ++i) buf[i] = step();
    for (int32_t g = 0;;) {
        if (mine) {
            if (BURST >= 4) {
#pragma unroll
                for (int i = 0; i + 3 < BURST; i += 4) {
                    typedef int v4i __attribute__((ext_vector_type(4)));
                    v4i v = {buf[i], buf[i + 1], buf[i + 2], buf[i + 3]};
                    *reinterpret_cast<v4i*>(out + g + i) = v;
                }
            } else {
                out[g] = buf[0];
            }
        }
        g += BURST;
        if (g >= L) break;
#pragma unroll
        for (int i = 0; i < BURST; ++i) buf[i] = step();
    }
}


// Validates a call's shard and fills *s (n_local = 0: nothing to do).  n2v_walk takes min_length 0, the others 1.
inline int check_shard(const char* who, const int32_t* starts, int64_t n_starts, int64_t pos_begin, int64_t pos_count,
                       int64_t round_begin, int64_t round_count, int32_t walk_length, int32_t min_length, WalkShard* s) {
    if (pos_count < 0 || round_count < 0 || pos_begin < 0 || round_begin < 0 || walk_length < min_length ||
        pos_begin + pos_count > n_starts)
        return fail(N2V_ERR_INVALID, "%s: bad shard (pos %lld+%lld of %lld, rounds %lld+%lld, L %d)", who,
                    (long long)pos_begin, (long long)pos_count, (long long)n_starts, (long long)round_begin,
                    (long long)round_count, (int)walk_length);
    *s = WalkShard{starts, n_starts, pos_begin, pos_count, round_begin, pos_count * round_count, walk_length};
    return N2V_OK;
}

// Runs f(std::integral_constant<int, V>) for the V of the list that equals v: a run-time choice (rng mode, burst) becomes
// a kernel's template argument.
template <int... Vs, typename F>
inline void dispatch(int v, F&& f) {
    (void)((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

}  // namespace n2v
