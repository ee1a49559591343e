// "Fat slot" walk — gfx950 (MI355X): one 32-byte gather per step.
//
// Same walk as n2v_walk (src/node2vec.py:55-95, :271-281) over a table layout that spends
// HBM capacity to halve the number of memory requests: alias slot k of a table carries, next
// to q, the walk records of BOTH outcomes of the draw (neighbour k and neighbour J[k]):
//
//     fat = fat_slots[table + floor(u1*K)];          one aligned 32-B load
//     rec = (u2 < fat.q) ? fat.keep : fat.alias;     (:278-281)
//     table = rec.slot, K = rec.deg, node = rec.dst
//
// The thin layout costs two dependent 16-B gathers per step and is bound by the chip's
// random-request rate (each gather is one 64-B request); a 32-B aligned slot
// never straddles a 64-B line, so a step is one request.  Memory: 32 B per alias slot, i.e.
// 2x the thin tables (C3: 58.5 GB) — the reason this layout only makes sense on a 288 GB part.
// The tables are written in this layout by n2v_build_edge_tables_wave (same bits as the thin, reference-exact tables).
#include "n2v_walk_step.h"

namespace {

struct FatArgs {
    const int64_t* row_ptr;
    const n2v_fat_slot* node_fat;
    const n2v_fat_slot* fat;
    n2v::WalkShard sh;
    const double* uniforms;
    const int64_t* walk_uoff;
    int64_t uoff_round_stride;
    uint64_t seed;
    int32_t* walks;
    int32_t* lens;
};

// Walk kernel.  tools/lab/gather_lab*.hip: the chip serves ~4.9e10 random 16-B gathers/s from a 56 GB table but only
// 3.8e10 32-B slots/s when a lane fetches its slot with two dwordx4 loads (each load instruction is its own request to
// the same 64-B line), and 16-B pieces of output rows cost a partial-line write each.  So:
//   PAIR : lanes 2i and 2i+1 fetch the two halves of ONE slot with ONE load instruction — 32 contiguous bytes per
//          lane pair, i.e. one request per walk step — first for the even lane's walk, then for the odd lane's, and
//          swap the halves they fetched for each other through DPP (quad_perm [1,0,3,2]);
//   BURST: node ids leave the lane as whole 64-B lines (16 steps buffered in registers) when L % 16 == 0, as 16-B
//          pieces when L % 4 == 0, one by one otherwise.
// Uniforms (parity mode), two layouts:
//   N2V_RNG_UNIFORMS       linear: walk lw reads double2 at uniforms[o + 2t] — lanes of a wave are 2(L-1) doubles apart;
//   N2V_RNG_UNIFORMS_TILED the walks' segments of numpy's stream regrouped 64 walks at a time, step-major inside the
//          group (n2v_mt19937_fill_tiled): step t of the 64 walks of a wavefront is ONE contiguous 1-KiB read, and the
//          next step's pair is requested before the current slot gather (it does not depend on the walk's state).
// The round-2 A/B variants of this kernel live in tools/lab/walk_fat_variants.hip.
__device__ __forceinline__ uint32_t dpp_swap1(uint32_t v) {   // value of lane ^ 1
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
}
__device__ __forceinline__ uint4 dpp_swap1(uint4 v) {
    return make_uint4(dpp_swap1(v.x), dpp_swap1(v.y), dpp_swap1(v.z), dpp_swap1(v.w));
}

template <int RNG, int BURST>
__global__ void __launch_bounds__(256) walk_fat2_kernel(FatArgs a) {
    const int64_t lw = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool mine = lw < a.sh.n_local;       // the last pair may have one lane without a walk: it still helps its partner
    const int32_t L = a.sh.L;
    const n2v::WalkId w = n2v::walk_id(a.sh, lw, mine);
    int64_t b0 = 0, b1 = 0;
    if (mine) { b0 = a.row_ptr[w.start]; b1 = a.row_ptr[w.start + 1]; }
    const n2v_fat_slot* tab = a.node_fat + b0;  // first step: node table (:69-70)
    uint32_t K = (uint32_t)(b1 - b0);
    int32_t len = 1;
    uint32_t t = 0;
    constexpr bool kBuf = RNG == N2V_RNG_UNIFORMS || RNG == N2V_RNG_UNIFORMS_TILED;
    const double* up = nullptr;
    double2 unext = make_double2(0.0, 0.0);
    if (kBuf && mine && K != 0 && L > 1) {
        up = n2v::uniform_base(a.uniforms, a.sh, w, lw, a.walk_uoff, a.uoff_round_stride);
        if (RNG == N2V_RNG_UNIFORMS_TILED) {
            up = n2v::uniform_base_tiled(a.uniforms, up - a.uniforms, L);
            unext = *reinterpret_cast<const double2*>(up);
        }
    }
    const int odd = threadIdx.x & 1;

    // step takes its invariants by value (emit_walk)
    auto step = [&, seed = a.seed, fat = a.fat, w, mine, odd, L]() -> int32_t {
        const bool live = mine && K != 0;       // dead end: stop, consume nothing (:76-77)
        double u1 = 0.0, u2 = 0.0;
        if (live) {
            if (RNG == N2V_RNG_UNIFORMS_TILED) {   // the next step's pair is requested before this step's slot
                u1 = unext.x; u2 = unext.y;
                if ((int32_t)t + 2 < L) unext = *reinterpret_cast<const double2*>(up + (int64_t)n2v::kTiledStride * (t + 1));
            } else {
                n2v::step_uniforms(RNG, up, seed, w.gw, t, u1, u2);
            }
            ++t;
        }
        const uint32_t kk = (uint32_t)(u1 * (double)K);  // :277
        const uint64_t addr = live ? (uint64_t)(uintptr_t)(tab + kk) : 0ull;
        const uint64_t other = ((uint64_t)dpp_swap1((uint32_t)(addr >> 32)) << 32) | dpp_swap1((uint32_t)addr);
        const uint64_t even_addr = odd ? other : addr, odd_addr = odd ? addr : other;
        uint4 x = make_uint4(0, 0, 0, 0), y = x;
        if (even_addr) x = *reinterpret_cast<const uint4*>(even_addr + (odd ? 16 : 0));   // the pair reads 32 contiguous bytes
        if (odd_addr) y = *reinterpret_cast<const uint4*>(odd_addr + (odd ? 16 : 0));
        const uint4 got = dpp_swap1(odd ? x : y);
        if (!live) return -1;
        const n2v::WalkRec r = n2v::decode_fat(odd ? got : x, odd ? y : got, u2);   // the slot's lo and hi halves
        tab = fat + r.tbl;
        K = r.K;
        ++len;
        return r.dst;
    };

    n2v::emit_walk<BURST>(a.walks + lw * (int64_t)L, L, mine, w.start, step);
    if (mine) a.lens[lw] = len;
}

// One wavefront expands one table: fat[t+k] = {thin[t+k].q, rec(base+k), rec(base+J[k])} where
// base = row_ptr[node the table draws from] and rec(e) is the thin walk record of CSR entry e.
__global__ void __launch_bounds__(256)
fat_expand_kernel(int64_t n_tables, const int64_t* __restrict__ tab_off, const int32_t* __restrict__ tab_node,
                  const int64_t* __restrict__ row_ptr, const n2v_alias_slot* __restrict__ thin,
                  const n2v_edge_rec* __restrict__ recs, n2v_fat_slot* __restrict__ fat) {
    const int lane = threadIdx.x & 63;
    const int64_t tb = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (tb >= n_tables) return;
    const int64_t t0 = tab_off[tb];
    const int32_t node = tab_node ? tab_node[tb] : (int32_t)tb;
    const int64_t base = row_ptr[node];
    const int K = (int)(row_ptr[node + 1] - base);
    for (int k = lane; k < K; k += 64) {
        const n2v_alias_slot s = thin[t0 + k];
        n2v::write_fat_slot(fat + t0 + k, s.q, recs + base + k, recs + base + s.J);
    }
}

}  // namespace

extern "C" int n2v_build_fat_slots(int64_t n_tables, const int64_t* tab_off, const int32_t* tab_node,
                                   const int64_t* row_ptr, const n2v_alias_slot* thin, const n2v_edge_rec* recs,
                                   n2v_fat_slot* fat, void* stream) {
    if (n_tables < 0) return n2v::fail(N2V_ERR_INVALID, "n2v_build_fat_slots: negative count");
    if (n_tables == 0) return N2V_OK;
    if (!tab_off || !row_ptr || !thin || !recs || !fat)
        return n2v::fail(N2V_ERR_INVALID, "n2v_build_fat_slots: null pointer");
    if (((uintptr_t)fat & 31) != 0) return n2v::fail(N2V_ERR_INVALID, "n2v_build_fat_slots: fat slots not 32-byte aligned");
    const int64_t blocks = (n_tables + 3) / 4;
    if (blocks > 0x7fffffff) return n2v::fail(N2V_ERR_INVALID, "n2v_build_fat_slots: too many tables in one call");
    hipLaunchKernelGGL(fat_expand_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n_tables, tab_off,
                       tab_node, row_ptr, thin, recs, fat);
    return n2v::check_launch("n2v_build_fat_slots");
}

extern "C" int n2v_walk_fat(const int64_t* row_ptr, const n2v_fat_slot* node_fat, const n2v_fat_slot* fat,
                            const int32_t* starts, int64_t n_starts, int64_t pos_begin, int64_t pos_count,
                            int64_t round_begin, int64_t round_count, int32_t walk_length, int32_t rng_mode,
                            const double* uniforms, const int64_t* walk_uoff, int64_t uoff_round_stride, uint64_t seed,
                            int32_t* walks, int32_t* lens, void* stream) {
    n2v::WalkShard sh;
    if (const int rc = n2v::check_shard("n2v_walk_fat", starts, n_starts, pos_begin, pos_count, round_begin, round_count,
                                        walk_length, 1, &sh))
        return rc;
    if (uoff_round_stride < 0) return n2v::fail(N2V_ERR_INVALID, "n2v_walk_fat: negative uoff_round_stride");
    if (sh.n_local == 0) return N2V_OK;
    if (!row_ptr || !node_fat || !starts || !lens || !walks || (walk_length > 1 && !fat))
        return n2v::fail(N2V_ERR_INVALID, "n2v_walk_fat: null pointer");
    if (rng_mode != N2V_RNG_UNIFORMS && rng_mode != N2V_RNG_PHILOX && rng_mode != N2V_RNG_UNIFORMS_TILED)
        return n2v::fail(N2V_ERR_INVALID, "n2v_walk_fat: rng_mode %d", (int)rng_mode);
    if (rng_mode != N2V_RNG_PHILOX && walk_length > 1 && !uniforms)
        return n2v::fail(N2V_ERR_INVALID, "n2v_walk_fat: parity mode needs a uniform buffer");
    if (((uintptr_t)uniforms & 15) != 0 || ((uintptr_t)node_fat & 31) != 0 || ((uintptr_t)fat & 31) != 0)
        return n2v::fail(N2V_ERR_INVALID, "n2v_walk_fat: misaligned buffer");
    if (sh.n_local > (int64_t)0x7fffffff * 256) return n2v::fail(N2V_ERR_INVALID, "n2v_walk_fat: too many walks in one call");
    FatArgs a{row_ptr, node_fat, fat, sh, uniforms, walk_uoff, uoff_round_stride, seed, walks, lens};
    const dim3 grid(n2v::grid_for(sh.n_local, 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    // whole 64-B output lines when the row length allows it, 16-B pieces or single ids otherwise
    const int burst = (walk_length % 16 == 0 && ((uintptr_t)walks & 63) == 0) ? 16
                      : (walk_length % 4 == 0 && ((uintptr_t)walks & 15) == 0) ? 4 : 1;
    n2v::dispatch<N2V_RNG_UNIFORMS, N2V_RNG_UNIFORMS_TILED, N2V_RNG_PHILOX>(rng_mode, [&](auto rng) {
        n2v::dispatch<16, 4, 1>(burst, [&](auto b) {
            hipLaunchKernelGGL((walk_fat2_kernel<decltype(rng)::value, decltype(b)::value>), grid, block, 0, st, a);
        });
    });
    return n2v::check_launch("n2v_walk_fat");
}
