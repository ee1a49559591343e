// Skip-gram with negative sampling over a device-resident walk corpus — gfx950 kernels.
//
// Replaces what `learn_embeddings` hands to gensim 3.2.0 (src/main.py:82-90:
// Word2Vec(walks, size=d, window=w, min_count=0, sg=1, iter=...), defaults negative=5,
// alpha .025 -> .0001, sample=1e-3).  gensim's source is not part of the reference tree;
// the update rule below restates its public `fast_sentence_sg_neg` / `train_batch_sg`
// (word2vec_inner.pyx) as summarised in SURVEY.md 8(a) row 9:
//
//   per sentence: drop sub-sampled words; per position i draw b in [0, window); for every
//   j in [i-window+b, i+window-b], j != i:   input row h = syn0[word_j]; targets = word_i
//   (label 1) + `negative` draws from the unigram^0.75 cum-table (a draw equal to word_i is
//   skipped); f = <h, syn1neg[t]>; |f| >= 6 skips; g = (label - sigmoid_table[f]) * alpha;
//   work += g * syn1neg[t]; syn1neg[t] += g * h; finally syn0[word_j] += work.
//
// Mapping to the machine: one wavefront owns one walk at a time; a row of d = 64*VPL floats
// is VPL consecutive floats per lane, so a row access is one coalesced wave-wide load or
// store (512 B at d = 128).  The centre word's syn1neg row stays in registers for all of
// its context pairs.  The up-to-8 dot products of a pair are reduced together
// (DPP / ds_swizzle butterflies that halve the value count at each of the first three
// steps), so that lane bitrev3(k) ends up with <h, row_k>, evaluates the sigmoid table and
// the gradient for its own target, and the g's return to all lanes by v_readlane.
// A row drawn by two slots of one group is trained after the group's parallel pass, from the row
// as the earlier slot left it, so that one wavefront follows the sequential per-target rule
// exactly: one walk on one wavefront is pinned to a float64 restatement at fp32 rounding
// (tests/test_gpu_sgns_exact.py).  Rows are updated with plain loads/stores, racing with other
// wavefronts exactly as gensim's Hogwild worker threads race with each other.  The path is HBM/L2
// gather-scatter bound; there is no dense contraction worth an MFMA.
#include <cmath>
#include <cstdlib>
#include <mutex>

#include "n2v_common.h"

#pragma clang fp contract(fast)

#include "n2v_w2v_device.h"

namespace {

struct SgnsArgs {
    W2vArgs w;        // id_base: id of walk 0
    const int32_t* walks;
    const int32_t* lens;
    int64_t n_walks;
    int32_t walk_stride;
    int32_t splits;   // wavefronts per walk (>= 1): split s trains the centres [s*n/S, (s+1)*n/S) of the sentence
    // span mode (n2v_sgns_train_span): which walks this launch trains is read from device memory, so that a captured
    // launch can be replayed for every merge interval of a pass
    const int64_t* dyn;          // NULL, or {base interval index, sentences of earlier epochs}
    int32_t dyn_sub, dyn_subs;   // this launch is sub-interval dyn_sub of dyn_subs per base interval
    int64_t dyn_n_sub_total, dyn_n_local, dyn_shard_offset;
};

// span mode: sub-interval s = interval * subs + sub of the pass covers the local walks [s*n/k, (s+1)*n/k) (the cut of
// n2v_hip/merge.py:chunk_plan); the schedule arguments follow as in the eager driver (n2v_hip/sgns.py:_train_tsum)
__device__ __forceinline__ void resolve_span(SgnsArgs& a) {
    if (!a.dyn) return;
    const int64_t epoch_base = a.dyn[1];
    const int64_t s = a.dyn[0] * a.dyn_subs + a.dyn_sub;
    const int64_t b = s * a.dyn_n_local / a.dyn_n_sub_total, e = (s + 1) * a.dyn_n_local / a.dyn_n_sub_total;
    a.n_walks = e - b;
    a.walks += b * a.walk_stride;
    if (a.lens) a.lens += b;
    a.w.sent_base = epoch_base + b * a.w.sent_step;
    a.w.id_base = (uint64_t)(epoch_base + a.dyn_shard_offset + b);
}

template <int VPL, int G, int MODE>
// 8 waves per SIMD: the default allocation (106 SGPRs) stops at 7; capped, the kernel fits 78 SGPRs / 61 VGPRs without
// spilling and the agent-row pass gains 1.4 % (10^6-row probe: 9.61 -> 9.74e8 pairs/s)
__attribute__((amdgpu_waves_per_eu(8, 8)))
__global__ void __launch_bounds__(256) sgns_kernel(SgnsArgs a_in) {
    SgnsArgs a = a_in;
    resolve_span(a);
    extern __shared__ int32_t smem[];
    const int lane = threadIdx.x & 63;
    // the wave index is the same in all 64 lanes: tell the compiler, so that everything derived from
    // it (walk id, loop bounds, table sizes) is scalar and loops branch on SCC instead of EXEC
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int32_t* sent = smem + wv * a.w.lpad;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    const int my_k = bitrev3(lane & 7);  // which of the 8 reduced values this lane ends up holding
    unsigned long long pairs_done = 0;

    // Work items are (walk, split): with splits == 1 one wavefront owns a walk (gensim's worker owns a sentence); with
    // S > 1 the centres of a sentence are dealt to S wavefronts — the same pairs, the same draws (the sentence's LCG is
    // advanced to each split's first centre in closed form), only the order inside the sentence becomes a race like the
    // one between sentences.  That is what lets a launch of a few hundred walks fill the chip (tiered merges).
    const int S = a.splits;
    const int64_t n_items = a.n_walks * S;
    // (every item comes off the counter, the first one too: a workgroup that only becomes resident late in the pass must not
    // start with the early sentence its index names — measured: -0.0037 at 3072 workgroups on the 400k fixture)
    for (int64_t item = a.w.work ? next_item(a.w.work, lane) : (int64_t)blockIdx.x * 4 + wv; item < n_items;
         item = a.w.work ? next_item(a.w.work, lane) : item + n_waves) {
        const int64_t wi = S == 1 ? item : item / S;
        const int sp = S == 1 ? 0 : (int)(item - wi * S);
        const int len = a.lens ? a.lens[wi] : a.walk_stride;
        const uint64_t wid = a.w.id_base + (uint64_t)wi;
        const int n_eff = stage_sentence<false>(a.w, a.walks + wi * a.walk_stride, len, wid, lane, sent, 0, a.w.lpad, false);
        slot_staged();
        const float alpha = sentence_alpha(a.w, wi);
        uint64_t lcg = sentence_lcg(a.w.seed, wid);
        int i_begin = 0, i_end = n_eff;
        if (S > 1) {
            i_begin = (int)((int64_t)sp * n_eff / S);
            i_end = (int)((int64_t)(sp + 1) * n_eff / S);
            lcg = lcg_skip_to_centre(a.w, wid, n_eff, i_begin, lcg, lane);
        }
        for (int i = i_begin; i < i_end; ++i)
            sg_centre_step<VPL, G, MODE>(a.w, sent, n_eff, i, wid, alpha, lane, my_k, lcg, pairs_done);
        __builtin_amdgcn_wave_barrier();  // LDS sentence is reused by the next walk
    }
    if (a.w.count && lane == 0 && pairs_done) atomicAdd(a.w.count, pairs_done);
}

// Opt-in variant (N2V_SGNS_SHARE_NEGATIVES): the `negative` draws are made once per CENTRE word
// and shared by all of its context pairs (the scheme of Ji et al., "Parallelizing Word2Vec in
// Shared and Distributed Memory", 2016) instead of once per pair as gensim does.  The target
// rows then stay in registers for the whole window and are written back once per centre, so a
// pair touches memory only for its context row: ~0.8 KB instead of 3.1 KB of atomic traffic.
// Same update rule per (pair, target); different (correlated) negative samples.  negative <= 7.
template <int VPL, int MODE>
__global__ void __launch_bounds__(256) sgns_shared_kernel(SgnsArgs a_in) {
    SgnsArgs a = a_in;
    resolve_span(a);
    extern __shared__ int32_t smem[];
    const int lane = threadIdx.x & 63;
    // the wave index is the same in all 64 lanes: tell the compiler, so that everything derived from
    // it (walk id, loop bounds, table sizes) is scalar and loops branch on SCC instead of EXEC
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int32_t* sent = smem + wv * a.w.lpad;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    const int my_k = bitrev3(lane & 7);
    unsigned long long pairs_done = 0;

    for (int64_t wi = (int64_t)blockIdx.x * 4 + wv; wi < a.n_walks; wi += n_waves) {
        const int len = a.lens ? a.lens[wi] : a.walk_stride;
        const uint64_t wid = a.w.id_base + (uint64_t)wi;
        const int n_eff = stage_sentence<false>(a.w, a.walks + wi * a.walk_stride, len, wid, lane, sent, 0, a.w.lpad, false);
        slot_staged();
        const float alpha = sentence_alpha(a.w, wi);
        uint64_t lcg = sentence_lcg(a.w.seed, wid);

        for (int i = 0; i < n_eff; ++i) {
            const int32_t ci = __builtin_amdgcn_readfirstlane(sent[i]);
            const Window w = shrunk_window(a.w, wid, i, n_eff);
            const int lo = w.lo, hi = w.hi;
            if (hi - lo <= 1) continue;
            // targets of this centre: slot 0 = the centre itself, slots 1..negative = one draw each
            const int32_t my_t = draw_group_target(a.w, lcg, 0, ci, lane);
            lcg = lcg_past_group(lcg, a.w.negative, 0);
            int32_t tgt[8];
            Row<VPL> n[8], dn[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                tgt[k] = (k == 0) ? ci : __builtin_amdgcn_readlane(my_t, k);
                // a target drawn twice is trained once (its second copy would race with the first)
#pragma unroll
                for (int k2 = 1; k2 < k; ++k2)
                    if (tgt[k] >= 0 && tgt[k] == tgt[k2]) tgt[k] = -1;
                if (tgt[k] >= 0) n[k] = load_row<VPL, MODE>(a.w.syn1neg, tgt[k], a.w.row_stride, lane);
#pragma unroll
                for (int v = 0; v < VPL; ++v) {
                    if (tgt[k] < 0) n[k].v[v] = 0.f;
                    dn[k].v[v] = 0.f;
                }
            }
            for (int j = lo; j < hi; ++j) {
                if (j == i) continue;
                const int32_t xj = __builtin_amdgcn_readfirstlane(sent[j]);
                Row<VPL> h = load_row<VPL, MODE>(a.w.syn0, xj, a.w.row_stride, lane);
                float p[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float acc = 0.f;
#pragma unroll
                    for (int v = 0; v < VPL; ++v) acc = fmaf(h.v[v], n[k].v[v], acc);
                    p[k] = acc;
                }
                const float f = reduce8(p, lane);
                const float g = target_gradient(f, my_k == 0 ? 1.f : 0.f, alpha);
                Row<VPL> work;
#pragma unroll
                for (int v = 0; v < VPL; ++v) work.v[v] = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (tgt[k] < 0) continue;
                    const float gk = __builtin_bit_cast(
                        float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g), bitrev3(k)));
                    if (gk == 0.f) continue;
#pragma unroll
                    for (int v = 0; v < VPL; ++v) {
                        work.v[v] = fmaf(gk, n[k].v[v], work.v[v]);
                        const float d = gk * h.v[v];
                        n[k].v[v] += d;
                        dn[k].v[v] += d;
                    }
                }
                if constexpr (MODE == kAtomic) {
                    add_row<VPL>(a.w.syn0, xj, a.w.row_stride, lane, work);
                } else {
#pragma unroll
                    for (int v = 0; v < VPL; ++v) h.v[v] += work.v[v];
                    store_row<VPL, MODE>(a.w.syn0, xj, a.w.row_stride, lane, h);
                }
                ++pairs_done;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (tgt[k] < 0) continue;
                if constexpr (MODE == kAtomic) add_row<VPL>(a.w.syn1neg, tgt[k], a.w.row_stride, lane, dn[k]);
                else store_row<VPL, MODE>(a.w.syn1neg, tgt[k], a.w.row_stride, lane, n[k]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (a.w.count && lane == 0 && pairs_done) atomicAdd(a.w.count, pairs_done);
}

// syn0 ~ U(-0.5/d, 0.5/d), syn1neg = 0 (gensim reset_weights); one Philox call per 4 floats,
// keyed by the seed and counted by (row, column block) so a row does not depend on n_words.
__global__ void __launch_bounds__(256)
sgns_init_kernel(float* syn0, float* syn1neg, int64_t n_words, int32_t dim, int32_t stride, uint64_t seed) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one thread per 4 columns
    const int blocks_per_row = stride / 4;
    const int64_t row = idx / blocks_per_row;
    const int cb = (int)(idx - row * blocks_per_row);
    if (row >= n_words) return;
    uint32_t rr[4];
    n2v::philox4x32_10(seed, (uint32_t)row, (uint32_t)(row >> 32), (uint32_t)cb, 0x5EEDu, rr);
    float4 o, z = make_float4(0.f, 0.f, 0.f, 0.f);
    float* po = &o.x;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int colx = cb * 4 + t;
        const float u = (float)(rr[t] >> 8) * (1.0f / 16777216.0f);  // [0,1), 24 bits
        po[t] = colx < dim ? (u - 0.5f) / (float)dim : 0.f;
    }
    *reinterpret_cast<float4*>(syn0 + row * stride + cb * 4) = o;
    *reinterpret_cast<float4*>(syn1neg + row * stride + cb * 4) = z;
}

__global__ void __launch_bounds__(256)
neg_lut_kernel(const uint32_t* __restrict__ cum, int64_t n_words, int shift, int64_t n_buckets, uint32_t* __restrict__ lut) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b > n_buckets) return;
    const uint64_t key = (uint64_t)b << shift;
    int64_t lo = 0, hi = n_words;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((uint64_t)cum[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    lut[b] = (uint32_t)lo;
}


}  // namespace

extern "C" int n2v_build_neg_lut(const uint32_t* cum_table, int64_t n_words, int32_t lut_bits, uint32_t* lut,
                                 void* stream) {
    if (!cum_table || !lut || n_words <= 0 || n_words >= ((int64_t)1 << 32) || lut_bits < 1 || lut_bits > 24)
        return n2v::fail(N2V_ERR_INVALID, "n2v_build_neg_lut: bad argument (n_words %lld, lut_bits %d)",
                         (long long)n_words, (int)lut_bits);
    const int64_t nb = (int64_t)1 << lut_bits;
    hipLaunchKernelGGL(neg_lut_kernel, dim3(n2v::grid_for(nb + 1, 256)), dim3(256), 0, (hipStream_t)stream, cum_table,
                       n_words, 31 - lut_bits, nb, lut);
    return n2v::check_launch("n2v_build_neg_lut");
}

extern "C" int n2v_sgns_init(float* syn0, float* syn1neg, int64_t n_words, int32_t dim, int32_t row_stride,
                             uint64_t seed, void* stream) {
    if (!syn0 || !syn1neg || n_words < 0 || dim < 1 || row_stride < dim || (row_stride % 4) != 0)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_init: bad argument");
    if (n_words == 0) return N2V_OK;
    const int64_t threads = n_words * (row_stride / 4);
    hipLaunchKernelGGL(sgns_init_kernel, dim3(n2v::grid_for(threads, 256)), dim3(256), 0, (hipStream_t)stream, syn0,
                       syn1neg, n_words, dim, row_stride, seed);
    return n2v::check_launch("n2v_sgns_init");
}

namespace {
struct SpanSpec {                // n2v_sgns_train_span; dyn == NULL: an ordinary launch
    const int64_t* dyn;
    int32_t sub, subs;
    int64_t n_sub_total, n_local, shard_offset;
};

// CUs of the current device (MI355X: 256), asked once
static int64_t n2v_cu_count() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
        else cus = 256;
    }
    return cus;
}

// the default grid's workgroup count (rules (1) and (2) in sgns_launch)
static int64_t default_grid(int64_t n_words, int32_t update_mode) {
    const int64_t cus = n2v_cu_count();
    int64_t cap = 3072;
    if (cap > n_words / 256) cap = n_words / 256 > 16 ? n_words / 256 : 16;
    // store-based rows (agent, plain) need ~4 workgroups per CU for their pair rate (131 019 rows: 256 workgroups 5.0e8
    // pairs/s, 1024 1.09e9) and, with the in-order hand-out, hold the band there (+0.0002 at 1024 ... 2048 workgroups)
    if (update_mode != kAtomic && cap < 4 * cus) cap = 4 * cus;
    if (cap > cus) cap -= cap % cus;
    return cap;
}

int sgns_launch(const char* who, const int32_t* walks, const int32_t* lens, int64_t n_walks, int32_t walk_stride,
                float* syn0, float* syn1neg, int64_t n_words, int32_t dim, int32_t row_stride,
                int32_t window, int32_t negative, const uint32_t* sample_int,
                const uint32_t* cum_table, const uint32_t* lut, int32_t lut_bits, float alpha,
                float min_alpha, int64_t sentences_base, int64_t sentences_step,
                int64_t sentences_total, int64_t alpha_batch,
                uint64_t seed, uint64_t walk_id_base, unsigned long long* pair_count,
                int32_t update_mode, int32_t max_blocks, int32_t walk_splits, const SpanSpec& span,
                unsigned long long* work_counter, void* stream) {
    if (walk_splits < 1 || walk_splits > walk_stride)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: walk_splits %d outside [1, %d]", (int)walk_splits, (int)walk_stride);
    if (n_walks < 0 || walk_stride < 1 || n_words < 1 || dim < 1 || window < 1 || negative < 0 || negative > 64)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: bad size (walks %lld x %d, words %lld, dim %d, window %d, negative %d)",
                         (long long)n_walks, (int)walk_stride, (long long)n_words, (int)dim, (int)window, (int)negative);
    if (n_walks == 0) return N2V_OK;
    if (!walks || !syn0 || !syn1neg || (negative > 0 && (!cum_table || !lut)))
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: null pointer");
    if (row_stride < dim || (row_stride % 64) != 0 || row_stride > 512)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: row_stride %d must be a multiple of 64 in [dim, 512]",
                         (int)row_stride);
    if (lut_bits < 1 || lut_bits > 24) return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: lut_bits %d", (int)lut_bits);
    const bool share = (update_mode & N2V_SGNS_SHARE_NEGATIVES) != 0;
    const bool unchecked = (update_mode & N2V_SGNS_UNCHECKED) != 0;
    update_mode &= ~(N2V_SGNS_SHARE_NEGATIVES | N2V_SGNS_UNCHECKED);
    if (update_mode < kPlain || update_mode > kAtomic)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: update_mode %d", (int)update_mode);
    if (share && negative > 7) return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: shared negatives need negative <= 7");
    if (share && walk_splits != 1) return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: shared negatives need walk_splits == 1");
    // the centres of ONE sentence dealt to several wavefronts update the same context rows at the same instant: with
    // non-atomic read-modify-write rows that is where updates are lost most — never scored against the comparator
    if (walk_splits > 1 && update_mode != kAtomic && !unchecked)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: walk_splits > 1 needs N2V_SGNS_ATOMIC (or N2V_SGNS_UNCHECKED)");
    if (sentences_total < 1 || alpha_batch < 1 || sentences_step < 1) return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: bad schedule");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_exp_table(who)) return rc;

    SgnsArgs a;
    // (the shared-negatives kernel keeps the static stride)
    a.w = w2v_args(syn0, syn1neg, n_words, row_stride, window, negative, sample_int, cum_table, lut, lut_bits, alpha,
                   min_alpha, sentences_base, sentences_step, sentences_total, alpha_batch, seed, walk_id_base, pair_count,
                   share ? nullptr : work_counter, (walk_stride + 63) & ~63);
    a.walks = walks; a.lens = lens; a.n_walks = n_walks; a.walk_stride = walk_stride;
    a.splits = walk_splits;
    a.dyn = span.dyn; a.dyn_sub = span.sub; a.dyn_subs = span.subs;
    a.dyn_n_sub_total = span.n_sub_total; a.dyn_n_local = span.n_local; a.dyn_shard_offset = span.shard_offset;
    const size_t shmem = (size_t)4 * a.w.lpad * sizeof(int32_t);
    if (a.w.lpad > kSlotTokens)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: walk_stride %d too long", (int)walk_stride);
    // default grid: 256 CUs x 12 workgroups of 4 waves (measured on C3: 2048 blocks 6.9e8 pairs/s, 3072 8.2e8, 4096
    // 8.0e8, 6144 8.3e8; at 8 waves per SIMD 8 of the 12 are resident at a time and the others follow as slots free up —
    // harmless with the in-order hand-out, and the reason the static stride lost the band at large grids: a workgroup
    // that starts late trains its whole strided share of the corpus after everybody else) — but
    //  (1) never more than one wavefront per 64 vocabulary rows: the racing waves read each other's rows stale, and
    //      the link-prediction AUC moves away from the sequential algorithm's in proportion to waves in flight per row.
    //      Against the sequential comparator (tests/probes/grid_band_probe.py, profiles/r03/logs), 131 019-row hub graph:
    //      3072 workgroups -0.0022 (atomic) / -0.0013 (agent), 1024 -0.0005 / -0.0008, 512 -0.0002 / -0.0002, 256 +0.0001 /
    //      -0.0001; 399 846 rows: 3072 -0.0023 / -0.0001, 1536 -0.0016 / -0.0005, 768 -0.0006 / -0.0002;
    //  (2) a whole number of workgroups per CU once there is more than one: with 6 workgroups on most CUs and 7 on a few,
    //      the waves of the fuller CUs fall behind, the pass takes 26 % longer and the AUC drops by 0.004 (399 846 rows:
    //      grids 1560 / 1561 / 1562 / 1600 -0.0041 ... -0.0042 in 4.35 s, 1536 -0.0005 in 3.44 s —
    //      tests/probes/grid_resonance_probe.py).  C3 (10^6 rows) keeps its 3072 = 12 x 256.
    // Both were measured with the static grid stride; with the in-order hand-out (next_item) the AUC no longer depends on
    // the grid (lossless rows: within 3e-5 of the comparator from 768 to 3072 workgroups).  The rules stay: they are what
    // the test suite validated, and they cost no speed.
    dim3 grid;
    const dim3 block(256);
    if (int rc = w2v_grid(who, n_walks * walk_splits, max_blocks > 0 ? max_blocks : default_grid(n_words, update_mode), a.w,
                          st, &grid))
        return rc;
#define N2V_SGNS_LAUNCH_M(V, M)                                                            \
    if (share) hipLaunchKernelGGL((sgns_shared_kernel<V, M>), grid, block, shmem, st, a);     \
    else if (negative <= 5) hipLaunchKernelGGL((sgns_kernel<V, 6, M>), grid, block, shmem, st, a); \
    else hipLaunchKernelGGL((sgns_kernel<V, 8, M>), grid, block, shmem, st, a)
#define N2V_SGNS_LAUNCH(V)                                   \
    if (update_mode == kPlain) { N2V_SGNS_LAUNCH_M(V, kPlain); }        \
    else if (update_mode == kAgent) { N2V_SGNS_LAUNCH_M(V, kAgent); }   \
    else { N2V_SGNS_LAUNCH_M(V, kAtomic); }
    switch (row_stride / 64) {
        case 1: N2V_SGNS_LAUNCH(1); break;
        case 2: N2V_SGNS_LAUNCH(2); break;
        case 4: N2V_SGNS_LAUNCH(4); break;
        case 8: N2V_SGNS_LAUNCH(8); break;
        default:
            return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train: row_stride %d must be 64, 128, 256 or 512", (int)row_stride);
    }
    return n2v::check_launch(who);
}
}  // namespace

extern "C" int n2v_sgns_train(const int32_t* walks, const int32_t* lens, int64_t n_walks, int32_t walk_stride,
                              float* syn0, float* syn1neg, int64_t n_words, int32_t dim, int32_t row_stride,
                              int32_t window, int32_t negative, const uint32_t* sample_int,
                              const uint32_t* cum_table, const uint32_t* lut, int32_t lut_bits, float alpha,
                              float min_alpha, int64_t sentences_base, int64_t sentences_step,
                              int64_t sentences_total, int64_t alpha_batch,
                              uint64_t seed, uint64_t walk_id_base, unsigned long long* pair_count,
                              int32_t update_mode, int32_t max_blocks, int32_t walk_splits,
                              unsigned long long* work_counter, void* stream) {
    return sgns_launch("n2v_sgns_train", walks, lens, n_walks, walk_stride, syn0, syn1neg, n_words, dim, row_stride, window,
                       negative, sample_int, cum_table, lut, lut_bits, alpha, min_alpha, sentences_base, sentences_step,
                       sentences_total, alpha_batch, seed, walk_id_base, pair_count, update_mode, max_blocks, walk_splits,
                       SpanSpec{nullptr, 0, 1, 1, 0, 0}, work_counter, stream);
}

extern "C" int n2v_sgns_train_span(const int32_t* walks, const int32_t* lens, int64_t n_local, int32_t walk_stride,
                                   float* syn0, float* syn1neg, int64_t n_words, int32_t dim, int32_t row_stride,
                                   int32_t window, int32_t negative, const uint32_t* sample_int,
                                   const uint32_t* cum_table, const uint32_t* lut, int32_t lut_bits, float alpha,
                                   float min_alpha, int64_t sentences_step, int64_t sentences_total, int64_t alpha_batch,
                                   uint64_t seed, unsigned long long* pair_count, int32_t update_mode, int32_t max_blocks,
                                   int32_t walk_splits, const int64_t* interval_state, int32_t sub_index,
                                   int32_t subs_per_interval, int64_t n_sub_total, int64_t shard_offset,
                                   unsigned long long* work_counter, void* stream) {
    if (!interval_state || subs_per_interval < 1 || sub_index < 0 || sub_index >= subs_per_interval || n_sub_total < subs_per_interval ||
        (n_sub_total % subs_per_interval) != 0 || n_local < 0 || shard_offset < 0)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_train_span: bad span (sub %d of %d, %lld sub-intervals, %lld walks)",
                         (int)sub_index, (int)subs_per_interval, (long long)n_sub_total, (long long)n_local);
    // the launch is sized for the longest sub-interval (they differ by at most one walk); the kernel reads its own range
    const int64_t max_walks = (n_local + n_sub_total - 1) / n_sub_total;
    if (max_walks == 0) return N2V_OK;
    return sgns_launch("n2v_sgns_train_span", walks, lens, max_walks, walk_stride, syn0, syn1neg, n_words, dim, row_stride, window,
                       negative, sample_int, cum_table, lut, lut_bits, alpha, min_alpha, 0, sentences_step, sentences_total,
                       alpha_batch, seed, 0, pair_count, update_mode, max_blocks, walk_splits,
                       SpanSpec{interval_state, sub_index, subs_per_interval, n_sub_total, n_local, shard_offset}, work_counter, stream);
}

extern "C" int32_t n2v_sgns_default_blocks(int64_t n_words, int32_t update_mode) {
    return (int32_t)default_grid(n_words < 0 ? 0 : n_words, update_mode & 3);
}
