// Skip-gram with negative sampling over a ragged (CSR) sentence corpus — gfx950 kernels.
//
// The other half of gensim 3.2.0's Word2Vec(sentences, ...): sg=1 over the corpus n2v_cbow.hip trains with sg=0.  gensim's
// source is not part of the reference tree; the update rule per (centre, context) pair is sgns_kernel's (n2v_sgns.hip),
// to the letter, and THAT file is its definition (parity with gensim is unpinned; tests/sgns_reference.py is the float64
// restatement, tests/sgcsr_reference.py drives it item by item):
//
//   per sentence: drop tokens < 0 and sub-sampled words (hash32, salt 0x5AB, by raw position); per centre i of the
//   effective sentence rb = hash32(.., i, 0xB17) % window, lo = max(0, i-window+rb), hi = min(n_eff, i+window+1-rb);
//   for every j in [lo, hi), j != i: h = syn0[sent[j]]; targets = sent[i] (label 1) + `negative` draws of the
//   sentence's LCG (a draw equal to the centre is skipped); sequential per target; syn0[sent[j]] += work.
//
// The pair step below is a restatement of n2v_sgns.hip:159-329 with MODE fixed to kAtomic (that file is what bench.py
// times and is not edited; folding the two copies is DESIGN.md 9 item 7).  What is new is the work item: a sentence of
// n_s raw tokens is dealt to S_s = ceil(n_s / chunk) wavefronts, item sp of which trains the effective centres
// [sp*n_eff/S_s, (sp+1)*n_eff/S_s) — sgns_kernel's walk_splits with a split count that follows the sentence — and stages
// only those centres plus `window` tokens on each side.  A wave's LDS slot is then chunk + 2*window tokens instead of
// the corpus' longest sentence (one 4 096-token sentence anywhere costs cbow_kernel 64 KiB per workgroup, 2 waves per
// SIMD), and no work item is longer than `chunk` centres (a 4 096-token sentence on ONE wavefront is ~65 ms).
// chunk == 0: every sentence is one item, the slot is max_len, the kernel is the sequential algorithm per sentence.
#include <cmath>
#include <cstdlib>
#include <mutex>

#include "n2v_common.h"

#pragma clang fp contract(fast)

#include "n2v_w2v_device.h"

namespace {

constexpr int kMaxSlot = 4096;  // tokens of one wave's LDS slot: 4 waves x 4096 x 4 B = the 64 KB a workgroup may ask for

struct SgCsrArgs {
    const int32_t* tokens;
    const int64_t* offsets;
    const int64_t* item_off;     // NULL (chunk == 0: item = sentence), else int64[n_sent + 1]: first item of each sentence
    int64_t n_sent, n_tokens, n_words;
    int64_t first_item, n_items;
    float* syn0;
    float* syn1neg;
    int32_t row_stride;
    int32_t window, negative;
    int32_t chunk, max_len;
    const uint32_t* sample_int;
    const uint32_t* cum_table;
    const uint32_t* lut;
    int32_t lut_shift;  // 31 - lut_bits
    float alpha0, min_alpha;
    int64_t sent_base, sent_step, sent_total, alpha_batch;
    uint64_t seed, sent_id_base;
    unsigned long long* pair_count;
    unsigned long long* work;    // NULL: static grid stride; else the in-order item counter (reset by the launch)
    int32_t lpad;                // LDS slot of a wave: chunk + 2 * window (chunk == 0: max_len), rounded up to 64
    int32_t predraw;             // 1: all negatives of a centre are drawn by the lanes in parallel before its pairs
};

// One ballot pass over the raw sentence tokens[tb, tb + len): returns the number of kept tokens and stores those whose
// effective index e lies in [w_lo, w_hi) at sent[e - w_lo] (w_hi - w_lo <= the slot).  stop: end at the first block
// that reaches w_hi (the count returned is then not the sentence's).
__device__ __forceinline__ int stage(const SgCsrArgs& a, int64_t tb, int len, uint64_t sid, int lane, int32_t* sent,
                                     int w_lo, int w_hi, bool stop) {
    int n_eff = 0;
    for (int base = 0; base < len; base += 64) {
        const int pos = base + lane;
        bool keep = false;
        int32_t tok = -1;
        if (pos < len) {
            tok = a.tokens[tb + pos];
            keep = tok >= 0 && (int64_t)tok < a.n_words;
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

// G = target slots in use per group of 8 (6 when negative <= 5: the centre + 5 draws).
// 8 waves per SIMD as sgns_kernel (the pair chain is latency bound) where a group's rows fit 64 VGPRs: d <= 64, and
// d <= 128 with 6 slots; the others keep the default allocation, which holds the rows in registers without scratch
// (forced to 8 waves, <2, 8> spills 24 bytes per lane).
template <int VPL, int G>
__attribute__((amdgpu_waves_per_eu(VPL * G <= 12 ? 8 : 1, 8)))
__global__ void __launch_bounds__(256) sgns_csr_kernel(SgCsrArgs a) {
    extern __shared__ int32_t smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int32_t* sent = smem + wv * a.lpad;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    const int my_k = bitrev3(lane & 7);  // which of the 8 reduced values this lane ends up holding
    unsigned long long pairs_done = 0;

    for (int64_t k = a.work ? next_item(a.work, lane) : (int64_t)blockIdx.x * 4 + wv; k < a.n_items;
         k = a.work ? next_item(a.work, lane) : k + n_waves) {
        // ---- item -> (sentence si, split sp of S)
        const int64_t item = a.first_item + k;
        int64_t si = item;
        int64_t sp64 = 0;
        if (a.item_off) {
            // the first sentence whose successor starts after `item` (empty sentences own no item); wave-uniform
            int64_t lo = 0, hi = a.n_sent;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (n2v::uni64(a.item_off[mid + 1]) <= item) lo = mid + 1;
                else hi = mid;
            }
            si = lo;
            if (si < a.n_sent) sp64 = item - n2v::uni64(a.item_off[si]);
        }
        if (si < 0 || si >= a.n_sent) continue;
        // a corpus that passed n2v_cbow_corpus_check needs none of these clamps; they keep a malformed one inside
        // tokens[0, T), the LDS slot and the tables
        int64_t tb = n2v::uni64(a.offsets[si]), te = n2v::uni64(a.offsets[si + 1]);
        tb = tb < 0 ? 0 : (tb > a.n_tokens ? a.n_tokens : tb);
        te = te < tb ? tb : (te > a.n_tokens ? a.n_tokens : te);
        const int len = (int)(te - tb > (int64_t)a.max_len ? (int64_t)a.max_len : te - tb);
        const int S = a.chunk > 0 ? (len + a.chunk - 1) / a.chunk : 1;
        if (sp64 < 0 || sp64 >= S) continue;
        const int sp = (int)sp64;
        const uint64_t sid = a.sent_id_base + (uint64_t)si;

        // ---- effective sentence: drop tokens < 0 and sub-sampled words, keep order; a chunked item counts first and
        //      then stages its own centres plus `window` tokens on each side
        int n_eff, i_begin = 0, i_end, w_lo = 0;
        if (a.chunk == 0) {
            n_eff = stage(a, tb, len, sid, lane, sent, 0, a.lpad, false);
            i_end = n_eff;
        } else {
            n_eff = stage(a, tb, len, sid, lane, sent, 0, 0, false);
            i_begin = (int)((int64_t)sp * n_eff / S);
            i_end = (int)((int64_t)(sp + 1) * n_eff / S);   // n_eff <= len <= S * chunk: at most `chunk` centres
            if (i_end > i_begin) {
                w_lo = max(0, i_begin - a.window);
                const int w_hi = min(min(n_eff, i_end + a.window), w_lo + a.lpad);
                stage(a, tb, len, sid, lane, sent, w_lo, w_hi, true);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ---- learning rate of this sentence (gensim: linear decay, stepped per job)
        const int64_t pushed = a.sent_base + (si / a.alpha_batch) * a.alpha_batch * a.sent_step;
        float alpha = a.alpha0 - (a.alpha0 - a.min_alpha) * (float)((double)pushed / (double)a.sent_total);
        alpha = fmaxf(alpha, a.min_alpha);

        uint64_t lcg = mix64(a.seed ^ mix64(sid + 0x632BE59BD9B4E019ULL)) & kLcgMask;
        if (i_begin > 0) {
            // draws of the centres before i_begin: `negative` per (centre, context) pair (n2v_sgns.hip:139-157)
            int pairs_before = 0;
            for (int base = 0; base < i_begin; base += 64) {
                const int i = base + lane;
                int np = 0;
                if (i < i_begin) {
                    const int rb = (int)(hash32(a.seed, sid, (uint32_t)i, 0xB17) % (uint32_t)a.window);
                    const int lo = max(0, i - a.window + rb), hi = min(n_eff, i + a.window + 1 - rb);
                    np = hi - lo > 1 ? hi - lo - 1 : 0;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) np += __shfl_xor(np, o, 64);
                pairs_before += np;
            }
            lcg = lcg_skip(lcg, (uint64_t)pairs_before * (uint64_t)a.negative);
        }

        // ---- the pair step of sgns_kernel (n2v_sgns.hip:159-329), MODE = kAtomic; sent[] is indexed from w_lo
        for (int i = i_begin; i < i_end; ++i) {
            const int32_t ci = __builtin_amdgcn_readfirstlane(sent[i - w_lo]);
            const int rb = (int)(hash32(a.seed, sid, (uint32_t)i, 0xB17) % (uint32_t)a.window);
            const int lo = max(0, i - a.window + rb), hi = min(n_eff, i + a.window + 1 - rb);
            if (hi - lo <= 1) continue;
            Row<VPL> c = load_row<VPL, kAtomic>(a.syn1neg, ci, a.row_stride, lane);
            Row<VPL> cd;  // this wave's accumulated change of the centre row
#pragma unroll
            for (int v = 0; v < VPL; ++v) cd.v[v] = 0.f;
            // predraw: the lanes make ALL draws of the centre at once — draw number d of the centre uses the sentence's
            // LCG advanced d times, exactly the state the pair-by-pair path reaches
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
                const int32_t xj = __builtin_amdgcn_readfirstlane(sent[j - w_lo]);
                Row<VPL> h = load_row<VPL, kAtomic>(a.syn0, xj, a.row_stride, lane);
                Row<VPL> work;
#pragma unroll
                for (int v = 0; v < VPL; ++v) work.v[v] = 0.f;
                // targets are processed 8 at a time: slot 0 of the first group is the centre word
                for (int t0 = 0; t0 < a.negative + 1; t0 += 8) {
                    // lane k (k < 8) draws the target of slot k of this group
                    int32_t my_t = -1;
                    if (pre) {   // negative <= 7: one group, lane k in [1, negative] holds target k
                        const int d = min(max(pidx * a.negative + lane - 1, 0), 127);
                        const int v0 = __builtin_amdgcn_ds_bpermute((d & 63) << 2, drawn0);
                        const int v1 = __builtin_amdgcn_ds_bpermute((d & 63) << 2, drawn1);
                        if (lane >= 1 && lane <= a.negative) my_t = d < 64 ? v0 : v1;
                    } else {
                        const int tk = t0 + lane;  // target number: 0 = positive, d >= 1 = d-th negative
                        if (lane < 8 && tk >= 1 && tk <= a.negative) {
                            uint64_t s = lcg;  // state of the first draw of this group
                            for (int d = max(t0, 1); d < tk; ++d) s = (s * kLcgA + kLcgC) & kLcgMask;
                            const uint32_t r = (uint32_t)((s >> 16) % 2147483647ULL);
                            my_t = draw_target(a.cum_table, a.lut, a.lut_shift, r);
                            if (my_t == ci) my_t = -1;  // `if target_index == word_index: continue`
                        }
                    }
                    int32_t tgt[G];
                    Row<VPL> n[G];
                    float p[8];
#pragma unroll
                    for (int k2 = 0; k2 < G; ++k2) {
                        tgt[k2] = __builtin_amdgcn_readlane(my_t, k2);
                        if (k2 == 0 && t0 == 0) tgt[k2] = ci;
                    }
                    // a row drawn by two slots of the group: the later slot sits out the parallel pass and is trained
                    // after it, from the row as this wave has updated it (see sgns_kernel)
                    uint32_t late = 0;
#pragma unroll
                    for (int k2 = 1; k2 < G; ++k2)
#pragma unroll
                        for (int k1 = 0; k1 < k2; ++k1)
                            if (tgt[k2] >= 0 && tgt[k2] == tgt[k1]) late |= 1u << k2;
#pragma unroll
                    for (int k2 = 0; k2 < G; ++k2) {
                        if (k2 == 0 && t0 == 0) {
                            n[k2] = c;
                        } else if (tgt[k2] >= 0 && !(late >> k2 & 1)) {
                            n[k2] = load_row<VPL, kAtomic>(a.syn1neg, tgt[k2], a.row_stride, lane);
                        } else {
#pragma unroll
                            for (int v = 0; v < VPL; ++v) n[k2].v[v] = 0.f;
                        }
                    }
#pragma unroll
                    for (int k2 = 0; k2 < 8; ++k2) {
                        float acc = 0.f;
                        if (k2 < G) {
#pragma unroll
                            for (int v = 0; v < VPL; ++v) acc = fmaf(h.v[v], n[k2].v[v], acc);
                        }
                        p[k2] = acc;
                    }
                    const float f = reduce8(p, lane);
                    // this lane's own target: sigmoid table, gradient
                    float g = 0.f;
                    if (f > -kMaxExp && f < kMaxExp) {
                        const float sig = c_exp_table[(int)((f + kMaxExp) * (float)(kExpTableSize / (int)kMaxExp / 2))];
                        const float label = (my_k == 0 && t0 == 0) ? 1.f : 0.f;
                        g = (label - sig) * alpha;
                    }
#pragma unroll
                    for (int k2 = 0; k2 < G; ++k2) {
                        if (tgt[k2] < 0 || (late >> k2 & 1)) continue;
                        const float gk = __builtin_bit_cast(
                            float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g), bitrev3(k2)));
                        if (gk == 0.f) continue;  // |f| >= MAX_EXP: no update at all
                        Row<VPL> dn;
#pragma unroll
                        for (int v = 0; v < VPL; ++v) {
                            work.v[v] = fmaf(gk, n[k2].v[v], work.v[v]);
                            dn.v[v] = gk * h.v[v];
                            n[k2].v[v] += dn.v[v];
                        }
                        if (k2 == 0 && t0 == 0) {
                            c = n[k2];
#pragma unroll
                            for (int v = 0; v < VPL; ++v) cd.v[v] += dn.v[v];
                        } else {
                            add_row<VPL>(a.syn1neg, tgt[k2], a.row_stride, lane, dn);
                        }
                    }
                    if (late) {
                        // the repeated slots, in slot order: a negative each (a draw equal to the centre is skipped)
#pragma unroll
                        for (int k2 = 1; k2 < G; ++k2) {
                            if (!(late >> k2 & 1)) continue;
                            Row<VPL> r = load_row<VPL, kAtomic>(a.syn1neg, tgt[k2], a.row_stride, lane);
                            const float gk = negative_gradient<VPL>(h, r, alpha);
                            if (gk == 0.f) continue;
                            Row<VPL> dn;
#pragma unroll
                            for (int v = 0; v < VPL; ++v) {
                                work.v[v] = fmaf(gk, r.v[v], work.v[v]);
                                dn.v[v] = gk * h.v[v];
                            }
                            add_row<VPL>(a.syn1neg, tgt[k2], a.row_stride, lane, dn);
                        }
                    }
                    // advance the sentence's LCG past this group's negatives
                    const int used = min(a.negative, t0 + 7) - max(t0, 1) + 1;
                    for (int d = 0; d < used; ++d) lcg = (lcg * kLcgA + kLcgC) & kLcgMask;
                }
                add_row<VPL>(a.syn0, xj, a.row_stride, lane, work);
                ++pidx;
                ++pairs_done;
            }
            // the centre row sat in registers for the whole window: its accumulated change is added once
            add_row<VPL>(a.syn1neg, ci, a.row_stride, lane, cd);
        }
        __builtin_amdgcn_wave_barrier();  // the LDS slot is reused by the next item
    }
    if (a.pair_count && lane == 0 && pairs_done) atomicAdd(a.pair_count, pairs_done);
}

// predraw: on whenever negative <= 7 (one target group); N2V_SGNS_PREDRAW=0 switches it off — n2v_sgns.hip's rule and switch
int predraw_mode(int negative) {
    if (negative < 1 || negative > 7) return 0;
    const char* e = getenv("N2V_SGNS_PREDRAW");
    return (e && e[0] == '0') ? 0 : 1;
}

}  // namespace

extern "C" int n2v_sgns_csr_train(const int32_t* tokens, const int64_t* offsets, int64_t n_sentences, int64_t n_tokens,
                                  int32_t max_len, const int64_t* item_off, int32_t chunk, int64_t first_item,
                                  int64_t n_items, float* syn0, float* syn1neg, int64_t n_words, int32_t dim,
                                  int32_t row_stride, int32_t window, int32_t negative, const uint32_t* sample_int,
                                  const uint32_t* cum_table, const uint32_t* lut, int32_t lut_bits, float alpha,
                                  float min_alpha, int64_t sentences_base, int64_t sentences_step, int64_t sentences_total,
                                  int64_t alpha_batch, uint64_t seed, uint64_t sentence_id_base,
                                  unsigned long long* pair_count, int32_t update_mode, int32_t max_blocks,
                                  unsigned long long* work_counter, void* stream) {
    if (n_sentences < 0 || n_tokens < 0 || n_words < 1 || n_words > 0x7fffffffLL || dim < 1 || window < 1 || negative < 0 ||
        negative > 64)
        return n2v::fail(N2V_ERR_INVALID,
                         "n2v_sgns_csr_train: bad size (sentences %lld, tokens %lld, words %lld, dim %d, window %d, negative %d)",
                         (long long)n_sentences, (long long)n_tokens, (long long)n_words, (int)dim, (int)window, (int)negative);
    if (max_len < 1 || max_len > kMaxSlot)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: max_len %d outside [1, %d]", (int)max_len, kMaxSlot);
    if (chunk < 0) return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: chunk %d is negative", (int)chunk);
    const int64_t slot = ((chunk > 0 ? (int64_t)chunk + 2 * (int64_t)window : (int64_t)max_len) + 63) & ~(int64_t)63;
    if (slot > kMaxSlot)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: slot of %lld tokens (chunk %d + 2 x window %d) above %d",
                         (long long)slot, (int)chunk, (int)window, kMaxSlot);
    if (update_mode != N2V_SGNS_ATOMIC)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: update_mode %d: only N2V_SGNS_ATOMIC (lossless rows) is offered",
                         (int)update_mode);
    if (row_stride < dim || (row_stride != 64 && row_stride != 128 && row_stride != 256 && row_stride != 512))
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: row_stride %d must be 64, 128, 256 or 512 and >= dim %d",
                         (int)row_stride, (int)dim);
    if (lut_bits < 1 || lut_bits > 24) return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: lut_bits %d", (int)lut_bits);
    if (sentences_total < 1 || alpha_batch < 1 || sentences_step < 1 || sentences_base < 0)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: bad schedule");
    if (chunk > 0 && !item_off && n_sentences > 0)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: item_off missing with chunk %d > 0", (int)chunk);
    // item_off lives on the device: its last entry is at most n_tokens (an item holds at least one raw token), and it
    // is the sentence count without chunks; the kernel skips whatever item_off itself does not cover
    const int64_t item_bound = chunk > 0 ? n_tokens : n_sentences;
    if (first_item < 0 || n_items < 0 || first_item > item_bound || n_items > item_bound - first_item)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: item range [%lld, %lld + %lld) outside item_off (at most %lld items)",
                         (long long)first_item, (long long)first_item, (long long)n_items, (long long)item_bound);
    if (n_sentences == 0 || n_tokens == 0 || n_items == 0) return N2V_OK;
    if (!tokens || !offsets || !syn0 || !syn1neg || (negative > 0 && (!cum_table || !lut)))
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_exp_table()) return rc;

    SgCsrArgs a;
    a.tokens = tokens; a.offsets = offsets; a.item_off = chunk > 0 ? item_off : nullptr;
    a.n_sent = n_sentences; a.n_tokens = n_tokens; a.n_words = n_words;
    a.first_item = first_item; a.n_items = n_items;
    a.syn0 = syn0; a.syn1neg = syn1neg; a.row_stride = row_stride;
    a.window = window; a.negative = negative; a.chunk = chunk; a.max_len = max_len; a.sample_int = sample_int;
    a.cum_table = cum_table; a.lut = lut; a.lut_shift = 31 - lut_bits;
    a.alpha0 = alpha; a.min_alpha = min_alpha;
    a.sent_base = sentences_base; a.sent_step = sentences_step; a.sent_total = sentences_total;
    a.alpha_batch = alpha_batch;
    a.seed = seed; a.sent_id_base = sentence_id_base; a.pair_count = pair_count;
    a.work = work_counter;
    a.lpad = (int32_t)slot;
    a.predraw = predraw_mode(negative);
    const size_t shmem = (size_t)4 * a.lpad * sizeof(int32_t);   // <= 64 KB by slot <= kMaxSlot
    int64_t blocks = (n_items + 3) / 4;
    // the SGNS grid for lossless rows (n2v_sgns_default_blocks: at most one wavefront per 64 vocabulary rows, whole
    // workgroups per CU)
    const int64_t cap = max_blocks > 0 ? max_blocks : n2v_sgns_default_blocks(n_words, N2V_SGNS_ATOMIC);
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks), block(256);
    if (n_items <= blocks * 4) a.work = nullptr;   // no wave gets a second item: no hand-out needed
    if (a.work && hipMemsetAsync(a.work, 0, sizeof(unsigned long long), st) != hipSuccess)
        return n2v::fail(N2V_ERR_HIP, "n2v_sgns_csr_train: resetting the work counter failed");
#define N2V_SGCSR_LAUNCH(V)                                                                          \
    if (negative <= 5) hipLaunchKernelGGL((sgns_csr_kernel<V, 6>), grid, block, shmem, st, a);       \
    else hipLaunchKernelGGL((sgns_csr_kernel<V, 8>), grid, block, shmem, st, a)
    switch (row_stride / 64) {
        case 1: N2V_SGCSR_LAUNCH(1); break;
        case 2: N2V_SGCSR_LAUNCH(2); break;
        case 4: N2V_SGCSR_LAUNCH(4); break;
        default: N2V_SGCSR_LAUNCH(8); break;
    }
#undef N2V_SGCSR_LAUNCH
    return n2v::check_launch("n2v_sgns_csr_train");
}
