// CBOW with negative sampling over a ragged (CSR) sentence corpus — gfx950 kernels.
//
// Replaces what src/extract_playlist.py:31-34 hands to gensim 3.2.0: Word2Vec(sentences, min_count=5), i.e. sg=0,
// cbow_mean=1, size 100, window 5, negative 5.  gensim's source is not part of the reference tree; the rule below
// restates its `fast_sentence_cbow_neg` (word2vec_inner.pyx) from memory and IS the definition (DESIGN.md 4.14;
// tests/cbow_reference.py is its float64 restatement):
//
//   per sentence: drop sub-sampled words; per centre i draw rb in [0, window); lo = max(0, i-window+rb),
//   hi = min(n_eff, i+window+1-rb); no context: nothing is trained and nothing drawn.  count = hi-lo-1,
//   neu1 = sum of syn0[sent[m]], m = lo..hi-1, m != i, in ascending m (times 1/count when cbow_mean);
//   targets = word_i (label 1) + `negative` draws (a draw equal to word_i is skipped); f = <neu1, syn1neg[t]>;
//   |f| >= 6 skips; g = (label - sigmoid_table[f]) * alpha; work += g * syn1neg[t]; syn1neg[t] += g * neu1;
//   (work *= 1/count when not cbow_mean); finally syn0[sent[m]] += work for every m of the window.
//
// Mapping to the machine: the one of n2v_sgns.hip.  One wavefront owns one sentence at a time (handed out in order
// by a device counter) and stages it in LDS; a row of 64*VPL floats is VPL floats per lane; neu1 and work live in
// registers; the targets go 8 at a time through reduce8, a row drawn by two slots of a group is trained after the
// group's parallel pass from the row as the earlier slot left it.  Rows are read with agent-scope loads and changed
// with memory-side float atomics only: the context rows are held (as neu1) for the whole target pass, so a whole-row
// store would erase what other wavefronts added meanwhile.  No lossy mode is offered.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "n2v_common.h"

#pragma clang fp contract(fast)

#include "n2v_w2v_device.h"

namespace {

struct CbowArgs {
    W2vArgs w;                   // count: centres trained; lpad >= max_len
    const int32_t* tokens;
    const int64_t* offsets;
    int64_t n_sent, n_tokens;
    int32_t cbow_mean;
};

// G = target slots in use per group of 8 (6 when negative <= 5: the centre + 5 draws)
template <int VPL, int G>
__global__ void __launch_bounds__(256) cbow_kernel(CbowArgs a) {
    extern __shared__ int32_t smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int32_t* sent = smem + wv * a.w.lpad;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    const int my_k = bitrev3(lane & 7);  // which of the 8 reduced values this lane ends up holding
    unsigned long long centres_done = 0;

    for (int64_t si = a.w.work ? next_item(a.w.work, lane) : (int64_t)blockIdx.x * 4 + wv; si < a.n_sent;
         si = a.w.work ? next_item(a.w.work, lane) : si + n_waves) {
        // a corpus that passed n2v_cbow_corpus_check needs none of these clamps; they keep a malformed one inside
        // tokens[0, T), the LDS slot and the tables
        int64_t tb = n2v::uni64(a.offsets[si]), te = n2v::uni64(a.offsets[si + 1]);
        tb = tb < 0 ? 0 : (tb > a.n_tokens ? a.n_tokens : tb);
        te = te < tb ? tb : (te > a.n_tokens ? a.n_tokens : te);
        const int len = (int)(te - tb > (int64_t)a.w.lpad ? (int64_t)a.w.lpad : te - tb);
        const uint64_t sid = a.w.id_base + (uint64_t)si;
        const int n_eff = stage_sentence<true>(a.w, a.tokens + tb, len, sid, lane, sent, 0, a.w.lpad, false);
        slot_staged();
        const float alpha = sentence_alpha(a.w, si);
        uint64_t lcg = sentence_lcg(a.w.seed, sid);

        for (int i = 0; i < n_eff; ++i) {
            const Window w = shrunk_window(a.w, sid, i, n_eff);
            const int lo = w.lo, hi = w.hi;
            if (hi - lo <= 1) continue;
            const int32_t ci = __builtin_amdgcn_readfirstlane(sent[i]);
            const float inv = 1.0f / (float)(hi - lo - 1);
            // ---- neu1: the context rows, summed in ascending position
            Row<VPL> neu1, work;
#pragma unroll
            for (int v = 0; v < VPL; ++v) neu1.v[v] = work.v[v] = 0.f;
            for (int m = lo; m < hi; ++m) {
                if (m == i) continue;
                const int32_t xm = __builtin_amdgcn_readfirstlane(sent[m]);
                const Row<VPL> r = load_row<VPL, kAtomic>(a.w.syn0, xm, a.w.row_stride, lane);
#pragma unroll
                for (int v = 0; v < VPL; ++v) neu1.v[v] += r.v[v];
            }
            if (a.cbow_mean) {
#pragma unroll
                for (int v = 0; v < VPL; ++v) neu1.v[v] *= inv;
            }
            // ---- targets, 8 at a time: slot 0 of the first group is the centre word
            for (int t0 = 0; t0 < a.w.negative + 1; t0 += 8) {
                const int32_t my_t = draw_group_target(a.w, lcg, t0, ci, lane);
                int32_t tgt[G];
                Row<VPL> n[G];
                float p[8];
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    tgt[k] = __builtin_amdgcn_readlane(my_t, k);
                    if (k == 0 && t0 == 0) tgt[k] = ci;
                }
                const uint32_t late = late_slots<G>(tgt);
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    if (tgt[k] >= 0 && !(late >> k & 1)) {
                        n[k] = load_row<VPL, kAtomic>(a.w.syn1neg, tgt[k], a.w.row_stride, lane);
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
                        for (int v = 0; v < VPL; ++v) acc = fmaf(neu1.v[v], n[k].v[v], acc);
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
                        dn.v[v] = gk * neu1.v[v];
                    }
                    add_row<VPL>(a.w.syn1neg, tgt[k], a.w.row_stride, lane, dn);
                }
                if (late) {
                    // the repeated slots, in slot order: a negative each, from the row as memory holds it by now
#pragma unroll
                    for (int k = 1; k < G; ++k) {
                        if (!(late >> k & 1)) continue;
                        const Row<VPL> r = load_row<VPL, kAtomic>(a.w.syn1neg, tgt[k], a.w.row_stride, lane);
                        const float gk = negative_gradient<VPL>(neu1, r, alpha);
                        if (gk == 0.f) continue;
                        Row<VPL> dn;
#pragma unroll
                        for (int v = 0; v < VPL; ++v) {
                            work.v[v] = fmaf(gk, r.v[v], work.v[v]);
                            dn.v[v] = gk * neu1.v[v];
                        }
                        add_row<VPL>(a.w.syn1neg, tgt[k], a.w.row_stride, lane, dn);
                    }
                }
                lcg = lcg_past_group(lcg, a.w.negative, t0);
            }
            if (!a.cbow_mean) {
#pragma unroll
                for (int v = 0; v < VPL; ++v) work.v[v] *= inv;
            }
            // ---- every context position gets the whole of work (a word twice in the window: twice)
            for (int m = lo; m < hi; ++m) {
                if (m == i) continue;
                const int32_t xm = __builtin_amdgcn_readfirstlane(sent[m]);
                add_row<VPL>(a.w.syn0, xm, a.w.row_stride, lane, work);
            }
            ++centres_done;
        }
        __builtin_amdgcn_wave_barrier();  // LDS sentence is reused by the next one
    }
    if (a.w.count && lane == 0 && centres_done) atomicAdd(a.w.count, centres_done);
}

// integers only: one lane per sentence and per token; reads offsets[0 .. S] and tokens[0 .. T) of the CLAIMED sizes
__global__ void __launch_bounds__(256)
cbow_corpus_check_kernel(const int32_t* __restrict__ tokens, const int64_t* __restrict__ offsets, int64_t S, int64_t T,
                         int64_t n_words, int64_t max_len, int32_t* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t bad = 0;
    if (t == 0) {
        if (offsets[0] != 0) bad |= N2V_CBOW_BAD_START;
        if (offsets[S] != T) bad |= N2V_CBOW_BAD_END;
    }
    if (t < S) {
        const int64_t b = offsets[t], e = offsets[t + 1];
        if (e < b) bad |= N2V_CBOW_BAD_ORDER;
        else if (e - b > max_len) bad |= N2V_CBOW_BAD_LENGTH;
    }
    if (t < T && (int64_t)tokens[t] >= n_words) bad |= N2V_CBOW_BAD_TOKEN;
    if (bad) atomicOr(status, bad);
}

}  // namespace

extern "C" int32_t n2v_cbow_max_sentence(void) { return kSlotTokens; }

extern "C" int n2v_cbow_corpus_check(const int32_t* tokens, const int64_t* offsets, int64_t n_sentences, int64_t n_tokens,
                                     int64_t n_words, int32_t max_len, int32_t* status, void* stream) {
    if (n_sentences < 0 || n_tokens < 0 || n_words < 1 || n_words > 0x7fffffffLL || max_len < 1 || max_len > kSlotTokens)
        return n2v::fail(N2V_ERR_INVALID, "n2v_cbow_corpus_check: bad size (sentences %lld, tokens %lld, words %lld, max_len %d)",
                         (long long)n_sentences, (long long)n_tokens, (long long)n_words, (int)max_len);
    if (!offsets || !status || (n_tokens > 0 && !tokens)) return n2v::fail(N2V_ERR_INVALID, "n2v_cbow_corpus_check: null pointer");
    const int64_t lanes = n_sentences > n_tokens ? n_sentences : n_tokens;
    if (lanes > (int64_t)0x7fffffff * 256) return n2v::fail(N2V_ERR_INVALID, "n2v_cbow_corpus_check: corpus too large");
    hipLaunchKernelGGL(cbow_corpus_check_kernel, dim3(n2v::grid_for(lanes > 0 ? lanes : 1, 256)), dim3(256), 0,
                       (hipStream_t)stream, tokens, offsets, n_sentences, n_tokens, n_words, (int64_t)max_len, status);
    return n2v::check_launch("n2v_cbow_corpus_check");
}

extern "C" int n2v_cbow_train(const int32_t* tokens, const int64_t* offsets, int64_t n_sentences, int64_t n_tokens,
                              int32_t max_len, float* syn0, float* syn1neg, int64_t n_words, int32_t dim, int32_t row_stride,
                              int32_t window, int32_t negative, int32_t cbow_mean, const uint32_t* sample_int,
                              const uint32_t* cum_table, const uint32_t* lut, int32_t lut_bits, float alpha, float min_alpha,
                              int64_t sentences_base, int64_t sentences_step, int64_t sentences_total, int64_t alpha_batch,
                              uint64_t seed, uint64_t sentence_id_base, unsigned long long* pair_count, int32_t update_mode,
                              int32_t max_blocks, unsigned long long* work_counter, void* stream) {
    const char* who = "n2v_cbow_train";
    char size_tail[32];
    snprintf(size_tail, sizeof(size_tail), ", cbow_mean %d", (int)cbow_mean);
    int32_t slot = 0;
    if (int rc = refuse_ragged(who, cbow_mean == 0 || cbow_mean == 1, size_tail, n_sentences, n_tokens, n_words, dim, window,
                               negative, max_len, 0, update_mode, row_stride, lut_bits, sentences_base, sentences_step,
                               sentences_total, alpha_batch, &slot))
        return rc;
    if (n_sentences == 0 || n_tokens == 0) return N2V_OK;
    if (int rc = refuse_ragged_null(who, tokens, offsets, syn0, syn1neg, negative, cum_table, lut)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_exp_table(who)) return rc;

    CbowArgs a;
    a.w = w2v_args(syn0, syn1neg, n_words, row_stride, window, negative, sample_int, cum_table, lut, lut_bits, alpha, min_alpha,
                   sentences_base, sentences_step, sentences_total, alpha_batch, seed, sentence_id_base, pair_count,
                   work_counter, slot);
    a.tokens = tokens; a.offsets = offsets; a.n_sent = n_sentences; a.n_tokens = n_tokens; a.cbow_mean = cbow_mean;
    const size_t shmem = (size_t)4 * slot * sizeof(int32_t);   // <= 64 KB by max_len <= kSlotTokens
    // the SGNS grid for lossless rows (n2v_sgns_default_blocks: at most one wavefront per 64 vocabulary rows, whole
    // workgroups per CU); nothing about CBOW was scored against a comparator at any grid
    dim3 grid;
    const dim3 block(256);
    if (int rc = w2v_grid(who, n_sentences, max_blocks > 0 ? max_blocks : n2v_sgns_default_blocks(n_words, N2V_SGNS_ATOMIC),
                          a.w, st, &grid))
        return rc;
#define N2V_CBOW_LAUNCH(V)                                                                       \
    if (negative <= 5) hipLaunchKernelGGL((cbow_kernel<V, 6>), grid, block, shmem, st, a);       \
    else hipLaunchKernelGGL((cbow_kernel<V, 8>), grid, block, shmem, st, a)
    switch (row_stride / 64) {
        case 1: N2V_CBOW_LAUNCH(1); break;
        case 2: N2V_CBOW_LAUNCH(2); break;
        case 4: N2V_CBOW_LAUNCH(4); break;
        default: N2V_CBOW_LAUNCH(8); break;
    }
#undef N2V_CBOW_LAUNCH
    return n2v::check_launch("n2v_cbow_train");
}
