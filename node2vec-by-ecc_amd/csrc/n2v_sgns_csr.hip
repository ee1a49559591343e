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
// The pair step is sg_centre_step (n2v_w2v_device.h), the one sgns_kernel trains through, at MODE = kAtomic.  What is new
// here is the work item: a sentence of n_s raw tokens is dealt to S_s = ceil(n_s / chunk) wavefronts, item sp of which
// trains the effective centres [sp*n_eff/S_s, (sp+1)*n_eff/S_s) — sgns_kernel's walk_splits with a split count that
// follows the sentence — and stages only those centres plus `window` tokens on each side.  A wave's LDS slot is then
// chunk + 2*window tokens instead of the corpus' longest sentence (one 4 096-token sentence anywhere costs cbow_kernel
// 64 KiB per workgroup, 2 waves per SIMD), and no work item is longer than `chunk` centres (a 4 096-token sentence on ONE
// wavefront is ~65 ms).  chunk == 0: every sentence is one item, the slot is max_len, the kernel is the sequential
// algorithm per sentence.
#include <cmath>
#include <cstdlib>
#include <mutex>

#include "n2v_common.h"

#pragma clang fp contract(fast)

#include "n2v_w2v_device.h"

namespace {

struct SgCsrArgs {
    W2vArgs w;                   // lpad: chunk + 2 * window (chunk == 0: max_len), rounded up to 64
    const int32_t* tokens;
    const int64_t* offsets;
    const int64_t* item_off;     // NULL (chunk == 0: item = sentence), else int64[n_sent + 1]: first item of each sentence
    int64_t n_sent, n_tokens;
    int64_t first_item, n_items;
    int32_t chunk, max_len;
};

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
    int32_t* sent = smem + wv * a.w.lpad;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    const int my_k = bitrev3(lane & 7);  // which of the 8 reduced values this lane ends up holding
    unsigned long long pairs_done = 0;

    for (int64_t k = a.w.work ? next_item(a.w.work, lane) : (int64_t)blockIdx.x * 4 + wv; k < a.n_items;
         k = a.w.work ? next_item(a.w.work, lane) : k + n_waves) {
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
        const uint64_t sid = a.w.id_base + (uint64_t)si;

        // ---- effective sentence: drop tokens < 0 and sub-sampled words, keep order; a chunked item counts first and
        //      then stages its own centres plus `window` tokens on each side
        const int32_t* raw = a.tokens + tb;
        int n_eff, i_begin = 0, i_end, w_lo = 0;
        if (a.chunk == 0) {
            n_eff = stage_sentence<true>(a.w, raw, len, sid, lane, sent, 0, a.w.lpad, false);
            i_end = n_eff;
        } else {
            n_eff = stage_sentence<true>(a.w, raw, len, sid, lane, sent, 0, 0, false);
            i_begin = (int)((int64_t)sp * n_eff / S);
            i_end = (int)((int64_t)(sp + 1) * n_eff / S);   // n_eff <= len <= S * chunk: at most `chunk` centres
            if (i_end > i_begin) {
                w_lo = max(0, i_begin - a.w.window);
                const int w_hi = min(min(n_eff, i_end + a.w.window), w_lo + a.w.lpad);
                stage_sentence<true>(a.w, raw, len, sid, lane, sent, w_lo, w_hi, true);
            }
        }
        slot_staged();
        const float alpha = sentence_alpha(a.w, si);
        uint64_t lcg = sentence_lcg(a.w.seed, sid);
        if (i_begin > 0) lcg = lcg_skip_to_centre(a.w, sid, n_eff, i_begin, lcg, lane);
        // the slot holds the effective indices from w_lo on: `sent - w_lo` points before the slot, and only indices >= w_lo
        // (the centres [i_begin, i_end) and their windows, all staged above) are ever read through it
        for (int i = i_begin; i < i_end; ++i)
            sg_centre_step<VPL, G, kAtomic>(a.w, sent - w_lo, n_eff, i, sid, alpha, lane, my_k, lcg, pairs_done);
        __builtin_amdgcn_wave_barrier();  // the LDS slot is reused by the next item
    }
    if (a.w.count && lane == 0 && pairs_done) atomicAdd(a.w.count, pairs_done);
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
    const char* who = "n2v_sgns_csr_train";
    int32_t slot = 0;
    if (int rc = refuse_ragged(who, true, "", n_sentences, n_tokens, n_words, dim, window, negative, max_len, chunk, update_mode,
                               row_stride, lut_bits, sentences_base, sentences_step, sentences_total, alpha_batch, &slot))
        return rc;
    if (chunk > 0 && !item_off && n_sentences > 0)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: item_off missing with chunk %d > 0", (int)chunk);
    // item_off lives on the device: its last entry is at most n_tokens (an item holds at least one raw token), and it
    // is the sentence count without chunks; the kernel skips whatever item_off itself does not cover
    const int64_t item_bound = chunk > 0 ? n_tokens : n_sentences;
    if (first_item < 0 || n_items < 0 || first_item > item_bound || n_items > item_bound - first_item)
        return n2v::fail(N2V_ERR_INVALID, "n2v_sgns_csr_train: item range [%lld, %lld + %lld) outside item_off (at most %lld items)",
                         (long long)first_item, (long long)first_item, (long long)n_items, (long long)item_bound);
    if (n_sentences == 0 || n_tokens == 0 || n_items == 0) return N2V_OK;
    if (int rc = refuse_ragged_null(who, tokens, offsets, syn0, syn1neg, negative, cum_table, lut)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_exp_table(who)) return rc;

    SgCsrArgs a;
    a.w = w2v_args(syn0, syn1neg, n_words, row_stride, window, negative, sample_int, cum_table, lut, lut_bits, alpha, min_alpha,
                   sentences_base, sentences_step, sentences_total, alpha_batch, seed, sentence_id_base, pair_count,
                   work_counter, slot);
    a.tokens = tokens; a.offsets = offsets; a.item_off = chunk > 0 ? item_off : nullptr;
    a.n_sent = n_sentences; a.n_tokens = n_tokens;
    a.first_item = first_item; a.n_items = n_items;
    a.chunk = chunk; a.max_len = max_len;
    const size_t shmem = (size_t)4 * slot * sizeof(int32_t);   // <= 64 KB by slot <= kSlotTokens
    // the SGNS grid for lossless rows (n2v_sgns_default_blocks: at most one wavefront per 64 vocabulary rows, whole
    // workgroups per CU)
    dim3 grid;
    const dim3 block(256);
    if (int rc = w2v_grid(who, n_items, max_blocks > 0 ? max_blocks : n2v_sgns_default_blocks(n_words, N2V_SGNS_ATOMIC), a.w,
                          st, &grid))
        return rc;
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
