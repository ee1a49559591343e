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
#include <cstdlib>
#include <mutex>

#include "n2v_common.h"

#pragma clang fp contract(fast)

#include "n2v_w2v_device.h"

namespace {

constexpr int kMaxSentence = 4096;  // tokens of one sentence: 4 waves x 4096 x 4 B = the 64 KB of LDS a workgroup may ask for

struct CbowArgs {
    const int32_t* tokens;
    const int64_t* offsets;
    int64_t n_sent, n_tokens, n_words;
    float* syn0;
    float* syn1neg;
    int32_t row_stride;
    int32_t window, negative, cbow_mean;
    const uint32_t* sample_int;
    const uint32_t* cum_table;
    const uint32_t* lut;
    int32_t lut_shift;  // 31 - lut_bits
    float alpha0, min_alpha;
    int64_t sent_base, sent_step, sent_total, alpha_batch;
    uint64_t seed, sent_id_base;
    unsigned long long* centre_count;
    unsigned long long* work;    // NULL: static grid stride; else the in-order item counter (reset by the launch)
    int32_t lpad;                // LDS slot of a wave, >= max_len
};

// G = target slots in use per group of 8 (6 when negative <= 5: the centre + 5 draws)
template <int VPL, int G>
__global__ void __launch_bounds__(256) cbow_kernel(CbowArgs a) {
    extern __shared__ int32_t smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int32_t* sent = smem + wv * a.lpad;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    const int my_k = bitrev3(lane & 7);  // which of the 8 reduced values this lane ends up holding
    unsigned long long centres_done = 0;

    for (int64_t si = a.work ? next_item(a.work, lane) : (int64_t)blockIdx.x * 4 + wv; si < a.n_sent;
         si = a.work ? next_item(a.work, lane) : si + n_waves) {
        // a corpus that passed n2v_cbow_corpus_check needs none of these clamps; they keep a malformed one inside
        // tokens[0, T), the LDS slot and the tables
        int64_t tb = n2v::uni64(a.offsets[si]), te = n2v::uni64(a.offsets[si + 1]);
        tb = tb < 0 ? 0 : (tb > a.n_tokens ? a.n_tokens : tb);
        te = te < tb ? tb : (te > a.n_tokens ? a.n_tokens : te);
        const int len = (int)(te - tb > (int64_t)a.lpad ? (int64_t)a.lpad : te - tb);
        const uint64_t sid = a.sent_id_base + (uint64_t)si;
        // ---- effective sentence: drop tokens < 0 and sub-sampled words, keep order
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
            if (keep) sent[n_eff + __popcll(m & ((1ULL << lane) - 1ULL))] = tok;
            n_eff += __popcll(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ---- learning rate of this sentence (gensim: linear decay, stepped per job)
        const int64_t pushed = a.sent_base + (si / a.alpha_batch) * a.alpha_batch * a.sent_step;
        float alpha = a.alpha0 - (a.alpha0 - a.min_alpha) * (float)((double)pushed / (double)a.sent_total);
        alpha = fmaxf(alpha, a.min_alpha);

        uint64_t lcg = mix64(a.seed ^ mix64(sid + 0x632BE59BD9B4E019ULL)) & kLcgMask;

        for (int i = 0; i < n_eff; ++i) {
            const int rb = (int)(hash32(a.seed, sid, (uint32_t)i, 0xB17) % (uint32_t)a.window);
            const int lo = max(0, i - a.window + rb), hi = min(n_eff, i + a.window + 1 - rb);
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
                const Row<VPL> r = load_row<VPL, kAtomic>(a.syn0, xm, a.row_stride, lane);
#pragma unroll
                for (int v = 0; v < VPL; ++v) neu1.v[v] += r.v[v];
            }
            if (a.cbow_mean) {
#pragma unroll
                for (int v = 0; v < VPL; ++v) neu1.v[v] *= inv;
            }
            // ---- targets, 8 at a time: slot 0 of the first group is the centre word
            for (int t0 = 0; t0 < a.negative + 1; t0 += 8) {
                // lane k (k < 8) draws the target of slot k of this group
                int32_t my_t = -1;
                const int tk = t0 + lane;  // target number: 0 = positive, d >= 1 = d-th negative
                if (lane < 8 && tk >= 1 && tk <= a.negative) {
                    uint64_t s = lcg;  // state of the first draw of this group
                    for (int d = max(t0, 1); d < tk; ++d) s = (s * kLcgA + kLcgC) & kLcgMask;
                    my_t = draw_target(a.cum_table, a.lut, a.lut_shift, (uint32_t)((s >> 16) % 2147483647ULL));
                    if (my_t == ci) my_t = -1;  // `if target_index == word_index: continue`
                }
                int32_t tgt[G];
                Row<VPL> n[G];
                float p[8];
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    tgt[k] = __builtin_amdgcn_readlane(my_t, k);
                    if (k == 0 && t0 == 0) tgt[k] = ci;
                }
                // a row drawn by two slots of the group: the later slot sits out the parallel pass (see sgns_kernel)
                uint32_t late = 0;
#pragma unroll
                for (int k = 1; k < G; ++k)
#pragma unroll
                    for (int k1 = 0; k1 < k; ++k1)
                        if (tgt[k] >= 0 && tgt[k] == tgt[k1]) late |= 1u << k;
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    if (tgt[k] >= 0 && !(late >> k & 1)) {
                        n[k] = load_row<VPL, kAtomic>(a.syn1neg, tgt[k], a.row_stride, lane);
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
                float g = 0.f;
                if (f > -kMaxExp && f < kMaxExp) {
                    const float sig = c_exp_table[(int)((f + kMaxExp) * (float)(kExpTableSize / (int)kMaxExp / 2))];
                    const float label = (my_k == 0 && t0 == 0) ? 1.f : 0.f;
                    g = (label - sig) * alpha;
                }
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
                    add_row<VPL>(a.syn1neg, tgt[k], a.row_stride, lane, dn);
                }
                if (late) {
                    // the repeated slots, in slot order: a negative each, from the row as memory holds it by now
#pragma unroll
                    for (int k = 1; k < G; ++k) {
                        if (!(late >> k & 1)) continue;
                        const Row<VPL> r = load_row<VPL, kAtomic>(a.syn1neg, tgt[k], a.row_stride, lane);
                        const float gk = negative_gradient<VPL>(neu1, r, alpha);
                        if (gk == 0.f) continue;
                        Row<VPL> dn;
#pragma unroll
                        for (int v = 0; v < VPL; ++v) {
                            work.v[v] = fmaf(gk, r.v[v], work.v[v]);
                            dn.v[v] = gk * neu1.v[v];
                        }
                        add_row<VPL>(a.syn1neg, tgt[k], a.row_stride, lane, dn);
                    }
                }
                // advance the sentence's LCG past this group's negatives
                const int used = min(a.negative, t0 + 7) - max(t0, 1) + 1;
                for (int d = 0; d < used; ++d) lcg = (lcg * kLcgA + kLcgC) & kLcgMask;
            }
            if (!a.cbow_mean) {
#pragma unroll
                for (int v = 0; v < VPL; ++v) work.v[v] *= inv;
            }
            // ---- every context position gets the whole of work (a word twice in the window: twice)
            for (int m = lo; m < hi; ++m) {
                if (m == i) continue;
                const int32_t xm = __builtin_amdgcn_readfirstlane(sent[m]);
                add_row<VPL>(a.syn0, xm, a.row_stride, lane, work);
            }
            ++centres_done;
        }
        __builtin_amdgcn_wave_barrier();  // LDS sentence is reused by the next one
    }
    if (a.centre_count && lane == 0 && centres_done) atomicAdd(a.centre_count, centres_done);
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

extern "C" int32_t n2v_cbow_max_sentence(void) { return kMaxSentence; }

extern "C" int n2v_cbow_corpus_check(const int32_t* tokens, const int64_t* offsets, int64_t n_sentences, int64_t n_tokens,
                                     int64_t n_words, int32_t max_len, int32_t* status, void* stream) {
    if (n_sentences < 0 || n_tokens < 0 || n_words < 1 || n_words > 0x7fffffffLL || max_len < 1 || max_len > kMaxSentence)
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
    if (n_sentences < 0 || n_tokens < 0 || n_words < 1 || n_words > 0x7fffffffLL || dim < 1 || window < 1 || negative < 0 ||
        negative > 64 || (cbow_mean != 0 && cbow_mean != 1))
        return n2v::fail(N2V_ERR_INVALID,
                         "n2v_cbow_train: bad size (sentences %lld, tokens %lld, words %lld, dim %d, window %d, negative %d, "
                         "cbow_mean %d)", (long long)n_sentences, (long long)n_tokens, (long long)n_words, (int)dim, (int)window,
                         (int)negative, (int)cbow_mean);
    if (max_len < 1 || max_len > kMaxSentence)
        return n2v::fail(N2V_ERR_INVALID, "n2v_cbow_train: max_len %d outside [1, %d]", (int)max_len, kMaxSentence);
    if (update_mode != N2V_SGNS_ATOMIC)
        return n2v::fail(N2V_ERR_INVALID, "n2v_cbow_train: update_mode %d: only N2V_SGNS_ATOMIC (lossless rows) is offered",
                         (int)update_mode);
    if (row_stride < dim || (row_stride != 64 && row_stride != 128 && row_stride != 256 && row_stride != 512))
        return n2v::fail(N2V_ERR_INVALID, "n2v_cbow_train: row_stride %d must be 64, 128, 256 or 512 and >= dim %d",
                         (int)row_stride, (int)dim);
    if (lut_bits < 1 || lut_bits > 24) return n2v::fail(N2V_ERR_INVALID, "n2v_cbow_train: lut_bits %d", (int)lut_bits);
    if (sentences_total < 1 || alpha_batch < 1 || sentences_step < 1 || sentences_base < 0)
        return n2v::fail(N2V_ERR_INVALID, "n2v_cbow_train: bad schedule");
    if (n_sentences == 0 || n_tokens == 0) return N2V_OK;
    if (!tokens || !offsets || !syn0 || !syn1neg || (negative > 0 && (!cum_table || !lut)))
        return n2v::fail(N2V_ERR_INVALID, "n2v_cbow_train: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_exp_table()) return rc;

    CbowArgs a;
    a.tokens = tokens; a.offsets = offsets; a.n_sent = n_sentences; a.n_tokens = n_tokens; a.n_words = n_words;
    a.syn0 = syn0; a.syn1neg = syn1neg; a.row_stride = row_stride;
    a.window = window; a.negative = negative; a.cbow_mean = cbow_mean; a.sample_int = sample_int;
    a.cum_table = cum_table; a.lut = lut; a.lut_shift = 31 - lut_bits;
    a.alpha0 = alpha; a.min_alpha = min_alpha;
    a.sent_base = sentences_base; a.sent_step = sentences_step; a.sent_total = sentences_total;
    a.alpha_batch = alpha_batch;
    a.seed = seed; a.sent_id_base = sentence_id_base; a.centre_count = pair_count;
    a.work = work_counter;
    a.lpad = (max_len + 63) & ~63;
    const size_t shmem = (size_t)4 * a.lpad * sizeof(int32_t);   // <= 64 KB by max_len <= kMaxSentence
    int64_t blocks = (n_sentences + 3) / 4;
    // the SGNS grid for lossless rows (n2v_sgns_default_blocks: at most one wavefront per 64 vocabulary rows, whole
    // workgroups per CU); nothing about CBOW was scored against a comparator at any grid
    const int64_t cap = max_blocks > 0 ? max_blocks : n2v_sgns_default_blocks(n_words, N2V_SGNS_ATOMIC);
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks), block(256);
    if (n_sentences <= blocks * 4) a.work = nullptr;   // no wave gets a second sentence: no hand-out needed
    if (a.work && hipMemsetAsync(a.work, 0, sizeof(unsigned long long), st) != hipSuccess)
        return n2v::fail(N2V_ERR_HIP, "n2v_cbow_train: resetting the work counter failed");
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
