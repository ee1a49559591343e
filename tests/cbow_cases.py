"""TEST INFRASTRUCTURE — the case table of tests/test_gpu_cbow.py, shared with tests/test_cbow_host.py, which checks
on the CPU what the GPU test relies on: no sigmoid evaluation of any case sits on a table-bin edge, and every planted
error of tests/cbow_reference.py moves the tables by far more than the GPU tolerance.

A case is a list of LAUNCHES; a launch is a small CSR corpus with at most one sentence that trains anything, so that
one wavefront decides the result (the other sentences of a launch are empty or hold one word).  The `data` numbers
were picked here, on the CPU, as the first for which the case has no evaluation near a bin edge."""
import os
import zlib
from collections import Counter

import numpy as np

import cbow_reference as C
import sgns_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTENCES_TOTAL = 2000
# 4 x the largest deviation of a case measured on MI355X (2.17e-6, tests/test_gpu_cbow.py)
TOL = 8.7e-6


def _case(dim=128, negative=5, window=5, cbow_mean=1, sample=1e-3, lens=(40, 33, 57), n_words=400, seed=7, sid_base=0,
          sentences_base=(0, 5, 9), minus1=False, kind="random", alpha=0.025, data=0):
    return dict(dim=dim, negative=negative, window=window, cbow_mean=cbow_mean, sample=sample, lens=tuple(lens),
                n_words=n_words, seed=seed, sid_base=sid_base, sentences_base=tuple(sentences_base), minus1=minus1,
                kind=kind, alpha=alpha, data=data)


CASES = [
    _case(), _case(cbow_mean=0),
    # row strides 64 / 128 / 256 / 512, dim < stride
    _case(dim=1, negative=1, window=1, n_words=60), _case(dim=50, negative=1, window=5, cbow_mean=0),
    _case(dim=64, negative=0, window=1), _case(dim=100, negative=5, window=5),
    _case(dim=200, negative=7, window=10, data=1), _case(dim=256, negative=5, window=5, cbow_mean=0),
    _case(dim=512, negative=8, window=5, lens=(30, 21)),
    # several target groups, the last one holding a single slot; both group widths
    _case(negative=15, window=5, lens=(30, 25)), _case(dim=64, negative=64, window=1, lens=(24, 17), cbow_mean=0),
    _case(negative=8, window=10, lens=(40,)), _case(negative=7, window=17, lens=(50, 41), cbow_mean=0),
    _case(dim=100, negative=5, window=17, lens=(45,)),
    # sentence lengths, empty sentences between full ones, -1 tokens inside a sentence
    _case(lens=(0, 1, 2, 3), window=5, sample=0, n_words=60), _case(lens=(63, 64, 65, 130), dim=64, negative=1, window=5),
    _case(lens=(0, 20, 0, 0, 31, 0), kind="empties", negative=0), _case(lens=(70, 64), minus1=True),
    _case(lens=(4096,), dim=64, negative=1, window=1, sample=0),
    # the same word twice in one window, the centre word also present as its own context
    _case(kind="dups", lens=(24, 24), n_words=60, window=5, sample=0), _case(kind="dups", lens=(24,), n_words=60, window=10, sample=0, cbow_mean=0),
    # nearly every group repeats a row (sgns_reference.repeated_draw_case); a draw equal to the centre
    _case(kind="repeat", dim=64, negative=5, window=3, sample=0, alpha=0.2, seed=3), _case(kind="repeat", dim=64, negative=12, window=3, sample=0, alpha=0.2, seed=3, cbow_mean=0),
    _case(kind="centre_draw", dim=64, negative=5, window=5, sample=0, lens=(30,), n_words=60),
    # sub-sampling rates, seeds, sentence ids and schedule positions
    _case(sample=0, window=5), _case(sample=1e-2, window=5, cbow_mean=0),
    _case(seed=2**32 + 12345, sid_base=10**6 + 7, sentences_base=(3, 777, 1500)),
    _case(seed=2**63 + 5, sid_base=2**40, sentences_base=(1999, 0, 1000), cbow_mean=0),
]


def case_id(c):
    return "d%d-n%d-w%d-m%d-s%g-L%s-%s%s%s" % (c["dim"], c["negative"], c["window"], c["cbow_mean"], c["sample"],
                                              "_".join(str(x) for x in c["lens"]), c["kind"],
                                              "-minus1" if c["minus1"] else "",
                                              "-seed%d" % c["seed"] if c["seed"] not in (3, 7) else "")


def case_data(c):
    """-> (counts int64[n], launches [(tokens int32, offsets int64, sentence_id_base, sentences_base)],
    syn0 float32 [n, dim], syn1neg float32 [n, dim])"""
    rs = np.random.RandomState((zlib.crc32(case_id(c).encode()) + 7919 * c["data"]) % 2**32)
    dim = c["dim"]
    if c["kind"] == "repeat":
        counts, walks, lens, s0, s1 = R.repeated_draw_case()
        sents = [walks[w, :lens[w]] for w in range(len(lens))]
        n = len(counts)
    else:
        n = c["n_words"]
        counts = (rs.pareto(1.0, n) * 20).astype(np.int64) + 1
        counts[:4] = [30000, 20000, 12000, 8000]     # a few frequent words, so that sample=1e-3 drops tokens
        p = counts / counts.sum()
        sents = [rs.choice(n, size=L, p=0.5 * p + 0.5 / n).astype(np.int32) for L in c["lens"]]
        if c["kind"] == "dups":        # a b a c a d ...: word a is centre and context at once, and twice in a window
            for s in sents:
                s[::2] = s[0]
                s[1::6] = s[1]
        if c["kind"] == "centre_draw":  # one word holds nearly all of the unigram^0.75 mass and is every other centre
            counts[5] = 10**7
            for s in sents:
                s[::2] = 5
        if c["minus1"]:
            for s in sents:
                s[5:9] = -1
                s[len(s) // 2] = -1
        s0 = ((rs.random_sample((n, dim)) - 0.5) / dim).astype(np.float32)
        s1 = ((rs.random_sample((n, dim)) - 0.5) * 0.2).astype(np.float32)
    launches = []
    if c["kind"] == "empties":          # one launch: the empty rows take part in the hand-out and the sentence ids
        tokens = np.concatenate(sents).astype(np.int32)
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int64)
        # the two full sentences share no wavefront: give each its own half of the vocabulary
        full = [i for i, s in enumerate(sents) if len(s)]
        tokens[offsets[full[1]]:offsets[full[1] + 1]] = n // 2 + tokens[offsets[full[1]]:offsets[full[1] + 1]] % (n // 2)
        tokens[offsets[full[0]]:offsets[full[0] + 1]] %= n // 2
        launches.append((tokens, offsets, c["sid_base"], c["sentences_base"][0]))
    else:
        for k, s in enumerate(sents):
            launches.append((np.asarray(s, np.int32), np.array([0, len(s)], np.int64), c["sid_base"] + k,
                             c["sentences_base"][k % len(c["sentences_base"])]))
    return counts, launches, s0, s1


def vocab(counts, sample):
    """(sample_int, cum_table) of n2v_hip.sgns.vocab_tables, imported late so that this file loads without torch."""
    from n2v_hip import sgns
    return sgns.vocab_tables(counts, sample)


def ref_kwargs(c, counts):
    sample_int, cum = vocab(counts, c["sample"])
    return dict(window=c["window"], negative=c["negative"], cbow_mean=c["cbow_mean"], alpha=c["alpha"], min_alpha=1e-4,
                sample_int=sample_int, cum_table=cum, seed=c["seed"], sentences_step=1, sentences_total=SENTENCES_TOTAL,
                alpha_batch=7)


def run_reference(c, variant=None):
    """-> (syn0 float64, syn1neg float64, Stats) after all launches of the case."""
    counts, launches, s0, s1 = case_data(c)
    kw = ref_kwargs(c, counts)
    r0, r1 = s0.astype(np.float64), s1.astype(np.float64)
    stats = R.Stats()
    for tokens, offsets, sid, sb in launches:
        C.train(r0, r1, tokens, offsets, sentence_id_base=sid, sentences_base=sb, stats=stats, variant=variant, **kw)
    return r0, r1, stats


_CACHE = {}


def reference(c):
    """The unplanted restatement of a case, computed once per process and never modified by its users."""
    key = case_id(c)
    if key not in _CACHE:
        _CACHE[key] = run_reference(c)
    return _CACHE[key]


def relative_deviation(a0, a1, r0, r1):
    """largest |a - r| over the largest magnitude of r, for both tables"""
    return float(np.abs(a0 - r0).max() / np.abs(r0).max()), float(np.abs(a1 - r1).max() / np.abs(r1).max())


def dict_corpus(sentences, min_count, max_len=4096):
    """gensim's build_vocab + the cut, with dicts and lists."""
    cnt = Counter(w for s in sentences for w in s)
    kept = sorted((w for w in cnt if cnt[w] >= max(min_count, 1)), key=lambda w: (-cnt[w], w))
    index = {w: i for i, w in enumerate(kept)}
    out = []
    for s in sentences:
        ids = [index[w] for w in s if w in index]
        out.extend([ids[k:k + max_len] for k in range(0, len(ids), max_len)] or [[]])
    return kept, [cnt[w] for w in kept], out
