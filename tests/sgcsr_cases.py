"""TEST INFRASTRUCTURE — the case table of tests/test_gpu_sgcsr.py, shared with tests/test_sgcsr_host.py, which checks
on the CPU what the GPU test relies on: no sigmoid evaluation of any case sits on a table-bin edge.

A case is one CSR corpus, trained ITEM BY ITEM (one item per launch on one wavefront, the items [first_item, end) in
order), so that sentences may share words and the result is still a deterministic function of the tables.  chunk == 0:
an item is a sentence.  The `data` numbers were picked here, on the CPU, as the first for which the case has no
evaluation near a bin edge."""
import zlib

import numpy as np

import sgcsr_reference as G
import sgns_reference as R

SENTENCES_TOTAL = 2000
ALPHA_BATCH = 2
# tests/test_gpu_sgns_exact.py's bound for this same arithmetic (2.7e-6 measured there)
TOL = 1e-5


def _case(dim=100, negative=5, window=10, sample=1e-3, lens=(40, 33, 57), chunk=0, n_words=400, seed=7, sid_base=0,
          sentences_base=0, minus1=False, kind="random", alpha=0.025, predraw=True, first_item=0, total=SENTENCES_TOTAL, batch=ALPHA_BATCH,
          data=0):
    return dict(dim=dim, negative=negative, window=window, sample=sample, lens=tuple(lens), chunk=chunk, n_words=n_words,
                seed=seed, sid_base=sid_base, sentences_base=sentences_base, minus1=minus1, kind=kind, alpha=alpha,
                predraw=predraw, first_item=first_item, total=total, batch=batch, data=data)


WHOLE = [
    _case(),
    # row strides 64 / 128 / 256 / 512, dim < stride
    _case(dim=50, negative=1, window=3, lens=(40, 33)), _case(dim=200, negative=6, window=3, lens=(40,)),
    _case(dim=400, negative=8, window=3, lens=(30,)),
    # sentence lengths, empty sentences among them
    _case(dim=60, negative=0, window=1, lens=(0, 1, 2, 63, 64, 65, 130)),
    _case(dim=60, negative=1, window=1, lens=(4096,), sample=0),
    # several target groups, the last one holding a single slot; both group widths
    _case(dim=128, negative=15, window=3, lens=(40,)), _case(dim=60, negative=64, window=1, lens=(24,)),
    _case(negative=5, window=17, lens=(50,)),
    # -1 tokens inside a sentence, sub-sampling rates
    _case(lens=(70, 64), minus1=True), _case(sample=0, window=3), _case(sample=1e-2, window=3),
    # seeds, sentence ids and schedule positions
    _case(seed=2**63 + 5, sid_base=2**40, sentences_base=1999), _case(seed=2**32 + 12345, sid_base=10**6 + 7, sentences_base=777),
    # predraw off (N2V_SGNS_PREDRAW=0), at one and two target groups' worth of negatives
    _case(predraw=False, data=1), _case(predraw=False, negative=7, lens=(40,)),
    # nearly every group repeats a row (sgns_reference.repeated_draw_case, with the schedule tests/test_gpu_sgns_exact.py
    # gives it: sentence s at position s of 100)
    _case(kind="repeat", dim=64, negative=5, window=3, sample=0, alpha=0.2, seed=3, total=100, batch=1),
    _case(kind="repeat", dim=64, negative=12, window=3, sample=0, alpha=0.2, seed=3, total=100, batch=1),
]

CHUNKED = [
    _case(chunk=2, window=3, lens=(7,), negative=2, sample=0, n_words=60),
    _case(chunk=1, window=1, lens=(5,), negative=2, sample=0, n_words=60),
    _case(chunk=64, window=10, lens=(63, 64, 65, 129), negative=2),
    _case(chunk=256, window=5, lens=(4096,), negative=1, dim=60, data=1),
    # sub-sampling leaves fewer tokens than the sentence has items: some items are empty
    _case(chunk=2, window=3, lens=(40,), negative=2, kind="sparse"),
    _case(chunk=8, window=3, lens=(20, 0, 30), negative=5, first_item=2),
]

CASES = WHOLE + CHUNKED


def case_id(c):
    return "c%d-d%d-n%d-w%d-s%g-L%s-%s%s%s%s%s" % (c["chunk"], c["dim"], c["negative"], c["window"], c["sample"],
                                                   "_".join(str(x) for x in c["lens"]), c["kind"],
                                                   "-minus1" if c["minus1"] else "", "-nopre" if not c["predraw"] else "",
                                                   "-seed%d" % c["seed"] if c["seed"] not in (3, 7) else "",
                                                   "-from%d" % c["first_item"] if c["first_item"] else "")


def case_data(c):
    """-> (counts int64[n], tokens int32[T], offsets int64[S + 1], syn0 float32 [n, dim], syn1neg float32 [n, dim])"""
    rs = np.random.RandomState((zlib.crc32(case_id(c).encode()) + 7919 * c["data"]) % 2**32)
    dim = c["dim"]
    if c["kind"] == "repeat":
        counts, walks, lens, s0, s1 = R.repeated_draw_case()
        sents = [walks[w, :lens[w]] for w in range(len(lens))]
    else:
        n = c["n_words"]
        counts = (rs.pareto(1.0, n) * 20).astype(np.int64) + 1
        counts[:4] = [30000, 20000, 12000, 8000]     # a few frequent words, so that sample=1e-3 drops tokens
        p = counts / counts.sum()
        sents = [rs.choice(n, size=L, p=0.5 * p + 0.5 / n).astype(np.int32) for L in c["lens"]]
        if c["kind"] == "sparse":                    # mostly the frequent words: sub-sampling drops most tokens
            for s in sents:
                s[rs.random_sample(len(s)) < 0.8] = rs.randint(0, 2)
        if c["minus1"]:
            for s in sents:
                s[5:9] = -1
                s[len(s) // 2] = -1
        s0 = ((rs.random_sample((n, dim)) - 0.5) / dim).astype(np.float32)
        s1 = ((rs.random_sample((n, dim)) - 0.5) * 0.2).astype(np.float32)
    tokens = np.concatenate(sents).astype(np.int32) if sents else np.zeros(0, np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int64)
    return counts, tokens, offsets, s0, s1


def vocab(counts, sample):
    """(sample_int, cum_table) of n2v_hip.sgns.vocab_tables, imported late so that this file loads without torch."""
    from n2v_hip import sgns
    return sgns.vocab_tables(counts, sample)


def ref_kwargs(c, counts):
    sample_int, cum = vocab(counts, c["sample"])
    return dict(window=c["window"], negative=c["negative"], alpha=c["alpha"], min_alpha=1e-4, sample_int=sample_int,
                cum_table=cum, seed=c["seed"], sentence_id_base=c["sid_base"], sentences_base=c["sentences_base"],
                sentences_step=1, sentences_total=c["total"], alpha_batch=c["batch"])


def run_reference(c, variant=None):
    """-> (syn0 float64, syn1neg float64, Stats) after the items [first_item, end) of the case."""
    counts, tokens, offsets, s0, s1 = case_data(c)
    r0, r1 = s0.astype(np.float64), s1.astype(np.float64)
    stats = R.Stats()
    G.train(r0, r1, tokens, offsets, c["chunk"], first_item=c["first_item"], stats=stats, variant=variant,
            **ref_kwargs(c, counts))
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


# ---- many wavefronts in one launch: sentences on disjoint vocabulary blocks, negative=0 (tests/test_gpu_sgcsr.py) --------

BLOCK, N_SENT, DISJOINT_BATCH, DISJOINT_STEP = 24, 150, 40, 3
_DISJOINT = []


def disjoint_case(seed=17):
    """-> (counts, tokens, offsets, syn0 f32, syn1neg f32, syn0 f64, syn1neg f64, Stats): the corpus and its restatement
    (chunk 0; the chunked launch trains the same pairs), computed once per process.  The seed is the first from 15 whose
    data has no sigmoid evaluation near a bin edge."""
    if _DISJOINT:
        return _DISJOINT[0]
    rs = np.random.RandomState(seed)
    lens = rs.randint(2, 200, N_SENT)
    lens[[3, 4, 77, N_SENT - 1]] = 0                      # empty sentences inside the launch, and at its end
    lens[[9, 10]] = 1
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tokens = np.concatenate([rs.randint(0, BLOCK, L) + s * BLOCK for s, L in enumerate(lens)]).astype(np.int32)
    tokens[rs.random_sample(len(tokens)) < 0.03] = -1
    n = N_SENT * BLOCK
    counts = np.bincount(tokens[tokens >= 0], minlength=n).astype(np.int64) + 1
    s0 = ((rs.random_sample((n, 100)) - 0.5) / 100).astype(np.float32)
    s1 = ((rs.random_sample((n, 100)) - 0.5) * 0.2).astype(np.float32)
    sample_int, cum = vocab(counts, 1e-3)
    r0, r1 = s0.astype(np.float64), s1.astype(np.float64)
    stats = R.Stats()
    G.train(r0, r1, tokens, offsets, 0, window=5, negative=0, alpha=0.025, min_alpha=1e-4, sample_int=sample_int,
            cum_table=cum, seed=21, sentence_id_base=1000, sentences_base=N_SENT * DISJOINT_STEP,
            sentences_step=DISJOINT_STEP, sentences_total=4 * N_SENT * DISJOINT_STEP, alpha_batch=DISJOINT_BATCH, stats=stats)
    _DISJOINT.append((counts, tokens, offsets, s0, s1, r0, r1, stats))
    return _DISJOINT[0]
