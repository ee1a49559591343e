"""GPU tests: the ragged skip-gram kernel (csrc/n2v_sgns_csr.hip: n2v_sgns_csr_train) against its restatement
(tests/sgcsr_reference.py, built on tests/sgns_reference.py), to fp32 rounding, then the layers above it
(n2v_hip/skipgram.py, word2vec.SkipGram, extract_playlist -sg 1).

One item on one wavefront (max_blocks=1, one item per launch) runs the sequential algorithm: every random choice is a
pure function of (seed, sentence id, position), so the tables after the launch are a deterministic function of the
tables before it — with chunk == 0 an item is a sentence, with chunk >= 1 a run of at most `chunk` centres of one.  A
launch with many wavefronts stays deterministic when no two ITEMS share a row: whole sentences (chunk 0) on disjoint
vocabulary blocks with negative=0.  The items of one chunked sentence do share rows, so a chunked multi-wave launch is
held here to its pair count only; tests/test_gpu_w2v_ledger.py pins its events (pairs, draws, learning rates) through
counting tables.

Tolerance: TOL = 1e-5 of a table's largest magnitude, tests/test_gpu_sgns_exact.py's bound for this same arithmetic
(2.7e-6 measured there).  MEASURED here on an MI355X: at most 2.35e-6.  The planted
errors of tests/test_sgcsr_host.py deviate by >= 1.3e-1.  The case table has no sigmoid evaluation near a table-bin
edge (checked on the CPU), so a failure is always a kernel difference."""
import os

import numpy as np
import pytest

import sgcsr_cases as K
import sgcsr_reference as G
import sgns_reference as R

pytestmark = pytest.mark.gpu

TOL = K.TOL


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _model(torch, counts, dim, s0, s1, **kw):
    from n2v_hip import skipgram
    n = len(counts)
    m = skipgram.SkipGramModel(n, dim=dim, **kw)
    m.build_vocab(counts)
    t0 = np.zeros((n, m.stride), np.float32)
    t1 = np.zeros((n, m.stride), np.float32)
    t0[:, :dim], t1[:, :dim] = s0, s1
    m.syn0.copy_(torch.from_numpy(t0))
    m.syn1neg.copy_(torch.from_numpy(t1))
    return m


def _corpus(torch, tokens, offsets, n_words, max_len=None):
    from n2v_hip.corpus import SentenceCorpus
    lens = np.diff(offsets)
    return SentenceCorpus(torch.from_numpy(np.asarray(tokens, np.int32)).cuda(), torch.from_numpy(np.asarray(offsets, np.int64)).cuda(),
                          np.arange(n_words), np.zeros(n_words, np.int64),
                          max_len if max_len is not None else max(1, int(lens.max()) if len(lens) else 1))


def _deviation(m, r0, r1):
    """largest |kernel - restatement| of each table over the table's largest magnitude"""
    import torch
    torch.cuda.synchronize()
    dim = m.dim
    g0, g1 = m.syn0.cpu().numpy(), m.syn1neg.cpu().numpy()
    assert (g0[:, dim:] == 0).all() and (g1[:, dim:] == 0).all(), "padding columns moved"
    assert np.isfinite(g0).all() and np.isfinite(g1).all()
    return K.relative_deviation(g0[:, :dim], g1[:, :dim], r0, r1)


def _assert_matches(m, r0, r1, stats, what):
    assert stats.near_edge == 0, (what, "data has sigmoid evaluations on a bin edge", stats.near_edge)
    pairs = m.pairs_trained()
    d0, d1 = _deviation(m, r0, r1)
    print("%s: %d pairs (restatement %d), %d sigmoid evaluations, deviation syn0 %.3g syn1neg %.3g (TOL %.3g)"
          % (what, pairs, stats.pairs, stats.evals, d0, d1, TOL))
    assert pairs == stats.pairs, (what, pairs, stats.pairs)
    assert d0 <= TOL and d1 <= TOL, (what, d0, d1)


# ---- 1, 2: one item per launch, whole sentences and chunks -------------------------------------------------------------

@pytest.mark.parametrize("case", K.CASES, ids=[K.case_id(c) for c in K.CASES])
def test_items_one_per_launch_match_restatement(torch_cuda, monkeypatch, case):
    torch = torch_cuda
    c = case
    monkeypatch.setenv("N2V_SGNS_PREDRAW", "1" if c["predraw"] else "0")
    from n2v_hip import skipgram
    counts, tokens, offsets, s0, s1 = K.case_data(c)
    m = _model(torch, counts, c["dim"], s0, s1, window=c["window"], negative=c["negative"], alpha=c["alpha"],
               sample=c["sample"], seed=c["seed"])
    kw = K.ref_kwargs(c, counts)
    r0, r1, stats = K.reference(c)
    corpus = _corpus(torch, tokens, offsets, len(counts))
    total = skipgram.n_items(corpus, c["chunk"])
    assert total == len(G.item_table(offsets, c["chunk"])) > c["first_item"]
    for item in range(c["first_item"], total):
        m.train_pass(corpus, sentences_base=c["sentences_base"], sentences_total=c["total"], sentence_id_base=c["sid_base"],
                     alpha_batch=c["batch"], chunk=c["chunk"], first_item=item, item_count=1, max_blocks=1)
    if c["sample"]:
        raw = int((tokens >= 0).sum())
        eff = sum(len(R.effective_sentence(tokens[offsets[s]:offsets[s + 1]], int(offsets[s + 1] - offsets[s]), kw["sample_int"],
                                           c["seed"], c["sid_base"] + s)) for s in range(len(offsets) - 1))
        assert eff < raw, "sub-sampling dropped nothing"
    _assert_matches(m, r0, r1, stats, K.case_id(c))


def test_walk_matrix_as_csr_trains_what_the_walk_kernel_trains(torch_cuda):
    """A -1-padded walk matrix seen through SentenceCorpus.from_walks: the same streams as n2v_sgns_train (walk by walk
    on one wavefront), so the same pairs and — one centre step behind both kernels — the same bits."""
    torch = torch_cuda
    import node2vec
    from n2v_hip import sgns
    from n2v_hip.corpus import SentenceCorpus
    rs = np.random.RandomState(12)
    n, W, L, dim = 300, 4, 60, 100
    counts = (rs.pareto(1.0, n) * 20).astype(np.int64) + 1
    counts[:4] = [30000, 20000, 12000, 8000]
    walks = rs.choice(n, size=(W, L), p=0.5 * counts / counts.sum() + 0.5 / n).astype(np.int32)
    lens = np.array([60, 41, 1, 33], np.int32)
    for w in range(W):
        walks[w, lens[w]:] = -1
    s0 = ((rs.random_sample((n, dim)) - 0.5) / dim).astype(np.float32)
    s1 = ((rs.random_sample((n, dim)) - 0.5) * 0.2).astype(np.float32)
    a = sgns.SgnsModel(n, dim=dim, window=5, negative=5, seed=9, update_mode="atomic")
    a.build_vocab(counts=counts)
    b = _model(torch, counts, dim, s0, s1, window=5, negative=5, seed=9)
    a.syn0.copy_(b.syn0)
    a.syn1neg.copy_(b.syn1neg)
    wt, lt = torch.from_numpy(walks).cuda(), torch.from_numpy(lens).cuda()
    corpus = SentenceCorpus.from_walks(node2vec.WalkCorpus(wt, lt, np.arange(n)))
    batch = sgns.MAX_WORDS_IN_BATCH // L
    for w in range(W):
        a.train_pass(wt[w:w + 1], lt[w:w + 1], sentences_base=3 + (w // batch) * batch, sentences_total=50, walk_id_base=100 + w,
                     max_blocks=1)
        b.train_pass(corpus, sentences_base=3, sentences_total=50, sentence_id_base=100, alpha_batch=batch, chunk=0,
                     first_item=w, item_count=1, max_blocks=1)
    torch.cuda.synchronize()
    assert a.pairs_trained() == b.pairs_trained() > 0
    d0, d1 = K.relative_deviation(b.syn0.cpu().numpy(), b.syn1neg.cpu().numpy(), a.syn0.cpu().numpy().astype(np.float64),
                                  a.syn1neg.cpu().numpy().astype(np.float64))
    print("walk matrix as CSR vs n2v_sgns_train: deviation syn0 %.3g syn1neg %.3g, bits equal: %s"
          % (d0, d1, torch.equal(a.syn0, b.syn0) and torch.equal(a.syn1neg, b.syn1neg)))
    assert torch.equal(a.syn0, b.syn0) and torch.equal(a.syn1neg, b.syn1neg)


# ---- 3: one launch, many waves -----------------------------------------------------------------------------------------

N_SENT, ALPHA_BATCH, STEP = K.N_SENT, K.DISJOINT_BATCH, K.DISJOINT_STEP


@pytest.fixture(scope="module")
def disjoint_case():
    return K.disjoint_case()


def _launch(torch, case, chunk, blocks=0, counter=True):
    counts, tokens, offsets, s0, s1 = case[:5]
    m = _model(torch, counts, 100, s0, s1, window=5, negative=0, sample=1e-3, seed=21)
    if not counter:
        m.work_counter = None
    m.train_pass(_corpus(torch, tokens, offsets, len(counts)), sentences_base=N_SENT * STEP, sentences_total=4 * N_SENT * STEP,
                 sentence_id_base=1000, sentences_step=STEP, alpha_batch=ALPHA_BATCH, chunk=chunk, max_blocks=blocks)
    torch.cuda.synchronize()
    return m


@pytest.mark.parametrize("blocks,counter", [(0, True), (7, True), (7, False)])
def test_many_wavefronts_on_disjoint_rows_are_deterministic(torch_cuda, disjoint_case, blocks, counter):
    """Every sentence trained once, with its own id and its job's learning rate, whichever wave takes it: two runs give
    the same bits, and those match the restatement."""
    torch = torch_cuda
    r0, r1, stats = disjoint_case[5:]
    runs = [_launch(torch, disjoint_case, 0, blocks, counter) for _ in range(2)]
    assert torch.equal(runs[0].syn0, runs[1].syn0) and torch.equal(runs[0].syn1neg, runs[1].syn1neg)
    _assert_matches(runs[1], r0, r1, stats, "%s grid, %s" % (blocks or "default", "counter" if counter else "static stride"))


@pytest.mark.parametrize("blocks,counter", [(0, True), (7, True), (7, False)])
def test_chunked_launch_trains_every_pair_once(torch_cuda, disjoint_case, blocks, counter):
    """chunk 16: the items of a sentence race on its rows, so the VALUES of the tables are not pinned (which pairs, draws
    and learning rates a chunked launch trains is: tests/test_gpu_w2v_ledger.py); every (centre, context) pair is
    still trained exactly once (the count is the restatement's), nothing leaves the tables' columns."""
    torch = torch_cuda
    stats = disjoint_case[7]
    m = _launch(torch, disjoint_case, 16, blocks, counter)
    assert m.pairs_trained() == stats.pairs
    g0, g1 = m.syn0.cpu().numpy(), m.syn1neg.cpu().numpy()
    assert np.isfinite(g0).all() and np.isfinite(g1).all() and (g0[:, 100:] == 0).all() and (g1[:, 100:] == 0).all()
    assert (g1[:, :100] != disjoint_case[4]).any()


# ---- 4: the acceptance band --------------------------------------------------------------------------------------------

AUC_BAND = 0.002  # BASELINE.json north_star: "agree on link-prediction AUC within +-0.002"


@pytest.mark.parametrize("chunk", [0, 16])
@pytest.mark.parametrize("name", ["uniform3k_10x80", "hub20k_10x80"])
def test_walks_as_ragged_sentences_stay_in_the_band(torch_cuda, name, chunk):
    torch = torch_cuda
    from test_gpu_sgns_band import gpu_case
    from n2v_hip import linkpred, skipgram
    from n2v_hip.corpus import SentenceCorpus
    g, walks, counts, te_d, neg_d, fx = gpu_case(name)
    m = skipgram.SkipGramModel(g.n_nodes, dim=fx["dim"], window=fx["window"], negative=fx["negative"], seed=fx["sgns_seed"])
    m.build_vocab(counts.cpu().numpy())
    skipgram.train(m, SentenceCorpus.from_walks(walks), epochs=1, chunk=chunk)
    torch.cuda.synchronize()
    auc, ap = linkpred.get_roc_score(m.vectors(), te_d, neg_d)
    print("%s chunk %d: AUC %.5f vs sequential comparator %.5f (%+.5f) | AP %.5f vs %.5f | pairs %d vs %d" % (
        name, chunk, auc, fx["auc_cpu"], auc - fx["auc_cpu"], ap, fx["ap_cpu"], m.pairs_trained(), fx["pairs_cpu"]))
    assert abs(m.pairs_trained() - fx["pairs_cpu"]) / fx["pairs_cpu"] < 0.01
    assert abs(auc - fx["auc_cpu"]) <= AUC_BAND, (name, chunk, auc, fx["auc_cpu"])


# ---- 5: refusals -------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(torch_cuda):
    torch = torch_cuda
    from n2v_hip import _lib
    rs = np.random.RandomState(4)
    n = 50
    counts = np.full(n, 7)
    s0 = ((rs.random_sample((n, 64)) - 0.5) / 64).astype(np.float32)
    s1 = ((rs.random_sample((n, 64)) - 0.5) * 0.2).astype(np.float32)
    m = _model(torch, counts, 64, s0, s1, window=3, negative=2)
    before = (m.syn0.clone(), m.syn1neg.clone())
    tokens = rs.randint(0, n, 30).astype(np.int32)
    good = np.array([0, 10, 10, 22, 30], np.int64)
    bad_token = tokens.copy()
    bad_token[17] = n
    kw = dict(sentences_base=0, sentences_total=10, sentence_id_base=0)
    for what, tok, off, max_len in (("decrease", tokens, np.array([0, 12, 10, 22, 30]), 30),
                                    ("last offset", tokens, np.array([0, 10, 10, 22, 29]), 30),
                                    ("start at 0", tokens, np.array([1, 10, 10, 22, 30]), 30),
                                    ("longer than max_len", tokens, good, 11),
                                    (">= n_words", bad_token, good, 30)):
        for chunk in (0, 4):
            with pytest.raises(ValueError, match=what):
                m.train_pass(_corpus(torch, tok, off, n, max_len=max_len), chunk=chunk, **kw)
    with pytest.raises(ValueError, match="max_len"):
        m.train_pass(_corpus(torch, tokens, good, n, max_len=4097), **kw)
    c = _corpus(torch, tokens, good, n)
    # a slot above 4 096 tokens
    for chunk in (4091, 4096, 10**6):
        with pytest.raises(_lib.N2VError, match="slot"):
            m.train_pass(c, chunk=chunk, **kw)
    # an item range outside item_off: chunk 4 -> 3 + 0 + 3 + 2 = 8 items; chunk 0 -> 4 sentences
    for chunk, first, count in ((4, 0, 9), (4, 8, 1), (4, 9, 0), (4, -1, 1), (0, 0, 5), (0, 4, 1), (0, 2, -1)):
        with pytest.raises(ValueError, match="items"):
            m.train_pass(c, chunk=chunk, first_item=first, item_count=count, **kw)
    # ... and through the C-ABI itself, which bounds the range by the token count, and refuses the lossy modes
    from n2v_hip import skipgram
    off = skipgram.item_offsets(c, 4)
    assert off.tolist() == [0, 3, 3, 6, 8]

    def raw(first, count, mode=2, item_off=off, chunk=4):
        return m.lib.n2v_sgns_csr_train(_lib.ptr(c.tokens), _lib.ptr(c.offsets), 4, 30, 12, _lib.ptr(item_off), chunk, first, count,
                                        _lib.ptr(m.syn0), _lib.ptr(m.syn1neg), n, 64, 64, 3, 2, _lib.ptr(m.sample_int),
                                        _lib.ptr(m.cum_table),
                                        _lib.ptr(m.lut), 20, 0.025, 1e-4, 0, 1, 10, 1, 1, 0, _lib.ptr(m.pair_count), mode, 1, None,
                                        _lib.stream_ptr(m.device))
    assert raw(0, 31) == -1 and "item range" in m.lib.n2v_last_error().decode()
    assert raw(0, 8, item_off=None) == -1 and "item_off missing" in m.lib.n2v_last_error().decode()
    for mode in (0, 1, 6):
        assert raw(0, 8, mode=mode) == -1 and "update_mode" in m.lib.n2v_last_error().decode()
    torch.cuda.synchronize()
    assert m.pairs_trained() == 0 and torch.equal(m.syn0, before[0]) and torch.equal(m.syn1neg, before[1])
    # items that item_off does not cover (8 ... 11, inside the entry point's bound) are skipped by the kernel, not read
    assert raw(6, 6) == 0
    torch.cuda.synchronize()
    pairs_tail = m.pairs_trained()
    m2 = _model(torch, counts, 64, s0, s1, window=3, negative=2)
    m2.train_pass(c, chunk=4, first_item=6, item_count=2, max_blocks=1, **kw)
    torch.cuda.synchronize()
    assert pairs_tail == m2.pairs_trained() > 0
    # -1 tokens are padding, not an error; and the well-formed corpus trains
    ok = tokens.copy()
    ok[3] = -1
    m.train_pass(_corpus(torch, ok, good, n, max_len=12), chunk=4, **kw)
    torch.cuda.synchronize()
    assert m.pairs_trained() > pairs_tail and not torch.equal(m.syn0, before[0])


# ---- 6: end to end -----------------------------------------------------------------------------------------------------

def _dict_corpus(sentences, min_count):
    from collections import Counter
    cnt = Counter(w for s in sentences for w in s)
    kept = sorted((w for w in cnt if cnt[w] >= max(min_count, 1)), key=lambda w: (-cnt[w], w))
    return kept, [cnt[w] for w in kept]


def test_skipgram_end_to_end(torch_cuda, tmp_path):
    from n2v_hip import io, skipgram
    from n2v_hip.word2vec import SkipGram
    rs = np.random.RandomState(6)
    sentences = [["w%d" % x for x in rs.zipf(1.5, rs.randint(2, 12)) if x < 60] for _ in range(120)]
    kept, counts = _dict_corpus(sentences, 2)
    runs = [SkipGram(sentences, min_count=2, size=32, iter=2, sequential=True) for _ in range(2)]
    a = runs[0]
    assert isinstance(a.sgns, skipgram.SkipGramModel)
    assert a.wv.index2word == kept and [a.wv.vocab[w].count for w in kept] == counts and len(kept) > 10
    assert a.wv.syn0.shape == (len(kept), 32) and np.isfinite(a.wv.syn0).all()
    assert a.wv.syn0.tobytes() == runs[1].wv.syn0.tobytes()
    assert a.pairs_trained == runs[1].pairs_trained > 0
    assert (a.sgns.syn1neg != 0).any() and -1.0 <= a.wv.similarity(kept[0], kept[1]) <= 1.0
    # chunked and sequential: reproducible too, and the same pairs; the default launch trains the same pairs
    c = [SkipGram(sentences, min_count=2, size=32, iter=1, sequential=True, chunk=3) for _ in range(2)]
    assert c[0].wv.syn0.tobytes() == c[1].wv.syn0.tobytes()
    b = SkipGram(sentences, min_count=2, size=32, iter=2)
    assert b.pairs_trained == a.pairs_trained and np.isfinite(b.wv.syn0).all()
    assert SkipGram(sentences, min_count=2, size=32, iter=1, chunk=3).pairs_trained == c[0].pairs_trained > 0
    path = os.path.join(str(tmp_path), "sg.emb")
    a.save_word2vec_format(path)
    words, vecs = io.load_word2vec_format(path)
    assert words == kept and np.allclose(vecs, a.wv.syn0, atol=1e-6)


def test_extract_playlist_sg1_writes_a_word2vec_file(torch_cuda, tmp_path):
    import extract_playlist as E
    from n2v_hip import io, skipgram
    rs = np.random.RandomState(3)
    rows, t = [], 1000
    for r in range(1500):
        if r and rs.random_sample() < 0.05:
            t += 5000                                           # a gap: the session ends
        play = int(rs.choice([10, 11, 200]))
        rows.append('%d,%d,%d,"user%d",%d' % (r, t, play, r // 300, rs.randint(0, 40)))
        t += play + int(rs.choice([0, 1, 150]))
    src = os.path.join(str(tmp_path), "events.csv")
    with open(src, "w") as f:
        f.write("\n".join(rows) + "\n")
    out = os.path.join(str(tmp_path), "emb", "song2vec_sg.emb")
    res = E.main(["-input", src, "-min-count", "3", "-output", out, "-size", "24", "-iter", "1", "-sg", "1", "-chunk", "8"])
    assert isinstance(res.sgns, skipgram.SkipGramModel) and res.pairs_trained > 0
    words, vecs = io.load_word2vec_format(out)
    assert words == res.wv.index2word and len(words) > 10 and vecs.shape == (len(words), 24) and np.isfinite(vecs).all()
    assert np.allclose(vecs, res.wv.syn0, atol=1e-6)
