"""GPU tests: the CBOW kernel (csrc/n2v_cbow.hip: n2v_cbow_train, n2v_cbow_corpus_check) against its sequential
restatement (tests/cbow_reference.py), to fp32 rounding, then the layers above it (n2v_hip/cbow.py, corpus.py,
word2vec.py, playlist.py, main.learn_embeddings(sg=0)).

One sentence on one wavefront (max_blocks=1, a launch in which a single sentence trains anything) runs the sequential
algorithm: every random choice is a pure function of (seed, sentence id, position), so the tables after the launch are
a deterministic function of the tables before it.  A launch with many wavefronts stays deterministic when no two
sentences share a row: every sentence gets its own block of vocabulary ids and negative=0.

Tolerance: a row element may differ from the float64 restatement by TOL times the largest magnitude in its table (the
rows start from float32 values; the kernel sums neu1 and the dot products in float32 and in another order, and every
update is a float32 atomic add).  MEASURED on MI355X over the case table of tests/cbow_cases.py: at most 2.17e-6
(negative=64, window=1, cbow_mean=0: 65 targets per centre; the 4096-word sentence 1.5e-6, the 150-sentence launch 4.3e-7);
TOL = 8.7e-6 is 4 x that (the margin tests/test_gpu_sgns_exact.py keeps).  The planted errors of
tests/test_cbow_host.py deviate by >= 7.4e-2 on their most sensitive case, >= 1.2e-4 on every case they touch at all.
The restatement counts sigmoid evaluations near a table-bin edge; the case table has none (checked on the CPU), so a
failure is always a kernel difference."""
import os

import numpy as np
import pytest

import cbow_cases as K
import cbow_reference as C
import sgns_reference as R

pytestmark = pytest.mark.gpu

TOL = K.TOL


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _model(torch, counts, dim, s0, s1, **kw):
    from n2v_hip import cbow
    n = len(counts)
    m = cbow.CbowModel(n, dim=dim, **kw)
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
    assert m.pairs_trained() == stats.pairs, (what, m.pairs_trained(), stats.pairs)
    d0, d1 = _deviation(m, r0, r1)
    print("%s: %d centres, %d sigmoid evaluations, deviation syn0 %.3g syn1neg %.3g (TOL %.3g)"
          % (what, stats.pairs, stats.evals, d0, d1, TOL))
    assert d0 <= TOL and d1 <= TOL, (what, d0, d1)


# ---- single-wave sequences ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.CASES, ids=[K.case_id(c) for c in K.CASES])
def test_single_wave_launches_match_restatement(torch_cuda, case):
    torch = torch_cuda
    c = case
    counts, launches, s0, s1 = K.case_data(c)
    m = _model(torch, counts, c["dim"], s0, s1, window=c["window"], negative=c["negative"], cbow_mean=c["cbow_mean"],
               alpha=c["alpha"], sample=c["sample"], seed=c["seed"])
    kw = K.ref_kwargs(c, counts)
    r0, r1, stats = K.reference(c)
    tokens_in = eff = 0
    for tokens, offsets, sid, sb in launches:
        m.train_pass(_corpus(torch, tokens, offsets, len(counts)), sentences_base=sb, sentences_total=K.SENTENCES_TOTAL,
                     sentence_id_base=sid, alpha_batch=kw["alpha_batch"], max_blocks=1)
        for s in range(len(offsets) - 1):
            raw = tokens[offsets[s]:offsets[s + 1]]
            tokens_in += int((raw >= 0).sum())
            eff += len(R.effective_sentence(raw, len(raw), kw["sample_int"], c["seed"], sid + s))
    if c["sample"]:
        assert eff < tokens_in, "sub-sampling dropped nothing"
    _assert_matches(m, r0, r1, stats, K.case_id(c))


def test_sub_sampling_compare_at_its_boundary(torch_cuda):
    """A token is dropped iff sample_int[w] < hash32(seed, sentence id, raw position): thresholds set to that hash - 1,
    the hash itself and the hash + 1 drop, keep and keep the token."""
    torch = torch_cuda
    rs = np.random.RandomState(8)
    n, seed, sid = 60, 99, 4
    tokens = rs.permutation(n).astype(np.int32)           # every word once
    offsets = np.array([0, n], np.int64)
    s0 = ((rs.random_sample((n, 64)) - 0.5) / 64).astype(np.float32)
    s1 = ((rs.random_sample((n, 64)) - 0.5) * 0.2).astype(np.float32)
    counts = np.full(n, 10)
    m = _model(torch, counts, 64, s0, s1, window=3, negative=2, sample=1e-3, seed=seed)
    sample_int = np.zeros(n, np.uint32)
    for pos, w in enumerate(tokens):
        sample_int[w] = R.hash32(seed, sid, pos, R.SALT_SAMPLE) + pos % 3 - 1
    m.sample_int.copy_(torch.from_numpy(sample_int.view(np.int32)))
    _, cum = K.vocab(counts, 1e-3)
    assert len(R.effective_sentence(tokens, n, sample_int, seed, sid)) == n - len(range(0, n, 3))
    r0, r1 = s0.astype(np.float64), s1.astype(np.float64)
    stats = R.Stats()
    C.train(r0, r1, tokens, offsets, window=3, negative=2, cbow_mean=1, alpha=0.025, min_alpha=1e-4, sample_int=sample_int,
            cum_table=cum, seed=seed, sentence_id_base=sid, sentences_base=0, sentences_step=1, sentences_total=10,
            alpha_batch=1, stats=stats)
    m.train_pass(_corpus(torch, tokens, offsets, n), sentences_base=0, sentences_total=10, sentence_id_base=sid,
                 alpha_batch=1, max_blocks=1)
    _assert_matches(m, r0, r1, stats, "sub-sampling boundary")


# ---- many wavefronts on disjoint rows ------------------------------------------------------------------------------------

BLOCK, N_SENT, ALPHA_BATCH, STEP = 24, 150, 40, 3


@pytest.fixture(scope="module")
def disjoint_case():
    rs = np.random.RandomState(15)
    lens = rs.randint(2, 200, N_SENT)
    lens[[3, 4, 77, N_SENT - 1]] = 0                      # empty rows between full ones, and at the end
    lens[[9, 10]] = 1
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tokens = np.concatenate([rs.randint(0, BLOCK, L) + s * BLOCK for s, L in enumerate(lens)]).astype(np.int32)
    n = N_SENT * BLOCK
    counts = np.bincount(tokens, minlength=n).astype(np.int64) + 1
    s0 = ((rs.random_sample((n, 100)) - 0.5) / 100).astype(np.float32)
    s1 = ((rs.random_sample((n, 100)) - 0.5) * 0.2).astype(np.float32)
    sample_int, cum = K.vocab(counts, 1e-3)
    r0, r1 = s0.astype(np.float64), s1.astype(np.float64)
    stats = R.Stats()
    C.train(r0, r1, tokens, offsets, window=5, negative=0, cbow_mean=1, alpha=0.025, min_alpha=1e-4, sample_int=sample_int,
            cum_table=cum, seed=21, sentence_id_base=1000, sentences_base=N_SENT * STEP, sentences_step=STEP,
            sentences_total=4 * N_SENT * STEP, alpha_batch=ALPHA_BATCH, stats=stats)
    return counts, tokens, offsets, s0, s1, r0, r1, stats


@pytest.mark.parametrize("blocks,counter", [(0, True), (7, True), (7, False)])
def test_many_wavefronts_on_disjoint_rows_are_deterministic(torch_cuda, disjoint_case, blocks, counter):
    """Every sentence trained once, with its own id and its job's learning rate, whichever wave takes it: two runs give
    the same bits, and those match the restatement."""
    torch = torch_cuda
    counts, tokens, offsets, s0, s1, r0, r1, stats = disjoint_case
    runs = []
    for _ in range(2):
        m = _model(torch, counts, 100, s0, s1, window=5, negative=0, sample=1e-3, seed=21)
        if not counter:
            m.work_counter = None
        m.train_pass(_corpus(torch, tokens, offsets, len(counts)), sentences_base=N_SENT * STEP, sentences_total=4 * N_SENT * STEP,
                     sentence_id_base=1000, sentences_step=STEP, alpha_batch=ALPHA_BATCH, max_blocks=blocks)
        torch.cuda.synchronize()
        runs.append((m.syn0.clone(), m.syn1neg.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    _assert_matches(m, r0, r1, stats, "%s grid, %s" % (blocks or "default", "counter" if counter else "static stride"))


# ---- the corpus check --------------------------------------------------------------------------------------------------

def test_malformed_corpora_are_value_errors_and_never_launched(torch_cuda):
    torch = torch_cuda
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
    for what, tok, off, max_len in (("decrease", tokens, np.array([0, 12, 10, 22, 30]), 30),
                                    ("last offset", tokens, np.array([0, 10, 10, 22, 29]), 30),
                                    ("last offset", tokens, np.array([0, 10, 10, 22, 31]), 30),
                                    ("start at 0", tokens, np.array([1, 10, 10, 22, 30]), 30),
                                    ("longer than max_len", tokens, good, 11),
                                    (">= n_words", bad_token, good, 30)):
        with pytest.raises(ValueError, match=what):
            m.train_pass(_corpus(torch, tok, off, n, max_len=max_len), sentences_base=0, sentences_total=10, sentence_id_base=0)
    with pytest.raises(ValueError, match="max_len"):
        m.train_pass(_corpus(torch, tokens, good, n, max_len=4097), sentences_base=0, sentences_total=10, sentence_id_base=0)
    torch.cuda.synchronize()
    assert m.pairs_trained() == 0 and torch.equal(m.syn0, before[0]) and torch.equal(m.syn1neg, before[1])
    # -1 tokens are padding, not an error; and the well-formed corpus trains
    ok = tokens.copy()
    ok[3] = -1
    m.train_pass(_corpus(torch, ok, good, n, max_len=12), sentences_base=0, sentences_total=10, sentence_id_base=0)
    torch.cuda.synchronize()
    assert m.pairs_trained() > 0 and not torch.equal(m.syn0, before[0])
    # the lossy skip-gram modes are refused by the C-ABI itself
    from n2v_hip import _lib
    c = _corpus(torch, tokens, good, n)
    for mode in (0, 1, 6):
        rc = m.lib.n2v_cbow_train(_lib.ptr(c.tokens), _lib.ptr(c.offsets), 4, 30, 30, _lib.ptr(m.syn0), _lib.ptr(m.syn1neg), n, 64, 64,
                                  3, 2, 1, None, _lib.ptr(m.cum_table), _lib.ptr(m.lut), 20, 0.025, 1e-4, 0, 1, 10, 1, 1, 0, None,
                                  mode, 1, None, None)
        assert rc == -1 and "update_mode" in m.lib.n2v_last_error().decode()


# ---- playlists -----------------------------------------------------------------------------------------------------------

def _log(rs, n_rows):
    """A 30Music-like log in file order: users in runs, gaps around playtime + 300, playtimes around 9 / 10."""
    uid, ts, pt, tid = [], [], [], []
    t, u = 1000, 0
    for r in range(n_rows):
        if r and rs.random_sample() < 0.04:
            u += 1                                              # a user change, often mid-session (no gap)
            if rs.random_sample() < 0.5:
                t = rs.randint(0, 5000)
        play = int(rs.choice([0, 5, 9, 10, 11, 200, 400]))
        uid.append("user%d" % u)
        ts.append(str(t))
        pt.append(str(play))
        tid.append(str(rs.randint(0, 80)))
        t += play + int(rs.choice([0, 1, 150, 299, 300, 301, 2000], p=[.2, .2, .2, .1, .1, .1, .1]))
    return uid, ts, pt, tid


@pytest.mark.parametrize("n_rows", [0, 1, 2, 2000])
def test_extract_playlists_matches_the_row_loop(torch_cuda, n_rows):
    import playlist_reference as P
    from n2v_hip.playlist import extract_playlists
    for seed in range(3):
        uid, ts, pt, tid = _log(np.random.RandomState(seed), n_rows)
        want = P.extract_playlist(uid, ts, pt, tid)
        got = extract_playlists(uid, [int(x) for x in ts], [int(x) for x in pt], tid)
        assert got == want
        if n_rows == 2000:
            assert len(want) > 20 and max(len(s) for s in want) > 5
            corpus = extract_playlists(uid, [int(x) for x in ts], [int(x) for x in pt], tid, as_corpus=True, min_count=3)
            kept, counts, rows = K.dict_corpus(want, 3)
            assert list(corpus.labels) == kept and corpus.counts.tolist() == counts and corpus.tolist() == [[kept[i] for i in r] for r in rows]
    # the edges by hand: gap of exactly playtime + 300 and one second either side; playtime 9 / 10; the last row of
    # the file inside a session; a user change mid-session; single-track sessions
    uid = ["a", "a", "a", "a", "a", "a", "b", "b", "b"]
    ts = [0, 399, 1099, 1800, 1809, 2119, 2120, 2130, 2140]
    pt = [100, 400, 400, 9, 10, 50, 10, 9, 10]
    tid = ["t0", "t1", "t2", "t3", "t4", "t5", "t6", "t7", "t8"]
    # 0->1: 399 < 400 joins; 1->2: 1099 < 1099 ends (exactly playtime + 300); 2->3: 1800 > 1799 ends: [t2] single, dropped;
    # 3->4 joins, t3 played 9: not kept; 4->5: 2119 < 2119 ends...
    want = P.extract_playlist(uid, ts, pt, tid)
    assert want == [["t0", "t1"], ["t6", "t8"]]
    assert extract_playlists(uid, ts, pt, tid) == want


# ---- end to end ----------------------------------------------------------------------------------------------------------

def test_word2vec_end_to_end(torch_cuda, tmp_path):
    from n2v_hip import io
    from n2v_hip.word2vec import Word2Vec
    rs = np.random.RandomState(6)
    sentences = [["w%d" % x for x in rs.zipf(1.5, rs.randint(2, 12)) if x < 60] for _ in range(200)]
    kept, counts, rows = K.dict_corpus(sentences, 2)
    runs = [Word2Vec(sentences, min_count=2, size=32, iter=2, sequential=True) for _ in range(2)]
    a = runs[0]
    assert a.wv.index2word == kept and [a.wv.vocab[w].count for w in kept] == counts and len(kept) > 10
    assert a.wv.syn0.shape == (len(kept), 32) and np.isfinite(a.wv.syn0).all()
    assert a.wv.syn0.tobytes() == runs[1].wv.syn0.tobytes()
    assert a.pairs_trained == runs[1].pairs_trained > 0
    assert (a.sgns.syn1neg != 0).any() and -1.0 <= a.wv.similarity(kept[0], kept[1]) <= 1.0
    assert np.array_equal(a.wv[kept[3]], a.wv.syn0[3]) and kept[3] in a.wv
    # the default launch (all wavefronts racing) trains the same centres
    b = Word2Vec(sentences, min_count=2, size=32, iter=2)
    assert b.pairs_trained == a.pairs_trained and np.isfinite(b.wv.syn0).all()
    path = os.path.join(str(tmp_path), "song2vec.emb")
    a.save_word2vec_format(path)
    words, vecs = io.load_word2vec_format(path)
    assert words == kept and np.allclose(vecs, a.wv.syn0, atol=1e-6)


def test_learn_embeddings_sg0_on_karate(torch_cuda):
    import main
    import node2vec
    from helpers import load_case
    from n2v_hip import csr
    e = load_case("karate_p1_q1")["edges"]
    g = node2vec.Graph.from_csr(csr.from_edges(e[:, 0], e[:, 1], None, directed=False), 1, 1, device="cuda:0", rng="philox")
    g.preprocess_transition_probs()
    walks = g.simulate_walks(4, 20)
    main.args = main.parse_args(["--dimensions", "48", "--window-size", "5"])
    emb = main.learn_embeddings(walks, sg=0)
    assert len(emb.wv.vocab) == 34 and emb.wv.syn0.shape == (34, 48) and np.isfinite(emb.wv.syn0).all()
    assert emb.pairs_trained > 0 and emb.wv["1"].shape == (48,)
    from n2v_hip import cbow
    assert isinstance(emb.sgns, cbow.CbowModel)
    # and the flag's default is still the skip-gram trainer
    from n2v_hip import sgns
    assert isinstance(main.learn_embeddings(walks).sgns, sgns.SgnsModel)
