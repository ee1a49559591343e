"""GPU tests of the skip-gram/negative-sampling kernel (run with -m gpu).

The SGNS half has no bit-level oracle for gensim itself (gensim absent; Hogwild is
order-dependent).  The single-wave algorithm is pinned to fp32 rounding against the float64
restatement of the kernels' own schedule in tests/test_gpu_sgns_exact.py; for racing waves on shared
rows and walk_splits > 1, tests/test_gpu_w2v_ledger.py pins WHICH events are trained (pairs, draws, learning
rates), while the values such a race leaves stay unpinned.  What is checked here: exact properties of one update
(against a numpy restatement of fast_sentence_sg_neg on a corpus where every quantity is
deterministic), structural invariants, and the acceptance band of BASELINE.json —
link-prediction AUC within +-0.002 of the single-thread CPU comparator (oracle/sgns_oracle.c)
trained on the same walks from the same initial tables."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AUC_BAND = 0.002  # BASELINE.json north_star: "agree on link-prediction AUC within +-0.002"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _planted_partition(n=3000, k=30, m_in=20000, m_out=4000, seed=0):
    rs = np.random.RandomState(seed)
    comm = rs.randint(0, k, n)
    src, dst = [], []
    while len(src) < m_in:
        a, b = rs.randint(0, n, 2)
        if a != b and comm[a] == comm[b]:
            src.append(a)
            dst.append(b)
    for _ in range(m_out):
        a, b = rs.randint(0, n, 2)
        if a != b:
            src.append(a)
            dst.append(b)
    src, dst = np.array(src), np.array(dst)
    key = np.minimum(src, dst) * n + np.maximum(src, dst)
    _, first = np.unique(key, return_index=True)
    first.sort()
    return np.stack([src[first], dst[first]], 1)


def test_init_matches_oracle_restatement(torch_cuda):
    from n2v_hip import sgns
    from oracle import c_oracle
    for dim in (128, 100, 256):
        m = sgns.SgnsModel(777, dim=dim, seed=12345)
        s0, s1 = c_oracle.sgns_init(777, dim, m.stride, 12345)
        assert np.array_equal(m.syn0.cpu().numpy(), s0)
        assert np.array_equal(m.syn1neg.cpu().numpy(), s1)
        assert np.abs(s0[:, :dim]).max() <= 0.5 / dim and (s0[:, dim:] == 0).all()


def test_neg_lut_is_exact_bisect(torch_cuda):
    torch = torch_cuda
    from n2v_hip import sgns
    rs = np.random.RandomState(1)
    counts = (rs.pareto(1.2, 5000) * 10).astype(np.int64) + 1
    counts[rs.randint(0, 5000, 300)] = 0
    m = sgns.SgnsModel(5000, dim=64, seed=1)
    m.build_vocab(counts=counts)
    cum = m.cum_table.cpu().numpy().view(np.uint32)
    lut = m.lut.cpu().numpy().view(np.uint32)
    shift = 31 - sgns.LUT_BITS
    b = np.arange((1 << sgns.LUT_BITS) + 1, dtype=np.uint64) << np.uint64(shift)
    assert np.array_equal(lut, np.searchsorted(cum, b, side="left").astype(np.uint32))
    assert cum[-1] == 2**31 - 1 and (np.diff(cum.astype(np.int64)) >= 0).all()


def test_single_pair_update_matches_numpy(torch_cuda):
    """Corpus of one 2-word sentence, window 1 (so the window shrink is always 0), no
    sub-sampling, negative = 0: the two (centre, context) pairs have no random choice left,
    so the tables after one pass are a deterministic function of the initial tables."""
    torch = torch_cuda
    from n2v_hip import sgns
    d = torch.device("cuda:0")
    for dim, mode, share in [(d_, m_, s_) for d_ in (128, 64, 100, 256, 512) for m_ in ("atomic", "agent", "plain")
                             for s_ in (False, True)]:
        m = sgns.SgnsModel(5, dim=dim, window=1, negative=0, sample=0, seed=3, update_mode=mode,
                           share_negatives=share, allow_out_of_band=True)
        # non-zero syn1neg so that both tables move
        m.syn1neg[:, :dim] = (torch.rand((5, dim), device=d) - 0.5) * 0.2
        walks = torch.tensor([[1, 3]], dtype=torch.int32, device=d)
        lens = torch.tensor([2], dtype=torch.int32, device=d)
        m.build_vocab(walks)
        s0 = m.syn0.cpu().numpy().astype(np.float64)
        s1 = m.syn1neg.cpu().numpy().astype(np.float64)
        sgns.train(m, walks, lens, epochs=1)
        torch.cuda.synchronize()
        assert m.pairs_trained() == 2
        alpha = 0.025

        def sig(f):
            x = (np.float32(int((f + 6) * 83)) / np.float32(1000) * 2 - 1) * 6  # table bin of f
            e = np.exp(np.float64(np.float32(x)))
            return e / (e + 1)
        # pair (centre 1, context 3), then (centre 3, context 1): fast_sentence_sg_neg, d == 0 only
        for ci, xj in ((1, 3), (3, 1)):
            f = float(np.dot(s0[xj], s1[ci]))
            g = (1.0 - sig(f)) * alpha
            work = g * s1[ci]
            s1[ci] = s1[ci] + g * s0[xj]
            s0[xj] = s0[xj] + work
        np.testing.assert_allclose(m.syn0.cpu().numpy(), s0, rtol=2e-5, atol=2e-7)
        np.testing.assert_allclose(m.syn1neg.cpu().numpy(), s1, rtol=2e-5, atol=2e-7)
        assert (m.syn0.cpu().numpy()[:, dim:] == 0).all()


def test_pair_count_matches_window_rule(torch_cuda):
    """No sub-sampling: pairs of a sentence of n words = sum_i (#j in window shrunk by b_i);
    with window 1 that is exactly 2(n-1); padding (-1) and short walks are skipped."""
    torch = torch_cuda
    from n2v_hip import sgns
    d = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    W, L, N = 500, 37, 300
    walks = rs.randint(0, N, size=(W, L)).astype(np.int32)
    lens = rs.randint(1, L + 1, size=W).astype(np.int32)
    for i in range(W):
        walks[i, lens[i]:] = -1
    m = sgns.SgnsModel(N, dim=128, window=1, negative=5, sample=0, seed=5)
    wt, lt = torch.from_numpy(walks).to(d), torch.from_numpy(lens).to(d)
    m.build_vocab(wt)
    assert np.array_equal(m.counts, np.bincount(walks[walks >= 0], minlength=N))
    sgns.train(m, wt, lt, epochs=2)
    torch.cuda.synchronize()
    assert m.pairs_trained() == 2 * int((2 * (lens - 1)).sum())
    assert torch.isfinite(m.syn0).all() and torch.isfinite(m.syn1neg).all()
    # window 10: expected pairs per full sentence E = sum_i E_b[...] within [lower, upper] bounds
    m2 = sgns.SgnsModel(N, dim=128, window=10, negative=5, sample=0, seed=5)
    m2.build_vocab(wt)
    full = torch.from_numpy(rs.randint(0, N, size=(2000, 80)).astype(np.int32)).to(d)
    sgns.train(m2, full, None, epochs=1)
    per = m2.pairs_trained() / 2000.0
    assert 800 < per < 870, per  # 836 expected for L=80, window=10


def test_walk_splits_train_the_same_pairs_and_stay_in_the_band(torch_cuda):
    """walk_splits > 1 deals the centres of a sentence to several wavefronts (the short launches of the tiered merges
    then fill the chip): exactly the same number of pairs, the same untouched rows, and — since only the ORDER inside a
    sentence turns into a race — a link-prediction AUC inside the band of the sequential comparator."""
    torch = torch_cuda
    from n2v_hip import linkpred, sgns
    g, corpus, counts, te_d, neg_d, rounds, auc_cpu = _band_case("uniform")
    ref = sgns.SgnsModel(g.n_nodes, dim=128, window=10, negative=5, seed=1)
    ref.build_vocab(counts=counts)
    ref.train_pass(corpus.walks, corpus.lens, sentences_base=0, sentences_total=corpus.walks.shape[0], walk_id_base=0)
    for S in (2, 8, 80):
        m = sgns.SgnsModel(g.n_nodes, dim=128, window=10, negative=5, seed=1)
        m.build_vocab(counts=counts)
        m.train_pass(corpus.walks, corpus.lens, sentences_base=0, sentences_total=corpus.walks.shape[0], walk_id_base=0,
                     splits=S)
        assert m.pairs_trained() == ref.pairs_trained(), S
        auc = linkpred.get_roc_score(m.vectors(), te_d, neg_d)[0]
        print("walk_splits %d: AUC %.5f vs sequential CPU %.5f (%+.5f)" % (S, auc, auc_cpu, auc - auc_cpu))
        assert abs(auc - auc_cpu) <= AUC_BAND, (S, auc, auc_cpu)
    with pytest.raises(Exception):
        ref.train_pass(corpus.walks, corpus.lens, sentences_base=0, sentences_total=1, walk_id_base=0, splits=81)


def test_in_order_items_train_every_sentence_once(torch_cuda):
    """Sentences are handed to the wavefronts through a device counter (n2v_sgns_train's work_counter) instead of a static
    grid stride: every item exactly once — the pair count (a deterministic function of the corpus and the seeds) equals
    the static stride's, at a grid far below and one far above the number of sentences per wave — and a single
    wavefront, which trains the corpus strictly in order either way, leaves bit-identical tables."""
    torch = torch_cuda
    from n2v_hip import sgns
    g, corpus, counts, te_d, neg_d, rounds, auc_cpu = _band_case("uniform")
    walks, lens = corpus.walks[:6000].contiguous(), corpus.lens[:6000].contiguous()

    def run(counter, blocks, n=None):
        m = sgns.SgnsModel(g.n_nodes, dim=128, window=10, negative=5, seed=1)
        m.build_vocab(counts=counts)
        if not counter:
            m.work_counter = None
        w, l = (walks, lens) if n is None else (walks[:n].contiguous(), lens[:n].contiguous())
        m.train_pass(w, l, sentences_base=0, sentences_total=walks.shape[0], walk_id_base=0, max_blocks=blocks)
        torch.cuda.synchronize()
        return m

    want = run(False, 64).pairs_trained()
    for blocks in (1, 7, 64, 3072):
        assert run(True, blocks).pairs_trained() == want, blocks
    a, b = run(True, 1, n=4), run(False, 1, n=4)       # 4 sentences on the 4 waves of one workgroup: one item per wave
    assert a.pairs_trained() == b.pairs_trained()
    one = torch.tensor([[int(x) for x in walks[0].tolist()]], dtype=torch.int32, device=walks.device)
    ln = lens[:1].contiguous()
    ms = []
    for counter in (True, False):
        m = sgns.SgnsModel(g.n_nodes, dim=128, window=10, negative=5, seed=1)
        m.build_vocab(counts=counts)
        if not counter:
            m.work_counter = None
        for rep in range(3):                               # the counter is reset by every launch
            m.train_pass(one, ln, sentences_base=rep, sentences_total=3, walk_id_base=rep, max_blocks=1)
        torch.cuda.synchronize()
        ms.append(m)
    assert torch.equal(ms[0].syn0, ms[1].syn0) and torch.equal(ms[0].syn1neg, ms[1].syn1neg)


def test_parallel_negative_draws_train_the_same_bits(torch_cuda, monkeypatch):
    """The kernel draws all negatives of a centre in parallel (draw d of the centre = the walk's LCG advanced d times)
    instead of pair by pair (N2V_SGNS_PREDRAW=0).  One walk on one wavefront is a sequential, deterministic
    run: both paths must leave bit-identical tables, for every row-sharing mode; on a full corpus (racing wavefronts)
    the pair count is identical."""
    torch = torch_cuda
    from n2v_hip import sgns
    g, corpus, counts, te_d, neg_d, rounds, auc_cpu = _band_case("uniform")
    for mode in ("atomic", "agent", "plain"):
        tables = []
        for flag in ("0", "1"):
            monkeypatch.setenv("N2V_SGNS_PREDRAW", flag)
            m = sgns.SgnsModel(g.n_nodes, dim=128, window=10, negative=5, seed=1, update_mode=mode, allow_out_of_band=True)
            m.build_vocab(counts=counts)
            for w in (0, 7, 1234):                      # three single-walk launches, one wavefront each
                m.train_pass(corpus.walks[w:w + 1], corpus.lens[w:w + 1], sentences_base=w,
                             sentences_total=corpus.walks.shape[0], walk_id_base=w, max_blocks=1)
            torch.cuda.synchronize()
            tables.append((m.syn0.clone(), m.syn1neg.clone(), m.pairs_trained()))
        assert tables[0][2] == tables[1][2] > 1000
        assert torch.equal(tables[0][0], tables[1][0]) and torch.equal(tables[0][1], tables[1][1]), mode
    counts_pairs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("N2V_SGNS_PREDRAW", flag)
        m = sgns.SgnsModel(g.n_nodes, dim=128, window=10, negative=5, seed=1)
        m.build_vocab(counts=counts)
        m.train_pass(corpus.walks, corpus.lens, sentences_base=0, sentences_total=corpus.walks.shape[0], walk_id_base=0,
                     splits=8)
        counts_pairs.append(m.pairs_trained())
    assert counts_pairs[0] == counts_pairs[1]


def test_untouched_rows_stay_put(torch_cuda):
    torch = torch_cuda
    from n2v_hip import sgns
    d = torch.device("cuda:0")
    m = sgns.SgnsModel(100, dim=128, window=5, negative=5, sample=0, seed=9)
    walks = torch.from_numpy(np.random.RandomState(2).randint(0, 50, size=(64, 20)).astype(np.int32)).to(d)
    m.build_vocab(walks)  # ids 50..99 have count 0: never a context, centre or negative
    s0, s1 = m.syn0.clone(), m.syn1neg.clone()
    sgns.train(m, walks, None, epochs=1)
    assert torch.equal(m.syn0[50:], s0[50:]) and torch.equal(m.syn1neg[50:], s1[50:])
    assert not torch.equal(m.syn0[:50], s0[:50])


def _auc_setup():
    from n2v_hip import csr
    from oracle import sgns_oracle
    edges = _planted_partition()
    tr, te = sgns_oracle.split_edges(edges)
    g = csr.from_edges(tr[:, 0], tr[:, 1], None, False)
    in_graph = set(g.labels.tolist())
    te = np.array([e for e in te.tolist() if e[0] in in_graph and e[1] in in_graph])
    neg = np.array(sgns_oracle.build_neg_samples(g.labels.tolist(), edges.tolist(), seed=0))
    return g, te, neg


def test_link_prediction_auc_within_band_of_cpu_comparator(torch_cuda):
    """End to end on one graph: walks on the GPU (bit-exact vs oracle elsewhere), then the same
    walks and the same initial tables into (a) the HIP SGNS kernel and (b) the single-thread
    CPU restatement; cosine link-prediction AUC on a 50/50 edge split must agree within
    +-0.002 (BASELINE.json)."""
    torch = torch_cuda
    import node2vec
    from n2v_hip import linkpred, sgns
    from oracle import c_oracle, sgns_oracle
    g, te, neg = _auc_setup()
    G = node2vec.Graph.from_csr(g, 1.0, 1.0, rng="philox", seed=1)
    G.preprocess_transition_probs()
    corpus = G.simulate_walks(10, 80)
    walks_h, lens_h = corpus.walks.cpu().numpy(), corpus.lens.cpu().numpy()

    m = sgns.SgnsModel(g.n_nodes, dim=128, window=10, negative=5, seed=1)
    m.build_vocab(corpus.walks)
    si, cum = sgns_oracle.vocab_tables(m.counts, 1e-3)
    assert np.array_equal(m.sample_int.cpu().numpy().view(np.uint32), si)
    assert np.array_equal(m.cum_table.cpu().numpy().view(np.uint32), cum)
    sgns.train(m, corpus.walks, corpus.lens, epochs=1)
    torch.cuda.synchronize()
    te_d = np.stack([g.dense_of(te[:, 0]), g.dense_of(te[:, 1])], 1)
    neg_d = np.stack([g.dense_of(neg[:, 0]), g.dense_of(neg[:, 1])], 1)
    auc_gpu, ap_gpu = linkpred.get_roc_score(m.vectors(), te_d, neg_d)

    syn0, syn1 = c_oracle.sgns_init(g.n_nodes, 128, 128, 1)
    pairs_cpu = c_oracle.sgns_train(walks_h, lens_h, syn0, syn1, 128, 10, 5, si, cum, n_threads=1)
    vec = {int(g.labels[i]): syn0[i] for i in range(g.n_nodes)}
    auc_cpu, ap_cpu = sgns_oracle.roc_score(vec, te.tolist(), neg.tolist())
    # the device evaluator agrees with sklearn on the CPU vectors
    auc_chk, ap_chk = linkpred.get_roc_score(torch.from_numpy(syn0).to("cuda:0"), te_d, neg_d)
    assert abs(auc_chk - auc_cpu) < 1e-6 and abs(ap_chk - ap_cpu) < 1e-5  # fp32 cosine on device vs fp64 numpy
    print("AUC gpu %.5f cpu %.5f | AP gpu %.5f cpu %.5f | pairs gpu %d cpu %d" % (
        auc_gpu, auc_cpu, ap_gpu, ap_cpu, m.pairs_trained(), pairs_cpu))
    assert abs(m.pairs_trained() - pairs_cpu) / pairs_cpu < 0.01
    assert auc_cpu > 0.85
    assert abs(auc_gpu - auc_cpu) <= AUC_BAND, (auc_gpu, auc_cpu)
    # opt-in variant: negatives drawn once per centre word and shared by its pairs
    ms = sgns.SgnsModel(g.n_nodes, dim=128, window=10, negative=5, seed=1, share_negatives=True, allow_out_of_band=True)
    ms.build_vocab(corpus.walks)
    sgns.train(ms, corpus.walks, corpus.lens, epochs=1)
    auc_sh, _ = linkpred.get_roc_score(ms.vectors(), te_d, neg_d)
    print("shared negatives: AUC %.5f pairs %d" % (auc_sh, ms.pairs_trained()))
    assert ms.pairs_trained() == m.pairs_trained()
    assert abs(auc_sh - auc_cpu) <= AUC_BAND, (auc_sh, auc_cpu)


def test_learn_embeddings_dropin_surface(torch_cuda, tmp_path):
    """src/main.py flow with the reference's argument names; the result has .wv[str(id)],
    .wv.similarity, .wv.vocab and word2vec text output (src/main.py:82-90, utils.py:417-426)."""
    import main as n2v_main
    from helpers import load_case
    z = load_case("karate_p1_q1")
    p = tmp_path / "karate.edgelist"
    p.write_text("".join("%d %d\n" % (u, v) for u, v in z["edges"].tolist()))
    args = n2v_main.parse_args(["--input", str(p), "--dimensions", "64", "--walk-length", "20", "--num-walks", "4"])
    np.random.seed(1)
    model = n2v_main.main(args)
    wv = model.wv
    assert len(wv.vocab) == 34 and set(wv.vocab) == {str(i) for i in range(1, 35)}
    assert wv["1"].shape == (64,) and wv["1"].dtype == np.float32
    assert -1.0 <= wv.similarity("1", "34") <= 1.0
    counts = [wv.vocab[w].count for w in wv.index2word]
    assert counts == sorted(counts, reverse=True) and sum(counts) == 34 * 4 * 20
    out = tmp_path / "karate.emb"
    wv.save_word2vec_format(str(out))
    lines = out.read_text().splitlines()
    assert lines[0] == "34 64" and len(lines) == 35 and len(lines[1].split()) == 65
    # learn_embeddings on plain lists of labels (walks reloaded from a file)
    n2v_main.args = args
    model2 = n2v_main.learn_embeddings([[1, 2, 3, 4], [4, 3, 2, 1, 34]])
    assert set(model2.wv.vocab) == {"1", "2", "3", "4", "34"}


_BAND_CASES = {}


def _band_case(kind):
    """(graph, walks, counts, test pairs, negative pairs, rounds, AUC of the single-thread CPU comparator).  The
    comparator's figure comes from the committed fixture (tests/golden/sgns_band/, made by make_sgns_band.py on the C
    oracle's walks; the GPU's walks are checked against the fixture's hash) — the hub comparator alone takes seven
    minutes of one core; test_link_prediction_auc_within_band_of_cpu_comparator still runs one comparison live."""
    if kind in _BAND_CASES:
        return _BAND_CASES[kind]
    from test_gpu_sgns_band import gpu_case
    g, corpus, counts, te_d, neg_d, fx = gpu_case({"uniform": "uniform3k_10x80", "hub": "hub20k_10x80"}[kind])
    _BAND_CASES[kind] = (g, corpus, counts, te_d, neg_d, fx["rounds"], fx["auc_cpu"])
    return _BAND_CASES[kind]


@pytest.mark.parametrize("kind,G", [("uniform", 1), ("uniform", 2), ("uniform", 4), ("uniform", 8),
                                    ("hub", 1), ("hub", 2), ("hub", 4), ("hub", 8)])
def test_multi_gpu_scheme_auc_within_band_simulated(torch_cuda, kind, G):
    """merge="hot", the faster optional multi-GPU scheme (start-vertex shards, one replica per rank, 'hot'-weighted
    merges at the auto_syncs cadence, synchronous merges, bf16 wire) scored on ONE GPU by training G
    replicas interval by interval with the same ReplicaMerger, kernels and schedule as n2v_hip.sgns.train: AUC
    within +-0.002 of the sequential CPU comparator on a uniform and on a hub-heavy graph (C4 is power-law)."""
    torch = torch_cuda
    from n2v_hip import linkpred, sgns
    g, corpus, counts, te_d, neg_d, rounds, auc_cpu = _band_case(kind)
    n = g.n_nodes
    models, shards = [], []
    for r in range(G):
        m = sgns.SgnsModel(n, dim=128, window=10, negative=5, seed=1)
        m.build_vocab(counts=counts)
        models.append(m)
        b, e = sgns.shard_bounds(n, G, r)
        idx = (torch.arange(rounds, device="cuda")[:, None] * n + torch.arange(b, e, device="cuda")[None, :]).reshape(-1)
        shards.append((corpus.walks[idx].contiguous(), corpus.lens[idx].contiguous(), b * rounds))
    if G == 1:
        sgns.train(models[0], corpus.walks, corpus.lens, epochs=1)
        n_syncs = 0
    else:
        n_syncs = sgns.train_simulated_replicas(models, shards, n_walks_global=corpus.walks.shape[0], merge="hot")
    torch.cuda.synchronize()
    for m in models[1:]:
        assert torch.equal(m.syn0, models[0].syn0) and torch.equal(m.syn1neg, models[0].syn1neg)
    auc, _ = linkpred.get_roc_score(models[0].vectors(), te_d, neg_d)
    print("%s G=%d syncs=%d: AUC %.5f vs sequential CPU %.5f (%+.5f)" % (kind, G, n_syncs, auc, auc_cpu, auc - auc_cpu))
    assert abs(auc - auc_cpu) <= AUC_BAND, (kind, G, n_syncs, auc, auc_cpu)


@pytest.mark.parametrize("kind,G", [("uniform", 2), ("uniform", 8), ("hub", 2), ("hub", 4)])
def test_tiered_sum_merges_auc_within_band_simulated(torch_cuda, kind, G):
    """merge="tsum", the default — pure sums at per-row cadences (every row 234 times per pass at 8 replicas, hub rows 4 / 16 / 64
    times as often), no damping, no fitted weights: inside the band on both graphs (uniform +0.0003 / -0.0004 at 2 / 8
    replicas, hub +0.0014 / +0.0005 at 2 / 4).  Eight replicas on a hub graph are scored at 131 072 nodes
    (tests/test_gpu_sgns_band.py: +0.0001) — on the 20k graph that case is two walks per launch, three minutes of
    launches for -0.0002 (profiles/r03/logs/pytest_sgns_band_splits_rule.log).  These graphs are below
    AUTO_SPLITS_MIN_WORDS rows: one wavefront per walk (with several, the 20k hub graph was +0.0026 at 2 replicas)."""
    torch = torch_cuda
    from n2v_hip import linkpred, sgns
    g, corpus, counts, te_d, neg_d, rounds, auc_cpu = _band_case(kind)
    n = g.n_nodes
    models, shards = [], []
    for r in range(G):
        m = sgns.SgnsModel(n, dim=128, window=10, negative=5, seed=1)
        m.build_vocab(counts=counts)
        models.append(m)
        b, e = sgns.shard_bounds(n, G, r)
        idx = (torch.arange(rounds, device="cuda")[:, None] * n + torch.arange(b, e, device="cuda")[None, :]).reshape(-1)
        shards.append((corpus.walks[idx].contiguous(), corpus.lens[idx].contiguous(), b * rounds))
    n_syncs = sgns.train_simulated_replicas(models, shards, n_walks_global=corpus.walks.shape[0], merge="tsum")
    torch.cuda.synchronize()
    for m in models[1:]:
        assert torch.equal(m.syn0, models[0].syn0) and torch.equal(m.syn1neg, models[0].syn1neg)
    auc, _ = linkpred.get_roc_score(models[0].vectors(), te_d, neg_d)
    print("tsum %s G=%d base syncs=%d: AUC %.5f vs sequential CPU %.5f (%+.5f)" % (kind, G, n_syncs, auc, auc_cpu, auc - auc_cpu))
    assert abs(auc - auc_cpu) <= AUC_BAND, (kind, G, n_syncs, auc, auc_cpu)


def test_fused_tiered_sum_kernels_equal_per_table_path(torch_cuda):
    """n2v_tsum_pack / n2v_tsum_apply (all tables of a merge level in one launch) against the per-table restatement in
    torch (tests/merge_reference.py), bit for bit, float32 and bfloat16 wires, every level of a three-tier plan."""
    torch = torch_cuda
    import numpy as np
    from merge_reference import TorchMergeOps
    from n2v_hip import sgns

    class Doubling:                          # stands in for the all-reduce of two identical replicas
        world, rank = 2, 0

        def __init__(self, wire):
            self.wire_dtype = wire

        def all_reduce_async(self, t):
            t.mul_(2)
            return None

    g = torch.Generator(device="cuda").manual_seed(11)
    n, stride = 1500, 128
    counts = (np.random.default_rng(2).random(n) ** 6 * 40000 + 1).astype(np.int64)
    plan = sgns.SumTierPlan(counts, 3.0e5, 2, 10, 5, torch.device("cuda"), theta=30.0, n_tiers=3, ratio=4)
    assert all(0 < plan.rows_ge[i][2].numel() < plan.rows_ge[i][1].numel() < n for i in range(2))
    for wire in (torch.float32, torch.bfloat16):
        t0 = [torch.randn(n, stride, device="cuda", generator=g) for _ in range(2)]
        a = [t.clone() for t in t0]
        b = [t.clone() for t in t0]
        fused = sgns.TieredSumMerger(a, plan, Doubling(wire))
        plain = sgns.TieredSumMerger(b, plan, Doubling(wire), ops=TorchMergeOps())
        assert fused.fused and not plain.fused
        for step, level in enumerate([2, 2, 1, 2, 0, 1, 2, 0]):
            d = [torch.randn(n, stride, device="cuda", generator=g) * 0.01 for _ in range(2)]
            for x, y, dd in zip(a, b, d):
                x += dd
                y += dd
            fused.merge(level)
            plain.merge(level)
            for x, y in zip(a, b):
                assert torch.equal(x, y), (wire, step, level)
        for i in range(2):
            assert torch.equal(fused.base[i], plain.base[i]) and torch.equal(a[i], fused.base[i])
        assert fused.n_merges == plain.n_merges == [2, 2, 4]


def test_merge_kernels_equal_torch_restatement(torch_cuda):
    """n2v_merge_snapshot / _hot_apply / _flush (csrc/n2v_merge.hip) against tests/merge_reference.py, bit for bit,
    with float32 and bfloat16 wires, with and without a hot tier and a pending cold sum."""
    torch = torch_cuda
    from merge_reference import TorchMergeOps
    from n2v_hip import sgns
    hip, ref = sgns.HipMergeOps(), TorchMergeOps()
    g = torch.Generator(device="cuda").manual_seed(3)
    n, stride = 777, 128
    for wire in (torch.float32, torch.bfloat16):
        for n_hot in (0, 40, n):
            hot_rows = torch.randperm(n, device="cuda", generator=g)[:n_hot].sort().values
            pos = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            pos[hot_rows] = torch.arange(n_hot, dtype=torch.int32, device="cuda")
            w = torch.rand(n, device="cuda", generator=g)
            state = [torch.randn(n, stride, device="cuda", generator=g) for _ in range(3)]
            prev = torch.randn(n, stride, device="cuda", generator=g).to(wire)
            hsum = torch.randn(max(n_hot, 1), stride, device="cuda", generator=g).to(wire)[:n_hot]
            for sum_prev in (None, prev):
                outs = []
                for ops in (hip, ref):
                    x, xs, base = (t.clone() for t in state)
                    cold = torch.full((n, stride), 7.0, device="cuda").to(wire) if n_hot < n else None
                    hw = torch.full((max(n_hot, 1), stride), 7.0, device="cuda").to(wire)[:n_hot] if n_hot else None
                    ops.snapshot(x, xs, base, w, pos if n_hot else None, sum_prev, cold, hw)
                    if n_hot:
                        ops.hot_apply(x, xs, base, w, hot_rows, hsum)
                    snap = [t.clone() for t in (x, xs, base)] + ([cold.clone()] if cold is not None else []) + ([hw.clone()] if n_hot else [])
                    ops.flush(x, xs, base, w, pos if n_hot else None, sum_prev)
                    outs.append(snap + [x, xs, base])
                assert len(outs[0]) == len(outs[1])
                for a_, b_ in zip(*outs):
                    assert torch.equal(a_, b_), (wire, n_hot, sum_prev is None)
            if n_hot:       # the row-list pack of the tiered pure-sum merges
                packs = []
                for ops in (hip, ref):
                    wbuf = torch.zeros((n, stride), device="cuda").to(wire)
                    ops.pack_rows(state[0], state[2], hot_rows, wbuf[:n_hot])
                    packs.append(wbuf)
                assert torch.equal(packs[0], packs[1])


def test_main_link_flow_end_to_end(torch_cuda):
    """src/main_link.py:519-563 flow on the device (split 50/50 seed 123, walk + embed on the
    training graph, cosine AUC/AP on test edges vs sampled non-edges), settings.py defaults."""
    from n2v_hip import linkpred
    edges = _planted_partition(n=2000, k=20, m_in=16000, m_out=3000, seed=3)
    res = linkpred.run(edges, p=1.0, q=1.0, num_walks=5, walk_length=40, dimensions=128, window_size=10)
    assert res["n_train"] + res["n_test"] == len(edges) and abs(res["n_train"] - res["n_test"]) <= 1
    assert 0.8 < res["roc"] <= 1.0 and 0.7 < res["ap"] <= 1.0, (res["roc"], res["ap"])
    print("main_link flow: AUC %.4f AP %.4f" % (res["roc"], res["ap"]))


def test_main_link_flow_with_user_edges(torch_cuda):
    """src/main_link.py:568-599: add similarity edges between user nodes (ids without the
    '9999999' item prefix), walk + embed on the augmented weighted graph, score again; the
    device selection equals the oracle's restatement on the embedding it was given."""
    torch = torch_cuda
    from n2v_hip import augment, linkpred
    from oracle import augment_oracle
    edges = _planted_partition(n=600, k=6, m_in=5000, m_out=800, seed=4)
    item = edges[:, 1] % 3 == 0                     # a third of the nodes play the item role
    edges = edges.copy()
    relabel = lambda x: np.where(x % 3 == 0, 99999990000 + x, x)
    edges = np.stack([relabel(edges[:, 0]), relabel(edges[:, 1])], 1)
    res = linkpred.run(edges, num_walks=5, walk_length=40, add_user_edges=True, user_edges_mode="ratio",
                       user_edges_ratio=0.02)
    assert res["roc_user"] is not None and 0.5 < res["roc_user"] <= 1.0
    g = res["graph"]._csr
    users = augment.user_nodes(g.labels[g.start_order])
    assert len(users) == int((g.labels < 99999990000).sum()) and res["edges_added"] == len(users) * int(len(users) * 0.02)
    assert res["graph_user"]._csr.w is not None     # the augmented graph is weighted
    # device selection == oracle on the same vectors
    vec = res["model"].vectors()
    ud = torch.as_tensor(g.dense_of(users).astype(np.int64), device=vec.device)
    s, d, w = augment.add_edges(vec[ud], "ratio", 0.02, 0.5)
    emb = {int(u): vec[int(i)].cpu().numpy() for u, i in zip(users, ud.tolist())}
    want = augment_oracle.add_user_edge([int(u) for u in users], emb, "ratio", 0.02, 0.5)
    got = list(zip(users[s.cpu().numpy()].tolist(), users[d.cpu().numpy()].tolist()))
    want_pairs = [(x[0], x[1]) for x in want]
    agree = sum(1 for a, b in zip(got, want_pairs) if a == b) / max(len(want), 1)
    same = len(set(got) & set(want_pairs)) / max(len(want), 1)
    # fp32 GEMM vs per-pair dot: near-ties may swap places (the vectors come out of a racing training run, so how many
    # there are differs from run to run: 0 ... 4 of 3 200) and, at the cut of a user's list, membership
    assert len(got) == len(want) and same > 0.999 and agree > 0.995, (same, agree)
    print("user edges: %d added, AUC %.4f -> %.4f" % (res["edges_added"], res["roc"], res["roc_user"]))


def test_tiered_merges_graph_replay_equals_eager_loop(torch_cuda):
    """The default multi-GPU path replays ONE captured base interval of the tiered merges ([train, pack, all-reduce,
    apply] x sub-intervals; the training launches read their walk range from a device counter) instead of issuing
    ~15 000 launches per pass from Python.  With one walk per launch on one wavefront the run is sequential, so the
    replayed graph must leave bit-identical tables, pair counts and merge counts — through a real RCCL all-reduce
    (one-rank group standing in for a world of four: what the collective returns for one rank is its input)."""
    torch = torch_cuda
    import os
    import torch.distributed as dist
    from n2v_hip import sgns
    from n2v_hip import dist as n2v_dist
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    had = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29910 + os.getpid() % 40)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        comm = n2v_dist._Comm(False)
        comm.world = 4                                   # plan the merges of a 4-GPU job; the wire is the one-rank group
        assert comm.graph_capturable and comm.wire_dtype == torch.bfloat16
        rs = np.random.RandomState(4)
        n_words, L, epochs = 1500, 24, 2
        p = rs.pareto(1.1, n_words) + 0.05
        p /= p.sum()
        results = []
        walks = None
        for graph in (False, True):
            m = sgns.SgnsModel(n_words, dim=64, window=5, negative=5, seed=5)
            if walks is None:
                # a corpus with exactly one walk per sub-interval: counts first (they fix the tier plan), then the size
                big = rs.choice(n_words, size=(4096, L), p=p).astype(np.int32)
                counts = np.bincount(big.reshape(-1), minlength=n_words)
                m.build_vocab(counts=counts)
                n_chunks, plan = sgns._tsum_setup(m, L, 4096 * 4, 4, 3)
                assert plan.n_tiers >= 2 and n_chunks == 3
                n_local = n_chunks * plan.sub
                walks = torch.from_numpy(big[:n_local].copy()).cuda()
            else:
                m.build_vocab(counts=counts)
            mg = sgns.train(m, walks, None, epochs=epochs, comm=comm, n_walks_global=4096 * 4, shard_offset=4096,
                            syncs_per_epoch=3, merge="tsum", graph=graph, splits=1)
            torch.cuda.synchronize()
            assert (getattr(mg, "graph_replays", 0) == 3 * epochs) == graph
            results.append((m.syn0.clone(), m.syn1neg.clone(), m.pairs_trained(), list(mg.n_merges),
                            [b.clone() for b in mg.base]))
        e, g = results
        assert e[2] == g[2] > 0 and e[3] == g[3] and sum(e[3]) == 3 * epochs * plan.sub
        assert torch.equal(e[0], g[0]) and torch.equal(e[1], g[1])
        assert all(torch.equal(a, b) for a, b in zip(e[4], g[4]))
        assert torch.equal(g[0], g[4][0])               # after the last (full) merge the table IS the agreed copy
    finally:
        dist.destroy_process_group()
        for k, v in had.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_rccl_path_of_the_merges_single_rank(torch_cuda):
    """The exact calls the multi-GPU merges make over RCCL (bf16 / fp32 wire formats, gathered hot rows), on a
    one-rank process group: what the collective returns for one rank is its input, so the results are known."""
    torch = torch_cuda
    import os
    import torch.distributed as dist
    from n2v_hip import bine, sgns
    from n2v_hip import dist as n2v_dist
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    had = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29950 + os.getpid() % 40)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        comm = n2v_dist._Comm(False)
        assert comm.world == 1 and comm.wire_dtype == torch.bfloat16 and comm.wire_dtype_f64 == torch.float32
        g = torch.Generator(device="cuda").manual_seed(1)
        base = torch.randn(64, 128, device="cuda", generator=g)
        # one interval and the flush of a one-rank "world": the sum of the changes is the rank's own change, sent
        # as bfloat16, for the synchronous tier (rows 3, 9) and for the delayed tier alike
        plan = sgns.MergePlan.__new__(sgns.MergePlan)
        rows = torch.tensor([3, 9], device="cuda")
        pos = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        pos[rows] = torch.arange(2, dtype=torch.int32, device="cuda")
        w = torch.full((64,), 0.5, device="cuda")
        plan.w, plan.hot_rows, plan.hot_pos, plan.n_hot, plan.n_cold, plan.world, plan.cold_delay = [w], [rows], [pos], [2], [62], 1, True
        for overlap in (True, False):
            t = base.clone()
            mg = sgns.ReplicaMerger([t], plan, comm, overlap=overlap)
            assert mg.hot_wire.dtype == torch.bfloat16 and mg.cold_wire[0].dtype == torch.bfloat16
            d = 0.01 * torch.randn(64, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
            t += d
            mg.end_interval(last=True)
            torch.cuda.synchronize()
            want = base + 0.5 * ((base + d) - base).bfloat16().float()
            assert torch.allclose(t, want, atol=1e-7), (overlap, (t - want).abs().max())
            assert torch.equal(mg.base[0], t) and torch.equal(mg.xs[0], t)
            sec = mg.seconds()
            assert sec["merge"] >= sec["wait"] >= 0.0 and mg.n_merges == 1
        import types
        b64 = base.double()
        eng = types.SimpleNamespace(emb=b64.clone(), ctx=b64.clone(), state=torch.zeros(8, dtype=torch.float64, device="cuda"))
        m = bine.ReplicaMerge(eng, comm)
        eng.emb += 1e-3
        eng.state[1] = -3.0
        m(eng)
        assert torch.allclose(eng.emb, b64 + 1e-3, atol=1e-9) and torch.equal(eng.ctx, b64) and eng.state[1].item() == -3.0
        counts = torch.ones(10, dtype=torch.int64, device="cuda")
        comm.all_reduce_sum(counts)
        assert int(counts.sum()) == 10
    finally:
        dist.destroy_process_group()
        for k, v in had.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
