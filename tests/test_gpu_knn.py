"""GPU tests of the fused k-NN kernel (csrc/n2v_knn.hip, n2v_sim_knn) and of n2v_hip/neighbors.py on top of it.

Every comparison is an equality: the score of a pair is an exact small integer (integer operands) or, by definition, the
bits n2v_sim_block writes for it (tests/test_gpu_sim_exact.py holds those to float64), and the order is the restatement
tests/knn_reference.py of csrc/n2v_rank.h.  No tolerance, no tie allowance; a NaN's sign and payload are the only bits
outside the contract.  The case tables are tests/knn_cases.py; tests/test_knn_host.py proves on the CPU what they hold.
Run with N2V_SIM_VECTOR unset (the oracle's n2v_sim_block must take its MFMA kernel)."""
import functools
import os
import sys

import numpy as np
import pytest

import knn_cases as K
import knn_reference as R
import sim_reference as SR
from helpers import ROOT

pytestmark = pytest.mark.gpu

GUARD = 256                         # sentinel bytes on both sides of the scratch
ISENT, SENT = -7, np.float32(-12345.5)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    assert os.environ.get("N2V_SIM_VECTOR", "0") != "1", "the oracle's n2v_sim_block must run its MFMA kernel"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _knn(torch, Q, B, k, n_seg, exclude, method="cos"):
    """n2v_sim_knn on device operands: cols / vals sit between sentinel rows, the scratch between sentinel bytes and is
    pre-filled with garbage.  Returns (cols, vals) as numpy after checking that nothing outside was written."""
    from n2v_hip import _lib, simsel
    lib = _lib.load()
    n_q, n_cols = int(Q.shape[0]), int(B.shape[0])
    nbytes = int(lib.n2v_sim_knn_scratch(n_q, k, n_seg))
    assert nbytes >= 0
    scratch = torch.full((nbytes + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=Q.device)
    if nbytes:
        scratch[GUARD:GUARD + nbytes] = _dev(torch, np.random.RandomState(nbytes % 9973).randint(0, 256, nbytes).astype(np.uint8))
    cols = torch.full((n_q + 2, k), ISENT, dtype=torch.int32, device=Q.device)
    vals = torch.full((n_q + 2, k), float(SENT), dtype=torch.float32, device=Q.device)
    ex = None if exclude is None else _dev(torch, exclude.astype(np.int32))
    _lib.check(lib.n2v_sim_knn(_lib.ptr(Q), n_q, _lib.ptr(B), n_cols, int(Q.shape[1]), simsel.METHODS[method], _lib.ptr(ex), k,
                               n_seg, scratch.data_ptr() + GUARD, cols.data_ptr() + 4 * k, vals.data_ptr() + 4 * k,
                               _lib.stream_ptr(Q.device)))
    torch.cuda.synchronize()
    s, c, v = scratch.cpu().numpy(), cols.cpu().numpy(), vals.cpu().numpy()
    assert (s[:GUARD] == 0x5A).all() and (s[GUARD + nbytes:] == 0x5A).all(), "wrote outside the scratch"
    assert (c[[0, -1]] == ISENT).all() and (v[[0, -1]].view(np.uint32) == SENT.view(np.uint32)).all(), "wrote outside cols / vals"
    return c[1:-1], v[1:-1]


@functools.lru_cache(maxsize=None)
def _int_oracle(i):
    c = K.int_case(i)
    return c, R.rank_rows(K.int_scores(c), c["k"], c["exclude"])


# ================================================================================================ 1. integer operands
@pytest.mark.parametrize("i", range(len(K.CASES)))
def test_integer_operands_equal_the_host_oracle(torch_cuda, i):
    """Scores are small integers, exact in any order, with ties by the thousand and duplicated rows across the wavefront,
    tile and segment borders: a wrong lane / register map, border guard, exclusion or tie rule cannot hide.  The
    sentinels around cols, vals and the scratch (garbage inside) stay untouched."""
    c, (wc, wv) = _int_oracle(i)
    cols, vals = _knn(torch_cuda, _dev(torch_cuda, c["Q"]), _dev(torch_cuda, c["B"]), c["k"], c["n_seg"], c["exclude"])
    assert R.same(cols, vals, wc, wv), K.CASES[i]


def test_one_repeated_row_returns_the_first_k_columns(torch_cuda):
    rs = np.random.RandomState(1)
    row = rs.randint(-2, 3, size=(1, 64)).astype(np.float32)
    B = np.repeat(row, 700, axis=0)
    Q = rs.randint(-2, 3, size=(130, 64)).astype(np.float32)
    ex = np.where(np.arange(130) % 2 == 0, np.arange(130) % 7, -1).astype(np.int32)
    for k, n_seg in ((256, 3), (65, 0), (1, 32)):
        cols, vals = _knn(torch_cuda, _dev(torch_cuda, Q), _dev(torch_cuda, B), k, n_seg, ex)
        for q in range(130):
            want = [c for c in range(k + 1) if c != ex[q]][:k]
            assert cols[q].tolist() == want
        assert np.array_equal(vals, np.repeat((Q @ row[0])[:, None], k, axis=1))


# ================================================================================================ 2. real operands
def _prepared(torch, vec, method):
    from n2v_hip import simsel
    return simsel.prepare(_dev(torch, vec), method)


def _block_scores(torch, Qp, Bp, method):
    from n2v_hip import simsel
    return simsel.score_block(Qp, 0, int(Qp.shape[0]), Bp, method).cpu().numpy()


@pytest.mark.parametrize("method", ["cos", "pearson"])
@pytest.mark.parametrize("i", range(len(K.REAL_CASES)))
def test_real_operands_equal_the_ranked_block_scores(torch_cuda, i, method):
    """The oracle's scores are n2v_sim_block's output on the same prepared operands: the fused kernel must reproduce
    them bit for bit at any tile position and rank them.  A NaN column is chosen only once everything else is; the
    all-zero row scores exactly 0 under "cos"."""
    torch = torch_cuda
    c = K.real_case(i)
    Qp, Bp = _prepared(torch, c["q"], method), _prepared(torch, c["b"], method)
    S = _block_scores(torch, Qp, Bp, method)
    assert np.isnan(S[:, K.REAL_NAN_ROW]).all()
    if method == "cos":
        assert (np.ascontiguousarray(S[:, K.REAL_ZERO_ROW]).view(np.uint32) == 0).all()
    wc, wv = R.rank_rows(S, c["k"], c["exclude"])
    for n_seg in (0, 2):
        cols, vals = _knn(torch, Qp, Bp, c["k"], n_seg, c["exclude"], method)
        assert R.same(cols, vals, wc, wv), (K.REAL_CASES[i], method, n_seg)
    if method == "cos":                              # the only NaN column; under "pearson" the zero row is one too
        ex = np.full(c["n_q"], -1) if c["exclude"] is None else c["exclude"]
        real = (c["n_cols"] - 1) - ((ex >= 0) & (ex < c["n_cols"]) & (ex != K.REAL_NAN_ROW))
        assert np.array_equal((cols == K.REAL_NAN_ROW).any(axis=1), (c["k"] > real) & (ex != K.REAL_NAN_ROW))


# ================================================================================================ 3. segmentation
@pytest.mark.parametrize("i", K.SEG_CASES)
def test_result_does_not_depend_on_the_segmentation(torch_cuda, i):
    torch = torch_cuda
    c, (wc, wv) = _int_oracle(i)
    Q, B = _dev(torch, c["Q"]), _dev(torch, c["B"])
    seen = set()
    for seg in K.SEGS + (K.SEGS[0],):               # the first one twice: two runs give the same bytes
        cols, vals = _knn(torch, Q, B, c["k"], K.seg_value(seg, c["n_cols"]), c["exclude"])
        seen.add(cols.tobytes() + vals.tobytes())
        assert R.same(cols, vals, wc, wv), (K.CASES[i], seg)
    assert len(seen) == 1


# ================================================================================================ 5. both paths
@functools.lru_cache(maxsize=None)
def _path_data():
    rs = np.random.RandomState(77)
    vec = rs.normal(size=(385, 40)).astype(np.float32)
    vec[200] = vec[10]                                # a duplicate row: equal scores in every query
    vec[300] = 0.0
    return vec


def _knn_oracle(torch, vec, k, method, queries=None, exclude=None):
    Bp = _prepared(torch, vec, method)
    Qp = Bp if queries is None else queries
    return R.rank_rows(_block_scores(torch, Qp, Bp, method), k, exclude)


@pytest.mark.parametrize("method", ["cos", "pearson"])
def test_block_and_fused_paths_agree_with_the_oracle(torch_cuda, method):
    torch = torch_cuda
    from n2v_hip import neighbors as N
    vec = _path_data()
    n = vec.shape[0]
    v = _dev(torch, vec)
    for k in (1, 10, 256):
        wc, wv = _knn_oracle(torch, vec, k, method, exclude=np.arange(n))
        for path in ("fused", "block", "auto"):
            idx, score = N.knn(v, k, method=method, path=path)
            assert idx.dtype == torch.int32 and score.dtype == torch.float32 and idx.is_cuda and tuple(idx.shape) == (n, k)
            assert R.same(idx.cpu().numpy(), score.cpu().numpy(), wc, wv), (k, path)
    for k in (257, 300, n - 1, n):
        for excl in (True, False):
            wc, wv = _knn_oracle(torch, vec, k, method, exclude=np.arange(n) if excl else None)
            idx, score = N.knn(v, k, method=method, path="block", exclude_self=excl)
            assert R.same(idx.cpu().numpy(), score.cpu().numpy(), wc, wv), (k, excl)
    with pytest.raises(ValueError, match="at most 256"):
        N.knn(v, 257, path="fused")


def test_auto_path_query_blocks_and_query_forms(torch_cuda, monkeypatch):
    torch = torch_cuda
    from n2v_hip import neighbors as N
    vec = _path_data()
    n = vec.shape[0]
    v = _dev(torch, vec)
    calls = []
    fused, block = N._fused, N._block
    monkeypatch.setattr(N, "_fused", lambda *a: (calls.append("fused"), fused(*a))[1])
    monkeypatch.setattr(N, "_block", lambda *a: (calls.append("block"), block(*a))[1])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert N.auto_path(n, n, 10, 64, cus) == "block"            # a small matrix: insertions cost more than stored scores
    N.knn(v, 10)
    N.knn(v, 257)
    monkeypatch.setattr(N, "BLOCK_SECONDS", 1.0)                # as if stored scores were dear: the documented other choice
    assert N.auto_path(n, n, 256, 64, cus) == "fused" and N.auto_path(n, n, 257, 64, cus) == "block"
    N.knn(v, 256)
    N.knn(v, 257)
    monkeypatch.undo()
    assert calls == ["block", "block", "fused", "block"]
    # the query-block size does not change the result, on either path
    wc, wv = _knn_oracle(torch, vec, 10, "cos", exclude=np.arange(n))
    for path in ("fused", "block"):
        for qb in (1, 100, 128):
            idx, score = N.knn(v, 10, path=path, query_block=qb)
            assert R.same(idx.cpu().numpy(), score.cpu().numpy(), wc, wv), (path, qb)
    # index queries (self kept or excluded) and a separate query tensor
    q_idx = np.array([200, 10, 0, 384, 300])
    Bp = _prepared(torch, vec, "cos")
    for excl in (False, True):
        wc, wv = R.rank_rows(_block_scores(torch, Bp[_dev(torch, q_idx)], Bp, "cos"), 7, q_idx if excl else None)
        for path in ("fused", "block"):
            idx, score = N.knn(v, 7, queries=torch.from_numpy(q_idx), exclude_self=excl, path=path)
            assert R.same(idx.cpu().numpy(), score.cpu().numpy(), wc, wv), (excl, path)
    other = np.random.RandomState(5).normal(size=(33, 40)).astype(np.float32)
    wc, wv = R.rank_rows(_block_scores(torch, _prepared(torch, other, "cos"), Bp, "cos"), 12)
    for path in ("fused", "block"):
        idx, score = N.knn(v, 12, queries=_dev(torch, other), path=path)
        assert R.same(idx.cpu().numpy(), score.cpu().numpy(), wc, wv), path
    with pytest.raises(ValueError, match="exclude_self"):
        N.knn(v, 3, queries=_dev(torch, other), exclude_self=True)


# ================================================================================================ 6. most_similar
def _vocab(kind):
    rs = np.random.RandomState(11)
    n, d = 300, 24
    vec = rs.normal(size=(n, d)).astype(np.float32)
    vec[50] = vec[3] * 2.0                                           # same direction: near-equal cosines
    if kind == "kv":
        from n2v_hip.sgns import KeyedVectors
        return KeyedVectors(np.arange(1000, 1000 + n), np.arange(n, 0, -1), vec)
    from n2v_hip.word2vec import LabelKeyedVectors
    return LabelKeyedVectors(["w%d" % i for i in range(n)], np.arange(n, 0, -1), vec)


def _most_similar_oracle(torch, kv, positive, negative, topn, restrict_vocab=None):
    """The restatement composed from the device's own prepared rows and block scores."""
    from n2v_hip import simsel
    P = kv.init_sims().prepared
    Ph = P.cpu().numpy()
    d = kv.syn0.shape[1]
    terms = [(1.0, t) for t in positive] + [(-1.0, t) for t in negative]
    words = [kv.vocab[t].index for _, t in terms if not isinstance(t, np.ndarray)]
    rows = [t if isinstance(t, np.ndarray) else Ph[kv.vocab[t].index, :d] for _, t in terms]
    q = R.mean_query([w for w, _ in terms], rows)
    Qp = simsel.prepare(_dev(torch, q[None, :]), "cos")
    limit = len(kv.index2word) if restrict_vocab is None else restrict_vocab
    S = _block_scores(torch, Qp, P[:limit], "cos")[0]
    return S if topn is None else R.most_similar(S, kv.index2word, words, topn)


@pytest.mark.parametrize("kind", ["kv", "lkv"])
def test_most_similar_equals_the_restatement(torch_cuda, kind):
    torch = torch_cuda
    kv = _vocab(kind)
    w = kv.index2word
    extra = np.random.RandomState(2).normal(size=kv.syn0.shape[1]).astype(np.float32)
    for positive, negative in (([w[3]], []), ([w[3], w[50], w[7]], [w[100]]), ([w[1], extra], [w[2]])):
        for topn, rv in ((10, None), (5, 120), (1000, None), (300, 64), (255, None)):
            got = kv.most_similar(positive=positive, negative=negative, topn=topn, restrict_vocab=rv)
            want = _most_similar_oracle(torch, kv, positive, negative, topn, rv)
            assert got == want and all(isinstance(s, float) for _, s in got), (positive, negative, topn, rv)
            limit = len(w) if rv is None else rv
            n_in = sum(1 for t in positive + negative if not isinstance(t, np.ndarray) and kv.vocab[t].index < limit)
            assert len(got) == min(topn, limit - n_in)
        full = kv.most_similar(positive=positive, negative=negative, topn=None)
        assert full.dtype == np.float32 and np.array_equal(full.view(np.uint32), _most_similar_oracle(torch, kv, positive, negative, None).view(np.uint32))
    assert kv.most_similar(w[3]) == kv.similar_by_word(w[3]) == _most_similar_oracle(torch, kv, [w[3]], [], 10)
    assert kv.similar_by_vector(extra, topn=4, restrict_vocab=90) == _most_similar_oracle(torch, kv, [extra], [], 4, 90)
    assert kv.most_similar(extra, topn=3) == kv.similar_by_vector(extra, topn=3)
    assert kv.init_sims() is kv.init_sims("cuda:0")


# ================================================================================================ 7. sanity against fp64
def test_arc_neighbours_equal_the_float64_order(torch_cuda):
    """Neighbouring cosines are at least 10^-3 apart (tests/test_knn_host.py asserts it in float64), over 100 times the
    fp32 bound: the labels must equal numpy float64's argsort, no case left out and no tie allowance."""
    torch = torch_cuda
    from n2v_hip import neighbors as N
    vec, query = R.arc_data()
    want = np.argsort(-R.arc_cosines(vec, query), kind="stable")
    for path in ("fused", "block"):
        idx, score = N.knn(_dev(torch, vec), R.ARC_N, queries=_dev(torch, query), path=path)
        assert idx[0].cpu().numpy().tolist() == want.tolist(), path
        # unit rows at dpad 128 and two normalisations of 100 terms, counted as tests/sim_reference.py counts them
        bound = float(SR.gamma(SR.dpad_of(R.ARC_D)) + 2 * SR.gamma(R.ARC_D + 3))
        assert np.abs(score[0].cpu().numpy().astype(np.float64) - R.arc_cosines(vec, query)[want]).max() <= bound


# ================================================================================================ 8. find_similar_users
def _write_emb(path, labels, vec):
    with open(path, "w") as f:
        f.write("%d %d\n" % vec.shape)
        for l, row in zip(labels, vec):
            f.write("%s %s\n" % (l, " ".join("%f" % x for x in row)))


def _similar_oracle(torch, path, target, n):
    from n2v_hip import io as nio
    words, vecs = nio.load_word2vec_format(path)
    pos = [i for i, w in enumerate(words) if not w.startswith("9999999")]
    users = [words[i] for i in pos]
    P = _prepared(torch, vecs[pos], "cos")
    t = users.index(target)
    cols, _ = R.rank(_block_scores(torch, P[t:t + 1], P, "cos")[0], n)
    return users, [users[c] for c in cols if c >= 0]


def test_find_similar_users_on_a_written_embedding(torch_cuda, tmp_path):
    import random
    from n2v_hip import neighbors as N
    rs = np.random.RandomState(4)
    labels = []
    for i in range(90):                                            # item labels interleaved with the users
        labels.append(str(10 + i) if i % 3 else "9999999%d" % i)
    vec = rs.normal(size=(90, 16)).astype(np.float32)
    path = str(tmp_path / "ue.emb")
    _write_emb(path, labels, vec)
    users, want = _similar_oracle(torch_cuda, path, "26", int(0.1 * 60))
    assert len(users) == 60
    got = N.find_similar_users(path, 0.1, target="26")
    assert got == want and len(got) == 6 and got[0] == "26" and len(set(got)) == 6
    # the default target is the seeded choice among the users, in file order
    t = random.Random(3).choice(users)
    assert N.find_similar_users(path, 0.5, seed=3) == _similar_oracle(torch_cuda, path, t, 30)[1]
    assert N.find_similar_users(path, 0.001, target="26") == []
    with pytest.raises(KeyError):
        N.find_similar_users(path, 0.1, target="99999990")
    # a KeyedVectors gives what its file gives (vocabulary order = file order)
    from n2v_hip.word2vec import LabelKeyedVectors
    from n2v_hip import io as nio
    words, vecs = nio.load_word2vec_format(path)
    assert N.find_similar_users(LabelKeyedVectors(words, np.ones(len(words)), vecs), 0.1, target="26") == want


def test_main_ecc_writes_the_similar_users_edgelist(torch_cuda, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "node2vec-by-ecc_amd"))
    import main_ecc
    from n2v_hip import eccsplit, neighbors as N
    rs = np.random.RandomState(6)
    uids = [3, 8, 1, 12, 5, 9, 20, 7, 4, 15]
    rows = [(uids[rs.randint(10)], 100 + rs.randint(8), 1 + rs.randint(5), 1000000 + 86400 * 40 * rs.randint(3)) for _ in range(30)]
    rows = list({(u, i): (u, i, r, t) for u, i, r, t in rows}.values())
    rows += [(u, 100, 3, 1000000) for u in uids if u not in {r[0] for r in rows}]
    csv = str(tmp_path / "ratings.csv")
    with open(csv, "w") as f:
        f.write("user,item,rating,timestamp\n" + "".join("%d,%d,%d,%d\n" % r for r in rows))
    labels = [str(u) for u in uids] + ["9999999%d" % i for i in range(100, 108)]
    emb = str(tmp_path / "ue.emb")
    _write_emb(emb, labels[::-1], rs.normal(size=(len(labels), 8)).astype(np.float32))
    plain, flagged = str(tmp_path / "plain"), str(tmp_path / "flagged")
    base = ["-input", csv, "-split-n", "3"]
    main_ecc.main(main_ecc.parse_args(base + ["-out", plain]))
    split = main_ecc.main(main_ecc.parse_args(base + ["-out", flagged, "-prefix", "p_", "-similar-emb", emb, "-similar-ratio", "0.4",
                                                      "-similar-target", "12"]))
    similar = N.find_similar_users(emb, 0.4, target="12")
    assert len(similar) == 4 and similar[0] == "12"
    keep = np.array([str(u) in similar for u, _, _, _ in rows])
    un = np.array([u for u, _, _, _ in rows])[keep]
    it = np.array([int("9999999%d" % i) for _, i, _, _ in rows])[keep]
    fb = np.array([float(r) for _, _, r, _ in rows])[keep]
    assert open(os.path.join(flagged, "p_cosine_onetenth.edgelist")).read() == eccsplit.edgelist_text(un, it, fb)
    # without the flags nothing changes: the split's own files are the same bytes, and no other file appears
    assert sorted(os.listdir(plain)) == split.file_names() and "cosine_onetenth.edgelist" not in os.listdir(plain)
    assert sorted(os.listdir(flagged)) == sorted(["p_" + f for f in split.file_names()] + ["p_cosine_onetenth.edgelist"])
    for f in split.file_names():
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(flagged, "p_" + f), "rb").read(), f
