"""GPU tests: the top-N recommendation kernels (csrc/n2v_rec.hip, C-ABI include/n2v_bine.h) against the restatement
tests/rec_reference.py, through the C-ABI unless a test says otherwise.

Exact comparisons only: ranked lists with `==` everywhere.  That is legitimate because tests/test_rec_host.py proves
from the restatement alone that every input here is either exact in fp64 (small integers) or has no two neighbouring
scores among a user's best k + 1 closer than the sum of their forward bounds gamma(d + 2) sum|a||b|, u = 2^-53: no
user is left out.  Scores on real data are held to that bound; the metrics kernel and the averages to fp64 equality.

Parity: unpinned, restated from the text (the reference module does not import on Python 3)."""
import math
import time

import numpy as np
import pytest

import rec_reference as R

pytestmark = pytest.mark.gpu

ISENT = -7
SSENT = -12345.5


def _lib():
    from n2v_hip import _lib as L
    return L


def c_topn(table, dim, u_idx, v_idx, top_n, segments=0, expect_rc=0):
    """n2v_bine_rec_topn on a host table (fp64 [n][stride]); returns (ranked, score) as numpy."""
    import torch
    L = _lib()
    lib = L.load()
    emb = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).cuda()
    du = torch.from_numpy(np.ascontiguousarray(u_idx, dtype=np.int32)).cuda()
    dv = torch.from_numpy(np.ascontiguousarray(v_idx, dtype=np.int32)).cuda()
    n_users, n_items = len(u_idx), len(v_idx)
    S = segments or lib.n2v_bine_rec_segments(n_users, n_items)
    k = max(1, min(n_items, top_n))
    ps = torch.full((max(n_users, 1), max(S, 1), k), SSENT, dtype=torch.float64, device="cuda")
    pp = torch.full((max(n_users, 1), max(S, 1), k), ISENT, dtype=torch.int32, device="cuda")
    ranked = torch.full((max(n_users, 1), k), ISENT, dtype=torch.int32, device="cuda")
    score = torch.full((max(n_users, 1), k), SSENT, dtype=torch.float64, device="cuda")
    rc = lib.n2v_bine_rec_topn(L.ptr(emb), emb.shape[0], dim, emb.shape[1], L.ptr(du), n_users, L.ptr(dv), n_items, top_n,
                               segments, L.ptr(ps), L.ptr(pp), L.ptr(ranked), L.ptr(score), L.stream_ptr(emb.device))
    torch.cuda.synchronize()
    if expect_rc:
        assert rc == expect_rc, rc
        return lib.n2v_last_error().decode()
    L.check(rc)
    return ranked.cpu().numpy(), score.cpu().numpy()


def check_exact(table, dim, u_idx, v_idx, top_n, segments=0, stride=None):
    tab = R.padded(table[:, :dim], stride or dim)
    want_r, want_s = R.ranked_lists(R.scores(table, dim, u_idx, v_idx), top_n)
    got_r, got_s = c_topn(tab, dim, u_idx, v_idx, top_n, segments)
    assert got_r.shape == want_r.shape and got_r.dtype == np.int32
    assert np.array_equal(got_r, want_r), np.nonzero((got_r != want_r).any(axis=1))[0][:10]
    assert np.array_equal(got_s, want_s)
    return got_r, got_s


# ================================================================================================ 1. integer operands
def test_integer_operands_exact():
    """Every product exact: pins the f64 lane / register map, the k-loop, the edge guards and the tie rule at once."""
    table, u_idx, v_idx = R.integer_case()
    check_exact(table, 64, u_idx, v_idx, 10)


@pytest.mark.parametrize("d", [1, 3, 4, 37, 100, 256, 512])
def test_integer_operands_any_dim_with_nan_padding(d):
    table, u_idx, v_idx = R.integer_case(200, 3000, d, seed=9)
    stride = d + 1 if d in (1, 37) else -(-d // 64) * 64 + (64 if d % 64 == 0 else 0)
    check_exact(table, d, u_idx, v_idx, 10, stride=stride)          # columns [d, stride) hold NaN


# ================================================================================================ 2. real data
@pytest.mark.parametrize("case", range(len(R.REAL_CASES)))
def test_real_data_lists_identical_scores_within_bound(case):
    users, items, d, top_n = R.REAL_CASES[case]
    table, u_idx, v_idx = R.real_case(users, items, d, R.REAL_SEEDS[case])
    S = R.scores(table, d, u_idx, v_idx)
    B = R.score_bound(table, d, u_idx, v_idx)
    assert R.ambiguous_users(S, B, top_n)[0] == []                  # the condition, on this very input
    want_r, want_s = R.ranked_lists(S, top_n)
    got_r, got_s = c_topn(R.padded(table, -(-d // 64) * 64 + 64), d, u_idx, v_idx, top_n)
    assert np.array_equal(got_r, want_r)                            # every user, none left out
    bound = np.take_along_axis(B, want_r.astype(np.int64), axis=1)
    err = np.abs(got_s - want_s)
    print("case %s: largest error / bound %.3f" % (R.REAL_CASES[case], (err[bound > 0] / bound[bound > 0]).max()))
    assert np.all(err <= bound)


# ================================================================================================ 3. unknowns
def test_unknown_vertices_score_zero_and_ties_follow_the_list():
    rs = np.random.RandomState(5)
    n_u, n_v, d = 70, 300, 20
    table = rs.normal(size=(n_u + n_v, d))
    table[3] = np.nan                                               # a known user with NaN scores
    table[n_u + 4] = -0.0                                           # -0.0 / +0.0 scores by the sign of the other end
    table[n_u + 9] = 0.0
    u_idx = np.arange(n_u, dtype=np.int32)
    v_idx = np.arange(n_u, n_u + n_v, dtype=np.int32)
    u_idx[[0, 17, 69]] = -1
    v_idx[[1, 2, 64, 128, 299]] = -1
    tab = R.padded(table, 32)
    S = R.scores(table, d, u_idx, v_idx)
    for top_n in (5, 40):
        want_r, want_s = R.ranked_lists(S, top_n)
        got_r, got_s = c_topn(tab, d, u_idx, v_idx, top_n)
        for u in (0, 17, 69):                                       # all-unknown user: items 0 .. k-1, all exactly 0.0
            assert got_r[u].tolist() == list(range(top_n)) and not got_s[u].any() and not np.signbit(got_s[u]).any()
        # the NaN user: the unknown items (exactly 0.0) first, in list order, then NaN scores in list order
        assert got_r[3].tolist()[:5] == [1, 2, 64, 128, 299]
        if top_n > 5:
            assert got_r[3].tolist()[5:8] == [0, 3, 4] and np.isnan(got_s[3][5:]).all()
        rest = [u for u in range(n_u) if u != 3]
        assert np.array_equal(got_r[rest], want_r[rest])
    # -0.0 versus +0.0 is decided by position: all-positive and all-negative users against rows of +0.0 and of -0.0,
    # whose products are zeros of both signs.  (A sum that starts from +0.0 ends in +0.0 whatever it adds, so on this
    # data the rule is what keeps a change of the accumulation from reordering the zeros.)
    t2 = np.zeros((n_u + n_v, d))
    t2[:n_u] = rs.randint(1, 4, size=(n_u, d))
    t2[1:n_u:2] *= -1
    t2[n_u::3] = rs.randint(-3, 4, size=(len(range(0, n_v, 3)), d))
    t2[n_u + 1::6] = -0.0
    for seg in (0, 1, 3):
        got_r, got_s = check_exact(t2, d, u_idx, v_idx, 30, seg)
        assert (got_s == 0).any()


# ================================================================================================ 4. shapes
@pytest.mark.parametrize("n_users", [1, 127, 128, 129, 257])
@pytest.mark.parametrize("n_items", [1, 7, 63, 64, 65, 129])
def test_shapes_around_tile_and_row_block(n_users, n_items):
    from n2v_hip import recommend as rec
    assert (rec.ROW_BLOCK, rec.ITEM_TILE) == (128, 64)
    table, u_idx, v_idx = R.integer_case(n_users, n_items, 5, seed=n_users + n_items)
    r, _ = check_exact(table, 5, u_idx, v_idx, 10, stride=8)
    assert r.shape == (n_users, min(10, n_items))                   # n_items < top_n: k = n_items


@pytest.mark.parametrize("top_n", [1, 2, 10, 63, 64, 65, 128, 256])
def test_top_n_range(top_n):
    table, u_idx, v_idx = R.integer_case(130, 700, 9, seed=top_n)
    check_exact(table, 9, u_idx, v_idx, top_n, stride=12)


def test_limits_are_errors():
    from n2v_hip import recommend as rec
    import torch
    L = _lib()
    table, u_idx, v_idx = R.integer_case(4, 300, 4)
    msg = c_topn(table, 4, u_idx, v_idx, rec.MAX_TOP_N + 1, expect_rc=-1)
    assert str(rec.MAX_TOP_N) in msg
    assert "top_n" in c_topn(table, 4, u_idx, v_idx, 0, expect_rc=-1)
    assert "nothing to rank" in c_topn(table, 4, u_idx[:0], v_idx, 3, expect_rc=-1)
    assert "nothing to rank" in c_topn(table, 4, u_idx, v_idx[:0], 3, expect_rc=-1)
    assert "segments" in c_topn(table, 4, u_idx, v_idx, 3, segments=65, expect_rc=-1)
    emb = torch.from_numpy(table).cuda()
    with pytest.raises(ValueError, match=str(rec.MAX_TOP_N)):
        rec.top_n_lists(emb, 4, u_idx, v_idx, rec.MAX_TOP_N + 1)
    with pytest.raises(ValueError):
        rec.top_n_lists(emb, 4, u_idx[:0], v_idx, 3)
    assert L.load().n2v_abi_version() == 5


# ================================================================================================ 5. the split
def test_result_does_not_depend_on_the_segments():
    table, u_idx, v_idx = R.integer_case()
    base = check_exact(table, 64, u_idx, v_idx, 10, segments=1)
    users, items, d, top_n = R.REAL_CASES[0]
    rt, ru, rv = R.real_case(users, items, d, 0)
    rbase = c_topn(rt, d, ru, rv, top_n, 1)
    for seg in (2, 3, 7, 64, 0):
        got = c_topn(table, 64, u_idx, v_idx, 10, seg)
        assert np.array_equal(got[0], base[0]) and got[1].tobytes() == base[1].tobytes(), seg
        got = c_topn(rt, d, ru, rv, top_n, seg)
        assert np.array_equal(got[0], rbase[0]) and got[1].tobytes() == rbase[1].tobytes(), seg


def test_tie_group_straddling_a_segment_border():
    """640 items = 10 tiles; with 2 segments the border is item 320, with 5 at 128, 256, 384, 512.  Items 300 .. 339 and
    120 .. 135 tie at the top score; the list must take them in position order across the borders."""
    n_u, n_v = 5, 640
    table = np.zeros((n_u + n_v, 2))
    table[:n_u, 0] = [1, 2, 3, 1, 2]
    table[n_u:, 0] = 1.0
    table[n_u + np.arange(300, 340), 0] = 5.0
    table[n_u + np.arange(120, 136), 0] = 5.0
    table[n_u + 500, 0] = 7.0
    u_idx, v_idx = np.arange(n_u, dtype=np.int32), np.arange(n_u, n_u + n_v, dtype=np.int32)
    want = [500] + list(range(120, 136)) + list(range(300, 340))
    for seg in (1, 2, 5, 10):
        for top_n in (10, 30, 57, 60):
            r, _ = check_exact(table, 2, u_idx, v_idx, top_n, seg)
            assert r[0].tolist() == (want + list(range(0, 60)))[:top_n]


# ================================================================================================ 6. metrics
def c_metrics(ranked, ptr, pos, lens):
    import torch
    from n2v_hip import recommend as rec
    return rec.user_metrics(torch.from_numpy(np.ascontiguousarray(ranked, dtype=np.int32)).cuda(), ptr, pos, lens).cpu().numpy()


def test_metrics_kernel_equals_the_restatement():
    from n2v_hip import recommend as rec
    # hand-made users: no hit; a hit at rank 1 only; truth longer than k; truth items outside the item list; all hits
    ranked = np.array([[5, 6, 7, 8], [9, 1, 2, 3], [0, 1, 2, 3], [4, 9, 2, 7], [3, 2, 1, 0]], dtype=np.int32)
    truth = [[0, 1], [9], [0, 1, 2, 3, 4, 5, 6, 7, 8], [2, 7], [0, 1, 2, 3]]
    lens = np.array([2, 1, 9, 6, 4])                                # user 3: four of its six test items are not listed
    ptr = np.concatenate([[0], np.cumsum([len(t) for t in truth])]).astype(np.int64)
    pos = np.array([p for t in truth for p in t], dtype=np.int32)
    want = R.user_metrics(ranked, ptr, pos, lens)
    got = c_metrics(ranked, ptr, pos, lens)
    assert got.tolist() == want.tolist()
    assert want[0].tolist() == [0, 0, 0, 0, 0] and want[1][3] == 1.0 and want[2][1] == 4 / 9.0
    assert want[3][1] == 2 / 6.0 and want[3][4] == (1 / math.log(4, 2) + 1 / math.log(5, 2)) / R.IDCG(6)
    assert rec.averages(got) == R.averages(want)
    with pytest.raises(ZeroDivisionError):
        c_metrics(ranked, ptr, pos, np.array([2, 1, 0, 6, 4]))
    # random lists, k up to 128, on the lists the device itself produced
    for seed, (n_users, n_items, top_n) in enumerate([(300, 900, 10), (77, 200, 128), (129, 40, 100), (10, 5000, 1)]):
        table, u_idx, v_idx = R.integer_case(n_users, n_items, 8, seed=seed)
        r, _ = c_topn(table, 8, u_idx, v_idx, top_n)
        ptr, pos, lens = R.random_truth(n_users, n_items, seed, max_len=40)
        want = R.user_metrics(r, ptr, pos, lens)
        got = c_metrics(r, ptr, pos, lens)
        assert got.tolist() == want.tolist()
        import torch
        f1, m_ap, mrr, ndcg, per_user = rec.evaluate(torch.from_numpy(table).cuda(), 8, u_idx, v_idx, ptr, pos, lens, top_n)
        assert (f1, m_ap, mrr, ndcg) == R.top_N(table, 8, u_idx, v_idx, ptr, pos, lens, top_n)[:4]
        assert per_user.tolist() == want.tolist()


# ================================================================================================ 7. drop-in
def _labelled(seed):
    rs = np.random.RandomState(seed)
    n_u, n_v, d = 60, 150, 16
    emb_u, emb_v = rs.normal(size=(n_u, d)), rs.normal(size=(n_v, d))
    emb_u[[4, 30]] = 0.0
    emb_v[[0, 77, 149]] = 0.0
    nlu = {"u%d" % i: {"embedding_vectors": emb_u[i:i + 1]} for i in range(n_u)}
    nlv = {"i%d" % i: {"embedding_vectors": emb_v[i:i + 1]} for i in range(n_v)}
    test_u = ["u%d" % i for i in rs.permutation(n_u)[:40]] + ["stranger", "u-1"]
    test_v = ["i%d" % i for i in rs.permutation(n_v)[:120]] + ["i-new", "i-other", "i-third"]
    rs.shuffle(test_v)
    test_rate = {u: {str(x): float(rs.randint(1, 6)) for x in list(rs.choice(test_v, rs.randint(1, 8), replace=False)) + ["off-list"]}
                 for u in test_u}
    return nlu, nlv, test_u, test_v, test_rate


def _fit(nlu, nlv, test_u, test_v, top_n):
    """The input condition on dict inputs: stack, bound, no ambiguous user."""
    d = next(iter(nlu.values()))["embedding_vectors"].shape[1]
    A = np.stack([nlu[u]["embedding_vectors"][0] if u in nlu else np.zeros(d) for u in test_u])
    Bm = np.stack([nlv[v]["embedding_vectors"][0] if v in nlv else np.zeros(d) for v in test_v])
    S = A @ Bm.T
    Bd = R.gamma(d + 2) * (np.abs(A) @ np.abs(Bm).T)
    return R.ambiguous_users(S, Bd, top_n)[0] == []


def test_drop_in_top_N_on_dicts_with_unknown_labels():
    import bine_train as bt
    for seed in (0, 1):
        nlu, nlv, test_u, test_v, test_rate = _labelled(seed)
        for top_n in (1, 10, 50):
            assert _fit(nlu, nlv, test_u, test_v, top_n)
            assert bt.top_N(test_u, test_v, test_rate, nlu, nlv, top_n) == R.top_N_literal(test_u, test_v, test_rate, nlu, nlv, top_n)
    with pytest.raises(KeyError):
        bt.top_N(test_u + ["not rated"], test_v, test_rate, nlu, nlv, 10)


def test_drop_in_train_metrics_come_from_the_device_tables(tmp_path):
    import bine_train as bt
    rs = np.random.RandomState(2)
    lines, test_rate = [], {}
    for u in range(90):
        liked = np.unique(np.minimum((60 * rs.random_sample(9) ** 2).astype(np.int64), 59))
        for k, i in enumerate(liked):
            if k == 0 and len(liked) > 3:
                test_rate.setdefault("u%d" % u, {})["i%d" % i] = 5.0
            else:
                lines.append("u%d\ti%d\t%d\n" % (u, i, rs.randint(3, 6)))
    f = tmp_path / "ratings_train.dat"
    f.write_text("".join(lines))
    gul = bt.GraphUtils(str(tmp_path), device="cuda:0", seed=5)
    gul.construct_training_graph(str(f))
    test_rate["u-unseen"] = {"i1": 4.0, "i-unseen": 2.0}
    test_u = list(test_rate)
    test_v = sorted({i for dct in test_rate.values() for i in dct}) + ["i-never"]
    args = bt.default_args(d=24, max_iter=8, maxT=6, model_path=str(tmp_path), test_rates=(test_u, test_v, test_rate), top_n=10)
    node_list_u, _, _ = bt.train(args, gul)
    node_list_v = bt.train.last["node_list_v"]
    assert _fit(node_list_u, node_list_v, test_u, test_v, 10)
    want = R.top_N_literal(test_u, test_v, test_rate, node_list_u, node_list_v, 10)
    assert bt.train.last["metrics"] == want
    assert gul.engine.last_recommend.shape == (len(test_u), 5)
    assert bt.top_N(test_u, test_v, test_rate, node_list_u, node_list_v, 10) == want


# ================================================================================================ 8. no score matrix
def test_large_evaluation_never_holds_the_score_matrix():
    """100 000 users x 400 000 items, d = 128, top 10 (about 10^13 FLOP): the score matrix would take 320 GB; the peak
    allocation rises by less than 1 % of that.  64 users are checked against the restatement.  Runs once."""
    import torch
    from n2v_hip import recommend as rec
    n_u, n_v, d = 100_000, 400_000, 128
    g = torch.Generator(device="cuda").manual_seed(11)
    emb = torch.randn((n_u + n_v, d), dtype=torch.float64, device="cuda", generator=g)
    u_idx = torch.arange(n_u, dtype=torch.int32, device="cuda")
    v_idx = torch.arange(n_u, n_u + n_v, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    t0 = time.time()
    ranked, score = rec.top_n_lists(emb, d, u_idx, v_idx, 10)
    torch.cuda.synchronize()
    dt = time.time() - t0
    rise = torch.cuda.max_memory_allocated() - before
    print("100000 x 400000 x 128: %.2f s, %.1f TFLOP/s fp64, peak allocation +%.1f MB" % (dt, 2.0 * n_u * n_v * d / dt / 1e12, rise / 1e6))
    assert rise < 0.01 * n_u * n_v * 8
    t0 = time.time()
    pick = np.random.RandomState(0).choice(n_u, 64, replace=False)
    table = np.concatenate([emb[torch.from_numpy(pick).cuda()].cpu().numpy(), emb[n_u:].cpu().numpy()])
    S = R.scores(table, d, np.arange(64), np.arange(64, 64 + n_v))
    B = R.score_bound(table, d, np.arange(64), np.arange(64, 64 + n_v))
    got_r, got_s = ranked.cpu().numpy()[pick], score.cpu().numpy()[pick]
    for u in range(64):
        # the restatement's order on the columns that can reach the best 11 (positions stay ascending, so ties keep theirs)
        cols = np.nonzero(S[u] >= np.partition(S[u], -11)[-11])[0]
        s, b = S[u][cols][None, :], B[u][cols][None, :]
        assert R.ambiguous_users(s, b, 10)[0] == []                 # the input condition: no user is left out
        want_r, want_s = R.ranked_lists(s, 10)
        assert got_r[u].tolist() == cols[want_r[0]].tolist()
        assert np.all(np.abs(got_s[u] - want_s[0]) <= b[0][want_r[0]])
    print("spot check of 64 users on the host: %.1f s" % (time.time() - t0))
