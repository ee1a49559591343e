"""CPU half of the BiNE preparation-kernel tests: what tests/test_gpu_bine_prep.py relies on is shown here first.

  * every launch of tests/bine_prep_cases.py is replayed with each index asserted inside the array that is passed, and
    the replays of the integer kernels (written after the kernels' text) give what oracle/bine_oracle.py gives;
  * every branch a case exists for is counted as taken in that case;
  * every planted error of tests/bine_prep_reference.py / oracle/bine_oracle.py changes some output bit of some case,
    so the bit comparison on the GPU would notice it."""
import types

import numpy as np
import pytest

import bine_prep_cases as K
import bine_prep_reference as P
from oracle import bine_oracle as bo


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------ bounds replay
@pytest.mark.parametrize("name", K.HITS_CASES)
def test_hits_launches_stay_in_bounds(name):
    L = K.spmv_launch(name)
    P.replay_spmv(L["n_rows"], L["row_ptr"], L["col"], L["w"], L["x"], L["y"])
    N = K.normalise_launch(name)
    P.replay_normalise(N["n"], N["h"], N["a"], N["h_last"], N["state"])
    n = L["n_rows"]                                   # the engine path: vectors of n elements on the same CSR
    P.replay_spmv(n, L["row_ptr"], L["col"], L["w"], np.zeros(n), np.zeros(n))
    assert L["col"].min() >= 0 and L["col"].max() < n and (np.diff(L["row_ptr"]) >= 0).all()


@pytest.mark.parametrize("n", K.NORMALISE_SIZES)
def test_normalise_launches_stay_in_bounds(n):
    N = K.normalise_launch(n)
    P.replay_normalise(N["n"], N["h"], N["a"], N["h_last"], N["state"])


@pytest.mark.parametrize("c", K.COUNTS_CASES, ids=K.counts_id)
def test_counts_launches_stay_in_bounds(c):
    L = K.counts_launch(c)
    assert 0 <= L["lo"] < L["hi"] and L["maxT"] >= 0 and L["minT"] >= 0
    P.replay_walk_counts(L["a"], L["lo"], L["hi"], L["counts"], L["auth_out"])


@pytest.mark.parametrize("c", K.WALK_CASES, ids=K.walk_id)
def test_walk_launches_stay_in_bounds_and_replay_equals_the_oracle(c):
    node, lens, off, want, _ = K.walk_expected(c)
    launches, tokens = K.walk_launches(c)
    assert sum(L["n_walks"] for L in launches) == len(node) and len(tokens) == off[-1]
    trips = 0
    for L in launches:
        assert L["n_walks"] > 0 and L["gw_base"] >= 0 and L["max_len"] >= 1 and L["percentage"] >= 0.0
        P.replay_walk_lengths(L["row_ptr"], L["cum2"], L["walk_node"], L["n_walks"], L["lens"])
        # walk_off holds the oracle's lengths for exactly these walks, and only a live start has more than one token
        b = L["first"]
        assert np.array_equal(np.diff(L["walk_off"]), lens[b:b + L["n_walks"]])
        rp, c2 = L["row_ptr"], L["cum2"]
        v = L["walk_node"].astype(np.int64)
        live = (c2[rp[v + 1]] - c2[rp[v]]) - (rp[v + 1] - rp[v]) > 0
        assert (np.diff(L["walk_off"])[~live] == 1).all() and (np.diff(L["walk_off"]) >= 1).all()
        trips += P.replay_walk(rp, L["col"], c2, L["walk_node"], L["walk_off"], L["n_walks"], L["gw_base"], L["seed"],
                               tokens)
    assert np.array_equal(tokens, want)
    assert (trips > 0) == (len(node) > 4 * 8192)


@pytest.mark.parametrize("c", K.POOL_CASES, ids=K.pool_id)
def test_pool_launches_stay_in_bounds_and_replay_equals_the_oracle(c):
    L = K.pool_launch(c)
    assert L["side_hi"] < 2**31
    P.replay_neg_pools(L["row_ptr"], L["col"], L["side_lo"], L["side_hi"], L["v_begin"], L["v_end"], L["pool_size"],
                       L["max_jaccard"], L["seed"], L["pool"])
    want, _ = K.pool_expected(c)
    assert np.array_equal(L["pool"].reshape(want.shape), want)
    inside = (want >= L["side_lo"]) & (want < L["side_hi"]) & (want != np.arange(L["v_begin"], L["v_end"])[:, None])
    assert (inside | (want == -1)).all() and ((want == -1).any() == (L["side_hi"] - L["side_lo"] == 1))


@pytest.mark.parametrize("c", K.INIT_CASES, ids=str)
def test_init_launches_stay_in_bounds(c):
    L = K.init_launch(c)
    P.replay_init(L["emb"], L["ctx"], L["n"], L["dim"], L["row_stride"])


@pytest.mark.parametrize("c", [c for c in K.ENGINE_CASES if c["walks"]], ids=lambda c: c["graph"])
def test_engine_walks_stay_in_bounds(c):
    """BineEngine.generate_walks launches each side with that side's part of walk_node / walk_off and all of tokens."""
    g, c2 = K.graph(c["graph"]), K.cum2(c["graph"])
    want = K.engine_expected(c)
    nw_u, nw_v = want["n_walks"]
    assert 0 < nw_u and 0 < nw_v and nw_u + nw_v < 1000
    tokens = np.full(len(want["tokens"]), K.FILL_I, np.int32)
    from n2v_hip import bine
    for base, cnt, k in ((0, nw_u, bine.SEED_WALK_U), (nw_u, nw_v, bine.SEED_WALK_V)):
        P.replay_walk_lengths(g.row_ptr, c2, want["node"][base:], cnt, np.zeros(len(want["node"]) - base, np.int32))
        P.replay_walk(g.row_ptr, g.col, c2, want["node"][base:], want["off"][base:], cnt, 0,
                      bine.derive_seed(c["seed"], k), tokens)
    assert np.array_equal(tokens, want["tokens"])


# ------------------------------------------------------------------------------------------ branches
def _walk_case(**kw):
    found = [c for c in K.WALK_CASES if all(c[k] == v for k, v in kw.items())]
    assert found, kw
    return found[0]


def test_walk_cases_take_the_branches_they_exist_for():
    stats = K.walk_expected(_walk_case(graph="skew", side="v", halves=False))[4]
    for k in ("retry_self", "rejected", "swap", "no_swap", "second_round", "early_exit"):
        assert stats.get(k, 0) > 0, (k, stats)
    assert stats.get("clamp", 0) == 0                   # unreachable (bine_prep_cases.py)
    halves = _walk_case(graph="skew", side="v", halves=True)
    assert K.walk_launches(halves)[0][1]["gw_base"] > 0 and K.walk_expected(halves)[4]["second_round"] > 0
    assert K.walk_expected(_walk_case(graph="pair", side="u"))[4]["retry_self"] > 0
    # lengths: the cap reached, percentage 0 / >= 1, max_len 1, dead-end starts on a live graph
    node, lens, _, _, _ = K.walk_expected(_walk_case(percentage=0.0, max_len=5))
    assert (lens == 5).all()
    for kw in (dict(percentage=1.0), dict(percentage=3.5), dict(max_len=1)):
        assert (K.walk_expected(_walk_case(**kw))[1] == 1).all()
    assert K.walk_expected(_walk_case(graph="skew", side="u", reps=2))[1].max() > 10
    node, lens, _, _, _ = K.walk_expected(_walk_case(graph="deadend", side="u", reps=3))
    assert (lens[node >= 15] == 1).all() and lens[node < 15].max() > 3
    assert (K.walk_expected(_walk_case(graph="pair", side="v"))[1] == 1).all()      # one item: a dead end
    assert len(K.walk_expected(_walk_case(reps=1700))[0]) > 4 * 8192                # grid-stride second trip


def _pool_case(**kw):
    found = [c for c in K.POOL_CASES if all(c[k] == v for k, v in kw.items())]
    assert found, kw
    return found[0]


def test_pool_cases_take_the_branches_they_exist_for():
    stats = K.pool_expected(_pool_case(graph="dense", side="u"))[1]
    assert stats["give_up"] > 0 and stats["fallback"] > 0 and stats["fallback_wrap"] > 0
    assert stats["fallback"] > stats["fallback_wrap"]                               # both arms of the fallback
    assert K.pool_expected(_pool_case(graph="skew", side="v"))[1]["swap"] > 0
    assert K.pool_expected(_pool_case(graph="skew", side="u", rows=None))[1]["no_swap"] > 0
    for g, side, n_side in (("single_user", "u", 1), ("pair", "v", 1), ("pair", "u", 2), ("single_user", "v", 3)):
        c = _pool_case(graph=g, side=side)
        lo, hi, _, _ = K.pool_rows(c)
        assert hi - lo == n_side
        assert (K.pool_expected(c)[1].get("no_negative", 0) > 0) == (n_side == 1)
    assert {c["pool_size"] for c in K.POOL_CASES} >= {1, 24, 64, 65, 130}
    assert {c["max_jaccard"] for c in K.POOL_CASES} >= {0.0, 0.1, 1.0}
    sliced = [K.pool_rows(c) for c in K.POOL_CASES if c["rows"]]
    assert sliced and all(lo < vb and ve < hi for lo, hi, vb, ve in sliced)


def test_a_side_of_one_vertex_has_no_negative_and_trains_without_one():
    c = _pool_case(graph="single_user", side="u")
    row = K.pool_expected(c)[0][0]
    assert (row == -1).all() and bo.pool_valid(row) == 0
    tokens = np.array([0, 0, 0], np.int32)
    _, negs = bo.occurrence_context(1, 0, tokens, np.zeros(3, np.int64), np.array([0, 3]), row, 2, 4, seed_neg=5)
    assert negs == []


def test_hits_and_counts_cases_reach_their_edges():
    n = [len(K.hits_csr(name)[0]) - 1 for name in K.HITS_CASES]
    assert n[0] == 2130 and 2100 > 2 * 1024 and n[1] % 4 != 0
    g = K.graph("wide")
    assert (g.n_u, g.n_v) == (2100, 30) and (np.diff(g.row_ptr)[:2100] == 2).all()
    deg = np.diff(K.graph("rows").row_ptr)
    assert {1, 63, 64, 65, 130} <= set(deg.tolist())
    rp, col, w = K.hits_csr("skew+users")
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    g = K.graph("skew")
    assert ((rows == 3) & (col == 3)).sum() == 1 and w[(rows == 3) & (col == 3)][0] == 0.25     # self loop, last weight
    assert w[(rows == 4) & (col == 9)][0] == 0.75 and w[(rows == 9) & (col == 4)][0] == 0.75    # repeated pair
    assert len(col) > len(g.col) and all((np.diff(col[rp[r]:rp[r + 1]]) > 0).all() for r in range(len(rp) - 1))
    for c in K.COUNTS_CASES:                     # the eighths sit on the ceil boundary: maxT * s is an integer
        if c["kind"].startswith("eighths"):
            L = K.counts_launch(c)
            _, s = P.walk_counts(L["a"], L["lo"], L["hi"], L["maxT"], L["minT"])
            assert np.array_equal(L["maxT"] * s, np.round(L["maxT"] * s)) and s.min() == 0.0 and s.max() == 1.0
    assert {c["m"] for c in K.COUNTS_CASES if c["lo"] > 0} >= {1, 1023, 1024, 1025, 2049}


def test_restatements_agree_with_the_oracles_other_order_closely():
    """The kernel-order restatements are the old oracle's values up to summation order (not a GPU tolerance)."""
    for name in K.HITS_CASES:
        a, iters = K.hits_expected(name)
        a0, iters0 = bo.hits_nx111(*K.hits_csr(name))
        assert iters == iters0 and np.allclose(a, a0, rtol=1e-12, atol=1e-15)
    e0, c0 = bo.init_rows(3, 100, K.INIT_SEED)
    e, c = K.init_expected((3, 100))
    assert np.allclose(e[:, :100], e0, rtol=1e-14) and np.allclose(c[:, :100], c0, rtol=1e-14)
    assert (e[:, 100:] == 0).all() and e.shape == (3, 128)
    L = K.counts_launch(K.COUNTS_CASES[9])
    cnt, s = P.walk_counts(L["a"], L["lo"], L["hi"], L["maxT"], L["minT"])
    cnt0, s0 = bo.walk_counts(L["a"], L["lo"], L["hi"], L["maxT"], L["minT"])
    assert np.array_equal(cnt, cnt0) and np.array_equal(bits(s), bits(s0))


# ------------------------------------------------------------------------------------------ planted errors
def _differs(a, b):
    return not np.array_equal(bits(a), bits(b))


def test_planted_float_errors_change_output_bits():
    # spmv: plain left-to-right sum
    assert any(_differs(P.spmv(*K.hits_csr(n), K.hits_vectors(n)[0]),
                        P.spmv(*K.hits_csr(n), K.hits_vectors(n)[0], variant="plain_sum")) for n in K.HITS_CASES)
    # normalise: division instead of multiplication by the reciprocal
    assert any(_differs(P.hits_normalise(*K.normalise_vectors(n))[0],
                        P.hits_normalise(*K.normalise_vectors(n), variant="divide")[0]) for n in K.NORMALISE_SIZES)
    assert _differs(K.hits_expected("wide")[0], P.hits(*K.hits_csr("wide"), variant="plain_sum")[0])
    # walk counts
    def counts(c, variant=None):
        L = K.counts_launch(c)
        return P.walk_counts(L["a"], L["lo"], L["hi"], L["maxT"], L["minT"], variant)
    for variant in ("inf_starts", "floor1"):
        assert any(not np.array_equal(counts(c)[0], counts(c, variant)[0]) for c in K.COUNTS_CASES), variant
        assert any(_differs(counts(c)[1], counts(c, variant)[1]) for c in K.COUNTS_CASES) == (variant == "inf_starts")
    # init
    for variant in ("swap_words", "norm_dim", "plain_sum"):
        hit = [c for c in K.INIT_CASES
               if _differs(K.init_expected(c)[0], P.init_tables(
                   P.init_uniforms(c[0], c[1], K.INIT_SEED, "swap_words") if variant == "swap_words"
                   else K.init_uniforms(c[1])[:, :c[0]], K.init_stride(c), variant)[0])]
        assert hit, variant


def test_planted_integer_errors_change_a_walk_or_a_pool_row():
    c = _walk_case(graph="skew", side="v", halves=False)
    g, c2 = K.graph("skew"), K.cum2("skew")
    node, lens, off, tokens, _ = K.walk_expected(c)
    for variant in ("keep_all", "entry_left"):
        got = np.concatenate([bo.device_walk(g.row_ptr, g.col, c2, int(v), i, int(lens[i]), c["seed"], None, variant)
                              for i, v in enumerate(node)])
        assert not np.array_equal(got, tokens), variant
    for variant, kw in (("no_wrap", dict(graph="dense", side="u")), ("no_wrap", dict(graph="single_user", side="u")),
                        ("early_give_up", dict(graph="dense", side="u"))):
        c = _pool_case(**kw)
        g = K.graph(c["graph"])
        lo, hi, vb, ve = K.pool_rows(c)
        got = [bo.neg_pool(g.row_ptr, g.col, lo, hi, v, c["pool_size"], c["max_jaccard"], c["seed"], None, variant)
               for v in range(vb, ve)]
        assert not np.array_equal(np.array(got), K.pool_expected(c)[0]), (variant, kw)


# ------------------------------------------------------------------------------------------ host-side refusals
def test_centrality_of_a_graph_without_ratings_is_a_value_error():
    from n2v_hip import bine
    g = bine.BipartiteGraph([], [], [])
    assert g.n == 0 and g.n_ratings == 0
    with pytest.raises(ValueError, match="no ratings"):
        bine.BineEngine.calculate_centrality(types.SimpleNamespace(g=g))


def test_user_edges_csr_is_what_add_user_edges_uploads():
    from n2v_hip import bine
    g = K.graph("deadend")
    rp, col, w, pairs = bine.user_edges_csr(g, [0, 3, 3, 2], [5, 3, 3, 7], [0.5, 2.0, 0.25, 1.0])
    assert pairs == 3 and rp[-1] == len(g.col) + 5 and col.dtype == np.int32 and rp.dtype == np.int64
    dense = np.zeros((g.n, g.n))
    dense[np.repeat(np.arange(g.n), np.diff(rp)), col] = w
    assert np.array_equal(dense, dense.T) and dense[3, 3] == 0.25 and dense[0, 5] == 0.5 and dense[7, 2] == 1.0
