"""CPU tests of the top-N path of the rating predictors: the restatement tests/topn_reference.py against a brute force over
the explicit anti-testset, the edges its case table claims (each asserted on the restatement itself), the option checks
of n2v_hip.eccknn / n2v_hip.svd, the -topn flags of main_rec.py and the three new C-ABI symbols.  No GPU."""
import os
import re

import numpy as np
import pytest

import eccknn_reference as E
import svd_reference as SV
import topn_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, MIN_K, N = 40, 1, 10


@pytest.fixture(scope="module")
def case():
    return T.make_case("int")


@pytest.fixture(scope="module")
def restated(case):
    """The user-based cosine model of the case at k = 40, min_k = 1 and at min_k = 3: (sim, yr, rankings, details)."""
    n_x, yr, w = T.side(case, True)
    sim = E.NUMPY["cosine"](n_x, yr, 1, w)["sim"]
    out = {}
    for min_k in T.MIN_KS:
        predict = T.knn_predictor(sim, yr, True, K, min_k, case["mean"], *case["scale"])
        owners = list(range(case["n_users"])) + [-1]
        out[min_k] = (sim, yr, owners, T.rankings(case["seen"], case["n_items"], owners, predict), predict)
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------

def test_restatement_equals_brute_force_over_the_anti_testset(case, restated):
    """algo.test(build_anti_testset()) as ONE list of queries through estimate_all / predict_all, then get_top_n's per-user
    stable sort: the same lists as the per-owner loop."""
    sim, yr, owners, ranked, _ = restated[MIN_K]
    anti = [(u, i) for u in owners for i in T.anti_testset(case["seen"], case["n_items"], u)]
    est, _, imp = E.estimate_all(sim, yr, [u for u, _ in anti], [i for _, i in anti], K, MIN_K)
    pred = E.predict_all(est, imp, case["mean"], *case["scale"])
    top = {u: [] for u in owners}
    for (u, i), p in zip(anti, pred):
        top[u].append((i, float(p)))
    for u in owners:
        top[u].sort(key=lambda x: x[1], reverse=True)
    assert [top[u] for u in owners] == ranked
    for n in (1, N, 256):
        items, score = T.lists(ranked, n)
        assert items.shape == score.shape == (len(owners), n) and items.dtype == np.int32 and score.dtype == np.float64
        for row, u in enumerate(owners):
            m = min(n, len(top[u]))
            assert items[row, :m].tolist() == [i for i, _ in top[u][:m]] and (items[row, m:] == -1).all()
            assert score[row, :m].tolist() == [s for _, s in top[u][:m]] and np.isnan(score[row, m:]).all()


def test_svd_restatement_equals_brute_force(case):
    for biased in (True, False):
        model = T.svd_tables(case, 8)
        predict = T.svd_predictor(model, biased, case["mean"], *case["scale"])
        owners = [0, 7, -1]
        ranked = T.rankings(case["seen"], case["n_items"], owners, predict)
        for u, got in zip(owners, ranked):
            cands = T.anti_testset(case["seen"], case["n_items"], u)
            est, imp = SV.estimate(model, [u] * len(cands), cands, biased)
            pred = E.predict_all(est, imp, case["mean"], *case["scale"])
            want = sorted(zip(cands, pred.tolist()), key=lambda x: x[1], reverse=True)
            assert got == want
            if u == -1 and not biased:                            # 'User and item are unknown.': the training mean
                assert imp.all() and got == [(i, min(case["scale"][1], max(case["scale"][0], case["mean"]))) for i in cands]


# ---- the edges the case table claims -----------------------------------------------------------------------------------

def test_case_has_the_planted_users_and_items(case):
    nu = np.bincount(case["u"], minlength=case["n_users"])
    ni = np.bincount(case["i"], minlength=case["n_items"])
    full, almost = case["users"].index("full"), case["users"].index("almost")
    assert 1400 <= len(case["r"]) <= 1700 and set(case["r"].tolist()) == {1.0, 2.0, 3.0, 4.0, 5.0}
    assert nu[full] == case["n_items"] and nu[almost] == case["n_items"] - 3
    assert ni[case["items"].index("lonely")] == 1
    assert [int(ni[case["items"].index(p)]) for p in ("p64", "p65", "p66")] == [64, 65, 66]
    assert T.anti_testset(case["seen"], case["n_items"], full) == []
    assert len(T.anti_testset(case["seen"], case["n_items"], almost)) == 3 < N
    assert T.anti_testset(case["seen"], case["n_items"], -1) == list(range(case["n_items"]))
    assert case["scale"] == T.INT_SCALE and (case["w_items"] < 0).any() and (case["w_items"] > 1).any()
    real = T.make_case("fp64")
    assert len(set(real["r"].tolist())) == len(real["r"]) and real["scale"] == (real["r"].min(), real["r"].max())


def test_case_has_ties_across_the_cut_and_across_every_segment_border(case, restated):
    _, _, owners, ranked, _ = restated[MIN_K]
    cut = [u for u, lst in zip(owners, ranked) if len(lst) > N and lst[N - 1][1] == lst[N][1]]
    assert cut, "no owner whose N-th and (N+1)-th scores are equal"
    assert any(len(lst) > n and lst[n - 1][1] == lst[n][1] for lst in ranked for n in (1, 64, 65))
    for S in (s for s in T.SEGMENTS if s):
        borders = T.segment_borders(case["n_items"], S)
        assert len(borders) == min(S, case["n_items"]) - 1
        for b in borders:                                         # two equal scores, one candidate on each side of b
            assert any(set(s for i, s in lst if i < b) & set(s for i, s in lst if i >= b) for lst in ranked), (S, b)
    # neighbouring candidates with equal scores right at a border, inside one owner's best N
    hit = 0
    for b in T.segment_borders(case["n_items"], 64):
        for lst in ranked:
            best = dict(lst[:N])
            below, above = [i for i in best if i < b], [i for i in best if i >= b]
            if below and above and best[max(below)] == best[min(above)]:
                hit += 1
                break
    assert hit >= 1


def test_case_has_short_lists_impossible_estimates_and_both_clips(case, restated):
    lo, hi = case["scale"]
    full, almost = case["users"].index("full"), case["users"].index("almost")
    for min_k in T.MIN_KS:
        _, _, owners, ranked, predict = restated[min_k]
        assert ranked[owners.index(full)] == []                   # rated everything: an all-filler row
        assert len(ranked[owners.index(almost)]) == 3
        items, score = T.lists(ranked, N)
        assert (items[owners.index(full)] == -1).all() and np.isnan(score[owners.index(full)]).all()
        assert (items[owners.index(almost)][3:] == -1).all() and (items[owners.index(almost)][:3] >= 0).all()
        # the unknown user: every estimate impossible, items 0 .. N - 1 at the clipped training mean
        mean = min(hi, max(lo, case["mean"]))
        assert ranked[owners.index(-1)] == [(i, mean) for i in range(case["n_items"])]
        kinds = set()
        for u in range(0, case["n_users"], 7):
            for i in T.anti_testset(case["seen"], case["n_items"], u):
                p, est, imp = predict(u, i)
                kinds.add("impossible" if imp else "hi" if est > hi else "lo" if est < lo else "inside")
                assert p == (case["mean"] if imp else min(hi, max(lo, est)))
        assert kinds == {"impossible", "hi", "lo", "inside"}, (min_k, kinds)


# ---- the option checks -------------------------------------------------------------------------------------------------

def test_option_checks_need_no_gpu():
    from n2v_hip import eccknn, svd
    assert eccknn.MAX_TOP_N == 256 and eccknn.MAX_SEGMENTS == 64
    assert eccknn.topn_options(1, None) == (1, 0) and eccknn.topn_options(256, 64) == (256, 64)
    assert eccknn.topn_options(np.int64(10), np.int32(3)) == (10, 3)
    for n, segments in ((0, None), (257, None), (-1, 1), (10, 0), (10, 65), (10, -1), (2.5, None), ("10", None), (True, None),
                        (10, 1.5), (10, True), (None, None)):
        with pytest.raises(ValueError):
            eccknn.topn_options(n, segments)
    assert eccknn.threshold_option(None) is None and eccknn.threshold_option(4) == 4.0 and eccknn.threshold_option(3.5) == 3.5
    for bad in (float("nan"), "4", True, [4]):
        with pytest.raises(ValueError):
            eccknn.threshold_option(bad)
    # the checks come before anything touches a device
    algo = eccknn.EccenKNN(k=5)
    model = svd.SVD(n_factors=4)
    for obj in (algo, model):
        with pytest.raises(ValueError, match="outside"):
            obj.top_n_lists(n=0)
        with pytest.raises(ValueError, match="segments"):
            obj.top_n_lists(n=10, segments=65)
        with pytest.raises(ValueError, match="outside"):
            obj.ranking_metrics([("u", "i", 1.0)], n=300)
        with pytest.raises(ValueError, match="threshold"):
            obj.ranking_metrics([("u", "i", 1.0)], n=10, threshold="high")
    for fn, args in ((eccknn.top_n, (None,) * 8), (svd.top_n, (None,) * 9)):
        with pytest.raises(ValueError, match="outside"):
            fn(*args, n=257)
        with pytest.raises(ValueError, match="segments"):
            fn(*args, n=10, segments=0)


def test_no_cpu_fallback(monkeypatch):
    import torch
    from n2v_hip import eccknn, svd
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eccknn.top_n(None, None, None, True, 40, 1, 3.0, (1, 5), 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        svd.top_n(3.0, True, None, None, None, None, None, 3.0, (1, 5), 10)


# ---- main_rec.py -------------------------------------------------------------------------------------------------------

def test_main_rec_flags(capsys):
    import main_rec
    a = main_rec.parse_args("-input r.csv".split())
    assert (a.topn, a.threshold, a.save_recs) == (None, None, None)
    # without -topn everything else parses as before
    assert (a.algo, a.k, a.mink, a.sim, a.form, a.item_based, a.test_ratio, a.seed, a.cv) == ("eccen", 40, 1, "cosine", "auto",
                                                                                           False, 0.2, 0, 0)
    b = main_rec.parse_args("-input r.csv -topn 10".split())
    assert {k: v for k, v in vars(b).items() if k != "topn"} == {k: v for k, v in vars(a).items() if k != "topn"}
    assert b.topn == 10 and b.threshold is None
    for algo in ("eccen", "knn", "mf"):
        c = main_rec.parse_args(("-input r.csv -algo %s -topn 256 -threshold 3.5 -save-recs out.csv -cv 3" % algo).split())
        assert (c.algo, c.topn, c.threshold, c.save_recs, c.cv) == (algo, 256, 3.5, "out.csv", 3)
    for bad, msg in (("-threshold 4", "needs -topn"), ("-save-recs f.csv", "needs -topn"), ("-topn 0", "outside"),
                     ("-topn 257", "outside"), ("-topn 10 -threshold nan", "threshold"), ("-topn ten", "invalid int"),
                     ("-algo svd -topn 10", "not built")):
        with pytest.raises(SystemExit):
            main_rec.parse_args(["-input", "r.csv"] + bad.split())
        assert msg in capsys.readouterr().err, bad
    for flag in ("-topn", "-threshold", "-save-recs"):
        assert flag in main_rec.__doc__


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_bound():
    from n2v_hip import _lib, eccknn
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    assert re.search(r"#define N2V_TOPN_MAX_N 256\b", hdr)
    assert re.search(r"#define N2V_ABI_VERSION 5\b", open(os.path.join(ROOT, "include", "n2v_hip.h")).read())
    section = hdr[hdr.index("Top-N lists of the rating predictors"):hdr.index("#define N2V_TOPN_MAX_N")]
    assert "UNPINNED" in T.__doc__ and "tests/topn_reference.py" in section and "n2v_rank.h" in section
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(n2v_[a-z0-9_]+)\s*\(", hdr))
    new = {"n2v_topn_segments": 2, "n2v_eccknn_topn": 24, "n2v_svd_topn": 24}
    assert set(new) <= declared and set(new) <= set(_lib.SIGNATURES)
    for name, count in new.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).strip()
        assert len(_lib.SIGNATURES[name][1]) == params.count(",") + 1 == count, name
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in new) and lib.n2v_abi_version() == 5
    # the default segment count: host arithmetic, inside [1, 64] and never above the number of candidates
    seg = lib.n2v_topn_segments
    assert seg(0, 10) == 1 and seg(10, 0) == 1 and seg(1, 1) == 1 and seg(1, 5) == 5 and seg(1, 10 ** 6) == 64 == eccknn.MAX_SEGMENTS
    assert seg(6040, 3706) == 11 and seg(10 ** 6, 3706) == 1 and all(1 <= seg(n, 150) <= 64 for n in (1, 70, 76, 10 ** 4))


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Every call below returns before the first HIP call: no GPU is needed (and none is touched)."""
    from n2v_hip import _lib
    lib = _lib.load()
    one = 8     # a non-NULL "pointer" that is never dereferenced: each call fails its argument checks first

    def knn(n_x=5, n_y=7, k=40, min_k=1, n_owners=3, top_n=10, segments=0, n_seen=4, sim=one, owners=one, items=one, seen_i=one):
        return lib.n2v_eccknn_topn(sim, n_x, one, one, one, n_y, 1, one, seen_i, n_seen, owners, n_owners, k, min_k, 3.0, 1.0,
                                   5.0, top_n, segments, one, one, items, one, None)

    def mf(n_users=5, n_items=7, nf=8, biased=1, bu=one, n_owners=3, top_n=10, segments=0, n_seen=4, pu=one, seen_i=one):
        return lib.n2v_svd_topn(bu, one, pu, one, n_users, n_items, nf, 3.0, biased, one, seen_i, n_seen, one, n_owners, 3.0,
                                1.0, 5.0, top_n, segments, one, one, one, one, None)

    for call, kw, msg in ((knn, dict(k=0), "k 0"), (knn, dict(k=257), "k 257"), (knn, dict(min_k=0), "min_k"),
                          (knn, dict(n_x=0), "n_x"), (knn, dict(n_owners=0), "n_owners"), (knn, dict(n_owners=2 ** 31), "n_owners"),
                          (knn, dict(n_y=2 ** 31 - 1), "n_items"), (knn, dict(top_n=0), "top_n 0"), (knn, dict(top_n=257), "top_n 257"),
                          (knn, dict(segments=-1), "segments"), (knn, dict(segments=65), "segments"), (knn, dict(n_seen=-1), "n_seen"),
                          (knn, dict(sim=None), "null"), (knn, dict(owners=None), "null"), (knn, dict(items=None), "null"),
                          (knn, dict(seen_i=None), "null"),
                          (mf, dict(n_users=0), "n_users"), (mf, dict(nf=0), "n_factors"), (mf, dict(nf=257), "n_factors"),
                          (mf, dict(top_n=257), "top_n"), (mf, dict(segments=65), "segments"), (mf, dict(n_owners=0), "n_owners"),
                          (mf, dict(bu=None), "null"), (mf, dict(pu=None), "null"), (mf, dict(seen_i=None), "null")):
        assert call(**kw) != 0, kw
        assert msg in lib.n2v_last_error().decode(), (kw, lib.n2v_last_error())
