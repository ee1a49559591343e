"""CPU tests of the KNNBasic baseline: the restatement tests/eccknn_pearson_reference.py against itself and against hand
values, the option checks of n2v_hip.eccknn.KNNBasic, the new flags of main_rec.py and the three new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

import eccknn_reference as E
import eccknn_pearson_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restate(name, form, n_x, yr, min_support, w, seed):
    """One similarity of the restatement; pearson_baseline with seeded baselines, a seeded mean and shrinkage 7.5."""
    fn = (P.LITERAL if form == "literal" else P.NUMPY)[name]
    if name == "pearson":
        return fn(n_x, yr, min_support, w)
    rs = np.random.RandomState(seed)
    n_y = (max(yr) + 1) if yr else 1
    return fn(n_x, yr, min_support, 3.25 + rs.normal(), rs.normal(size=n_x), rs.normal(size=n_y), 7.5, w)


@pytest.mark.parametrize("kind", ["int", "half", "fp64"])
@pytest.mark.parametrize("n_y", [1, 7])
@pytest.mark.parametrize("n_x", [1, 2, 9])
@pytest.mark.parametrize("name", ["pearson", "pearson_baseline"])
def test_numpy_form_equals_the_literal_loops(name, n_x, n_y, kind):
    n = max(1, int(0.6 * n_x * n_y))
    x, y, r, w = E.make_case(100 * n_x + n_y, n_x, n_y, n, kind, zeros=1 if n >= 4 else 0)
    yr = E.build_yr(x, y, r)
    for weights in (None, w, np.ones(n_y)):
        for ms in (1, 3):
            lit = restate(name, "literal", n_x, yr, ms, weights, n_x + n_y)
            fast = restate(name, "numpy", n_x, yr, ms, weights, n_x + n_y)
            assert set(lit) == set(fast) == {"sim", "freq"} | set(P.ACCUMULATORS[name])
            for key in lit:
                assert E.canon(lit[key]) == E.canon(fast[key]), (key, ms)
            assert np.array_equal(np.diag(lit["sim"]), np.ones(n_x))
            assert E.canon(lit["sim"]) == E.canon(lit["sim"].T)
            if weights is not None and (weights == 1.0).all():   # ones are the absent weights, bit for bit
                none = restate(name, "literal", n_x, yr, ms, None, n_x + n_y)
                assert all(E.canon(none[key]) == E.canon(lit[key]) for key in lit)


def test_pearson_hand_values():
    # x0 rates y0..y2 with (1, 2, 3), x1 with (2, 4, 6); x2 shares only y0 with both
    yr = {0: [(0, 1.0), (1, 2.0), (2, 5.0)], 1: [(0, 2.0), (1, 4.0)], 2: [(0, 3.0), (1, 6.0)]}
    for fn in (P.pearson_literal, P.pearson_numpy):
        out = fn(3, yr, 1)
        assert out["freq"][0, 1] == 3 and out["prods"][0, 1] == 28.0 and out["si"][0, 1] == 6.0 and out["sj"][0, 1] == 12.0
        assert out["sqi"][0, 1] == 14.0 and out["sqj"][0, 1] == 56.0
        # num = 3 * 28 - 6 * 12 = 12; denum = sqrt((3 * 14 - 36) * (3 * 56 - 144)) = sqrt(6 * 24) = 12
        assert out["sim"][0, 1] == 1.0 == out["sim"][1, 0]
        assert out["freq"][0, 2] == 1 and out["sim"][0, 2] == 0.0 and out["sim"][1, 2] == 0.0    # one common y: denum 0
        assert fn(3, yr, 4)["sim"][0, 1] == 0.0                   # min_support
        # the mirror swaps the per-side sums
        assert out["si"][1, 0] == 12.0 and out["sj"][1, 0] == 6.0 and out["sqi"][1, 0] == 56.0
    # weights multiply the products only: w = 2 doubles prods and leaves the sums
    out = P.pearson_numpy(3, yr, 1, np.array([2.0, 2.0, 2.0]))
    assert out["prods"][0, 1] == 56.0 and out["sqi"][0, 1] == 14.0


def test_baselines_hand_values():
    # two users rate one item 3 and 5: mean 4
    ur, ir = [[(0, 3.0)], [(0, 5.0)]], [[(0, 3.0), (1, 5.0)]]
    for n_epochs in (1, 10):
        bu, bi = P.baselines_als(ur, ir, 4.0, n_epochs=n_epochs)
        assert bi.tolist() == [0.0] and bu.tolist() == [-0.0625, 0.0625]       # -1 / (15 + 1)
    bu, bi = P.baselines_als(ur, ir, 4.0, n_epochs=0)
    assert bu.tolist() == [0.0, 0.0] and bi.tolist() == [0.0]
    bu, bi = P.baselines_als(ur, ir, 4.0, n_epochs=1, reg_u=1, reg_i=2)
    assert bu.tolist() == [-0.5, 0.5]
    # an empty row: 0.0 / (reg + 0)
    bu, bi = P.baselines_als([[(0, 3.0)], []], [[(0, 3.0)]], 3.0, n_epochs=2)
    assert bu.tolist() == [0.0, 0.0]
    assert P.rows_of([1, 0, 1], [5, 6, 7], [1.0, 2.0, 3.0], 3) == [[(6, 2.0)], [(5, 1.0), (7, 3.0)], []]


def test_pearson_baseline_raises_min_support_to_two():
    yr = {0: [(0, 1.0), (1, 2.0)], 1: [(0, 4.0), (2, 3.0)], 2: [(0, 2.0), (2, 5.0)]}
    bx, by = np.array([0.1, -0.2, 0.3]), np.array([0.0, 0.5, -0.5])
    for fn in (P.pearson_baseline_literal, P.pearson_baseline_numpy):
        out = fn(3, yr, 1, 3.0, bx, by, 100)
        assert out["freq"][0, 1] == 1 and out["sim"][0, 1] == 0.0 and out["prods"][0, 1] != 0.0
        assert out["freq"][0, 2] == 2 and out["sim"][0, 2] != 0.0
        d0, d2 = [4.0 - (3.5 + 0.1), 2.0 - (2.5 + 0.1)], [3.0 - (3.5 + 0.3), 5.0 - (2.5 + 0.3)]
        prods = d0[0] * d2[0] + d0[1] * d2[1]
        want = prods / np.sqrt((d0[0] * d0[0] + d0[1] * d0[1]) * (d2[0] * d2[0] + d2[1] * d2[1])) * (1.0 / (1.0 + 100.0))
        assert out["sim"][0, 2] == want == out["sim"][2, 0]
        assert out["sq_diff_i"][2, 0] == out["sq_diff_j"][0, 2]


def test_knnbasic_options():
    import torch
    from n2v_hip import eccknn
    for name in ("cosine", "msd", "pearson", "pearson_baseline"):
        for form in ("auto", "dense", "sparse"):
            algo = eccknn.KNNBasic(sim_options={"name": name, "form": form})
            assert (algo.name, algo.form, algo.shrinkage) == (name, form, 100.0)
    assert eccknn.KNNBasic(sim_options={"name": "pearson_baseline", "shrinkage": 50}).shrinkage == 50.0
    assert eccknn.KNNBasic().bsl_options == {"method": "als", "n_epochs": 10, "reg_u": 15, "reg_i": 10}
    with pytest.raises(NameError, match=r"Wrong sim name jaccard\. Allowed values are cosine, msd, pearson, pearson_baseline\."):
        eccknn.KNNBasic(sim_options={"name": "jaccard"})
    with pytest.raises(ValueError, match="sgd"):
        eccknn.KNNBasic(sim_options={"name": "pearson_baseline"}, bsl_options={"method": "sgd"})
    with pytest.raises(ValueError, match="reg_u"):
        eccknn.KNNBasic(bsl_options={"reg_u": -1})
    with pytest.raises(ValueError, match="learning_rate"):
        eccknn.KNNBasic(bsl_options={"learning_rate": 0.1})
    with pytest.raises(ValueError, match="bogus"):
        eccknn.KNNBasic(sim_options={"name": "pearson", "form": "bogus"})
    with pytest.raises(ValueError, match="k 0 outside"):
        eccknn.KNNBasic(k=0)
    # EccenKNN still refuses surprise's own names
    with pytest.raises(NameError, match="surprise's own similarity"):
        eccknn.EccenKNN(sim_options={"name": "pearson_baseline"})
    ts = eccknn.Trainset.from_ratings([1, 2, 1], [5, 5, 6], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="weights"):
        eccknn.KNNBasic(sim_options={"name": "pearson"}).fit(ts, np.ones(3))
    if not torch.cuda.is_available():
        for name in ("cosine", "pearson", "pearson_baseline"):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                eccknn.KNNBasic(sim_options={"name": name}).fit(ts)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            eccknn.baselines(ts)
    with pytest.raises(ValueError, match="sgd"):
        eccknn.baselines(ts, {"method": "sgd"})


def test_main_rec_algo_and_shrinkage_flags():
    import main_rec
    a = main_rec.parse_args(["-input", "r.csv"])
    assert (a.algo, a.shrinkage, a.sim) == ("eccen", 100, "cosine")
    a = main_rec.parse_args("-input r.csv -algo knn -sim pearson_baseline -shrinkage 50".split())
    assert (a.algo, a.sim, a.shrinkage) == ("knn", "pearson_baseline", 50.0)
    assert main_rec.parse_args("-input r.csv -algo knn -sim pearson -weights w.csv".split()).weights == "w.csv"
    for bad in ("-input r.csv -algo eccen -sim pearson", "-input r.csv -sim pearson_baseline", "-input r.csv -algo svd",
                "-input r.csv -algo bogus"):
        with pytest.raises(SystemExit):
            main_rec.parse_args(bad.split())


def test_symbols_are_declared_and_bound():
    from n2v_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    for macro, v in (("N2V_ECCKNN_PEARSON", 0), ("N2V_ECCKNN_PEARSON_BASELINE", 1)):
        assert re.search(r"#define %s %d\b" % (macro, v), hdr)
    assert "UNPINNED" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(n2v_[a-z0-9_]+)\s*\(", hdr))
    new = {"n2v_eccknn_baselines", "n2v_eccknn_pearson", "n2v_eccknn_pearson_sparse"}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    # (that each binding has the header's parameters, type by type: tests/test_host_logic.py)
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in new)
    from n2v_hip import eccknn
    assert eccknn._PEARSON_KIND == {"pearson": 0, "pearson_baseline": 1}
