"""CPU tests of the centred k-NN predictors (KNNWithMeans, KNNWithZScore, KNNBaseline): the restatement
tests/knn_centered_reference.py against estimates worked out by hand on a 4 x 5 toy, proof that the hand-made table sees
each of the restatement's deliberate errors, the constructors, the -algo flags of main_rec.py, the "no CPU fallback"
errors and the three new C-ABI symbols.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import eccknn_reference as E
import knn_centered_reference as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

# ---- the toy: 4 users x 5 items, 10 ratings in training order, global mean 3 ---------------------------------------------
#   u0: i0 = 1, i1 = 5           mean 3, sigma 2
#   u1: i0 = 2, i2 = 4           mean 3, sigma 1
#   u2: i0 = 3, i1 = 3           mean 3, sigma 0 -> the overall sigma sqrt(26 / 10)
#   u3: i1 = 1, i2 = 5, i3 = 5, i4 = 1      mean 3, sigma 2
U = [0, 0, 1, 1, 2, 2, 3, 3, 3, 3]
I = [0, 1, 0, 2, 0, 1, 1, 2, 3, 4]
R = [1.0, 5.0, 2.0, 4.0, 3.0, 3.0, 1.0, 5.0, 5.0, 1.0]
R0 = [r - 3.0 for r in R]
GM = 3.0
OVERALL = math.sqrt(26.0 / 10.0)
SIM_U = np.array([[1.0, 0.5, 0.25, -0.5],                         # chosen, not computed: a non-positive one and a zero
                  [0.5, 1.0, 0.0, 0.5],
                  [0.25, 0.0, 1.0, 0.25],
                  [-0.5, 0.5, 0.25, 1.0]])
SIM_I = np.full((5, 5), 0.5) + 0.5 * np.eye(5)                    # item-based: every pair 0.5
BU = np.array([0.7, 0.7, -0.3, 0.2])                              # chosen so that the order of the additions shows
BI = np.array([0.3, -0.1, 0.1, 0.0, -0.2])


def toy(mode, user_based=True, ratings=R, mutant=None):
    x, y = (U, I) if user_based else (I, U)
    n_x, n_y = (4, 5) if user_based else (5, 4)
    gm = E.global_mean(ratings)
    tab = C.tables(mode, x, y, ratings, n_x, n_y, user_based, gm, BU, BI, mutant)
    return tab, (SIM_U if user_based else SIM_I), E.build_yr(x, y, ratings)


# (mode, user_based, ratings, x, y, k, min_k) -> (est, actual_k, impossible), every number worked out by hand
d_u1 = 4.0 - ((3.0 + 0.7) + 0.1)                                  # u1's rating of i2 against its baseline
d_i0, d_i1 = 1.0 - ((3.0 + 0.3) + 0.7), 5.0 - ((3.0 + -0.1) + 0.7)   # u0's ratings of i0, i1 against theirs (item-based)
CASES = [
    # means: i2 was rated by u1 (sim 0.5, r 4) and u3 (sim -0.5): one neighbour, 0.5 * (4 - 3) / 0.5
    (("means", True, R, 0, 2, 2, 1), (3.0 + 1.0, 1, 0)),
    # the same with min_k 2: 0 < actual_k < min_k zeroes the sum and is NOT impossible
    (("means", True, R, 0, 2, 2, 2), (3.0, 1, 0)),
    # i4 was rated by u3 alone, sim -0.5: actual_k 0, the mean alone
    (("means", True, R, 0, 4, 2, 1), (3.0, 0, 0)),
    # i1: u0 (0.5, r 5), u2 (0.0), u3 (0.5, r 1); k 1 keeps u0 (the tie goes to the earlier rater), k 2 both
    (("means", True, R, 1, 1, 1, 1), (3.0 + (0.5 * 2.0) / 0.5, 1, 0)),
    (("means", True, R, 1, 1, 2, 1), (3.0 + (1.0 + -1.0) / 1.0, 2, 0)),
    (("means", True, R, -1, 2, 2, 1), (0.0, 0, 1)),
    (("means", True, R, 0, 5, 2, 1), (0.0, 0, 1)),
    (("means", True, R, -1, -1, 2, 1), (0.0, 0, 1)),
    # z-score: u2's sigma is 0 and becomes the overall one; i2: u1 (sim 0), u3 (0.25, r 5, sigma 2)
    (("zscore", True, R, 2, 2, 2, 1), (3.0 + ((0.25 * ((5.0 - 3.0) / 2.0)) / 0.25) * OVERALL, 1, 0)),
    # i0: u0 (0.25, r 1, sigma 2), u1 (0), u2 itself (1.0, r 3, the overall sigma): the quotient first, then sigma
    (("zscore", True, R, 2, 0, 3, 1), (3.0 + ((1.0 * ((3.0 - 3.0) / OVERALL) + 0.25 * ((1.0 - 3.0) / 2.0)) / 1.25) * OVERALL, 2, 0)),
    # the same on the ratings minus 3 (every mean 0, the sigmas unchanged): nothing hides the order of / and *
    (("zscore", True, R0, 2, 0, 3, 1), (0.0 + ((1.0 * ((0.0 - 0.0) / OVERALL) + 0.25 * ((-2.0 - 0.0) / 2.0)) / 1.25) * OVERALL, 2, 0)),
    (("zscore", True, R, 0, 2, 2, 2), (3.0 + (0.0 / 0.5) * 2.0, 1, 0)),
    (("zscore", True, R, 0, 4, 2, 1), (3.0, 0, 0)),
    (("zscore", True, R, 4, 0, 2, 1), (0.0, 0, 1)),
    # every rating equal: every sigma and the overall one are 0, (3 - 3) / 0 is NaN and stays
    (("zscore", True, [3.0] * 10, 0, 2, 2, 1), (NAN, 1, 0)),
    (("zscore", True, [3.0] * 10, 0, 4, 2, 1), (3.0, 0, 0)),
    (("means", True, [3.0] * 10, 0, 2, 2, 1), (3.0, 1, 0)),
    # baseline, user-based: (gm + bu[u0]) + bi[i2], the neighbour u1 against (gm + bu[u1]) + bi[i2]
    (("baseline", True, R, 0, 2, 2, 1), (((3.0 + 0.7) + 0.1) + (0.5 * d_u1) / 0.5, 1, 0)),
    (("baseline", True, R, 0, 2, 2, 2), (((3.0 + 0.7) + 0.1) + 0.0 / 0.5, 1, 0)),
    (("baseline", True, R, 0, 4, 2, 1), ((3.0 + 0.7) + -0.2, 0, 0)),
    (("baseline", True, R, -1, 2, 2, 1), (3.0 + 0.1, 0, 0)),      # unknown user: gm + bi
    (("baseline", True, R, 0, -1, 2, 1), (3.0 + 0.7, 0, 0)),      # unknown item: gm + bu
    (("baseline", True, R, 4, 5, 2, 1), (3.0, 0, 0)),             # both
    # baseline, item-based: x = i2, y = u0, whose list is (i0, 1), (i1, 5); the user's bias still comes first
    (("baseline", False, R, 2, 0, 2, 1), (((3.0 + 0.7) + 0.1) + (0.5 * d_i0 + 0.5 * d_i1) / 1.0, 2, 0)),
    (("baseline", False, R, 2, -1, 2, 1), (3.0 + 0.1, 0, 0)),     # unknown user, x = i2 known
    (("baseline", False, R, 7, 0, 2, 1), (3.0 + 0.7, 0, 0)),      # unknown item, y = u0 known
]


def run(case, mutant=None):
    mode, user_based, ratings, x, y, k, min_k = case
    tab, sim, yr = toy(mode, user_based, ratings, mutant)
    return C.estimate(tab, sim, yr, x, y, k, min_k, mutant)


def same(got, want):
    return E.canon(np.array([got[0]])) == E.canon(np.array([want[0]])) and tuple(got[1:]) == tuple(want[1:])


# ---- the restatement ---------------------------------------------------------------------------------------------------

def test_moments_by_hand():
    assert E.global_mean(R) == GM
    mu, sd = C.row_moments(C.x_rows(U, R, 4))
    assert mu.tolist() == [3.0, 3.0, 3.0, 3.0] and sd.tolist() == [2.0, 1.0, 0.0, 2.0]
    assert C.moments(R) == (3.0, OVERALL)
    assert C.row_moments(C.x_rows(U, R, 4), OVERALL)[1].tolist() == [2.0, 1.0, OVERALL, 2.0]
    assert C.row_moments(C.x_rows(U, R, 4), NAN)[1].tolist() == [2.0, 1.0, 0.0, 2.0]       # NaN: no replacement
    mu, sd = C.row_moments([[], [4.0], [0.1, 0.2, 0.3]], 7.0)
    assert np.isnan(mu[0]) and np.isnan(sd[0]) and (mu[1], sd[1]) == (4.0, 7.0)
    m = ((0.0 + 0.1) + 0.2 + 0.3) / 3.0                          # left to right
    assert mu[2] == m and sd[2] == math.sqrt((((0.1 - m) * (0.1 - m) + (0.2 - m) * (0.2 - m)) + (0.3 - m) * (0.3 - m)) / 3.0)
    tab = toy("zscore")[0]
    assert tab["overall_sd"] == OVERALL and tab["sd"].tolist() == [2.0, 1.0, OVERALL, 2.0]
    flat = toy("zscore", ratings=[3.0] * 10)[0]
    assert flat["overall_sd"] == 0.0 and flat["sd"].tolist() == [0.0] * 4


@pytest.mark.parametrize("n", range(len(CASES)), ids=["%d-%s-%s-x%d-y%d-k%d-mink%d" % ((n, c[0][0], "user" if c[0][1] else "item") + c[0][3:])
                                                      for n, c in enumerate(CASES)])
def test_restatement_equals_the_hand_computed_table(n):
    case, want = CASES[n]
    got = run(case)
    assert same(got, want), (case[0], case[3:], got, want)


def test_the_table_covers_what_it_claims():
    got = [(c[0], run(c)) for c, _ in CASES]
    for mode in C.MODES:
        mine = [(c, g) for c, g in got if c == mode]
        assert any(g[1] == 0 and g[2] == 0 for _, g in mine), mode          # actual_k 0, the base alone
    by_case = {c[:2] + c[3:]: w for c, w in CASES}
    assert by_case[("means", True, 0, 2, 2, 2)][1:] == (1, 0)               # 0 < actual_k < min_k
    assert any(math.isnan(g[0]) for _, g in got)                            # the NaN path
    assert sum(g[2] for c, g in got if c != "baseline") == 4 and not any(g[2] for c, g in got if c == "baseline")


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_the_table_catches_every_deliberate_error(mutant):
    changed = [case for case, want in CASES if not same(run(case, mutant), want)]
    assert changed, "no case of the table sees the mutant %s" % mutant
    # and only the mode it belongs to
    mode = {"keep_neighbour_mean": "means", "sigma_before_division": "zscore", "item_bias_first": "baseline",
            "neighbour_biases_first": "baseline", "zero_sigma_kept": "zscore"}.get(mutant)
    assert mode is None or {c[0] for c in changed} == {mode}


def test_estimate_all_and_top_n_of_the_restatement():
    tab, sim, yr = toy("baseline")
    est, ak, imp = C.estimate_all(tab, sim, yr, [0, -1, 0], [2, 2, 4], 2, 1)
    assert est.tolist() == [CASES[17][1][0], 3.0 + 0.1, (3.0 + 0.7) + -0.2] and ak.tolist() == [1, 0, 0] and not imp.any()
    # an unknown owner under the baseline mode: the items ranked by the clipped gm + bi[i], ties by item id
    case = dict(seen=[{0, 1}, {0, 2}, {0, 1}, {1, 2, 3, 4}], n_items=5, mean=GM, scale=(1.0, 3.25))
    ranked = C.rankings(case, tab, sim, yr, [-1, 3], 2, 1)
    assert ranked[0] == [(0, 3.25), (2, 3.1), (3, 3.0), (1, 3.0 + -0.1), (4, 3.0 + -0.2)]
    assert [i for i, _ in ranked[1]] == [0]                                 # u3 rated everything else
    tab, sim, yr = toy("means")
    assert C.rankings(case, tab, sim, yr, [-1], 2, 1)[0] == [(i, 3.0) for i in range(5)]   # impossible: the training mean


# ---- the classes and the flags -------------------------------------------------------------------------------------------

def test_constructors():
    from n2v_hip import eccknn
    assert eccknn.CENTERINGS == {"means": 1, "zscore": 2, "baseline": 3}
    for cls, mode in ((eccknn.KNNWithMeans, "means"), (eccknn.KNNWithZScore, "zscore"), (eccknn.KNNBaseline, "baseline")):
        assert issubclass(cls, eccknn.KNNBasic) and cls.MODE == mode
        for name in eccknn.SIM_NAMES:
            for form in eccknn.FORMS:
                algo = cls(k=7, min_k=2, sim_options={"name": name, "form": form, "user_based": False})
                assert (algo.k, algo.min_k, algo.name, algo.form, algo.shrinkage) == (7, 2, name, form, 100.0)
        assert cls().bsl_options == eccknn.BSL_DEFAULTS and cls(sim_options={"shrinkage": 50}).shrinkage == 50.0
        with pytest.raises(NameError, match="Wrong sim name jaccard"):
            cls(sim_options={"name": "jaccard"})
        with pytest.raises(ValueError, match="sgd"):
            cls(bsl_options={"method": "sgd"})
        with pytest.raises(ValueError, match="k 257 outside"):
            cls(k=257)
        with pytest.raises(ValueError, match="min_k"):
            cls(min_k=0)
        for text in ("surprise", "restated" if cls is not eccknn.KNNBaseline else "unknown owner"):
            assert text in (cls.__doc__ + eccknn._CenteredKNN.__doc__)
    c = eccknn.Centering("means", True, 3.0, None, None, None)
    assert (c.mode, c.user_based, c.global_mean) == ("means", True, 3.0)
    for bad in (None, ("means",), eccknn.Centering("median", True, 3.0, None, None, None), c):
        with pytest.raises(ValueError, match="centering"):
            eccknn._centering_args(bad, 4, 5)                    # a table the mode needs is missing: no launch


def test_no_cpu_fallback(monkeypatch):
    import torch
    from n2v_hip import eccknn
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    c = eccknn.Centering("means", True, 3.0, None, None, None)
    for call in (lambda: eccknn.row_moments(None, None), lambda: eccknn.yr_check(None, 4),
                 lambda: eccknn.estimate_batch_centered(None, None, None, None, 40, 1, c),
                 lambda: eccknn.top_n_centered(None, None, None, 40, 1, (1, 5), 10, c)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    ts = eccknn.Trainset.from_ratings(U, I, R)
    for cls in (eccknn.KNNWithMeans, eccknn.KNNWithZScore, eccknn.KNNBaseline):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls().fit(ts)
    with pytest.raises(ValueError, match="outside"):             # the option checks still come first
        eccknn.top_n_centered(None, None, None, 40, 1, (1, 5), 257, c)


def test_main_rec_flags(capsys):
    import main_rec
    for algo in ("knnmeans", "knnzscore", "knnbaseline"):
        a = main_rec.parse_args(("-input r.csv -algo %s" % algo).split())
        assert (a.algo, a.k, a.mink, a.sim, a.form, a.item_based, a.shrinkage) == (algo, 40, 1, "cosine", "auto", False, 100)
        a = main_rec.parse_args(("-input r.csv -algo %s -sim pearson_baseline -shrinkage 50 -k 20 -mink 3 -weights w.csv "
                                 "-item-based -form sparse -topn 10 -threshold 4 -save-recs o.csv -cv 3" % algo).split())
        assert (a.algo, a.sim, a.shrinkage, a.k, a.mink, a.weights, a.item_based, a.form, a.topn, a.threshold, a.save_recs,
                a.cv) == (algo, "pearson_baseline", 50.0, 20, 3, "w.csv", True, "sparse", 10, 4.0, "o.csv", 3)
        assert main_rec.parse_args(("-input r.csv -algo %s -sim pearson" % algo).split()).sim == "pearson"
        for flag in ("-factors 8", "-epochs 3", "-lr 0.1", "-reg 0.1", "-strata 2", "-unbiased"):
            with pytest.raises(SystemExit):
                main_rec.parse_args(("-input r.csv -algo %s %s" % (algo, flag)).split())
            assert "does not go with -algo %s" % algo in capsys.readouterr().err
        assert algo in main_rec.__doc__
    for bad, msg in (("-algo svd", "not built"), ("-algo bogus", "-algo bogus"), ("-algo eccen -sim pearson", "needs -algo knn"),
                     ("-algo mf -sim pearson", "does not go with")):
        with pytest.raises(SystemExit):
            main_rec.parse_args(["-input", "r.csv"] + bad.split())
        assert msg in capsys.readouterr().err, bad
    assert main_rec.parse_args("-input r.csv -algo knn -sim pearson".split()).algo == "knn"


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported():
    from n2v_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    for macro, v in (("N2V_ECCKNN_CENTER_MEANS", 1), ("N2V_ECCKNN_CENTER_ZSCORE", 2), ("N2V_ECCKNN_CENTER_BASELINE", 3)):
        assert re.search(r"#define %s %d\b" % (macro, v), hdr)
    section = hdr[hdr.index("Centred k-NN"):hdr.index("#define N2V_ECCKNN_CENTER_MEANS")]
    assert "UNPINNED" in section and "tests/knn_centered_reference.py" in section and "UNPINNED" in C.__doc__
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(n2v_[a-z0-9_]+)\s*\(", hdr))
    new = {"n2v_eccknn_row_moments": 8, "n2v_eccknn_estimate_centered": 21, "n2v_eccknn_topn_centered": 28}
    assert set(new) <= declared and set(new) <= set(_lib.SIGNATURES)
    for name, count in new.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(",") + 1 == count, name
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in new)
    # the old entry points keep their argument counts
    assert len(_lib.SIGNATURES["n2v_eccknn_estimate"][1]) == 15 and len(_lib.SIGNATURES["n2v_eccknn_topn"][1]) == 24


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Every call below returns before the first HIP call: no GPU is needed (and none is touched)."""
    from n2v_hip import _lib
    lib = _lib.load()
    one = 8     # a non-NULL "pointer" that is never dereferenced: each call fails its argument checks first

    def est(k=40, min_k=1, n_q=3, n_x=5, centering=1, tx=one, sd=one, by=one, sim=one, out=one):
        return lib.n2v_eccknn_estimate_centered(sim, n_x, one, one, one, 7, one, one, n_q, k, min_k, centering, 1, 3.0, tx, sd,
                                                by, out, one, one, None)

    def top(k=40, min_k=1, n_owners=3, top_n=10, segments=0, centering=3, tx=one, sd=one, by=one, sim=one, items=one):
        return lib.n2v_eccknn_topn_centered(sim, 5, one, one, one, 7, 1, one, one, 4, one, n_owners, k, min_k, 3.0, 1.0, 5.0,
                                            top_n, segments, centering, tx, sd, by, one, one, items, one, None)

    def mom(n_rows=3, n=5, ptr=one, r=one, mu=one, sd=one):
        return lib.n2v_eccknn_row_moments(ptr, r, n_rows, n, NAN, mu, sd, None)

    for call, kw, msg in ((est, dict(k=0), "k 0"), (est, dict(k=257), "k 257"), (est, dict(min_k=0), "min_k"), (est, dict(n_q=0), "n_q"),
                          (est, dict(n_x=0), "n_x"), (est, dict(centering=0), "centering 0"), (est, dict(centering=4), "centering 4"),
                          (est, dict(centering=-1), "centering -1"), (est, dict(tx=None), "tx"), (est, dict(centering=2, sd=None), "sd"),
                          (est, dict(centering=3, by=None), "by"), (est, dict(centering=3, tx=None), "tx"), (est, dict(sim=None), "null"),
                          (est, dict(out=None), "null"),
                          (top, dict(k=257), "k 257"), (top, dict(min_k=0), "min_k"), (top, dict(centering=0), "centering 0"),
                          (top, dict(centering=7), "centering 7"), (top, dict(by=None), "by"), (top, dict(centering=2, sd=None), "sd"),
                          (top, dict(centering=1, tx=None), "tx"), (top, dict(n_owners=0), "n_owners"), (top, dict(top_n=257), "top_n 257"),
                          (top, dict(segments=65), "segments"), (top, dict(sim=None), "null"), (top, dict(items=None), "null"),
                          (mom, dict(n_rows=0), "n_rows"), (mom, dict(n=-1), "n=-1"), (mom, dict(ptr=None), "null"),
                          (mom, dict(r=None), "null"), (mom, dict(mu=None), "null"), (mom, dict(sd=None), "null")):
        assert call(**kw) != 0, kw
        assert msg in lib.n2v_last_error().decode(), (kw, lib.n2v_last_error())
