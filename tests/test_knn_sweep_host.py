"""CPU tests of the k-NN sweep: the grid rules (eccknn.sweep_options and the C entry points, which refuse a bad grid
before any launch), the three new C-ABI symbols, main_rec.py's -sweep-k / -sweep-mink / -mae flags, and the restatement
tests/knn_sweep_reference.py itself: the prefix claim the sweep rests on, against heapq.nlargest on crafted lists, and
proof that the crafted case tells the cells of a grid apart.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import eccknn_reference as E
import knn_sweep_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

BAD_GRIDS = (((), (1,), "0 values"), ((1,), (), "0 values"), (tuple(range(1, 18)), (1,), "17 values"),
             ((1,), tuple(range(1, 18)), "17 values"), ((5, 5), (1,), "ascending"), ((10, 5), (1,), "ascending"),
             ((5,), (2, 2), "ascending"), ((5,), (3, 1), "ascending"), ((0, 5), (1,), "k 0"), ((5, 257), (1,), "k 257"),
             ((-3,), (1,), "k -3"), ((5,), (0, 1), "min_k"), ((5,), (-1,), "min_k"))


# ---- the grid rules --------------------------------------------------------------------------------------------------------

def test_sweep_options():
    from n2v_hip import eccknn
    assert eccknn.MAX_SWEEP == 16
    assert eccknn.sweep_options((5, 10, 20, 40, 80), [1, 5]) == ([5, 10, 20, 40, 80], [1, 5])
    assert eccknn.sweep_options(np.array([1, 256]), (300,)) == ([1, 256], [300])          # a min_k above every k is legal
    assert eccknn.sweep_options(range(1, 17), range(2, 18)) == (list(range(1, 17)), list(range(2, 18)))
    assert eccknn.sweep_options([40], [1]) == ([40], [1])
    for ks, min_ks, msg in BAD_GRIDS:
        with pytest.raises(ValueError, match=msg):
            eccknn.sweep_options(ks, min_ks)
    for ks, min_ks in (((5.0,), (1,)), ((5,), (1.5,)), ((True,), (1,)), ("5", (1,)), (5, (1,)), ((5,), None), (None, (1,))):
        with pytest.raises(ValueError):
            eccknn.sweep_options(ks, min_ks)


def test_no_cpu_fallback_and_the_grid_comes_first(monkeypatch):
    import torch
    from n2v_hip import eccknn
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for call in (lambda: eccknn.estimate_sweep(None, None, None, None, (5, 10), (1,)),
                 lambda: eccknn.errors(None, None)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="ascending"):
        eccknn.estimate_sweep(None, None, None, None, (10, 5), (1,))
    for cls in (eccknn.EccenKNN, eccknn.KNNBasic, eccknn.KNNWithMeans, eccknn.KNNWithZScore, eccknn.KNNBaseline):
        assert cls.test_sweep is eccknn._SymmetricKNN.test_sweep and cls.accuracy_sweep is eccknn._SymmetricKNN.accuracy_sweep
        with pytest.raises(ValueError, match="17 values"):
            cls().accuracy_sweep([("u", "i", 3.0)], range(1, 18), (1,))
    from n2v_hip import coclustering, nmf, slopeone, svd
    for cls in (eccknn.KNNBasic, svd.SVD, nmf.NMF, slopeone.SlopeOne, coclustering.CoClustering):
        assert cls.mae is eccknn.Predictor.mae and cls.rmse is eccknn.Predictor.rmse


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported():
    from n2v_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    assert re.search(r"#define N2V_ECCKNN_MAX_SWEEP 16\b", hdr)
    section = hdr[hdr.index("k-NN sweep"):hdr.index("#define N2V_ECCKNN_MAX_SWEEP")]
    for text in ("prefix", "total order", "HOST", "bit for bit", "cell-major"):
        assert text in section, text
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    new = {"n2v_eccknn_estimate_sweep": 17, "n2v_eccknn_estimate_sweep_centered": 23, "n2v_eccknn_errors": 7}
    for name, count in new.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(",") + 1 == count, name
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in new)
    assert lib.n2v_abi_version() == 5
    # the calls the sweep stands beside keep their argument counts
    assert len(_lib.SIGNATURES["n2v_eccknn_estimate"][1]) == 15 and len(_lib.SIGNATURES["n2v_eccknn_estimate_centered"][1]) == 21
    assert len(_lib.SIGNATURES["n2v_eccknn_predict"][1]) == 10


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Every call below returns before the first HIP call: no GPU is needed (and none is touched).  ks and min_ks are real
    host arrays, as the call reads them."""
    from n2v_hip import _lib
    lib = _lib.load()
    one = 8     # a non-NULL "pointer" that is never dereferenced: each call fails its argument checks first

    def arr(values):
        return (ctypes.c_int32 * max(1, len(values)))(*values)

    def sweep(ks=(5, 10), min_ks=(1, 5), n_k=None, n_m=None, n_q=3, n_x=5, sim=one, est=one, ak=one, imp=one, ksp=0, mksp=0):
        return lib.n2v_eccknn_estimate_sweep(sim, n_x, one, one, one, 7, one, one, n_q, arr(ks) if ksp == 0 else ksp,
                                             len(ks) if n_k is None else n_k, arr(min_ks) if mksp == 0 else mksp,
                                             len(min_ks) if n_m is None else n_m, est, ak, imp, None)

    def centred(ks=(5, 10), min_ks=(1, 5), centering=1, tx=one, sd=one, by=one, est=one):
        return lib.n2v_eccknn_estimate_sweep_centered(one, 5, one, one, one, 7, one, one, 3, arr(ks), len(ks), arr(min_ks),
                                                      len(min_ks), centering, 1, 3.0, tx, sd, by, est, one, one, None)

    def errs(n_q=4, n_cols=2, pred=one, r_true=one, rmse=one, mae=one):
        return lib.n2v_eccknn_errors(pred, r_true, n_q, n_cols, rmse, mae, None)

    cases = [(sweep, dict(ks=ks, min_ks=min_ks), msg) for ks, min_ks, msg in BAD_GRIDS if ks and min_ks and len(ks) < 17 and len(min_ks) < 17]
    cases += [(centred, dict(ks=ks, min_ks=min_ks), msg) for ks, min_ks, msg in BAD_GRIDS if ks and min_ks and len(ks) < 17 and len(min_ks) < 17]
    cases += [(sweep, dict(n_k=0), "n_k 0"), (sweep, dict(n_k=17), "n_k 17"), (sweep, dict(n_m=0), "n_m 0"), (sweep, dict(n_m=17), "n_m 17"),
              (sweep, dict(n_k=-1), "n_k -1"), (sweep, dict(ksp=None), "ks"), (sweep, dict(mksp=None), "min_ks"),
              (sweep, dict(n_q=0), "n_q"), (sweep, dict(n_x=0), "n_x"), (sweep, dict(sim=None), "null"), (sweep, dict(est=None), "null"),
              (sweep, dict(ak=None), "null"), (sweep, dict(imp=None), "null"),
              (centred, dict(centering=0), "centering 0"), (centred, dict(centering=4), "centering 4"), (centred, dict(tx=None), "tx"),
              (centred, dict(centering=2, sd=None), "sd"), (centred, dict(centering=3, by=None), "by"), (centred, dict(est=None), "null"),
              (errs, dict(n_q=0), "n_q 0"), (errs, dict(n_cols=0), "n_cols 0"), (errs, dict(n_cols=1 << 31), "n_cols"),
              (errs, dict(pred=None), "null"), (errs, dict(r_true=None), "null"), (errs, dict(rmse=None, mae=None), "null")]
    for call, kw, msg in cases:
        assert call(**kw) != 0, kw
        assert msg in lib.n2v_last_error().decode(), (kw, lib.n2v_last_error())


# ---- main_rec.py ------------------------------------------------------------------------------------------------------------

def test_main_rec_flags(capsys):
    import main_rec
    a = main_rec.parse_args("-input r.csv -k 40 -mink 1".split())
    assert (a.k, a.mink, a.sweep_k, a.sweep_mink, a.mae) == (40, 1, None, None, False) and type(a.k) is int and type(a.mink) is int
    for algo in ("eccen",) + main_rec.KNN_ALGOS:
        a = main_rec.parse_args(("-input r.csv -algo %s -sweep-k 5,10,20,40,80 -sweep-mink 1,5 -cv 3 -mae" % algo).split())
        assert (a.sweep_k, a.sweep_mink, a.cv, a.mae) == ([5, 10, 20, 40, 80], [1, 5], 3, True)
        a = main_rec.parse_args(("-input r.csv -algo %s -mink 3 -sweep-k 7" % algo).split())
        assert (a.sweep_k, a.sweep_mink, a.k, a.mink) == ([7], [3], 40, 3)              # -sweep-mink defaults to the run's -mink
    for algo in ("mf", "nmf", "slopeone", "coclustering"):
        assert main_rec.parse_args(("-input r.csv -algo %s -mae" % algo).split()).mae is True
        with pytest.raises(SystemExit):
            main_rec.parse_args(("-input r.csv -algo %s -sweep-k 5,10" % algo).split())
        assert "-sweep-k does not go with -algo %s" % algo in capsys.readouterr().err
    for bad, msg in (("-sweep-k 5,10 -topn 5", "-sweep-k does not go with -topn"), ("-sweep-mink 1,5", "-sweep-mink needs -sweep-k"),
                     ("-sweep-k 10,5", "ascending"), ("-sweep-k 5,5", "ascending"), ("-sweep-k 0,5", "k 0"), ("-sweep-k 5,257", "k 257"),
                     ("-sweep-k 5 -sweep-mink 0", "min_k"), ("-sweep-k 5 -sweep-mink 2,1", "ascending"), ("-sweep-k five", "-sweep-k"),
                     ("-sweep-k 5,", "-sweep-k"), ("-sweep-k " + ",".join(map(str, range(1, 18))), "17 values")):
        with pytest.raises(SystemExit):
            main_rec.parse_args(["-input", "r.csv"] + bad.split())
        assert msg in capsys.readouterr().err, bad
    for text in ("-sweep-k", "-sweep-mink", "-mae", "best: k K mink M mean RMSE"):
        assert text in main_rec.__doc__


# ---- the restatement: the prefix claim --------------------------------------------------------------------------------------

CRAFTED = {
    "ties": [0.5, 0.25, 0.5, 0.5, 0.25, 0.25, 0.5, 0.75, 0.25, 0.75],
    "zeros": [0.0, -0.0, 0.5, -0.0, 0.0, -0.5, 0.0, -0.0],
    "nan": [NAN, 0.5, NAN, -1.0, NAN, 0.5, 0.0, NAN, -0.0],
    "all-nan": [NAN] * 5,
    "non-positive-between": [0.9, -0.1, 0.8, 0.0, 0.7, -0.0, -2.0, 0.6, NAN, 0.5, -0.1],
    "descending": [1.0, 0.9, 0.8, 0.7], "ascending": [0.1, 0.2, 0.3, 0.4], "one": [0.3], "none": [],
}


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_the_selection_for_k_is_the_head_of_the_stable_descending_sort(name):
    """heapq.nlargest(k) under the restatements' key is the first k of the order the device keeps its list in, for every k:
    so the selection for k is the head of the selection for any larger k.  The third field tells tied entries apart."""
    neighbors = [(s, float(10 + p), p) for p, s in enumerate(CRAFTED[name])]
    order = S.ranked(neighbors)
    assert sorted(t[2] for t in order) == list(range(len(neighbors)))
    real = [t for t in order if t[0] == t[0]]
    assert order[len(real):] == [t for t in neighbors if t[0] != t[0]]                    # NaN last, in list order
    assert all(a[0] > b[0] or (a[0] == b[0] and a[2] < b[2]) for a, b in zip(real, real[1:]))   # -0.0 == 0.0: by position
    for k in range(1, len(neighbors) + 3):
        got = S.selection(neighbors, k)
        assert [t[2] for t in got] == [t[2] for t in order[:k]], k
        for k2 in range(1, k):
            assert S.selection(neighbors, k2) == got[:k2]


def test_the_sums_for_k_are_a_prefix_of_the_sums_for_a_larger_k():
    """The rank-order sums, restated: walking the largest selection and stopping at k gives the single-cell restatement's
    estimate for k, bit for bit, on lists with ties, signed zeros, NaN and non-positive sims between positive ones."""
    rs = np.random.RandomState(1)
    for name, sims in CRAFTED.items():
        n = len(sims)
        sim = np.full((1, max(n, 1)), NAN)
        sim[0, :n] = sims
        yr = {0: [(p, float(r)) for p, r in enumerate(rs.randint(1, 11, n) * 0.5)]} if n else {}
        order = S.ranked([(float(sim[0, x2]), r) for x2, r in yr.get(0, [])])
        for k in range(1, n + 2):
            ss = sr = 0.0
            ak = 0
            for s, r in order[:k]:
                if s > 0:
                    ss, sr, ak = ss + s, sr + s * r, ak + 1
            for min_k in (1, 2, 4):
                est, wak, imp = E.estimate_all(sim, yr, [0], [0], k, min_k)
                assert (int(wak[0]), int(imp[0])) == (ak, int(ak < min_k)), (name, k, min_k)
                assert imp[0] or E.canon(est) == E.canon(np.array([sr / ss])), (name, k, min_k)


# ---- the restatement: the crafted case tells the cells apart ----------------------------------------------------------------

@pytest.fixture(scope="module")
def case():
    return S.make_case()


def test_the_crafted_case_has_what_it_claims(case):
    sim, qx, qy = case["sim"], case["qx"], case["qy"]
    assert np.isnan(sim).any() and (sim < 0).any() and (np.signbit(sim) & (sim == 0)).any() and (~np.signbit(sim) & (sim == 0)).any()
    assert len({v for v in sim[0] if v == v}) == 4 and np.isnan(sim[1]).sum() >= 150 and np.nanmax(sim[2]) > 2
    lens = np.diff(case["ptr"])
    assert tuple(lens) == S.LENGTHS and {0, 1, 63, 64, 65, 129, 300} <= set(lens.tolist())
    assert [len(case["yr"].get(y, [])) for y in range(case["n_y"])] == list(S.LENGTHS)
    assert (qx == -1).sum() == 2 and (qy == -1).sum() == 2 and ((qx == -1) & (qy == -1)).sum() == 1
    assert S.HUGE in case["yr_r"] and -S.HUGE in case["yr_r"]


@pytest.mark.parametrize("mode", [None, "means"])
def test_adjacent_cells_of_the_main_grid_differ(case, mode):
    """A kernel that returned one column for every cell could not pass the GPU tests: by the restatement's own values,
    adjacent ks give at least one different estimate and adjacent min_ks at least one different impossible flag (plain) or
    estimate (centred: too few neighbours is the base alone, never impossible)."""
    ks, min_ks = S.MAIN_GRID
    est, ak, imp = S.estimate_sweep(case["sim"], case["yr"], case["qx"], case["qy"], ks, min_ks, S.tab(case, mode))
    bits = lambda a: [E.canon(row) for row in a]
    for j in range(len(ks) - 1):
        assert any(bits(est[j])[m] != bits(est[j + 1])[m] for m in range(len(min_ks))), ks[j:j + 2]
        assert not np.array_equal(ak[j], ak[j + 1]), ks[j:j + 2]
    for m in range(len(min_ks) - 1):
        if mode is None:
            assert any(not np.array_equal(imp[j, m], imp[j, m + 1]) for j in range(len(ks))), min_ks[m:m + 2]
        else:
            assert not imp[:, :, :-3].any()
            assert any(bits(est[j, m:m + 1]) != bits(est[j, m + 1:m + 2]) for j in range(len(ks))), min_ks[m:m + 2]
    # a NaN estimate comes from inf - inf in sum_ratings alone (row 2 against the planted +-1e308): a NaN similarity is
    # never added and sum_sim is positive wherever there is a quotient
    assert np.isnan(est).any() and np.isinf(est).any()
    assert (ak == 0).any() and (ak[-1] > 128).any()


def test_errors_of_the_restatement():
    r_true = [1.0, 2.0, 4.0]
    rmse, mae = S.errors([[1.0, 4.0, 1.0], [1.0, 2.0, 4.0]], r_true)
    assert rmse.tolist() == [np.sqrt((0.0 + 4.0 + 9.0) / 3.0), 0.0] and mae.tolist() == [(0.0 + 2.0 + 3.0) / 3.0, 0.0]
    assert S.errors([1.0, 4.0, 1.0], r_true)[0][0] == E.rmse(r_true, [1.0, 4.0, 1.0])   # 1-D: one column; eccknn_reference's rmse
    rmse, mae = S.errors([[NAN, 2.0, 4.0]], r_true)
    assert np.isnan(rmse[0]) and np.isnan(mae[0])
