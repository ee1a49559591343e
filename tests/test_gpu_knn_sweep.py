"""GPU tests of the k-NN sweep: n2v_eccknn_estimate_sweep, n2v_eccknn_estimate_sweep_centered and n2v_eccknn_errors, with
eccknn.estimate_sweep / errors, test_sweep / accuracy_sweep / mae of the classes and main_rec.py's -sweep-k / -mae on top.

Everything is compared by equality of bits, NaN as NaN (eccknn_reference.canon): every cell of a sweep against the
restatement tests/knn_sweep_reference.py, which is the single-cell restatement called with that (k, min_k), and against the
device's own estimate_batch / estimate_batch_centered for that cell.  The similarity and the lists are crafted
(knn_sweep_reference.make_case: n_x = 300, one list per length around every k in use, ties, signed zeros, NaN, +-1e308), so
most tests need no fit; tests/test_knn_sweep_host.py proves on the CPU that the case tells adjacent cells apart.  One test
hands a rating list with ids outside [0, n_x) straight to the C call: the header promises that such an id is never an
index (its similarity is NaN and no table is read for it), and the kernel tests the id before every read it guards."""
import numpy as np
import pytest
import torch

import eccknn_reference as E
import knn_sweep_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_GRIDS = ("borders", "adjacent", "1x1", "one-k", "one-min_k", "all-impossible")
MODE_SIDES = [(None, True)] + [(mode, side) for mode in S.MODES[1:] for side in (True, False)]
MODE_IDS = ["%s-%s" % (m or "plain", "user" if u else "item") for m, u in MODE_SIDES]


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)


@pytest.fixture(scope="module")
def world():
    """The crafted case on the host and on the device, once."""
    case = S.make_case()
    t = case["tables"]
    d = dict(sim=dev(case["sim"], torch.float64), qx=dev(case["qx"], torch.int32), qy=dev(case["qy"], torch.int32),
             yr=(dev(case["ptr"], torch.int64), dev(case["yr_x"], torch.int32), dev(case["yr_r"], torch.float64)),
             mu=dev(t["mu"], torch.float64), sd=dev(t["sd"], torch.float64), bx=dev(t["bx"], torch.float64),
             by=dev(t["by"], torch.float64))
    return case, d


def centering(case, d, mode, user_based):
    from n2v_hip import eccknn
    if mode is None:
        return None
    gm = case["tables"]["gm"]
    if mode == "baseline":
        return eccknn.Centering(mode, user_based, gm, d["bx"], None, d["by"])
    return eccknn.Centering(mode, user_based, gm, d["mu"], d["sd"] if mode == "zscore" else None, None)


def single_cell(d, qx, qy, k, min_k, c):
    from n2v_hip import eccknn
    if c is None:
        return eccknn.estimate_batch(d["sim"], d["yr"], qx, qy, k, min_k)
    return eccknn.estimate_batch_centered(d["sim"], d["yr"], qx, qy, k, min_k, c, check=False)


def assert_sweep(case, d, grid, mode, user_based, keep=None, sim=None, yr=None, d_yr=None):
    """One estimate_sweep over `grid`: shapes and types, then every cell against the restatement and the single-cell call.
    keep: indices of the queries used (None: all of them)."""
    from n2v_hip import eccknn
    ks, min_ks = grid
    qx, qy = (case["qx"], case["qy"]) if keep is None else (case["qx"][keep], case["qy"][keep])
    dqx, dqy = dev(qx, torch.int32), dev(qy, torch.int32)
    c = centering(case, d, mode, user_based)
    dd = dict(d, yr=d_yr) if d_yr is not None else d
    est, ak, imp = eccknn.estimate_sweep(dd["sim"], dd["yr"], dqx, dqy, ks, min_ks, c, check=False)
    n_k, n_m, n_q = len(ks), len(min_ks), len(qx)
    assert est.dtype == torch.float64 and ak.dtype == torch.int32 and imp.dtype == torch.uint8
    assert est.shape == imp.shape == (n_k, n_m, n_q) and ak.shape == (n_k, n_q) and est.is_contiguous() and imp.is_contiguous()
    west, wak, wimp = S.estimate_sweep(case["sim"] if sim is None else sim, case["yr"] if yr is None else yr, qx, qy, ks, min_ks,
                                       S.tab(case, mode, user_based))
    est_h, ak_h, imp_h = est.cpu().numpy(), ak.cpu().numpy(), imp.cpu().numpy()
    for j, k in enumerate(ks):
        assert np.array_equal(ak_h[j], wak[j]), (k, "actual_k vs restatement")
        for m, min_k in enumerate(min_ks):
            what = (mode, user_based, k, min_k)
            assert np.array_equal(imp_h[j, m], wimp[j, m]), what + ("impossible vs restatement",)
            assert E.canon(est_h[j, m]) == E.canon(west[j, m]), what + ("est vs restatement",)
            e1, a1, i1 = single_cell(dd, dqx, dqy, k, min_k, c)
            assert torch.equal(ak[j], a1) and torch.equal(imp[j, m], i1), what + ("vs the single-cell call",)
            assert E.canon(est_h[j, m]) == E.canon(e1.cpu().numpy()), what + ("est vs the single-cell call",)
    return west, wak, wimp


# ---- the estimates ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,user_based", MODE_SIDES, ids=MODE_IDS)
def test_every_cell_equals_the_restatement_and_the_single_cell_call(world, mode, user_based):
    case, d = world
    for name in SMALL_GRIDS:
        west, wak, wimp = assert_sweep(case, d, S.GRIDS[name], mode, user_based)
        known = slice(0, -3)
        if name == "all-impossible":
            # every min_k is above every k: plain, every cell is impossible; centred, the base alone and nothing is
            if mode is None:
                assert wimp.all() and not west.any()
            else:
                assert not wimp[:, :, known].any() and all(E.canon(west[j, m]) == E.canon(west[0, 0]) for j in range(3) for m in range(2))
        if name == "borders":
            lens = np.diff(case["ptr"])[case["qy"][known]]
            assert (wak[-1][known] <= lens).all() and (lens < 63).any() and (lens > 256).any()   # past L for all, some, none
            assert np.isnan(west).any()                                                        # inf - inf in the sums
    # unknown x, unknown y, both: impossible and 0, or under the baseline mode the biases that are known
    west, wak, wimp = assert_sweep(case, d, ((2, 9), (1, 3)), mode, user_based, keep=np.arange(len(case["qx"]) - 3, len(case["qx"])))
    assert not wak.any() and wimp.all() == (mode != "baseline") and wimp.any() == (mode != "baseline")
    if mode == "baseline":
        t = case["tables"]
        assert west[1, 1].tolist() == [t["gm"] + t["by"][5], t["gm"] + t["bx"][7], t["gm"]]


@pytest.mark.parametrize("mode,user_based", [(None, True), ("baseline", False), ("zscore", True)], ids=["plain", "baseline-item", "zscore-user"])
def test_the_full_16_by_16_grid(world, mode, user_based):
    """256 cells from one launch; two queries per list and the three unknown ones keep the restatement quick."""
    case, d = world
    n = len(case["qx"])
    keep = np.array([q for q in range(n - 3) if q % 5 in (0, 3)] + [n - 3, n - 2, n - 1])
    assert_sweep(case, d, S.GRIDS["16x16"], mode, user_based, keep=keep)


def test_a_1_by_1_grid_is_the_plain_call(world):
    from n2v_hip import eccknn
    case, d = world
    for k, min_k in ((40, 1), (1, 1), (256, 3), (64, 70)):
        est, ak, imp = eccknn.estimate_sweep(d["sim"], d["yr"], d["qx"], d["qy"], [k], [min_k])
        e1, a1, i1 = eccknn.estimate_batch(d["sim"], d["yr"], d["qx"], d["qy"], k, min_k)
        assert est.shape == (1, 1, len(case["qx"])) and torch.equal(ak[0], a1) and torch.equal(imp[0, 0], i1)
        assert E.canon(est[0, 0].cpu().numpy()) == E.canon(e1.cpu().numpy())


@pytest.mark.parametrize("mode", S.MODES[1:])
def test_a_rating_list_with_ids_outside_the_range(world, mode):
    """Straight to the C call (check=False skips yr_check): an entry of yr_x outside [0, n_x) has a NaN similarity, ranks
    last, adds nothing, and no table is read for it.  The restatement sees the same through one more, all-NaN, column."""
    from n2v_hip import eccknn
    case, d = world
    n_x, bad = case["n_x"], case["yr_x"].copy()
    rs = np.random.RandomState(8)
    where = rs.permutation(len(bad))[:400]
    bad[where] = rs.choice([-1, -2, n_x, n_x + 3, 2 ** 31 - 1, -2 ** 31], size=len(where))
    sim = np.concatenate([case["sim"], np.full((n_x, 1), np.nan)], axis=1)
    yr, ptr = {}, case["ptr"]
    for y in range(case["n_y"]):
        if ptr[y + 1] > ptr[y]:
            yr[y] = [(int(a) if 0 <= a < n_x else n_x, float(b)) for a, b in zip(bad[ptr[y]:ptr[y + 1]], case["yr_r"][ptr[y]:ptr[y + 1]])]
    d_yr = (d["yr"][0], dev(bad, torch.int32), d["yr"][2])
    with pytest.raises(ValueError, match="yr"):
        eccknn.estimate_sweep(d["sim"], d_yr, d["qx"], d["qy"], (5,), (1,), centering(case, d, mode, True))
    assert_sweep(case, d, S.GRIDS["borders"], mode, True, sim=sim, yr=yr, d_yr=d_yr)


def test_host_checks_of_estimate_sweep(world):
    from n2v_hip import eccknn
    case, d = world
    c = centering(case, d, "zscore", True)
    for ks, min_ks in (((5, 5), (1,)), ((5,), (0,)), ((257,), (1,)), (tuple(range(1, 18)), (1,)), ((), (1,))):
        with pytest.raises(ValueError):
            eccknn.estimate_sweep(d["sim"], d["yr"], d["qx"], d["qy"], ks, min_ks)
    with pytest.raises(ValueError, match="centering"):
        eccknn.estimate_sweep(d["sim"], d["yr"], d["qx"], d["qy"], (5,), (1,), c._replace(sd=None))
    with pytest.raises(ValueError, match="nothing to estimate"):
        eccknn.estimate_sweep(d["sim"], d["yr"], d["qx"][:0], d["qy"][:0], (5,), (1,))


# ---- errors -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_q", [1, 255, 256, 257, 600])
def test_errors_equal_the_restatement_and_predict(n_q):
    from n2v_hip import eccknn
    rs = np.random.RandomState(n_q)
    r_true = rs.randint(1, 11, n_q) * 0.5
    d_true = dev(r_true, torch.float64)
    for n_cols in (1, 3, 256):
        pred = np.clip(rs.normal(size=(n_cols, n_q)) * 1.5 + 3.0, 1.0, 5.0)
        d_pred = dev(pred, torch.float64)
        rmse, mae = eccknn.errors(d_pred, d_true)
        wrmse, wmae = S.errors(pred, r_true)
        assert rmse.dtype == mae.dtype == np.float64 and rmse.shape == mae.shape == (n_cols,)
        assert E.canon(rmse) == E.canon(wrmse) and E.canon(mae) == E.canon(wmae), n_cols
        # the rmse of a column is n2v_eccknn_predict's: the predictions are inside the scale, so predict leaves them
        zeros = torch.zeros(n_q, dtype=torch.uint8, device=DEV)
        for c in range(n_cols):
            same, err = eccknn.predict(d_pred[c], zeros, 3.0, (1.0, 5.0), d_true)
            assert torch.equal(same, d_pred[c]) and err == rmse[c], (n_cols, c)
    one = eccknn.errors(d_pred[2], d_true)                         # 1-D: one column
    assert one[0].shape == (1,) and one[0][0] == rmse[2] and one[1][0] == mae[2]


def test_errors_keep_nan_and_inf_and_refuse_bad_arguments():
    from n2v_hip import eccknn
    r_true = np.array([1.0, 2.0, 4.0, 5.0])
    pred = np.array([[1.0, np.nan, 4.0, 5.0], [np.inf, 2.0, 4.0, 5.0], [1.0, 2.0, 4.0, 5.0], [-0.0, 1e308, -1e308, 5.0]])
    rmse, mae = eccknn.errors(dev(pred, torch.float64), dev(r_true, torch.float64))
    wrmse, wmae = S.errors(pred, r_true)
    assert E.canon(rmse) == E.canon(wrmse) and E.canon(mae) == E.canon(wmae)
    assert np.isnan(rmse[0]) and np.isinf(mae[1]) and (rmse[2], mae[2]) == (0.0, 0.0) and np.isinf(rmse[3])
    good, true = dev(pred, torch.float64), dev(r_true, torch.float64)
    for p, t in ((good.to(torch.float32), true), (good, true[:3]), (good, true.to(torch.float32)), (good[:, :0], true[:0]),
                 (good.view(2, 2, 4), true), (good, true.view(2, 2))):
        with pytest.raises(ValueError, match="errors"):
            eccknn.errors(p, t)


# ---- end to end on a 40 x 30 ratings file -------------------------------------------------------------------------------------

KS, MIN_KS = (1, 3, 5, 10), (1, 2, 4)


def small_rows():
    rs = np.random.RandomState(21)
    cells = rs.permutation(40 * 30)[:420]
    return [("u%02d" % (c // 30), "i%02d" % (c % 30), float(rs.randint(1, 6))) for c in cells]


@pytest.fixture(scope="module")
def split():
    """(trainset, testset) of the 40 x 30 file: 340 ratings to train on, 80 to test, two of them on unknown ids."""
    from n2v_hip import eccknn
    rows = small_rows()
    train, test = rows[:340], rows[340:] + [("nobody", "i03", 4.0), ("u05", "nothing", 2.0)]
    ts = eccknn.Trainset.from_ratings([t[0] for t in train], [t[1] for t in train], [t[2] for t in train], rating_scale=(1.0, 5.0))
    return ts, test


def knn_classes():
    from n2v_hip import eccknn
    return {"eccen": eccknn.EccenKNN, "knn": eccknn.KNNBasic, "knnmeans": eccknn.KNNWithMeans, "knnzscore": eccknn.KNNWithZScore,
            "knnbaseline": eccknn.KNNBaseline}


@pytest.mark.parametrize("name,user_based", [("eccen", True), ("knn", True), ("knn", False), ("knnmeans", True), ("knnzscore", False),
                                             ("knnbaseline", True), ("knnbaseline", False)])
def test_accuracy_sweep_equals_a_loop_of_fresh_fits(split, name, user_based):
    ts, testset = split
    cls = knn_classes()[name]
    opts = {"name": "cosine", "user_based": user_based}
    w = np.random.RandomState(2).random_sample(ts.n_items if user_based else ts.n_users) + 0.5
    algo = cls(k=7, min_k=2, sim_options=opts, device=DEV).fit(ts, w)
    acc = algo.accuracy_sweep(testset, KS, MIN_KS)
    cells = algo.test_sweep(testset, KS, MIN_KS)
    assert (algo.k, algo.min_k) == (7, 2)
    assert list(acc) == list(cells) == [(k, m) for k in KS for m in MIN_KS]
    r_true = [t[2] for t in testset]
    for (k, min_k), got in acc.items():
        fresh = cls(k=k, min_k=min_k, sim_options=opts, device=DEV).fit(ts, w)
        pred, ak, imp = fresh.test(testset)
        assert E.canon(cells[(k, min_k)][0]) == E.canon(pred), (k, min_k)
        assert np.array_equal(cells[(k, min_k)][1], ak) and np.array_equal(cells[(k, min_k)][2], imp), (k, min_k)
        assert cells[(k, min_k)][2].dtype == bool
        wrmse, wmae = S.errors(pred, r_true)
        assert got == {"rmse": fresh.rmse(testset), "mae": fresh.mae(testset)} == {"rmse": wrmse[0], "mae": wmae[0]}, (k, min_k)
    assert len({v["rmse"] for v in acc.values()}) > len(KS)         # the cells are not one column
    # the fit's own k and min_k: rmse / mae / test are the cell (7, 2) of a 1 x 1 sweep
    assert algo.accuracy_sweep(testset, [7], [2]) == {(7, 2): {"rmse": algo.rmse(testset), "mae": algo.mae(testset)}}
    with pytest.raises(ValueError, match="empty testset"):
        algo.accuracy_sweep([], KS, MIN_KS)


def test_mae_of_every_predictor(split):
    from n2v_hip import coclustering, eccknn, nmf, slopeone, svd
    ts, testset = split
    r_true = [t[2] for t in testset]
    algos = [cls(k=5, device=DEV).fit(ts, np.ones(ts.n_items)) for cls in knn_classes().values()]
    algos += [svd.SVD(n_factors=8, n_epochs=3, device=DEV).fit(ts), nmf.NMF(n_factors=4, n_epochs=3, device=DEV).fit(ts),
              slopeone.SlopeOne(device=DEV).fit(ts), coclustering.CoClustering(n_epochs=3, device=DEV).fit(ts)]
    for algo in algos:
        pred = algo.test(testset)[0]
        wrmse, wmae = S.errors(pred, r_true)
        mae = algo.mae(testset)
        assert type(mae) is float and mae == wmae[0] and algo.rmse(testset) == wrmse[0], type(algo).__name__
        assert 0.0 < mae <= algo.rmse(testset)                      # the mean absolute error never exceeds the rmse
    with pytest.raises(ValueError, match="empty testset"):
        algos[0].mae([])


def test_main_rec_sweep_end_to_end(tmp_path, capsys):
    import main_rec
    path = tmp_path / "ratings.csv"
    path.write_text("user,item,rating\n" + "".join("%s,%s,%r\n" % t for t in small_rows()))
    base = ["-input", str(path), "-seed", "4", "-algo", "knnmeans", "-sim", "msd"]
    grid = [(k, m) for k in (2, 5, 9) for m in (1, 3)]
    folds = main_rec.main(base + ["-sweep-k", "2,5,9", "-sweep-mink", "1,3", "-cv", "3"])
    out = capsys.readouterr().out.strip().split("\n")
    assert len(folds) == 3 and all(list(f) == grid for f in folds) and len(out) == 3 * 6 + 6 + 1
    want = [l for f in folds for c in grid for l in ["k %d mink %d RMSE: %r MAE: %r" % (c + (f[c]["rmse"], f[c]["mae"]))]]
    assert out[:18] == want
    mean = {c: (float(np.mean([f[c]["rmse"] for f in folds])), float(np.mean([f[c]["mae"] for f in folds]))) for c in grid}
    assert out[18:24] == ["k %d mink %d mean RMSE: %r mean MAE: %r" % (c + mean[c]) for c in grid]
    best = min(grid, key=lambda c: mean[c][0])
    assert out[24] == "best: k %d mink %d mean RMSE %r" % (best + (mean[best][0],))
    # every cell is what a run with that -k and -mink prints and returns
    for c in grid:
        single = main_rec.main(base + ["-k", str(c[0]), "-mink", str(c[1]), "-cv", "3", "-mae"])
        lines = capsys.readouterr().out.strip().split("\n")
        assert single == [f[c]["rmse"] for f in folds], c
        assert lines == [l for f in folds for l in ("RMSE: %r" % f[c]["rmse"], "MAE: %r" % f[c]["mae"])] + \
            ["mean RMSE: %r" % mean[c][0], "mean MAE: %r" % mean[c][1]], c
    # one split: the cells, then the best one; -sweep-mink absent is the run's -mink; the plain run is as it was
    cells = main_rec.main(base + ["-sweep-k", "2,5", "-mink", "3", "-item-based"])
    out = capsys.readouterr().out.strip().split("\n")
    assert list(cells) == [(2, 3), (5, 3)] and len(out) == 3 and out[2].startswith("best: k ")
    rmse = main_rec.main(base + ["-k", "5", "-mink", "3", "-item-based"])
    assert capsys.readouterr().out == "RMSE: %r\n" % rmse and rmse == cells[(5, 3)]["rmse"]
    rmse, metrics = main_rec.main(base + ["-k", "5", "-topn", "3", "-mae"])
    out = capsys.readouterr().out.strip().split("\n")
    assert [l.split(":")[0] for l in out] == ["RMSE", "MAE", "F1 / MAP / MRR / NDCG @3"] and out[0] == "RMSE: %r" % rmse
