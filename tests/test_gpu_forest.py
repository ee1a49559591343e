"""n2v_hip.forest (csrc/n2v_forest.hip) against its definition, tests/forest_reference.py, by equality: bins, edges, bootstrap
weights, every tree table with the node id each level starts at (the tables are append-only and breadth first, so equal
tables and equal level starts are equal tables after every level), leaf values, predict, predict_proba and score.  NaN is
compared as NaN.  Every case is at most 5 000 x 70."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import forest_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "forest")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def _forest():
    from n2v_hip import forest
    return forest


def _data(n, F, seed, kind="regressor", distinct=None, K=5):
    rs = np.random.RandomState(seed)
    X = rs.normal(size=(n, F)) if distinct is None else rs.randint(0, distinct, size=(n, F)).astype(np.float64)
    signal = X[:, 0] + 0.5 * X[:, F // 2] * X[:, F - 1] + 0.3 * rs.normal(size=n)
    if kind == "regressor":
        return X, np.round(signal * 4.0) / 4.0
    cuts = np.quantile(signal, np.linspace(0, 1, K + 1)[1:-1]) if n > 1 else []
    return X, np.searchsorted(cuts, signal).astype(np.int64) if n > K else rs.permutation(np.arange(n) % K)


def _pair(kind, X, y, **kw):
    forest = _forest()
    budget = kw.pop("hist_budget_bytes", None)
    ref = R.Forest(kind, **kw).fit(X, y)
    cls = forest.RandomForestRegressor if kind == "regressor" else forest.RandomForestClassifier
    dev = cls(device="cuda:0", **kw, **({} if budget is None else {"hist_budget_bytes": budget})).fit(X, y)
    return ref, dev


def _tables(dev):
    t = {k: v.cpu().numpy() for k, v in dev.trees_.items()}
    return [{k: t[k][a:b] for k in ("feature", "threshold", "left", "value")} for a, b in zip(t["tree_ptr"], t["tree_ptr"][1:])]


def _same(ref, dev, X, y, Xq=None):
    assert np.array_equal(dev.bins_.cpu().numpy(), ref.bins)
    edges, n_edges = dev.trees_["edges"].cpu().numpy(), dev.trees_["n_edges"].cpu().numpy()
    for f, e in enumerate(ref.edges):
        assert n_edges[f] == len(e) and np.array_equal(edges[f, :len(e)], e), f
    trees = _tables(dev)
    assert len(trees) == len(ref.trees)
    for t, (want, got) in enumerate(zip(ref.trees, trees)):
        assert np.array_equal(dev.weights_[t].cpu().numpy(), ref.weights[t]), t
        assert np.array_equal(dev.level_ptr_[t], want["level_ptr"]), (t, dev.level_ptr_[t], want["level_ptr"])
        for k in ("feature", "threshold", "left"):
            assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (t, k)
        assert np.array_equal(got["value"], want["value"], equal_nan=True), t
    for Q in (X,) if Xq is None else (X, Xq):
        assert np.array_equal(dev.predict(Q), ref.predict(Q), equal_nan=True)
        if ref.kind == "classifier":
            assert np.array_equal(dev.predict_proba(Q), ref.predict_proba(Q), equal_nan=True)
    assert dev.score(X, y) == ref.score(X, y) or (np.isnan(dev.score(X, y)) and np.isnan(ref.score(X, y)))


def _query(X, seed=5):
    rs = np.random.RandomState(seed)
    return X[rs.randint(0, len(X), size=100)] + rs.normal(size=(100, X.shape[1])) * 0.5


# ---- sizes --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_row_counts(kind, n):
    if kind == "classifier" and n == 1:
        with pytest.raises(ValueError, match="classes"):
            _forest().RandomForestClassifier(device="cuda:0").fit(np.zeros((1, 3)), np.zeros(1))
        return
    X, y = _data(n, 3, n, kind, K=2 if n < 5 else 5)
    ref, dev = _pair(kind, X, y, n_estimators=3, max_features=None, seed=n)
    _same(ref, dev, X, y, _query(X))


@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_5000_by_70(kind):
    X, y = _data(5000, 70, 1, kind)
    ref, dev = _pair(kind, X, y, n_estimators=2, max_depth=5, n_bins=64, seed=3)
    assert ref.trees[0]["level_ptr"][-1] > 20
    _same(ref, dev, X, y, _query(X))


@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 70])
def test_feature_counts_at_the_widest_tile(F):
    assert _forest().feature_tile(2, 0) == 64                      # 63 / 64 / 65 are the tile's border here
    X, y = _data(257, F, F, distinct=6)
    ref, dev = _pair("regressor", X, y, n_estimators=2, max_depth=6, n_bins=2, max_features=None, seed=F)
    _same(ref, dev, X, y)


@pytest.mark.parametrize("kind,K", [("regressor", 0), ("classifier", 5), ("classifier", 32)])
@pytest.mark.parametrize("off", [-1, 0, 1])
def test_feature_counts_at_the_tile_border_of_256_bins(kind, K, off):
    tile = _forest().feature_tile(256, K)
    assert tile == {0: 16, 5: 8, 32: 2}[K]
    F = tile + off
    X, y = _data(400, F, 7 + off, kind, K=K)
    ref, dev = _pair(kind, X, y, n_estimators=1, max_depth=4, max_features=None, seed=1)
    _same(ref, dev, X, y)


@pytest.mark.parametrize("n_bins", [2, 3, 64, 255, 256])
@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_bin_counts(kind, n_bins):
    X, y = _data(600, 4, n_bins, kind)
    ref, dev = _pair(kind, X, y, n_estimators=2, max_depth=6, n_bins=n_bins, max_features=None, seed=2)
    assert max(len(e) for e in ref.edges) == n_bins - 1
    _same(ref, dev, X, y, _query(X))


# ---- features -----------------------------------------------------------------------------------------------------------

def test_constant_wide_and_duplicated_columns():
    rs = np.random.RandomState(3)
    n = 700
    X = np.stack([np.full(n, 2.5), rs.normal(size=n), rs.randint(0, 9, n).astype(float), rs.normal(size=n), rs.normal(size=n)], 1)
    X[:, 4] = X[:, 1]                                              # an exact tie between features 1 and 4: the lower one wins
    y = np.round((X[:, 1] + 0.2 * X[:, 2]) * 8) / 8
    for kind, target in (("regressor", y), ("classifier", (y > 0).astype(int) + (y > 1))):
        ref, dev = _pair(kind, X, target, n_estimators=2, max_depth=5, max_features=None, seed=1)
        assert len(ref.edges[0]) == 0 and len(ref.edges[1]) == 255 and len(np.unique(X[:, 1])) > 256
        assert 1 in ref.trees[0]["feature"] and 4 not in ref.trees[0]["feature"]
        _same(ref, dev, X, target, _query(X))


def test_gap_middle_over_0_1_and_2_empty_bins():
    # feature 1 takes 0 .. 9 where feature 0 is 0 and only 0, 1, 3, 6 where it is 1: below the root's split on feature 0 the
    # occupied bins of feature 1 leave runs of 0, 1 and 2 empty bins
    rs = np.random.RandomState(0)
    f0 = np.repeat([0.0, 1.0], 200)
    f1 = np.concatenate([rs.randint(0, 10, 200), rs.choice([0, 1, 3, 6], 200)]).astype(float)
    X = np.stack([f0, f1], 1)
    y = 100.0 * f0 + f1 * f1
    ref, dev = _pair("regressor", X, y, n_estimators=1, bootstrap=False, max_features=None, max_depth=4)
    tree = ref.trees[0]
    assert tree["feature"][0] == 0
    below = {(int(f), int(t)) for f, t in zip(tree["feature"], tree["threshold"])}
    assert {(1, 0), (1, 1), (1, 4)} <= below, below                # 0|1: no gap; 1|3: (1 + 3 - 1) // 2 = 1; 3|6: (3 + 6 - 1) // 2 = 4
    _same(ref, dev, X, y, np.stack([np.repeat([0.0, 1.0], 10), np.tile(np.arange(10.0), 2)], 1))


def test_all_targets_equal():
    X, _ = _data(100, 3, 0)
    y = np.full(100, 3.5)
    ref, dev = _pair("regressor", X, y, n_estimators=2)
    assert all(len(t["feature"]) == 1 for t in ref.trees)
    _same(ref, dev, X, y)
    assert dev.score(X, y) == 1.0


def test_target_sums_at_the_2_53_bound():
    forest = _forest()
    top = 2.0 ** 31 - 2.0 ** -20                                   # round(top * 2^20) = 2^51 - 1; 4 rows: 2^53 - 4
    X = np.arange(4.0).reshape(4, 1)
    y = np.array([top, top, -top, 1.0])
    ref, dev = _pair("regressor", X, y, n_estimators=1, bootstrap=False, max_features=None)
    _same(ref, dev, X, y)
    for refuse in (lambda a, b: R.Forest("regressor", n_estimators=1).fit(a, b),
                   lambda a, b: forest.RandomForestRegressor(n_estimators=1, device="cuda:0").fit(a, b)):
        with pytest.raises(ValueError, match="y_bits"):
            refuse(X, np.array([2.0 ** 31, 0.0, 0.0, 0.0]))
    with pytest.raises(ValueError, match="y_bits"):
        forest.RandomForestRegressor(n_estimators=1, device="cuda:0").fit(X, np.array([np.inf, 0.0, 0.0, 0.0]))


@pytest.mark.parametrize("K", [2, 10, 32])
def test_class_counts(K):
    X, y = _data(640, 5, K, "classifier", K=K)
    ref, dev = _pair("classifier", X, y, n_estimators=2, max_depth=6, max_features=None, seed=K)
    assert len(ref.classes_) == K
    assert any((t["value"] == 0.0).any() for t in ref.trees)       # a class absent from a node
    assert K == 2 or any((t["value"][t["left"] >= 0] == 0.0).any() for t in ref.trees)     # and from one that splits
    _same(ref, dev, X, y, _query(X))
    labels = np.array(["r%02d" % v for v in y])                    # labels of any sortable kind
    again = _forest().RandomForestClassifier(n_estimators=2, max_depth=6, max_features=None, seed=K, device="cuda:0").fit(X, labels)
    assert np.array_equal(again.predict(X), labels[0:0].dtype.type("r") + np.char.zfill(dev.predict(X).astype(str), 2))


# ---- parameters ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [0, 1, 16])
@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_depths(kind, depth):
    X, y = _data(300, 4, depth, kind)
    ref, dev = _pair(kind, X, y, n_estimators=2, max_depth=depth, max_features=None)
    deepest = len(ref.trees[0]["level_ptr"]) - 2                   # 300 rows end before level 16; 0 and 1 are reached
    assert deepest == depth if depth < 16 else 1 < deepest <= 16
    _same(ref, dev, X, y, _query(X))


def test_min_samples_on_both_sides_of_a_count():
    X = np.repeat([0.0, 1.0], [20, 44]).reshape(64, 1)
    y = X[:, 0] * 2.0
    for kw, n_nodes in ((dict(min_samples_split=64), 3), (dict(min_samples_split=65), 1), (dict(min_samples_leaf=20), 3),
                        (dict(min_samples_leaf=21), 1)):
        ref, dev = _pair("regressor", X, y, n_estimators=1, bootstrap=False, max_features=None, **kw)
        assert len(ref.trees[0]["feature"]) == n_nodes, kw
        _same(ref, dev, X, y)
        ref, dev = _pair("classifier", X, y, n_estimators=1, bootstrap=False, max_features=None, **kw)
        assert len(ref.trees[0]["feature"]) == n_nodes, kw
        _same(ref, dev, X, y)


@pytest.mark.parametrize("max_features", [1, "sqrt", 9, 0.5, "log2"])
@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_feature_subsets(kind, max_features):
    X, y = _data(500, 9, 4, kind)
    ref, dev = _pair(kind, X, y, n_estimators=3, max_depth=5, max_features=max_features, seed=11)
    _same(ref, dev, X, y, _query(X))


def test_feature_subsets_differ_by_node_and_take_lower_features_on_equal_keys():
    assert [R.resolve_max_features(m, 9) for m in (1, "sqrt", 9, 0.5, "log2", None, 1.0)] == [1, 3, 9, 4, 3, 9, 9]
    picks = {tuple(R.feature_subset(11, 0, v, 9, 3)) for v in range(20)}
    assert len(picks) > 5 and all(len(set(p)) == 3 for p in picks)


@pytest.mark.parametrize("bootstrap", [True, False])
def test_bootstrap_on_and_off(bootstrap):
    X, y = _data(200, 3, 9)
    ref, dev = _pair("regressor", X, y, n_estimators=2, bootstrap=bootstrap, max_depth=6)
    if bootstrap:
        assert all(w.sum() == 200 and (w == 0).any() and (w >= 3).any() for w in ref.weights)
    else:
        assert all((w == 1).all() for w in ref.weights)
    _same(ref, dev, X, y, _query(X))


@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_histogram_budget_batches(kind):
    X, y = _data(900, 5, 12, kind)
    kw = dict(n_estimators=2, max_depth=6, n_bins=32, max_features=None, seed=4)
    ref, dev = _pair(kind, X, y, **kw)
    _same(ref, dev, X, y)
    node_bytes = 5 * 32 * (16 if kind == "regressor" else 4 * len(ref.classes_))
    sizes = np.diff(ref.trees[0]["level_ptr"])
    five = [b for s in sizes for b in range(1, s + 1) if -(-s // b) == 5]
    two = [b for s in sizes for b in range(1, s + 1) if -(-s // b) == 2]
    assert five and two, sizes
    for b in (five[0], two[0], 1):                                 # some level in 5 batches, in 2, and one node per batch
        _, small = _pair(kind, X, y, hist_budget_bytes=node_bytes * b, **kw)
        for k in ("feature", "threshold", "left", "value", "tree_ptr"):
            assert np.array_equal(small.trees_[k].cpu().numpy(), dev.trees_[k].cpu().numpy(), equal_nan=True), (b, k)


def test_two_fits_give_the_same_bytes_and_save_load_predicts_the_same(tmp_path):
    import torch
    forest = _forest()
    for kind in ("regressor", "classifier"):
        X, y = _data(800, 6, 21, kind)
        cls = forest.RandomForestRegressor if kind == "regressor" else forest.RandomForestClassifier
        a = cls(n_estimators=4, max_depth=8, seed=5, device="cuda:0").fit(X, y)
        b = cls(n_estimators=4, max_depth=8, seed=5, device="cuda:0").fit(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda())
        for k in forest.TABLES:
            assert a.trees_[k].cpu().numpy().tobytes() == b.trees_[k].cpu().numpy().tobytes(), k
        path = str(tmp_path / (kind + ".npz"))
        a.save(path)
        c = cls.load(path)
        Q = _query(X)
        assert np.array_equal(c.predict(Q), a.predict(Q)) and c.score(X, y) == a.score(X, y)
        got = b.predict(torch.from_numpy(Q).cuda())
        assert np.array_equal(got.cpu().numpy() if kind == "regressor" else got, a.predict(Q))
        if kind == "classifier":
            assert np.array_equal(c.predict_proba(Q), a.predict_proba(Q))
        with pytest.raises(ValueError, match="holds a"):
            (forest.RandomForestClassifier if kind == "regressor" else forest.RandomForestRegressor).load(path)


# ---- malformed input: out-of-range integers in otherwise valid tables, found before any launch that trusts them -----------

def test_malformed_input_raises_and_names_the_cause(tmp_path):
    import torch
    forest = _forest()
    X, y = _data(300, 4, 2)
    model = forest.RandomForestRegressor(n_estimators=2, max_depth=4, n_bins=16, device="cuda:0").fit(X, y)
    good = {k: v.clone() for k, v in model.trees_.items()}
    split_node = int((good["left"] >= 0).nonzero()[0])
    second = int(good["tree_ptr"][1])

    def spoiled(key, at, v):
        model.trees_ = {k: t.clone() for k, t in good.items()}
        model.trees_[key][at] = v
        return model

    for key, at, v, word in (("feature", split_node, 4, "feature"), ("feature", split_node, -2, "feature"),
                             ("left", split_node, split_node, "child"), ("left", split_node, second - 1, "child"),
                             ("left", split_node, -7, "child"), ("left", second, good["left"].numel(), "child"),
                             ("threshold", split_node, 16, "threshold"), ("n_edges", 1, 16, "edges"),
                             ("tree_ptr", 1, 0, "tree_ptr")):
        with pytest.raises(ValueError, match=word):
            spoiled(key, at, v).predict(X)
    model.trees_ = good
    path = str(tmp_path / "m.npz")
    model.save(path)
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    arrays["feature"] = arrays["feature"].copy()
    arrays["feature"][split_node] = 99
    np.savez(str(tmp_path / "bad.npz"), **arrays)
    with pytest.raises(ValueError, match="feature"):
        forest.RandomForestRegressor.load(str(tmp_path / "bad.npz"))

    bins = model.bins_.clone()
    assert model.predict_bins(bins).shape == (300, 1)
    bins[17, 2] = 16
    with pytest.raises(ValueError, match="bin"):
        model.predict_bins(bins)
    with pytest.raises(ValueError, match="bin"):
        forest.check_bins(bins, 16)
    cls = torch.tensor([0, 1, 4, 2], dtype=torch.int32, device="cuda:0")
    forest.check_classes(cls, 5)
    for bad in (5, -1):
        cls[1] = bad
        with pytest.raises(ValueError, match="class"):
            forest.check_classes(cls, 5)
    Xn = X.copy()
    Xn[5, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        model.predict(Xn)
    with pytest.raises(ValueError, match="NaN"):
        forest.RandomForestRegressor(device="cuda:0").fit(Xn, y)
    with pytest.raises(ValueError, match="NaN"):
        R.Forest("regressor").fit(Xn, y)


def test_limits_are_refused_before_anything_is_allocated():
    forest = _forest()
    for kw, word in ((dict(n_bins=257), "n_bins"), (dict(n_bins=1), "n_bins"), (dict(max_depth=33), "max_depth"),
                     (dict(min_samples_leaf=0), "min_samples_leaf"), (dict(y_bits=53), "y_bits")):
        with pytest.raises(ValueError, match=word):
            forest.RandomForestRegressor(device="cuda:0", **kw)
    with pytest.raises(ValueError, match="entropy"):
        forest.RandomForestClassifier(criterion="gini")

    class Shape:                                                   # a shape alone: nothing of this size is ever allocated
        ndim = 2

        def __init__(self, *shape):
            self.shape = shape

        def __len__(self):
            return self.shape[0]

    model = forest.RandomForestRegressor(device="cuda:0")
    model._features = lambda X: X
    with pytest.raises(ValueError, match="rows"):
        model.fit(Shape(2 ** 31, 3), Shape(2 ** 31))
    with pytest.raises(ValueError, match="features"):
        model.fit(Shape(10, 4097), Shape(10))
    with pytest.raises(ValueError, match="classes"):
        forest.RandomForestClassifier(device="cuda:0").fit(np.zeros((40, 2)), np.arange(40))


# ---- the command line and the data set of tests/test_forest_host.py (c) -------------------------------------------------

def test_main_forest_end_to_end(tmp_path):
    X, y = _data(300, 6, 8)
    y = np.clip(np.round(y) + 3, 1, 5)
    np.save(str(tmp_path / "X.npy"), X), np.save(str(tmp_path / "Y.npy"), y)
    for task in ("regression", "classification"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "node2vec-by-ecc_amd", "main_forest.py"), "-x", str(tmp_path / "X.npy"),
                              "-y", str(tmp_path / "Y.npy"), "-task", task, "-trees", "5", "-depth", "6", "-seed", "3",
                              "-save", str(tmp_path / "m.npz")], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        lines = dict(l.split(": ", 1) for l in out.stdout.splitlines() if l.startswith(("train score", "test score")))
        import main_forest
        train, test = main_forest.split_rows(300, 0.3, 3)
        assert len(test) == 90 and sorted(np.concatenate([train, test]).tolist()) == list(range(300))
        kind = "regressor" if task == "regression" else "classifier"
        ref = R.Forest(kind, n_estimators=5, max_depth=6, seed=3).fit(X[train], y[train])
        assert float(lines["train score"]) == ref.score(X[train], y[train]) and float(lines["test score"]) == ref.score(X[test], y[test])
        assert "fit:" in out.stdout and os.path.exists(str(tmp_path / "m.npz"))


def test_the_forest_data_set_scores_equal_the_restatements():
    import make_forest_golden as G
    forest = _forest()
    with open(os.path.join(GOLDEN, "forest_c.json")) as fh:
        doc = json.load(fh)
    Xa, ya, Xb, yb = G.dataset_c()
    kw = dict(n_estimators=doc["trees"], max_depth=doc["depth"], n_bins=doc["bins"], seed=0, device="cuda:0")
    assert forest.RandomForestRegressor(**kw).fit(Xa, ya).score(Xb, yb) == doc["restatement_r2"][0]
    assert forest.RandomForestClassifier(**kw).fit(Xa, G.labels(ya)).score(Xb, G.labels(yb)) == doc["restatement_accuracy"][0]
