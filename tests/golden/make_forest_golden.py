"""Writes tests/golden/forest/: what tests/forest_reference.py (the definition of n2v_hip.forest) owes sklearn, measured on
the CPU.  Needs sklearn; the tests read the files and need none.

    python tests/golden/make_forest_golden.py

single_tree.npz  (a) and (b) of tests/test_forest_host.py: 20 seeds of X = randint(0, 16) [500, 6] and a noisy y rounded to
                 2^-20, DecisionTreeRegressor(max_depth=d)'s predictions on the training rows for d = 1, 3, 6, 12 and on a
                 grid of 400 off-sample integer points for d = 1, 3.
forest_c.npz     the data set of (c): RandomState(20261021), 4 000 train and 1 000 test rows, 8 Dirichlet(0.5) columns and 4
                 normal columns, half-star y clipped to 0.5 .. 5.
forest_c.json    sklearn's test R^2 and entropy-classifier accuracy over 8 seeds (50 trees, depth 8), their mean and
                 single-seed standard deviation, the restatement's over 4 seeds (256 bins), and sklearn's version.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "forest")
SEEDS_A = 20
DEPTHS_A = (1, 3, 6, 12)
DEPTHS_B = (1, 3)
C_TREES, C_DEPTH, C_BINS = 50, 8, 256
C_SKLEARN_SEEDS, C_OWN_SEEDS = 8, 4


def single_tree_case(seed):
    """X [500, 6] of integers 0 .. 15, y rounded to 2^-20, and 400 integer grid points in -1 .. 17."""
    rs = np.random.RandomState(seed)
    X = rs.randint(0, 16, size=(500, 6)).astype(np.float64)
    y = X[:, 0] * 0.3 + np.sin(X[:, 1]) + X[:, 2] * X[:, 3] * 0.02 + rs.normal(size=500) * 0.5
    y = np.round(y * 2.0 ** 20) / 2.0 ** 20
    grid = rs.randint(-1, 18, size=(400, 6)).astype(np.float64)
    return X, y, grid


def dataset_c():
    """(X_train, y_train, X_test, y_test); y in half stars."""
    rs = np.random.RandomState(20261021)
    n = 5000
    P = rs.dirichlet([0.5] * 8, size=n)
    Z = rs.normal(size=(n, 4))
    raw = (2.75 + 3.0 * (P[:, 0] - P[:, 1]) + 1.5 * P[:, 2] * Z[:, 0] + 0.8 * Z[:, 1] + 0.5 * np.sin(2.0 * Z[:, 2])
           + 0.6 * rs.normal(size=n))
    y = np.clip(np.round(2.0 * raw) / 2.0, 0.5, 5.0)
    X = np.concatenate([P, Z], axis=1)
    return X[:4000], y[:4000], X[4000:], y[4000:]


def labels(y):
    """The ratings as strings, as the reference's classifier takes them."""
    return np.array(["%.1f" % v for v in y])


def restatement_scores(seeds):
    sys.path.insert(0, os.path.dirname(HERE))
    import forest_reference as R
    Xa, ya, Xb, yb = dataset_c()
    r2, acc = [], []
    for s in seeds:
        kw = dict(n_estimators=C_TREES, max_depth=C_DEPTH, n_bins=C_BINS, seed=s)
        r2.append(R.Forest("regressor", **kw).fit(Xa, ya).score(Xb, yb))
        acc.append(R.Forest("classifier", **kw).fit(Xa, labels(ya)).score(Xb, labels(yb)))
    return r2, acc


def main():
    import sklearn
    from sklearn.ensemble import RandomForestClassifier, RandomForestRegressor
    from sklearn.tree import DecisionTreeRegressor
    os.makedirs(OUT, exist_ok=True)
    arrays = {}
    for seed in range(SEEDS_A):
        X, y, grid = single_tree_case(seed)
        arrays["X_%d" % seed], arrays["y_%d" % seed], arrays["grid_%d" % seed] = X.astype(np.uint8), y, grid.astype(np.int8)
        for d in DEPTHS_A:
            tree = DecisionTreeRegressor(max_depth=d).fit(X, y)
            arrays["train_%d_%d" % (seed, d)] = tree.predict(X)
            if d in DEPTHS_B:
                arrays["grid_%d_%d" % (seed, d)] = tree.predict(grid)
    np.savez_compressed(os.path.join(OUT, "single_tree.npz"), **arrays)

    Xa, ya, Xb, yb = dataset_c()
    np.savez_compressed(os.path.join(OUT, "forest_c.npz"), X_train=Xa, y_train=ya, X_test=Xb, y_test=yb)
    r2, acc = [], []
    for s in range(C_SKLEARN_SEEDS):
        r2.append(float(RandomForestRegressor(n_estimators=C_TREES, max_depth=C_DEPTH, random_state=s, n_jobs=-1).fit(Xa, ya).score(Xb, yb)))
        acc.append(float(RandomForestClassifier(n_estimators=C_TREES, max_depth=C_DEPTH, criterion="entropy", random_state=s, n_jobs=-1)
                         .fit(Xa, labels(ya)).score(Xb, labels(yb))))
    own_r2, own_acc = restatement_scores(range(C_OWN_SEEDS))
    doc = {"sklearn_version": sklearn.__version__, "numpy_version": np.__version__,
           "trees": C_TREES, "depth": C_DEPTH, "bins": C_BINS,
           "sklearn_r2": r2, "sklearn_r2_mean": float(np.mean(r2)), "sklearn_r2_std": float(np.std(r2, ddof=1)),
           "sklearn_accuracy": acc, "sklearn_accuracy_mean": float(np.mean(acc)), "sklearn_accuracy_std": float(np.std(acc, ddof=1)),
           "restatement_r2": own_r2, "restatement_r2_mean": float(np.mean(own_r2)),
           "restatement_accuracy": own_acc, "restatement_accuracy_mean": float(np.mean(own_acc))}
    with open(os.path.join(OUT, "forest_c.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
