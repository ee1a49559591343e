"""The last stage of the reference's src/main_ecc.py:160-202: a random forest on the feature rows of the ie-profile study,
fitted and applied on the device (n2v_hip.forest).

    python main_forest.py -x X.npy -y Y.npy -task regression|classification [-trees N] [-depth 16] [-bins 256]
                          [-max-features 1.0|sqrt|log2|N] [-test-size 0.3] [-seed 0] [-device cuda:0] [-save model.npz]

-x / -y        the files `consistency.py -profile ... -features X.npy Y.npy` writes: fp64 [n, F] rows and their feedback.
-task          regression: RandomForestRegressor, 100 trees by default, score R^2.  classification: the entropy
               RandomForestClassifier on the distinct values of y as labels (at most 32), 50 trees by default, score accuracy.
-max-features  a number of features, a share with a decimal point, sqrt or log2; by default all for regression and sqrt
               for classification, as in sklearn 1.7.
-test-size     the share of the rows held out.  The split is seeded: a permutation of the rows by numpy's
               RandomState(seed), the first round(n * share) of it are the test rows, the rest, in file order, the training
               rows.  (The reference draws random.sample and train_test_split; neither is restated.)
-seed          also seeds the forest's bootstrap and feature subsets.
Prints `train score: <repr>`, `test score: <repr>`, and the fit and predict times in seconds.
"""
import argparse
import sys
import time

import numpy as np


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("-x", required=True)
    p.add_argument("-y", required=True)
    p.add_argument("-task", required=True, choices=["regression", "classification"])
    p.add_argument("-trees", type=int, default=None)
    p.add_argument("-depth", type=int, default=16)
    p.add_argument("-bins", type=int, default=256)
    p.add_argument("-max-features", dest="max_features", default=None)
    p.add_argument("-test-size", dest="test_size", type=float, default=0.3)
    p.add_argument("-seed", type=int, default=0)
    p.add_argument("-device", default="cuda:0")
    p.add_argument("-save", default=None)
    a = p.parse_args(argv)
    if a.trees is not None and a.trees < 1:
        p.error("-trees must be at least 1")
    if not 0 <= a.depth <= 32:
        p.error("-depth must be 0 .. 32")
    if not 2 <= a.bins <= 256:
        p.error("-bins must be 2 .. 256")
    if not 0.0 < a.test_size < 1.0:
        p.error("-test-size must lie inside (0, 1)")
    if a.max_features is not None and a.max_features not in ("sqrt", "log2"):
        try:
            a.max_features = float(a.max_features) if "." in a.max_features else int(a.max_features)
        except ValueError:
            p.error("-max-features takes a number of features, a share with a decimal point, sqrt or log2")
    return a


def split_rows(n, test_size, seed):
    """(train rows in file order, test rows in the permutation's order)."""
    perm = np.random.RandomState(seed).permutation(n)
    n_test = int(round(n * test_size))
    return np.sort(perm[n_test:]), perm[:n_test]


def main(a):
    import torch
    from n2v_hip import forest
    X, y = np.load(a.x), np.load(a.y)
    if X.ndim != 2 or y.shape != (X.shape[0],):
        sys.exit("main_forest: %s is %s and %s is %s; expected [n, F] and [n]" % (a.x, X.shape, a.y, y.shape))
    train, test = split_rows(X.shape[0], a.test_size, a.seed)
    if len(train) < 1 or len(test) < 1:
        sys.exit("main_forest: %d rows leave an empty side at -test-size %r" % (X.shape[0], a.test_size))
    kw = dict(max_depth=a.depth, n_bins=a.bins, seed=a.seed, device=a.device)
    if a.trees is not None:
        kw["n_estimators"] = a.trees
    if a.max_features is not None:
        kw["max_features"] = a.max_features
    model = (forest.RandomForestRegressor if a.task == "regression" else forest.RandomForestClassifier)(**kw)
    t0 = time.perf_counter()
    model.fit(X[train], y[train])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    model.predict(X[test])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print("%s forest: %d trees, depth %d, %d bins, %d train and %d test rows x %d features"
          % (a.task, model.n_estimators, a.depth, a.bins, len(train), len(test), X.shape[1]))
    print("train score: %r" % model.score(X[train], y[train]))
    print("test score: %r" % model.score(X[test], y[test]))
    print("fit: %.3f s, predict: %.3f s" % (t1 - t0, t2 - t1))
    if a.save:
        model.save(a.save)
    return model


if __name__ == "__main__":
    main(parse_args())
