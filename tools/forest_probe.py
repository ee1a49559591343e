"""Times n2v_hip.forest on one GPU (timing only; tests/test_gpu_forest.py holds the results to the definition).

    python tools/forest_probe.py [--rows 700000] [--features 200] [--trees 100] [--depth 16] [--runs 7] [--warmup 2]
                                 [--forest-runs 7] [--predict-rows 300000]
    python tools/forest_probe.py --sklearn-rows 100000      (one fit each of this module and of sklearn, n_jobs=16)

Synthetic regression rows of the ie-profile study's shape: 100 profile shares (a Dirichlet row) and a 100-wide item vector,
half-star y.  Prints medians (min - max): binning, one tree's fit by level split into histogram, split and route, the fit
of --trees trees, predict of --predict-rows rows, and the histogram kernel's floor (the bin bytes it reads per level).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "node2vec-by-ecc_amd"))


def med(ts):
    return "%.4f s (%.4f - %.4f)" % (float(np.median(ts)), min(ts), max(ts))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=700000)
    p.add_argument("--features", type=int, default=200)
    p.add_argument("--trees", type=int, default=100)
    p.add_argument("--depth", type=int, default=16)
    p.add_argument("--runs", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--forest-runs", type=int, default=7)
    p.add_argument("--predict-rows", type=int, default=300000)
    p.add_argument("--out", default=None)
    p.add_argument("--sklearn-rows", type=int, default=0)
    a = p.parse_args()
    import torch
    from n2v_hip import forest
    g = torch.Generator(device="cuda:0").manual_seed(1)
    half = a.features // 2
    prof = torch.empty((a.rows, half), dtype=torch.float64, device="cuda:0").exponential_(generator=g)
    prof /= prof.sum(1, keepdim=True)
    X = torch.cat([prof, torch.randn((a.rows, a.features - half), dtype=torch.float64, device="cuda:0", generator=g)], 1)
    y = torch.clamp(torch.round(2 * (3 + 4 * (X[:, 0] - X[:, 1]) + X[:, half] * X[:, half + 1] + 0.5 * torch.randn(
        a.rows, dtype=torch.float64, device="cuda:0", generator=g))) / 2, 0.5, 5.0)
    del prof
    res = {"rows": a.rows, "features": a.features, "depth": a.depth, "device": torch.cuda.get_device_name(0)}

    def timed(fn, runs, warmup):
        ts = []
        for r in range(warmup + runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ts.append(time.perf_counter() - t0)
        return ts

    if a.sklearn_rows:                                             # the yardstick alone: one run each on the same subset
        try:
            from sklearn.ensemble import RandomForestRegressor
        except ImportError:
            print("sklearn: not installed here, not measured")
            return
        Xs, ys = X[:a.sklearn_rows].contiguous(), y[:a.sklearn_rows].contiguous()
        ours = forest.RandomForestRegressor(n_estimators=a.trees, max_depth=a.depth, device="cuda:0")
        ts = timed(lambda: ours.fit(Xs, ys), 1, 1)
        print("n2v_hip.forest, %d trees, depth %d, %d x %d: fit %.2f s" % (a.trees, a.depth, a.sklearn_rows, a.features, ts[0]), flush=True)
        Xh, yh = Xs.cpu().numpy(), ys.cpu().numpy()
        t0 = time.perf_counter()
        sk = RandomForestRegressor(n_estimators=a.trees, max_depth=a.depth, n_jobs=16, random_state=0).fit(Xh, yh)
        print("sklearn n_jobs=16, same rows: fit %.2f s" % (time.perf_counter() - t0), flush=True)
        Xt, yt = X[a.sklearn_rows:a.sklearn_rows + 100000], y[a.sklearn_rows:a.sklearn_rows + 100000]
        print("R^2 on the next %d rows: ours %.4f, sklearn %.4f" % (Xt.shape[0], ours.score(Xt, yt), sk.score(Xt.cpu().numpy(), yt.cpu().numpy())),
              flush=True)
        return
    one = forest.RandomForestRegressor(n_estimators=1, max_depth=a.depth, device="cuda:0")
    one.fit(X, y)
    res["binning"] = timed(lambda: one.bin_features(X), a.runs, a.warmup)
    print("binning %d x %d: %s" % (a.rows, a.features, med(res["binning"])), flush=True)
    res["one_tree"] = timed(lambda: one.fit(X, y), a.runs, a.warmup)
    print("fit of 1 tree, depth %d (edges and binning included): %s, %d nodes" % (a.depth, med(res["one_tree"]), one.trees_["feature"].numel()),
          flush=True)
    stages = []
    for r in range(a.warmup + a.runs):
        one.timing_ = {}
        one.fit(X, y)
        if r >= a.warmup:
            stages.append(dict(one.timing_))
    one.timing_ = None
    res["levels"] = {}
    for level in range(a.depth + 1):
        row = {s: [st.get((s, level), 0.0) for st in stages] for s in ("hist", "split", "route")}
        res["levels"][level] = row
        print("level %2d: %5d nodes  hist %s  split %s  route %s" % (level, int(np.diff(one.level_ptr_[0])[level]) if level < len(one.level_ptr_[0]) - 1 else 0,
                                                                   med(row["hist"]), med(row["split"]), med(row["route"])), flush=True)
    bin_bytes = a.rows * a.features
    print("histogram floor per level: %.1f MB of bins and %.1e LDS atomic pairs" % (bin_bytes / 1e6, bin_bytes), flush=True)
    if a.forest_runs:
        many = forest.RandomForestRegressor(n_estimators=a.trees, max_depth=a.depth, device="cuda:0")
        res["forest"] = timed(lambda: many.fit(X, y), a.forest_runs, min(a.warmup, 1))
        print("fit of %d trees, depth %d: %s" % (a.trees, a.depth, med(res["forest"])), flush=True)
        Q = X[:a.predict_rows].contiguous()
        res["predict"] = timed(lambda: many.predict(Q), a.runs, a.warmup)
        print("predict of %d rows, %d trees: %s" % (Q.shape[0], a.trees, med(res["predict"])), flush=True)
        print("train R^2 on the first %d rows: %.4f" % (Q.shape[0], many.score(Q, y[:a.predict_rows])), flush=True)
    if a.out:
        res["levels"] = {str(k): v for k, v in res["levels"].items()}
        with open(a.out, "w") as fh:
            json.dump(res, fh)


if __name__ == "__main__":
    main()
