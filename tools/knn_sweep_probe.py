"""Timing probe of the k-NN sweep (n2v_hip.eccknn.estimate_sweep) on the synthetic MovieLens-1M-shaped set of
tools/eccknn_probe.py.  Timing only: what the kernels compute is the business of tests/test_gpu_knn_sweep.py.

    python tools/knn_sweep_probe.py [--users 6040 --items 3706 --ratings 1000000 --queries 200000 --repeats 7]
                                    [--ks 5,10,20,40,80] [--min-ks 1,5] [--algo knnmeans|knnzscore|knnbaseline]

Three paths over the same similarity matrix, rating lists and queries, alternating run by run, each run bracketed by device
events, medians (min, max) over `repeats` timed runs after two warm-up runs (after the timing the probe asserts, at
the size it timed, that every cell of the sweep equals the call it replaces: `cells_equal`):
  sweep_ms        one estimate_sweep over ks x min_ks;
  cells_ms        the len(ks) * len(min_ks) estimate_batch calls it replaces, one after the other;
  largest_k_ms    one estimate_batch at the largest k, the least the selection can cost.
First for the plain mode, then for one centred mode (--algo, the default knnmeans) as `centered_*`.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "node2vec-by-ecc_amd"), os.path.dirname(os.path.abspath(__file__))]


def timed_round(fns, repeats, warmup=2):
    """(median, min, max) ms of every call of fns, the calls alternating run by run."""
    import torch
    out = [[] for _ in fns]
    for n in range(warmup + repeats):
        for which, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if n >= warmup:
                out[which].append(a.elapsed_time(b))
    return [(statistics.median(v), min(v), max(v)) for v in out]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--ratings", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ks", default="5,10,20,40,80")
    ap.add_argument("--min-ks", dest="min_ks", default="1,5")
    ap.add_argument("--algo", default="knnmeans", choices=["knnmeans", "knnzscore", "knnbaseline"])
    a = ap.parse_args(argv)
    import torch
    from n2v_hip import eccknn
    from eccknn_probe import centering_tables, synthetic
    ks, min_ks = eccknn.sweep_options([int(v) for v in a.ks.split(",")], [int(v) for v in a.min_ks.split(",")])
    u, i, r = synthetic(a.users, a.items, a.ratings, 0)
    ts = eccknn.Trainset.from_ratings(u.tolist(), i.tolist(), r)
    dev = torch.device("cuda:0")
    to = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v)).to(device=dev, dtype=dt)
    n_x, n_y = ts.n_users, ts.n_items
    w = to(np.random.RandomState(1).normal(size=n_y), torch.float64)
    sim = eccknn.similarity(*eccknn.densify(to(ts.u, torch.int32), to(ts.i, torch.int32), to(ts.r, torch.float64), n_x, n_y), w, "cosine")
    yr = tuple(to(v, dt) for v, dt in zip(ts.ir, (torch.int64, torch.int32, torch.float64)))
    eccknn.yr_check(yr, n_x)
    rs = np.random.RandomState(2)
    qx, qy = to(rs.randint(0, n_x, a.queries), torch.int32), to(rs.randint(0, n_y, a.queries), torch.int32)
    res = {"metric": "knn_sweep_probe", "device": torch.cuda.get_device_name(0), "n_x": n_x, "n_y": n_y, "ratings": len(r),
           "queries": a.queries, "ks": ks, "min_ks": min_ks, "repeats": a.repeats}

    def cells(batch):
        for k in ks:
            for min_k in min_ks:
                batch(k, min_k)

    plain = lambda k, min_k: eccknn.estimate_batch(sim, yr, qx, qy, k, min_k)
    res["sweep_ms"], res["cells_ms"], res["largest_k_ms"] = timed_round(
        [lambda: eccknn.estimate_sweep(sim, yr, qx, qy, ks, min_ks), lambda: cells(plain), lambda: plain(ks[-1], min_ks[0])], a.repeats)
    c = centering_tables(a.algo, ts, dev)
    centred = lambda k, min_k: eccknn.estimate_batch_centered(sim, yr, qx, qy, k, min_k, c, check=False)
    res["algo"] = a.algo
    res["centered_sweep_ms"], res["centered_cells_ms"], res["centered_largest_k_ms"] = timed_round(
        [lambda: eccknn.estimate_sweep(sim, yr, qx, qy, ks, min_ks, c, check=False), lambda: cells(centred),
         lambda: centred(ks[-1], min_ks[0])], a.repeats)
    # the outputs at the size that was timed: every cell of the sweep against the call it replaces, NaN as NaN
    def same(a, b):
        nan = torch.isnan(a)
        return bool(torch.equal(nan, torch.isnan(b))) and bool(torch.equal(a[~nan].view(torch.int64), b[~nan].view(torch.int64)))
    for prefix, centering, batch in (("", None, plain), ("centered_", c, centred)):
        est, ak, imp = eccknn.estimate_sweep(sim, yr, qx, qy, ks, min_ks, centering, check=False)
        singles = [[batch(k, min_k) for min_k in min_ks] for k in ks]
        res[prefix + "cells_equal"] = all(same(est[j, m], e) and torch.equal(ak[j], a_k) and torch.equal(imp[j, m], i)
                                          for j, row in enumerate(singles) for m, (e, a_k, i) in enumerate(row))
        assert res[prefix + "cells_equal"], "a cell of the sweep differs from its estimate_batch call"
    for prefix in ("", "centered_"):
        res[prefix + "sweep_over_largest_k"] = res[prefix + "sweep_ms"][0] / res[prefix + "largest_k_ms"][0]
        res[prefix + "cells_over_sweep"] = res[prefix + "cells_ms"][0] / res[prefix + "sweep_ms"][0]
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
