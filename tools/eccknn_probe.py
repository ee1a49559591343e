"""Timing probe of the EccenKNN path (n2v_hip.eccknn) on a synthetic MovieLens-1M-shaped set.  Timing only: what the
kernels compute is the business of tests/test_gpu_eccknn.py.

    python tools/eccknn_probe.py [--users 6040 --items 3706 --ratings 1000000 --queries 200000 --k 20 --repeats 7]

Prints one JSON line: medians over `repeats` timed runs after two warm-up runs, each run bracketed by device events;
pair-y updates per second of the similarity kernel (every pair of the upper triangle of 64x64 tiles visits every y, the
work the dense kernel actually does), the same as a fraction of the device's vector fp64 peak (78.6 TFLOP/s is AMD's
published MI355X figure; an update is counted as the 5 flops of the cosine form), and the numpy restatement's time on a
300-user subset on one core (--numpy-subset 0 skips it).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "node2vec-by-ecc_amd"), os.path.join(ROOT, "tests")]

FP64_VECTOR_PEAK = 78.6e12


def synthetic(n_users, n_items, n_ratings, seed):
    """Distinct (user, item) cells with a power-law item popularity, half-star ratings."""
    rs = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, n_items + 1) ** 0.9
    pop /= pop.sum()
    keys = np.empty(0, dtype=np.int64)
    while len(keys) < n_ratings:
        u = rs.randint(0, n_users, size=n_ratings // 2)
        i = rs.choice(n_items, size=n_ratings // 2, p=pop)
        keys = np.unique(np.concatenate([keys, u.astype(np.int64) * n_items + i]))
    keys = rs.permutation(keys)[:n_ratings]
    return keys // n_items, keys % n_items, rs.randint(1, 11, size=n_ratings) * 0.5


def timed(fn, repeats, warmup=2):
    import torch
    out = []
    for n in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if n >= warmup:
            out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--ratings", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=200000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-subset", type=int, default=300)
    ap.add_argument("--sim", default="cosine")
    a = ap.parse_args(argv)
    import torch
    from n2v_hip import eccknn
    u, i, r = synthetic(a.users, a.items, a.ratings, 0)
    ts = eccknn.Trainset.from_ratings(u.tolist(), i.tolist(), r)
    w = np.random.RandomState(1).normal(size=ts.n_items)
    dev = torch.device("cuda:0")
    to = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v)).to(device=dev, dtype=dt)
    dx, dy, dr, dw = to(ts.u, torch.int32), to(ts.i, torch.int32), to(ts.r, torch.float64), to(w, torch.float64)
    n_x, n_y = ts.n_users, ts.n_items
    dense, mask = eccknn.densify(dx, dy, dr, n_x, n_y)
    res = {"metric": "eccknn_probe", "device": torch.cuda.get_device_name(0), "n_x": n_x, "n_y": n_y, "ratings": len(r),
           "queries": a.queries, "k": a.k, "sim": a.sim, "repeats": a.repeats}
    res["sim_kernel_ms"] = timed(lambda: eccknn.similarity(dense, mask, dw, a.sim), a.repeats)
    res["densify_plus_sim_ms"] = timed(lambda: eccknn.similarity(*eccknn.densify(dx, dy, dr, n_x, n_y), dw, a.sim), a.repeats)
    tiles = (n_x + 63) // 64
    updates = tiles * (tiles + 1) // 2 * 64 * 64 * n_y
    res["pair_y_updates_per_s"] = updates / (res["sim_kernel_ms"][0] * 1e-3)
    res["fraction_of_fp64_vector_peak"] = res["pair_y_updates_per_s"] * 5 / FP64_VECTOR_PEAK
    sim = eccknn.similarity(dense, mask, dw, a.sim)
    yr = tuple(to(v, dt) for v, dt in zip(ts.ir, (torch.int64, torch.int32, torch.float64)))
    rs = np.random.RandomState(2)
    qx, qy = to(rs.randint(0, n_x, a.queries), torch.int32), to(rs.randint(0, n_y, a.queries), torch.int32)
    res["estimate_ms"] = timed(lambda: eccknn.estimate_batch(sim, yr, qx, qy, a.k, 1), a.repeats)
    est, _, imp = eccknn.estimate_batch(sim, yr, qx, qy, a.k, 1)
    rt = to(rs.randint(1, 11, a.queries) * 0.5, torch.float64)
    res["predict_rmse_ms"] = timed(lambda: eccknn.predict(est, imp, ts.global_mean, ts.rating_scale, rt), a.repeats)
    if a.numpy_subset:
        import eccknn_reference as E
        keep = ts.u < a.numpy_subset
        yr_sub = E.build_yr(ts.u[keep], ts.i[keep], ts.r[keep])
        t0 = time.perf_counter()
        E.NUMPY[a.sim](a.numpy_subset, yr_sub, 1, w)
        res["numpy_subset_users"] = a.numpy_subset
        res["numpy_subset_s"] = time.perf_counter() - t0
        res["numpy_subset_pair_updates"] = int(sum(len(v) ** 2 for v in yr_sub.values()))
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
