"""Timing probe of the EccenKNN path (n2v_hip.eccknn) on a synthetic MovieLens-1M-shaped set.  Timing only: what the
kernels compute is the business of tests/test_gpu_eccknn.py.

    python tools/eccknn_probe.py [--users 6040 --items 3706 --ratings 1000000 --queries 200000 --k 20 --repeats 7]
                                 [--form dense|sparse|both] [--shape ml1m|30music-users]
                                 [--sim cosine|msd|pearson|pearson_baseline] [--baselines]
                                 [--algo knn|knnmeans|knnzscore|knnbaseline]

Prints one JSON line: medians over `repeats` timed runs after two warm-up runs, each run bracketed by device events;
pair-y updates per second of the similarity kernel (every pair of the upper triangle of 64x64 tiles visits every y, the
work the dense kernel actually does), the same as a fraction of the device's vector fp64 peak (78.6 TFLOP/s is AMD's
published MI355X figure; an update is counted as the 5 flops of the cosine form), and the numpy restatement's time on a
300-user subset on one core (--numpy-subset 0 skips it).

--form    which similarity kernel is timed: dense (the default), sparse (rating lists: `csr_by_x_ms` is the sort,
          `check_plus_sim_ms` the CSR check and the kernel), or both: the two on the same data in one session, and an
          assertion that their `sim` matrices are equal by bytes.  Every form also prints `useful_updates` =
          sum over y of |raters(y)|^2, the updates the reference's loops make, and the rate against it.
--sim     cosine / msd (EccenKNN's kernels) or pearson / pearson_baseline (KNNBasic's, with the same weights; the second
          one with the trainset's ALS baselines, computed once outside the timed region).  The numpy restatement is timed
          for cosine / msd only.  ml1m shape only for the Pearson names.
--algo    knn (the default) times the plain estimate kernel only; knnmeans / knnzscore / knnbaseline also time the centred
          one (KNNWithMeans / KNNWithZScore / KNNBaseline) on the same similarity, lists and queries, the two alternating run
          by run: `estimate_ms` and `estimate_centered_ms`, and `tables_ms`, the row moments or ALS baselines of the mode.
--baselines  also time eccknn.baselines (10 ALS epochs, both sides, uploads included) as `baselines_ms`.
--shape   ml1m (the default; --users / --items / --ratings apply) or 30music-users: 4e4 users x 5e6 items, 3e7 ratings,
          power-law items and users, de-duplicated on (user, item).  Past the dense limit, so sparse only; the estimate
          and predict timings are skipped, `fit_ms` is the sort, the check and the kernel once, and
          `peak_device_bytes` is torch.cuda.max_memory_allocated.
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


def synthetic_30music(n_users, n_items, n_ratings, seed):
    """The generators of tools/eccstats_probe.py (item power 0.9, user power 0.6), de-duplicated on (user, item)."""
    rs = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, n_items + 1) ** 0.9
    act = 1.0 / np.arange(1, n_users + 1) ** 0.6
    pop /= pop.sum(); act /= act.sum()
    keys = np.empty(0, dtype=np.int64)
    while len(keys) < n_ratings:
        m = max(n_ratings - len(keys), n_ratings // 8)
        u = rs.choice(n_users, size=m, p=act)
        i = rs.choice(n_items, size=m, p=pop)
        keys = np.unique(np.concatenate([keys, u.astype(np.int64) * n_items + i]))
    keys = rs.permutation(keys)[:n_ratings]
    return keys // n_items, keys % n_items, rs.randint(1, 11, size=n_ratings) * 0.5


def useful_updates(y, n_y):
    c = np.bincount(y, minlength=n_y).astype(np.int64)
    return int((c * c).sum())


def numpy_subset(res, x, y, r, w, subset, sim):
    import eccknn_reference as E
    if sim not in E.NUMPY:
        return
    keep = x < subset
    yr_sub = E.build_yr(x[keep], y[keep], r[keep])
    t0 = time.perf_counter()
    E.NUMPY[sim](subset, yr_sub, 1, w)
    res["numpy_subset_users"] = subset
    res["numpy_subset_s"] = time.perf_counter() - t0
    res["numpy_subset_pair_updates"] = int(sum(len(v) ** 2 for v in yr_sub.values()))
    res["numpy_subset_updates_per_s"] = res["numpy_subset_pair_updates"] / res["numpy_subset_s"]


def big_shape(a):
    """30music-users: inner ids are the generator's own (the first-appearance relabelling is a host loop this probe does
    not time); sparse only."""
    import torch
    from n2v_hip import eccknn
    n_x, n_y, n = 40000, 5000000, 30000000
    if a.users != 6040 or a.items != 3706 or a.ratings != 1000000:
        n_x, n_y, n = a.users, a.items, a.ratings                 # a smaller run of the same generator
    u, i, r = synthetic_30music(n_x, n_y, n, 0)
    w = np.random.RandomState(1).normal(size=n_y)
    dev = torch.device("cuda:0")
    to = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v)).to(device=dev, dtype=dt)
    dx, dy, dr, dw = to(u, torch.int32), to(i, torch.int32), to(r, torch.float64), to(w, torch.float64)
    res = {"metric": "eccknn_probe", "device": torch.cuda.get_device_name(0), "shape": a.shape, "form": "sparse", "n_x": n_x,
           "n_y": n_y, "ratings": len(r), "sim": a.sim, "useful_updates": useful_updates(i, n_y)}
    torch.cuda.reset_peak_memory_stats()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    xr = eccknn.csr_by_x(dx, dy, dr, n_x, n_y)
    ev[1].record()
    sim = eccknn.similarity_sparse(xr, dw, n_y, a.sim)
    ev[2].record()
    torch.cuda.synchronize()
    res["csr_by_x_ms"], res["check_plus_sim_ms"] = ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])
    res["fit_ms"] = ev[0].elapsed_time(ev[2])
    res["peak_device_bytes"] = int(torch.cuda.max_memory_allocated())
    res["useful_updates_per_s"] = res["useful_updates"] / (res["check_plus_sim_ms"] * 1e-3)
    res["sim_diag_ok"] = bool((torch.diagonal(sim) == 1.0).all().item())
    if a.numpy_subset:
        numpy_subset(res, u, i, r, w, a.numpy_subset, a.sim)
    print(json.dumps(res))
    return res


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


def timed_pair(f, g, repeats, warmup=2):
    """timed() of two calls that alternate run by run."""
    import torch
    out = ([], [])
    for n in range(warmup + repeats):
        for which, fn in enumerate((f, g)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if n >= warmup:
                out[which].append(a.elapsed_time(b))
    return tuple((statistics.median(v), min(v), max(v)) for v in out)


def centering_tables(algo, ts, dev):
    """The user-based Centering of one centred algorithm, from the trainset: uploads, row moments or ALS baselines."""
    import torch
    from n2v_hip import eccknn
    if algo == "knnbaseline":
        bu, bi = eccknn.baselines(ts, device=dev)
        return eccknn.Centering("baseline", True, ts.global_mean, bu, None, bi)
    to = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v)).to(device=dev, dtype=dt)
    ptr, r = to(ts.ur[0], torch.int64), to(ts.ur[2], torch.float64)
    if algo == "knnmeans":
        return eccknn.Centering("means", True, ts.global_mean, eccknn.row_moments(ptr, r)[0], None, None)
    all_r = to(ts.r, torch.float64)
    overall = float(eccknn.row_moments(to([0, len(ts.r)], torch.int64), all_r)[1].item())
    mu, sd = eccknn.row_moments(ptr, r, zero_sigma=overall)
    return eccknn.Centering("zscore", True, ts.global_mean, mu, sd, None)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--ratings", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=200000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-subset", type=int, default=300)
    ap.add_argument("--sim", default="cosine", choices=["cosine", "msd", "pearson", "pearson_baseline"])
    ap.add_argument("--baselines", action="store_true")
    ap.add_argument("--algo", default="knn", choices=["knn", "knnmeans", "knnzscore", "knnbaseline"])
    ap.add_argument("--form", default="dense", choices=["dense", "sparse", "both"])
    ap.add_argument("--shape", default="ml1m", choices=["ml1m", "30music-users"])
    a = ap.parse_args(argv)
    if a.shape == "30music-users":
        if a.form != "sparse":
            ap.error("--shape 30music-users is past the dense limit: --form sparse")
        if a.sim.startswith("pearson") or a.baselines:
            ap.error("--shape 30music-users times cosine / msd only")
        return big_shape(a)
    import torch
    from n2v_hip import eccknn
    u, i, r = synthetic(a.users, a.items, a.ratings, 0)
    ts = eccknn.Trainset.from_ratings(u.tolist(), i.tolist(), r)
    w = np.random.RandomState(1).normal(size=ts.n_items)
    dev = torch.device("cuda:0")
    to = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v)).to(device=dev, dtype=dt)
    dx, dy, dr, dw = to(ts.u, torch.int32), to(ts.i, torch.int32), to(ts.r, torch.float64), to(w, torch.float64)
    n_x, n_y = ts.n_users, ts.n_items
    res = {"metric": "eccknn_probe", "device": torch.cuda.get_device_name(0), "shape": a.shape, "form": a.form, "n_x": n_x,
           "n_y": n_y, "ratings": len(r), "queries": a.queries, "k": a.k, "sim": a.sim, "repeats": a.repeats,
           "useful_updates": useful_updates(ts.i, n_y)}
    if a.baselines:
        res["baselines_ms"] = timed(lambda: eccknn.baselines(ts, device=dev), a.repeats)
    if a.sim.startswith("pearson"):
        kw = {"w": dw}
        if a.sim == "pearson_baseline":
            bx, by = eccknn.baselines(ts, device=dev)
            kw.update(global_mean=ts.global_mean, bx=bx, by=by)
        sim_dense = lambda dense, mask: eccknn.similarity_pearson(dense, mask, a.sim, **kw)
        sim_sparse = lambda xr: eccknn.similarity_pearson_sparse(xr, n_y, a.sim, **kw)
    else:
        sim_dense = lambda dense, mask: eccknn.similarity(dense, mask, dw, a.sim)
        sim_sparse = lambda xr: eccknn.similarity_sparse(xr, dw, n_y, a.sim)
    sim = None
    if a.form in ("dense", "both"):
        dense, mask = eccknn.densify(dx, dy, dr, n_x, n_y)
        res["sim_kernel_ms"] = timed(lambda: sim_dense(dense, mask), a.repeats)
        res["densify_plus_sim_ms"] = timed(lambda: sim_dense(*eccknn.densify(dx, dy, dr, n_x, n_y)), a.repeats)
        tiles = (n_x + 63) // 64
        updates = tiles * (tiles + 1) // 2 * 64 * 64 * n_y
        res["pair_y_updates_per_s"] = updates / (res["sim_kernel_ms"][0] * 1e-3)
        res["fraction_of_fp64_vector_peak"] = res["pair_y_updates_per_s"] * 5 / FP64_VECTOR_PEAK
        res["dense_useful_updates_per_s"] = res["useful_updates"] / (res["sim_kernel_ms"][0] * 1e-3)
        sim = sim_dense(dense, mask)
        del dense, mask
    if a.form in ("sparse", "both"):
        xr = eccknn.csr_by_x(dx, dy, dr, n_x, n_y)
        res["csr_by_x_ms"] = timed(lambda: eccknn.csr_by_x(dx, dy, dr, n_x, n_y), a.repeats)
        res["check_plus_sim_ms"] = timed(lambda: sim_sparse(xr), a.repeats)
        res["sparse_useful_updates_per_s"] = res["useful_updates"] / (res["check_plus_sim_ms"][0] * 1e-3)
        sparse = sim_sparse(xr)
        if sim is not None:
            assert torch.equal(sim.view(torch.int64), sparse.view(torch.int64)), "dense and sparse sim differ"
            res["sim_equal_by_bytes"] = True
        sim = sparse
    yr = tuple(to(v, dt) for v, dt in zip(ts.ir, (torch.int64, torch.int32, torch.float64)))
    rs = np.random.RandomState(2)
    qx, qy = to(rs.randint(0, n_x, a.queries), torch.int32), to(rs.randint(0, n_y, a.queries), torch.int32)
    if a.algo == "knn":
        res["estimate_ms"] = timed(lambda: eccknn.estimate_batch(sim, yr, qx, qy, a.k, 1), a.repeats)
    else:
        res["algo"] = a.algo
        res["tables_ms"] = timed(lambda: centering_tables(a.algo, ts, dev), a.repeats)
        c = centering_tables(a.algo, ts, dev)
        eccknn.yr_check(yr, n_x)
        res["estimate_ms"], res["estimate_centered_ms"] = timed_pair(
            lambda: eccknn.estimate_batch(sim, yr, qx, qy, a.k, 1),
            lambda: eccknn.estimate_batch_centered(sim, yr, qx, qy, a.k, 1, c, check=False), a.repeats)
        res["centered_over_plain"] = res["estimate_centered_ms"][0] / res["estimate_ms"][0]
    est, _, imp = eccknn.estimate_batch(sim, yr, qx, qy, a.k, 1)
    rt = to(rs.randint(1, 11, a.queries) * 0.5, torch.float64)
    res["predict_rmse_ms"] = timed(lambda: eccknn.predict(est, imp, ts.global_mean, ts.rating_scale, rt), a.repeats)
    if a.numpy_subset:
        numpy_subset(res, ts.u, ts.i, ts.r, w, a.numpy_subset, a.sim)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
