"""Timing probe of the matrix-factorisation path (n2v_hip.svd) on a synthetic MovieLens-1M-shaped set.  Timing only: what
the kernels compute is the business of tests/test_gpu_svd.py.

    python tools/svd_probe.py [--users 6040 --items 3706 --ratings 800000 --factors 100 --strata 64,256,1024,4096]
                              [--queries 200000 --repeats 5 --numpy-ratings 20000]

Prints one JSON line.  Per n_strata: the time of build_blocks + the block check (once), and the median / min / max over
`repeats` epochs after two warm-up epochs, each epoch bracketed by device events, as ms per epoch and rating updates per
second; `auto` is what svd.auto_strata picks for the shape and is always among the values timed.  Then the estimate
kernel on `queries` random known pairs, and the numpy restatement's updates per second on one core over the first
`numpy-ratings` ratings (0 skips it).

`bytes_per_update` is the traffic one rating needs if nothing is cached: the qi row read and written (16 * n_factors),
the pu row read and written once per run of one user inside a block (16 * n_factors / mean run length), bu, bi and the
16-byte (u, i, r) entry.  `hbm_bound_updates_per_s` is 8 TB/s (AMD's published MI355X figure) over that.  At this shape
the whole model (users + items) * n_factors * 8 bytes is a few MB and stays in the caches, so the bound says how far the
kernel is from being a streaming kernel, not what limits it: a wavefront's ratings are a dependent chain (row read, 64
lane butterfly, row write), and an epoch is n_strata launches.
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

HBM_BYTES_PER_S = 8e12


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--ratings", type=int, default=800000)
    ap.add_argument("--factors", type=int, default=100)
    ap.add_argument("--strata", default="64,256,1024,4096")
    ap.add_argument("--queries", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-ratings", type=int, default=20000)
    a = ap.parse_args(argv)
    import torch
    from n2v_hip import eccknn, svd
    if not torch.cuda.is_available():
        raise RuntimeError("svd_probe: no GPU visible; a timing needs the device")
    u, i, r = synthetic(a.users, a.items, a.ratings, 0)
    ts = eccknn.Trainset.from_ratings(u.tolist(), i.tolist(), r)
    dev = torch.device("cuda:0")
    to = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v)).to(device=dev, dtype=dt)
    du = to(np.repeat(np.arange(ts.n_users, dtype=np.int64), np.diff(ts.ur[0])), torch.int64)
    di, dr = to(ts.ur[1], torch.int64), to(ts.ur[2], torch.float64)
    auto = svd.auto_strata(ts.n_users, ts.n_items, ts.n_ratings)
    res = {"metric": "svd_probe", "device": torch.cuda.get_device_name(0), "n_users": ts.n_users, "n_items": ts.n_items,
           "ratings": ts.n_ratings, "n_factors": a.factors, "repeats": a.repeats, "auto": auto, "strata": {}}
    algo = svd.SVD(n_factors=a.factors, n_epochs=0, n_strata=1, device=dev).fit(ts)       # the initial model
    rates = algo.rates
    for P in sorted(set(int(v) for v in a.strata.split(",")) | {auto}):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        blocks = svd.Blocks(svd.build_blocks(du, di, dr, ts.n_users, ts.n_items, P), ts.n_users, ts.n_items, P)
        ev[1].record()
        torch.cuda.synchronize()
        runs = torch.count_nonzero(blocks.u[1:] != blocks.u[:-1]).item() + 1          # a lower bound on the row reloads
        model = [t.clone() for t in (algo.bu, algo.bi, algo.pu, algo.qi)]
        times = []
        for n in range(2 + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            svd.epoch(blocks, algo.mu, True, rates, *model)
            e1.record()
            torch.cuda.synchronize()
            if n >= 2:
                times.append(e0.elapsed_time(e1))
        med = statistics.median(times)
        per_update = 16 * a.factors * (1 + runs / ts.n_ratings) + 16 * (1 + runs / ts.n_ratings) + 16
        res["strata"][str(P)] = {"blocks_ms": ev[0].elapsed_time(ev[1]), "epoch_ms": [med, min(times), max(times)],
                                 "updates_per_s": ts.n_ratings / (med * 1e-3), "user_runs": int(runs),
                                 "bytes_per_update": per_update, "hbm_bound_updates_per_s": HBM_BYTES_PER_S / per_update,
                                 "finite": bool(torch.isfinite(model[2]).all().item())}
        del blocks, model
    rs = np.random.RandomState(2)
    qu, qi = to(rs.randint(0, ts.n_users, a.queries), torch.int32), to(rs.randint(0, ts.n_items, a.queries), torch.int32)
    times = []
    for n in range(2 + a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        svd.estimate_batch(algo.mu, True, algo.bu, algo.bi, algo.pu, algo.qi, qu, qi)
        e1.record()
        torch.cuda.synchronize()
        if n >= 2:
            times.append(e0.elapsed_time(e1))
    res["queries"] = a.queries
    res["estimate_ms"] = [statistics.median(times), min(times), max(times)]
    if a.numpy_ratings:
        import svd_reference as S
        m = min(a.numpy_ratings, ts.n_ratings)
        par = S.params(n_factors=a.factors)
        t0 = time.perf_counter()
        S.fit(ts.u[:m], ts.i[:m], ts.r[:m], ts.n_users, ts.n_items, par, 1, 1)
        res["numpy_ratings"] = m
        res["numpy_updates_per_s"] = m / (time.perf_counter() - t0)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
