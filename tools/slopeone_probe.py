"""Timing probe of the SlopeOne path (n2v_hip.slopeone) on the synthetic MovieLens-1M-shaped set of tools/eccknn_probe.py.
Timing only: what the kernels compute is the business of tests/test_gpu_slopeone.py (the probe still asserts that the two
forms of the table and the two top-N paths agree).

    python tools/slopeone_probe.py [--users 6040 --items 3706 --ratings 1000000 --queries 200000 --n 10 --repeats 7]
                                   [--cache-items 5600] [--restatement-users 60]

Prints one JSON line per stage: medians (min, max) in ms of `repeats` timed runs after two warm-up runs, the paths of a
stage alternating run by run, each run bracketed by device events.
  fit      the deviation table, dense (densify + kernel) and sparse (sort + CSR check + kernel), beside the item-based msd
           similarity of eccknn on the same data and in the same two forms: the same frame with a heavier accumulator, so
           it is the fit's yardstick.  `useful_updates` is the sum over users of |ur[u]|^2, what surprise's loop performs.
  estimate `queries` random (user, item) pairs through n2v_slopeone_estimate.
  topn     the fused top-n lists of all users against the stored path (all-pairs estimate_batch + predict + a stable
           device sort, as tools/topn_probe.py builds it).  `table_bytes` is dev + freq; `traffic_bytes` the bound the time
           is compared with, rows read x 12 B x n_items = ratings x n_items x 12 B (every rated item of every user
           contributes its whole row of dev and freq once); `effective_TBps` = traffic_bytes / fused time.  A rate above
           what HBM sustains (about 6 TB/s on an MI355X) can only come from the last-level cache.
  --cache-items M   repeats the fused top-n at M items (0: skip), a table past the 256 MiB last-level cache, with the same
           users and ratings: the drop of effective_TBps between the two shapes is the cache's share.
  --restatement-users K   the plain-Python restatement's fit on the first K users on one core, as pair updates per second.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "node2vec-by-ecc_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]


def timed_round_robin(fns, repeats, warmup=2):
    """{name: [median, min, max]} in ms of calls that alternate run by run."""
    import torch
    out = {name: [] for name in fns}
    for n in range(warmup + repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if n >= warmup:
                out[name].append(a.elapsed_time(b))
    return {name: [statistics.median(v), min(v), max(v)] for name, v in out.items()}


def setup(n_users, n_items, n_ratings):
    import torch
    from eccknn_probe import synthetic
    from n2v_hip import eccknn
    u, i, r = synthetic(n_users, n_items, n_ratings, 0)
    ts = eccknn.Trainset.from_ratings(u.tolist(), i.tolist(), r)
    dev = torch.device("cuda:0")
    to = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v)).to(device=dev, dtype=dt)
    return ts, (to(ts.u, torch.int32), to(ts.i, torch.int32), to(ts.r, torch.float64))


def fit_stage(a, ts, d, base):
    import torch
    from n2v_hip import eccknn, slopeone
    du, di, dr = d
    ones = torch.ones(ts.n_users, dtype=torch.float64, device=du.device)
    slope_dense = lambda: slopeone.deviations(*eccknn.densify(di, du, dr, ts.n_items, ts.n_users))
    slope_sparse = lambda: slopeone.deviations_sparse(eccknn.csr_by_x(di, du, dr, ts.n_items, ts.n_users), ts.n_users)
    msd_dense = lambda: eccknn.similarity(*eccknn.densify(di, du, dr, ts.n_items, ts.n_users), ones, "msd")
    msd_sparse = lambda: eccknn.similarity_sparse(eccknn.csr_by_x(di, du, dr, ts.n_items, ts.n_users), ones, ts.n_users, "msd")
    (d0, f0), (d1, f1) = slope_dense(), slope_sparse()
    assert torch.equal(f0, f1) and torch.equal(d0.view(torch.int64), d1.view(torch.int64)), "dense and sparse tables differ"
    del d0, f0, d1, f1
    t = timed_round_robin({"slope_dense": slope_dense, "slope_sparse": slope_sparse, "msd_dense": msd_dense,
                           "msd_sparse": msd_sparse}, a.repeats)
    useful = int((np.diff(ts.ur[0]).astype(np.int64) ** 2).sum())
    rec = dict(base, metric="slopeone_probe", stage="fit", forms_equal=True, useful_updates=useful)
    rec.update({k + "_ms": v for k, v in t.items()})
    rec["useful_updates_per_s"] = useful / (t["slope_dense"][0] * 1e-3)
    print(json.dumps(rec), flush=True)


def estimate_stage(a, ts, algo, base):
    import torch
    from n2v_hip import slopeone
    rs = np.random.RandomState(1)
    to = lambda v: torch.as_tensor(v).to(device=algo.dev.device, dtype=torch.int32)
    qu, qi = to(rs.randint(0, ts.n_users, a.queries)), to(rs.randint(0, ts.n_items, a.queries))
    t = timed_round_robin({"estimate": lambda: slopeone.estimate_batch(algo.dev, algo.freq, algo.ur, algo.user_mean, qu, qi,
                                                                       check=False)}, a.repeats)
    print(json.dumps(dict(base, metric="slopeone_probe", stage="estimate", queries=a.queries, estimate_ms=t["estimate"])), flush=True)


def topn_stage(a, ts, d, algo, base, stored=True):
    import torch
    from topn_probe import compare
    from n2v_hip import eccknn, slopeone
    du, di, dr = d
    dev = du.device
    seen = algo._seen()
    fused = lambda: slopeone.top_n(algo.dev, algo.freq, algo.ur, algo.user_mean, seen, ts.global_mean, ts.rating_scale, a.n,
                                   None, None, check=False)
    table = algo.dev.numel() * 12
    traffic = len(ts.r) * ts.n_items * 12
    extra = dict(base, stage="topn", n=a.n, pairs=ts.n_users * ts.n_items, table_bytes=table, traffic_bytes=traffic)
    if stored:
        seen_mask = torch.zeros((ts.n_users, ts.n_items), dtype=torch.bool, device=dev)
        seen_mask[du.long(), di.long()] = True
        qu = torch.arange(ts.n_users, dtype=torch.int32, device=dev).repeat_interleave(ts.n_items)
        qi = torch.arange(ts.n_items, dtype=torch.int32, device=dev).repeat(ts.n_users)
        estimate = lambda: slopeone.estimate_batch(algo.dev, algo.freq, algo.ur, algo.user_mean, qu, qi, check=False)
        predict = lambda est: eccknn.predict(est[0], est[2], ts.global_mean, ts.rating_scale)
        rec = compare("slopeone", fused, estimate, predict, seen_mask, a.n, a.repeats, extra)
        ms = rec["fused_ms"][0]
    else:
        t = timed_round_robin({"fused": fused}, a.repeats)
        ms = t["fused"][0]
        print(json.dumps(dict(extra, metric="slopeone_probe", fused_ms=t["fused"])), flush=True)
    print(json.dumps(dict(base, metric="slopeone_probe", stage="topn_traffic", table_bytes=table, traffic_bytes=traffic,
                          fused_ms=ms, effective_TBps=traffic / (ms * 1e-3) / 1e12)), flush=True)


def restatement_stage(a, ts, base):
    import slopeone_reference as S
    keep = ts.u < a.restatement_users
    t0 = time.perf_counter()
    model = S.fit(ts.u[keep], ts.i[keep], ts.r[keep], a.restatement_users, ts.n_items)
    s = time.perf_counter() - t0
    updates = int(sum(len(lst) ** 2 for lst in model["ur"]))
    print(json.dumps(dict(base, metric="slopeone_probe", stage="restatement", users=a.restatement_users, seconds=s,
                          pair_updates=updates, pair_updates_per_s=updates / s)), flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--users", type=int, default=6040)
    p.add_argument("--items", type=int, default=3706)
    p.add_argument("--ratings", type=int, default=1000000)
    p.add_argument("--queries", type=int, default=200000)
    p.add_argument("--n", type=int, default=10)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--cache-items", dest="cache_items", type=int, default=5600)
    p.add_argument("--restatement-users", dest="restatement_users", type=int, default=60)
    a = p.parse_args(argv)
    import torch
    from n2v_hip import slopeone
    ts, d = setup(a.users, a.items, a.ratings)
    base = {"device": torch.cuda.get_device_name(0), "n_users": ts.n_users, "n_items": ts.n_items, "ratings": len(ts.r),
            "repeats": a.repeats}
    fit_stage(a, ts, d, base)
    algo = slopeone.SlopeOne(device="cuda:0").fit(ts)
    estimate_stage(a, ts, algo, base)
    topn_stage(a, ts, d, algo, base)
    if a.restatement_users:
        restatement_stage(a, ts, base)
    if a.cache_items:
        del algo
        torch.cuda.empty_cache()
        ts, d = setup(a.users, a.cache_items, a.ratings)
        base.update(n_users=ts.n_users, n_items=ts.n_items, ratings=len(ts.r))
        algo = slopeone.SlopeOne(device="cuda:0").fit(ts)
        topn_stage(a, ts, d, algo, base, stored=False)


if __name__ == "__main__":
    main(sys.argv[1:])
