"""Timing probe of the fused top-N kernels (n2v_hip.eccknn.top_n, n2v_hip.svd.top_n) against the stored path, on the
synthetic MovieLens-1M-shaped set of tools/eccknn_probe.py.  Timing only: what the kernels compute is the business of
tests/test_gpu_topn.py (the probe still asserts that the two paths return the same lists).

    python tools/topn_probe.py [--users 6040 --items 3706 --ratings 1000000 --k 40 --n 10 --factors 100 --repeats 7]
                               [--models user,item,mf] [--segments S]
    python tools/topn_probe.py --big [--big-users 40000 --big-items 500000 --big-ratings 3000000 --budget-s 20]

The stored path is built only from calls that exist without the fused kernels: every (user, item) pair through
estimate_batch + predict, the pairs of the training set masked, and one stable device sort per user under the same order.
Each model prints one JSON line: medians (min, max) in ms of `repeats` timed runs after two warm-up runs, the two paths
alternating, each run bracketed by device events; the query arrays of the stored path are built outside the timed region,
its estimate / predict / sort stages are also timed apart, and `stored_bytes` is what it keeps on the device per run.

--big   one shape the stored path cannot hold: the power-law generator of eccknn_probe's 30music-users shape, user-based
        cosine with the sparse-form similarity.  The run first times 2 048 owners (enough wavefronts to fill the device),
        estimates the time of all of them from that rate, and then ranks as many owners as fit --budget-s (all of them
        when they do); it prints both numbers.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "node2vec-by-ecc_amd"), os.path.join(ROOT, "tools")]
CALIBRATION_OWNERS = 2048


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def summary(ms):
    return [statistics.median(ms), min(ms), max(ms)]


def stored_lists(pred, seen_mask, n):
    """The n best unseen items per row of the stored predictions: a stable ascending sort of the negated rows."""
    import torch
    neg = torch.where(seen_mask, torch.full_like(pred, float("inf")), -pred)
    val, idx = torch.sort(neg, dim=1, stable=True)
    val, idx = val[:, :n], idx[:, :n]
    none = torch.isinf(val)
    return (torch.where(none, torch.full_like(idx, -1), idx).to(torch.int32),
            torch.where(none, torch.full_like(val, float("nan")), -val))


def same_lists(a, b):
    import torch
    real = a[0] >= 0
    return bool(torch.equal(a[0], b[0])) and bool(torch.equal(a[1][real], b[1][real]))


def compare(name, fused, estimate, predict, seen_mask, n, repeats, extra):
    """Alternates the fused call and the stored path; returns the JSON record."""
    import torch
    t = {"fused": [], "stored": [], "stored_estimate": [], "stored_predict": [], "stored_sort": []}
    for rep in range(2 + repeats):
        ms_f, got = event_ms(fused)
        ms_e, est = event_ms(estimate)
        ms_p, pred = event_ms(lambda: predict(est).view(seen_mask.shape))
        ms_s, want = event_ms(lambda: stored_lists(pred, seen_mask, n))
        if rep == 0:
            assert same_lists(got, want), "%s: the fused lists differ from the stored path's" % name
            extra["stored_bytes"] = int(sum(x.numel() * x.element_size() for x in est) + pred.numel() * 8)
        if rep >= 2:
            for key, ms in (("fused", ms_f), ("stored", ms_e + ms_p + ms_s), ("stored_estimate", ms_e),
                            ("stored_predict", ms_p), ("stored_sort", ms_s)):
                t[key].append(ms)
        del est, pred, want, got
    rec = {"metric": "topn_probe", "model": name, "device": torch.cuda.get_device_name(0), "repeats": repeats, "lists_equal": True}
    rec.update(extra)
    rec.update({k + "_ms": summary(v) for k, v in t.items()})
    rec["fused_over_stored"] = rec["fused_ms"][0] / rec["stored_ms"][0]
    print(json.dumps(rec), flush=True)
    return rec


def ml1m(a):
    import torch
    from eccknn_probe import synthetic
    from n2v_hip import _lib, eccknn, svd
    u, i, r = synthetic(a.users, a.items, a.ratings, 0)
    ts = eccknn.Trainset.from_ratings(u.tolist(), i.tolist(), r)
    dev = torch.device("cuda:0")
    to = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v)).to(device=dev, dtype=dt)
    du, di, dr = to(ts.u, torch.int32), to(ts.i, torch.int32), to(ts.r, torch.float64)
    seen = eccknn.csr_by_x(du, di, dr, ts.n_users, ts.n_items)
    seen_mask = torch.zeros((ts.n_users, ts.n_items), dtype=torch.bool, device=dev)
    seen_mask[du.long(), di.long()] = True
    qu = torch.arange(ts.n_users, dtype=torch.int32, device=dev).repeat_interleave(ts.n_items)
    qi = torch.arange(ts.n_items, dtype=torch.int32, device=dev).repeat(ts.n_users)
    shape = {"n_users": ts.n_users, "n_items": ts.n_items, "ratings": len(r), "n": a.n, "pairs": ts.n_users * ts.n_items,
             "segments": a.segments or int(_lib.load().n2v_topn_segments(ts.n_users, ts.n_items))}
    out = []
    for model in a.models.split(","):
        if model in ("user", "item"):
            user_based = model == "user"
            w = np.random.RandomState(1).normal(size=ts.n_items if user_based else ts.n_users)
            algo = eccknn.EccenKNN(k=a.k, sim_options={"name": "cosine", "user_based": user_based}, device="cuda:0").fit(ts, w)
            qx, qy = (qu, qi) if user_based else (qi, qu)
            fused = lambda: eccknn.top_n(algo.sim, algo.yr, seen, user_based, a.k, 1, ts.global_mean, ts.rating_scale, a.n,
                                         None, a.segments)
            estimate = lambda: eccknn.estimate_batch(algo.sim, algo.yr, qx, qy, a.k, 1)
            predict = lambda est: eccknn.predict(est[0], est[2], ts.global_mean, ts.rating_scale)
            out.append(compare(model + "-based cosine k-NN", fused, estimate, predict, seen_mask, a.n, a.repeats, dict(shape, k=a.k)))
            del algo
        elif model == "mf":
            algo = svd.SVD(n_factors=a.factors, n_epochs=2, device="cuda:0").fit(ts)
            fused = lambda: svd.top_n(algo.mu, True, algo.bu, algo.bi, algo.pu, algo.qi, seen, ts.global_mean, ts.rating_scale,
                                      a.n, None, a.segments)
            estimate = lambda: svd.estimate_batch(algo.mu, True, algo.bu, algo.bi, algo.pu, algo.qi, qu, qi)
            predict = lambda est: eccknn.predict(est[0], est[1], ts.global_mean, ts.rating_scale)
            out.append(compare("mf", fused, estimate, predict, seen_mask, a.n, a.repeats, dict(shape, factors=a.factors)))
        else:
            raise SystemExit("--models: user, item or mf, not %r" % model)
        torch.cuda.empty_cache()
    return out


def big(a):
    """A shape whose predictions cannot be stored: n_users x n_items pairs at about 25 B each."""
    import torch
    from eccknn_probe import synthetic_30music
    from n2v_hip import eccknn
    n_users, n_items = a.big_users, a.big_items
    u, i, r = synthetic_30music(n_users, n_items, a.big_ratings, 0)
    dev = torch.device("cuda:0")
    to = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v)).to(device=dev, dtype=dt)
    du, di, dr = to(u, torch.int32), to(i, torch.int32), to(r, torch.float64)
    dw = to(np.random.RandomState(1).normal(size=n_items), torch.float64)
    rec = {"metric": "topn_probe", "model": "user-based cosine k-NN, sparse-form similarity", "n_users": n_users,
           "n_items": n_items, "ratings": len(r), "k": a.k, "n": a.n, "pairs": n_users * n_items,
           "stored_path_bytes": n_users * n_items * 25, "device": torch.cuda.get_device_name(0)}
    seen = eccknn.csr_by_x(du, di, dr, n_users, n_items)
    rec["similarity_ms"], sim = event_ms(lambda: eccknn.similarity_sparse(seen, dw, n_items, "cosine"))
    yr = eccknn.csr_by_x(di, du, dr, n_items, n_users)           # the raters of every item (here ascending, not in training order)
    mean, scale = float(r.mean()), (float(r.min()), float(r.max()))
    owners = torch.as_tensor(np.random.RandomState(2).permutation(n_users).astype(np.int32)).to(dev)
    run = lambda m: eccknn.top_n(sim, yr, seen, True, a.k, 1, mean, scale, a.n, owners[:m])
    c = min(CALIBRATION_OWNERS, n_users)
    run(c)
    ms_c, _ = event_ms(lambda: run(c))
    rec["calibration_owners"], rec["calibration_ms"] = c, ms_c
    rec["estimate_all_owners_s"] = ms_c * 1e-3 * n_users / c
    m = int(min(n_users, max(c, a.budget_s / (ms_c * 1e-3) * c)))
    torch.cuda.reset_peak_memory_stats()
    ms, (items, score) = event_ms(lambda: run(m))
    rec.update(owners_ranked=m, fused_ms=ms, pairs_ranked=m * n_items, pairs_per_s=m * n_items / (ms * 1e-3),
               peak_device_bytes=int(torch.cuda.max_memory_allocated()),
               full_lists=bool((items >= 0).all().item()), ties_at_hi=float((score == scale[1]).double().mean().item()))
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--ratings", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--factors", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--models", default="user,item,mf")
    ap.add_argument("--segments", type=int, default=None)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--big-users", type=int, default=40000)
    ap.add_argument("--big-items", type=int, default=500000)
    ap.add_argument("--big-ratings", type=int, default=3000000)
    ap.add_argument("--budget-s", type=float, default=20.0)
    a = ap.parse_args(argv)
    return big(a) if a.big else ml1m(a)


if __name__ == "__main__":
    main()
