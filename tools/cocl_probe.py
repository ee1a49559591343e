"""Timing probe of the CoClustering path (n2v_hip.coclustering) on a synthetic MovieLens-1M-shaped set.  Timing only: what
the kernels compute is the business of tests/test_gpu_coclustering.py.

    python tools/cocl_probe.py [--users 6040 --items 3706 --ratings 1000000 --clusters 3x3,64x64]
                               [--repeats 7 --queries 200000 --numpy-ratings 20000]

Prints one JSON line.  Every figure is the median / min / max over `repeats` runs after two warm-ups, bracketed by device
events.  `lists_ms`: what a fit does apart from its epochs, once: both lists to the device, their checks, the two means and
the two row order tables.  Per cluster count: `averages_ms`, `user_pass_ms`, `item_pass_ms` and `epoch_ms` (the three
together, as coclustering.epoch runs them), `identity_order_ms` (the epoch with the rows handed out in id order instead of
longest first) and rating updates per second (an epoch visits every rating once per side; `updates_per_s` counts ratings).
`nmf_epoch_ms`: one NMF epoch at 15 factors on the same lists, the yardstick: the same frame, one sequential chain per row.
`longest_list` is the longest row of either side; `chain_ns_per_entry` = the slower pass / longest_list is what one entry
of that wavefront's chain would cost if the chain alone set the pass time; `longest_user_row_alone_ms` is the user pass
over the longest user list as a problem of that one row: where it is close to `user_pass_ms`, the pass sits at the bound of
its longest row and packing several rows into a wavefront has nothing to win.  `estimate_ms`: `queries` estimates.
`topn_fused_ms` / `topn_stored_ms`: the top-10 lists of all users by the fused kernel, and by estimate_batch over all pairs
+ predict + a mask + torch.topk.  Then the numpy restatement's rating updates per second on one core over the first
`numpy-ratings` ratings (0 skips it).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "node2vec-by-ecc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def timed(fn, repeats, warmup=2):
    import torch
    times = []
    for n in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if n >= warmup:
            times.append(e0.elapsed_time(e1))
    return [statistics.median(times), min(times), max(times)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--ratings", type=int, default=1000000)
    ap.add_argument("--clusters", default="3x3,64x64")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--queries", type=int, default=200000)
    ap.add_argument("--numpy-ratings", type=int, default=20000)
    a = ap.parse_args(argv)
    import torch
    from n2v_hip import coclustering as cc, eccknn, nmf
    from svd_probe import synthetic
    if not torch.cuda.is_available():
        raise RuntimeError("cocl_probe: no GPU visible; a timing needs the device")
    u, i, r = synthetic(a.users, a.items, a.ratings, 0)
    ts = eccknn.Trainset.from_ratings(u.tolist(), i.tolist(), r)
    dev = torch.device("cuda:0")
    box = {}

    def build():
        ur, ir = eccknn._csr_to_device(ts.ur, dev), eccknn._csr_to_device(ts.ir, dev)
        eccknn.yr_check(ur, ts.n_items)
        eccknn.yr_check(ir, ts.n_users)
        box.update(ur=ur, ir=ir, um=eccknn.row_moments(ur[0], ur[2])[0], im=eccknn.row_moments(ir[0], ir[2])[0],
                   order=(nmf.row_order(ur[0]), nmf.row_order(ir[0])))

    longest = int(max(np.diff(ts.ur[0]).max(), np.diff(ts.ir[0]).max()))
    res = {"metric": "cocl_probe", "device": torch.cuda.get_device_name(0), "n_users": ts.n_users, "n_items": ts.n_items,
           "ratings": ts.n_ratings, "repeats": a.repeats, "lists_ms": timed(build, a.repeats), "longest_list": longest,
           "clusters": {}}
    ur, ir, um, im, order = (box[k] for k in ("ur", "ir", "um", "im", "order"))
    rs = np.random.RandomState(0)
    for spec in a.clusters.split(","):
        n_cu, n_ci = (int(v) for v in spec.split("x"))
        cu = torch.as_tensor(rs.randint(n_cu, size=ts.n_users)).to(device=dev, dtype=torch.int32)
        ci = torch.as_tensor(rs.randint(n_ci, size=ts.n_items)).to(device=dev, dtype=torch.int32)
        args = (ur, ir, cu, ci, n_cu, n_ci, ts.global_mean, um, im)
        avgs = cc.averages(ur, ts.n_items, cu, ci, n_cu, n_ci, ts.global_mean, check=False)
        entry = {"averages_ms": timed(lambda: cc.averages(ur, ts.n_items, cu, ci, n_cu, n_ci, ts.global_mean, check=False), a.repeats),
                 "user_pass_ms": timed(lambda: cc.assign(ur, True, cu, ci, avgs, um, im, order[0], check=False), a.repeats),
                 "item_pass_ms": timed(lambda: cc.assign(ir, False, cu, ci, avgs, um, im, order[1], check=False), a.repeats),
                 "identity_order_ms": timed(lambda: cc.epoch(*args, check=False), a.repeats),
                 "epoch_ms": timed(lambda: cc.epoch(*args, order=order, check=False), a.repeats)}
        # the longest user list as a problem of one row: what its wavefront alone costs, launch included
        k = int(np.diff(ts.ur[0]).argmax())
        b, e = int(ts.ur[0][k]), int(ts.ur[0][k + 1])
        one = (torch.tensor([0, e - b], dtype=torch.int64, device=dev), ur[1][b:e].contiguous(), ur[2][b:e].contiguous())
        cu1, um1 = cu[k:k + 1].clone(), um[k:k + 1].clone()
        entry["longest_user_list"] = e - b
        entry["longest_user_row_alone_ms"] = timed(lambda: cc.assign(one, True, cu1, ci, avgs, um1, im, check=False), a.repeats)
        entry["updates_per_s"] = ts.n_ratings / (entry["epoch_ms"][0] * 1e-3)
        entry["chain_ns_per_entry"] = max(entry["user_pass_ms"][0], entry["item_pass_ms"][0]) * 1e6 / longest
        res["clusters"][spec] = entry
    # the yardstick: an NMF epoch at 15 factors on the same ratings
    lists = nmf.lists(ur, ts.n_users, ts.n_items)
    algo = nmf.NMF(n_factors=15, n_epochs=0, device=dev).fit(ts)
    tabs = [algo.pu, algo.qi, torch.empty_like(algo.pu), torch.empty_like(algo.qi)]

    def nmf_epoch():
        nmf.epoch(lists, algo.reg_pu, algo.reg_qi, *tabs)
        tabs[0], tabs[1], tabs[2], tabs[3] = tabs[2], tabs[3], tabs[0], tabs[1]

    res["nmf_epoch_ms"] = timed(nmf_epoch, a.repeats)
    for spec, entry in res["clusters"].items():
        entry["epoch_over_nmf_epoch"] = entry["epoch_ms"][0] / res["nmf_epoch_ms"][0]
    # estimates and lists of a fitted default model
    model = cc.CoClustering(n_epochs=2, device=dev).fit(ts)
    qu = torch.as_tensor(rs.randint(-1, ts.n_users, size=a.queries)).to(device=dev, dtype=torch.int32)
    qi = torch.as_tensor(rs.randint(-1, ts.n_items, size=a.queries)).to(device=dev, dtype=torch.int32)
    res["queries"] = a.queries
    res["estimate_ms"] = timed(lambda: model._estimate_batch(qu, qi), a.repeats)
    seen = model._seen()
    res["topn_fused_ms"] = timed(lambda: model.top_n_lists(10), a.repeats)
    all_u = torch.arange(ts.n_users, dtype=torch.int32, device=dev).repeat_interleave(ts.n_items)
    all_i = torch.arange(ts.n_items, dtype=torch.int32, device=dev).repeat(ts.n_users)
    rows = torch.arange(ts.n_users, device=dev).repeat_interleave(seen[0][1:] - seen[0][:-1])

    def stored():
        est, imp = model._estimate_batch(all_u, all_i)
        pred = eccknn.predict(est, imp, ts.global_mean, ts.rating_scale).view(ts.n_users, ts.n_items)
        pred[rows, seen[1].long()] = -float("inf")
        return torch.topk(pred, 10, dim=1)

    res["topn_stored_ms"] = timed(stored, a.repeats)
    if a.numpy_ratings:
        import coclustering_reference as C
        m = min(a.numpy_ratings, ts.n_ratings)
        t0 = time.perf_counter()
        C.fit(ts.u[:m], ts.i[:m], ts.r[:m], ts.n_users, ts.n_items, C.params(n_epochs=1))
        res["numpy_ratings"] = m
        res["numpy_updates_per_s"] = m / (time.perf_counter() - t0)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
