"""Timing probe of the NMF path (n2v_hip.nmf) on a synthetic MovieLens-1M-shaped set.  Timing only: what the kernels
compute is the business of tests/test_gpu_nmf.py.

    python tools/nmf_probe.py [--users 6040 --items 3706 --ratings 1000000 --factors 15,64,256]
                              [--repeats 7 --numpy-ratings 20000]

Prints one JSON line.  `lists_ms`: what a fit does apart from its epochs, once: the item-major list (one stable sort on
the device), the list check and the two row order tables.  Per n_factors: the median / min / max over `repeats` epochs
after two warm-up epochs, each epoch bracketed by device events, as ms per epoch and rating updates per second (an epoch
updates with every rating twice, once per side; `updates_per_s` counts ratings, not sides); `identity_order_ms` is the
same with the rows handed out in id order instead of longest first.  Then the numpy restatement's rating updates per
second on one core over the first `numpy-ratings` ratings (0 skips it).

Two figures to hold the epoch time against.  `row_read_bytes` = 2 * ratings * n_factors * 8: every rating reads one row
of the other table on each side, if nothing is cached; `hbm_bound_ms` is that over 8 TB/s (AMD's published MI355X
figure).  `longest_list` is the length of the longest row on either side: its wavefront is a serial chain of that many
dependent steps (lane butterfly, then the fp64 add into den), and `chain_ns_per_entry` = epoch time / longest_list is
what one step of it would cost if that chain alone set the epoch time.
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

HBM_BYTES_PER_S = 8e12


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
    ap.add_argument("--factors", default="15,64,256")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-ratings", type=int, default=20000)
    a = ap.parse_args(argv)
    import torch
    from n2v_hip import eccknn, nmf
    from svd_probe import synthetic
    if not torch.cuda.is_available():
        raise RuntimeError("nmf_probe: no GPU visible; a timing needs the device")
    u, i, r = synthetic(a.users, a.items, a.ratings, 0)
    ts = eccknn.Trainset.from_ratings(u.tolist(), i.tolist(), r)
    dev = torch.device("cuda:0")
    to = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v)).to(device=dev, dtype=dt)
    ur = to(ts.ur[0], torch.int64), to(ts.ur[1], torch.int32), to(ts.ur[2], torch.float64)
    box = {}

    def build():
        box["lists"] = nmf.lists(ur, ts.n_users, ts.n_items)

    longest = int(max(np.diff(ts.ur[0]).max(), np.diff(ts.ir[0]).max()))
    res = {"metric": "nmf_probe", "device": torch.cuda.get_device_name(0), "n_users": ts.n_users, "n_items": ts.n_items,
           "ratings": ts.n_ratings, "repeats": a.repeats, "lists_ms": timed(build, a.repeats), "longest_list": longest,
           "factors": {}}
    lists, plain = box["lists"], nmf.lists(ur, ts.n_users, ts.n_items, order="identity")
    for nf in [int(v) for v in a.factors.split(",")]:
        algo = nmf.NMF(n_factors=nf, n_epochs=0, device=dev).fit(ts)                      # the initial tables
        tabs = [algo.pu, algo.qi, torch.empty_like(algo.pu), torch.empty_like(algo.qi)]

        def one(which):
            nmf.epoch(which, algo.reg_pu, algo.reg_qi, *tabs)
            tabs[0], tabs[1], tabs[2], tabs[3] = tabs[2], tabs[3], tabs[0], tabs[1]

        ms = timed(lambda: one(lists), a.repeats)
        ident = timed(lambda: one(plain), a.repeats)
        row_bytes = 2 * ts.n_ratings * nf * 8
        res["factors"][str(nf)] = {"epoch_ms": ms, "identity_order_ms": ident, "updates_per_s": ts.n_ratings / (ms[0] * 1e-3),
                                   "row_read_bytes": row_bytes, "hbm_bound_ms": row_bytes / HBM_BYTES_PER_S * 1e3,
                                   "chain_ns_per_entry": ms[0] * 1e6 / longest,
                                   "finite": bool(torch.isfinite(tabs[0]).all().item())}
    if a.numpy_ratings:
        import nmf_reference as N
        m = min(a.numpy_ratings, ts.n_ratings)
        par = N.params(n_factors=15)
        t0 = time.perf_counter()
        N.fit(ts.u[:m], ts.i[:m], ts.r[:m], ts.n_users, ts.n_items, par, 1)
        res["numpy_ratings"] = m
        res["numpy_updates_per_s"] = m / (time.perf_counter() - t0)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
