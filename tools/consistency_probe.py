#!/usr/bin/env python3
"""Timing of the eccentricity consistency analysis (n2v_hip.consistency).  Timing only.

    python tools/consistency_probe.py [--shape ml1m|30music] [--n 7] [--bins 100] [--runs 7] [--warmup 2] [--host]

Shapes (synthetic rows of the data sets' sizes, power-law items, 24 time windows cut into two halves, integer raw ids):
    ml1m      1 000 209 rows,  6 040 users,     3 706 items        (MovieLens-1M)
    30music   3 * 10^7  rows, 40 000 users, 5 * 10^6 items
Method: one run is consistency.transitions (upload, two period statistics, three joins, marks and tables, download) and
one is consistency.user_ie_profile, each from host arrays to host arrays, wall clock around a synchronised call.  Medians of
--runs runs after --warmup warm-ups.  --host alternates every device run with the numpy restatement
(tests/consistency_reference.py) on one core of this host as the yardstick and reports its medians and whether the tables
are equal.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "node2vec-by-ecc_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"ml1m": (1000209, 6040, 3706), "30music": (30000000, 40000, 5000000)}
FIRST, SECOND = (201301, 201312), (201401, 201412)


def make_rows(shape, seed=0):
    n_rows, n_users, n_items = SHAPES[shape]
    rs = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, n_items + 1) ** 0.8
    cdf = np.cumsum(pop / pop.sum())
    item = np.minimum(np.searchsorted(cdf, rs.random_sample(n_rows)), n_items - 1).astype(np.int64)
    user = rs.randint(0, n_users, size=n_rows).astype(np.int64)
    fb = rs.randint(1, 11, size=n_rows) * 0.5
    month = rs.randint(0, 24, size=n_rows)
    return user + 1, item + 1, fb, (2013 + month // 12) * 100 + month % 12 + 1


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml1m", choices=sorted(SHAPES))
    ap.add_argument("--n", type=int, default=7)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args(argv)
    import torch
    from n2v_hip import consistency as C
    assert torch.cuda.is_available(), "needs a GPU"
    uid, iid, fb, tw = make_rows(a.shape)
    print("rows ready", file=sys.stderr, flush=True)

    def device_transitions():
        res = C.transitions(uid, iid, fb, tw, FIRST, SECOND, n=a.n)
        torch.cuda.synchronize()
        return res

    def device_profile():
        res = C.user_ie_profile(uid, iid, fb, tw, n_bins=a.bins)
        torch.cuda.synchronize()
        return res

    t_dev, p_dev, t_host, p_host, equal = [], [], [], [], True
    for it in range(a.warmup + a.runs):
        res, t = timed(device_transitions)
        prof, p = timed(device_profile)
        print("run %d: transitions %.1f ms, profile %.1f ms" % (it, t, p), file=sys.stderr, flush=True)
        if it >= a.warmup:
            t_dev.append(t)
            p_dev.append(p)
        if a.host and it >= a.warmup:
            import consistency_reference as R
            want, t = timed(lambda: R.transitions(uid.tolist(), iid.tolist(), fb, tw, FIRST, SECOND, n=a.n))
            hprof, p = timed(lambda: R.user_ie_profile(uid.tolist(), iid.tolist(), fb, tw, a.bins))
            print("host %d: transitions %.1f ms, profile %.1f ms" % (it, t, p), file=sys.stderr, flush=True)
            t_host.append(t)
            p_host.append(p)
            equal = equal and all(np.array_equal(getattr(res, k).count, want[k]["count"]) for k in C.KINDS) \
                and R.canon(prof.profile) == R.canon(hprof[3])
    out = {"shape": a.shape, "rows": len(fb), "n": a.n, "bins": a.bins, "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "transitions_ms": float(np.median(t_dev)), "profile_ms": float(np.median(p_dev)),
           "joined": {k: len(getattr(res, k).ids) for k in C.KINDS},
           "transitions_ms_all": [round(x, 1) for x in t_dev], "profile_ms_all": [round(x, 1) for x in p_dev]}
    if a.host:
        out.update(host_transitions_ms=float(np.median(t_host)), host_profile_ms=float(np.median(p_host)), host_equal=bool(equal))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
