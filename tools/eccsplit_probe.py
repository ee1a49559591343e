#!/usr/bin/env python3
"""Timing of the eccentricity split (n2v_hip.eccsplit): ue -> n bins -> n + 1 CSR graphs on the device.  Timing only.

    python tools/eccsplit_probe.py [--shape ml1m|30music] [--n 10] [--runs 7] [--warmup 2] [--host]

Shapes (synthetic rows of the data sets' sizes, power-law items, 12 time windows):
    ml1m      1 000 209 rows,  6 040 users,     3 706 items        (MovieLens-1M)
    30music   3 * 10^7  rows, 40 000 users, 5 * 10^6 items        (one row per user, item and time window)
Method: the rows, ue and the names are on the device already (the state n2v_hip.eccstats leaves); one run is mark_n plus
the n + 1 graphs, each downloaded.  Medians of --runs event-timed runs after --warmup warm-ups.  The sorts (torch) are
timed apart by events around each of them, and so are the downloads of the finished graphs (to pageable host memory);
"kernels" is the rest: the HIP passes and the two count readbacks per graph.
--host adds the reference-speed line: the same split by the numpy restatement (tests/eccsplit_reference.py) plus
csr.from_edges per graph on one core of this host, timed once.
Prints one JSON line.
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


def make_rows(shape, seed=0):
    n_rows, n_users, n_items = SHAPES[shape]
    rs = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, n_items + 1) ** 0.8
    cdf = np.cumsum(pop / pop.sum())
    item = np.minimum(np.searchsorted(cdf, rs.random_sample(n_rows)), n_items - 1).astype(np.int64)
    user = rs.randint(0, n_users, size=n_rows).astype(np.int64)
    user[:n_users], item[:n_items] = np.arange(n_users), np.arange(n_items)        # every id appears: inner ids as they are
    fb = rs.randint(1, 11, size=n_rows) * 0.5
    ue = rs.normal(size=n_users)
    user_names = np.arange(1, n_users + 1, dtype=np.int64)
    item_names = np.array([int("9999999%d" % i) for i in range(1, n_items + 1)], dtype=np.int64)
    return user, item, fb, ue, user_names, item_names


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml1m", choices=sorted(SHAPES))
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args(argv)
    import torch
    from n2v_hip import eccsplit
    assert torch.cuda.is_available(), "needs a GPU"
    user, item, fb, ue, user_names, item_names = make_rows(a.shape)
    dev = torch.device("cuda:0")
    to = lambda x: torch.from_numpy(x).to(dev)
    du, di, dw, dun, dit, due = to(user), to(item), to(fb), to(user_names), to(item_names), to(ue)
    tie_rank = np.arange(len(ue), dtype=np.int64)
    sort_events = []
    plain_sort = eccsplit._sort

    def timed_sort(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = plain_sort(*args, **kw)
        e1.record()
        sort_events.append((e0, e1))
        return out

    eccsplit._sort = timed_sort
    copy_events = []
    plain_download = eccsplit._download

    def timed_download(t):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = plain_download(t)
        e1.record()
        copy_events.append((e0, e1))
        return out

    eccsplit._download = timed_download

    def run():
        bins = eccsplit._mark_device(due, a.n, tie_rank)
        graphs = []
        for k in range(a.n + 1):
            counts = torch.zeros(3, dtype=torch.int64, device=dev)
            rows = eccsplit._select(du, bins, k, counts)
            graphs.append(eccsplit._graph(du, di, dw, dun, dit, rows, len(fb), counts))
        return bins, graphs

    total, sorts, copies = [], [], []
    print("rows ready", file=sys.stderr, flush=True)
    for it in range(a.warmup + a.runs):
        del sort_events[:]
        del copy_events[:]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        bins, graphs = run()
        e1.record()
        torch.cuda.synchronize()
        print("run %d: %.1f ms" % (it, e0.elapsed_time(e1)), file=sys.stderr, flush=True)
        if it >= a.warmup:
            total.append(e0.elapsed_time(e1))
            sorts.append(sum(x.elapsed_time(y) for x, y in sort_events))
            copies.append(sum(x.elapsed_time(y) for x, y in copy_events))
    out = {"shape": a.shape, "rows": len(fb), "users": len(ue), "items": len(item_names), "n": a.n, "runs": a.runs,
           "device": torch.cuda.get_device_name(0), "total_ms": float(np.median(total)), "sorts_ms": float(np.median(sorts)),
           "download_ms": float(np.median(copies)),
           "kernels_ms": float(np.median(np.array(total) - np.array(sorts) - np.array(copies))),
           "download_bytes": int(sum(g.labels.nbytes + g.row_ptr.nbytes + g.col.nbytes + g.w.nbytes + g.start_order.nbytes for g in graphs)), "total_ms_all": [round(x, 3) for x in total],
           "nnz": [int(g.nnz) for g in graphs]}
    if a.host:
        import eccsplit_reference as R
        from n2v_hip import csr
        t0 = time.perf_counter()
        hbins = R.mark_n(ue, a.n, tie_rank)
        hgraphs = []
        for k in range(a.n + 1):
            r = R.rows_of_bin(user, hbins, k)
            hgraphs.append(csr.from_edges(user_names[user[r]], item_names[item[r]], fb[r], directed=False))
            print("host graph %d of %d: %.1f s" % (k, a.n, time.perf_counter() - t0), file=sys.stderr, flush=True)
        out["host_ms"] = (time.perf_counter() - t0) * 1e3
        out["host_equal"] = bool(np.array_equal(hbins, bins.cpu().numpy()) and all(
            np.array_equal(x.col, y.col) and np.array_equal(x.row_ptr, y.row_ptr) and x.w.tobytes() == y.w.tobytes()
            for x, y in zip(hgraphs, graphs)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
