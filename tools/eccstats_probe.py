"""Timing probe of the eccentricity statistics (n2v_hip.eccstats).  Timing only: what the kernels compute is the business
of tests/test_gpu_eccstats.py.

    python tools/eccstats_probe.py [--shape ml1m|30music] [--rows N --users N --items N --windows N] [--repeats 7]
                                   [--numpy-rows 2000000]

ml1m:    1 000 209 rows, 6 040 users, 3 706 items, power-law items, timestamps over 36 months (cut by timewindow_utc).
30music: 3e7 rows, 4e4 users, 5e6 items, power-law items and users, 12 windows, repeated (user, item) rows allowed.
Prints one JSON line: medians (min, max) in ms over `repeats` event-timed runs after two warm-ups of the torch sorts
(`sort_ms`: unique of the windows, three stable sorts, two CSR pointers) and of the HIP kernels with the log table
(`kernels_ms`, which holds one read-back of two counts and the table's upload); the per-item segment sums on their own and
the same call on the longest item alone (`longest_segment_ms`: one wavefront's serial chain); and the vectorised
restatement's time on one core for the first --numpy-rows rows (all of them when the set is smaller; 0 skips it).
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

SHAPES = {"ml1m": dict(rows=1000209, users=6040, items=3706, windows=36, user_power=0.0),
          "30music": dict(rows=30000000, users=40000, items=5000000, windows=12, user_power=0.6)}


def synthetic(rows, users, items, windows, user_power, seed):
    rs = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, items + 1) ** 0.9
    i = rs.choice(items, size=rows, p=pop / pop.sum())
    act = 1.0 / np.arange(1, users + 1) ** user_power
    u = rs.choice(users, size=rows, p=act / act.sum())
    return u.astype(np.int64), i.astype(np.int64), rs.randint(1, 11, size=rows) * 0.5, rs.randint(0, windows, size=rows)


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
    ap.add_argument("--shape", default="ml1m", choices=sorted(SHAPES))
    for k in ("rows", "users", "items", "windows"):
        ap.add_argument("--" + k, type=int, default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-rows", type=int, default=2000000)
    a = ap.parse_args(argv)
    shape = dict(SHAPES[a.shape])
    shape.update({k: getattr(a, k) for k in ("rows", "users", "items", "windows") if getattr(a, k) is not None})
    import torch
    from n2v_hip import eccstats as S
    u, i, fb, w = synthetic(seed=0, **shape)
    if a.shape == "ml1m":                                        # timestamps, cut into UTC months
        tw = S.timewindow_utc(946684800 + w.astype(np.int64) * 2629800 + 86400)
    else:
        tw = 201401 + w.astype(np.int64)
    iu, users = S.first_appearance(u)
    ii, items = S.first_appearance(i)
    dev = torch.device("cuda:0")
    du, di, dfb, dtw = (torch.from_numpy(v).to(dev) for v in (iu, ii, fb, tw))
    n_u, n_i = len(users), len(items)
    res = {"metric": "eccstats_probe", "device": torch.cuda.get_device_name(0), "shape": a.shape, "rows": len(fb),
           "users": n_u, "items": n_i, "repeats": a.repeats}
    res["sort_ms"] = timed(lambda: (S.prepare(du, di, dtw, n_i), S._csr_ptr(du, n_u), S._csr_ptr(di, n_i)), a.repeats)
    prep = S.prepare(du, di, dtw, n_i)
    res["kernels_ms"] = timed(lambda: S.device_statistics(du, di, dfb, prep, n_u, n_i), a.repeats)
    cols, _ = S.device_statistics(du, di, dfb, prep, n_u, n_i)
    res["groups"] = int(cols["unum"].numel())
    res["largest_group"] = int(cols["unum"].max().item())
    ptr = S._csr_ptr(di, n_i)
    du32 = du.to(torch.int32)
    res["item_segsum_ms"] = timed(lambda: S.segsum(ptr, dfb, perm=prep[4], idx=du32, g=cols["ue"]), a.repeats)
    lens = ptr[1:] - ptr[:-1]
    top = int(lens.argmax().item())
    one = ptr[top:top + 2].contiguous()
    res["longest_segment_rows"] = int(lens[top].item())
    res["longest_segment_ms"] = timed(lambda: S.segsum(one, dfb, perm=prep[4], idx=du32, g=cols["ue"]), a.repeats)
    if a.numpy_rows:
        import eccstats_reference as R
        m = min(a.numpy_rows, len(fb))
        t0 = time.perf_counter()
        R.statistics_numpy(u[:m], i[:m], fb[:m], tw[:m])
        res["numpy_rows"] = m
        res["numpy_one_core_s"] = time.perf_counter() - t0
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
