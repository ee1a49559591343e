"""Timing of the top-N recommendation path (n2v_hip/recommend.py, csrc/n2v_rec.hip) on one MI355X.

  python tools/rec_probe.py [--config5] [--compare] [--reps N]

--compare   20 000 users x 100 000 items, d = 128, top 10: the largest shape whose 16 GB score matrix the earlier path
            (library fp64 GEMM + torch.topk, tables already on the device) holds comfortably.  Both paths, and the GEMM
            alone, are timed interleaved in one process with device events after a warm-up; medians are printed.
--config5   one evaluation at BASELINE config-5 shape: 500 000 users x 500 000 items, d = 256, top 10 (2 TB of scores if
            they were stored; there is nothing to compare with).
One JSON line per measurement.  Timing only: nothing here checks results (tests/test_gpu_rec.py does)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node2vec-by-ecc_amd"))

import torch  # noqa: E402

from n2v_hip import recommend as rec  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    del out
    return a.elapsed_time(b)


def tables(n_u, n_v, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    emb = torch.randn((n_u + n_v, d), dtype=torch.float64, device="cuda", generator=g)
    u_idx = torch.arange(n_u, dtype=torch.int32, device="cuda")
    v_idx = torch.arange(n_u, n_u + n_v, dtype=torch.int32, device="cuda")
    return emb, u_idx, v_idx


def report(name, n_u, n_v, d, ms, **extra):
    flop = 2.0 * n_u * n_v * d
    med = statistics.median(ms)
    print(json.dumps(dict(what=name, users=n_u, items=n_v, d=d, ms_median=round(med, 3), ms_min=round(min(ms), 3),
                          ms_max=round(max(ms), 3), reps=len(ms), fp64_tflops=round(flop / med / 1e9, 2), **extra)), flush=True)


def compare(reps, top_n=10):
    n_u, n_v, d = 20_000, 100_000, 128
    emb, u_idx, v_idx = tables(n_u, n_v, d, 1)
    A, B = emb[:n_u], emb[n_u:]
    new = lambda: rec.top_n_lists(emb, d, u_idx, v_idx, top_n)
    gemm = lambda: A @ B.T
    old = lambda: torch.topk(A @ B.T, top_n, dim=1).indices
    for fn in (new, gemm, old):                                    # warm-up of every timed shape
        timed(fn)
    t = {"new": [], "gemm": [], "old": []}
    for _ in range(reps):                                          # interleaved
        t["new"].append(timed(new))
        t["gemm"].append(timed(gemm))
        t["old"].append(timed(old))
    report("fused score + top-n (this library)", n_u, n_v, d, t["new"], segments=int(rec._lib.load().n2v_bine_rec_segments(n_u, n_v)))
    report("library fp64 GEMM alone", n_u, n_v, d, t["gemm"])
    report("library fp64 GEMM + torch.topk (earlier path)", n_u, n_v, d, t["old"])


def config5(reps, top_n=10):
    n_u, n_v, d = 500_000, 500_000, 256
    emb, u_idx, v_idx = tables(n_u, n_v, d, 2)
    ms = [timed(lambda: rec.top_n_lists(emb, d, u_idx, v_idx, top_n)) for _ in range(reps)]
    report("fused score + top-n, config-5 shape", n_u, n_v, d, ms)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--config5", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rec_probe: no GPU visible; timings are taken on the device only")
    if a.compare or not a.config5:
        compare(a.reps)
    if a.config5:
        config5(1)      # seconds per evaluation; the kernel is warm when --compare ran first
