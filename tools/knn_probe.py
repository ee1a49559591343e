"""Timing of the nearest-neighbour paths (n2v_hip/neighbors.py): all-pairs self k-NN through the fused kernel
(csrc/n2v_knn.hip) against the stored-block path (n2v_sim_block + n2v_sim_rows_topk, both exports older than the fused
kernel) in one process, runs alternating, and one most_similar query.  Timing only: it is not a test.

    python tools/knn_probe.py [--shapes 799000x100,100000x128] [--k 10] [--reps 7 --warmup 2] [--paths fused,block]

Defaults: the song2vec vocabulary shape (7.99e5 words, d = 100 -> dpad 128), then 1e5 x 128.  Prints the median, the spread (min .. max)
and the rate 2 n^2 dpad / t of every path; the f32 MFMA peak of an MI355X is 155 TFLOP/s."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node2vec-by-ecc_amd"))
import numpy as np
import torch

from n2v_hip import neighbors
from n2v_hip.word2vec import LabelKeyedVectors


def run(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def report(name, times, flops=None):
    med = statistics.median(times)
    rate = "" if flops is None else "  %.1f TFLOP/s (%.0f%% of 155)" % (flops / med / 1e12, flops / med / 1.55e12)
    print("%-28s median %.4fs  min %.4fs  max %.4fs  (%d runs)%s" % (name, med, min(times), max(times), len(times), rate), flush=True)
    return med


def probe(n, d, a):
    paths = a.paths.split(",")
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.randn(256, d, device="cuda", generator=g)
    x = centres[torch.randint(0, 256, (n,), device="cuda", generator=g)] + 0.8 * torch.randn(n, d, device="cuda", generator=g)
    dpad = -(-d // 32) * 32
    flops = 2.0 * n * n * dpad
    print("all-pairs self k-NN: n = %d, d = %d (dpad %d), k = %d, %s" % (n, d, dpad, a.k, torch.cuda.get_device_name(0)), flush=True)
    times = {path: [] for path in paths}
    out = {}
    for rep in range(a.warmup + a.reps):
        for path in paths:                              # alternating: both paths see the same machine state
            dt, out[path] = run(lambda: neighbors.knn(x, a.k, path=path))
            if rep >= a.warmup:
                times[path].append(dt)
    med = {path: report("knn path=%s" % path, times[path], flops) for path in paths}
    if len(paths) == 2:
        (i0, s0), (i1, s1) = out[paths[0]], out[paths[1]]
        print("paths agree: idx %s, scores %s; %s / %s = %.3f" % (
            bool(torch.equal(i0, i1)), bool(torch.equal(torch.nan_to_num(s0, nan=-9.0), torch.nan_to_num(s1, nan=-9.0))),
            paths[0], paths[1], med[paths[0]] / med[paths[1]]), flush=True)
    kv = LabelKeyedVectors(np.arange(n), np.ones(n), x.cpu().numpy())
    dt, _ = run(lambda: kv.init_sims())
    print("init_sims (upload + prepare): %.4fs" % dt, flush=True)
    t = []
    for rep in range(a.warmup + a.reps):
        dt, res = run(lambda: kv.most_similar(positive=[17, 4242 % n], negative=[99], topn=10))
        if rep >= a.warmup:
            t.append(dt)
    report("most_similar, topn=10", t)
    print("   ->", res[:3], flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="799000x100,100000x128", help="comma-separated NxD")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--paths", default="fused,block")
    a = p.parse_args()
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.lower().split("x"))
        probe(n, d, a)


if __name__ == "__main__":
    main()
