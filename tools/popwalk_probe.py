"""Popularity-biased walk rates on C3 (timing only; the walks themselves are pinned by tests/test_gpu_popwalk.py).

  1. precomputed mode: preprocess_transition_probs() against preprocess_transition_probs_popularity() (the extra cost is one
     more node-table launch and its fat expansion), and the walk rate over either table set (same kernel, same table sizes);
  2. on the fly: n2v_walk_on_the_fly_pop against n2v_walk_on_the_fly on the SAME graph with explicit fp64 weights (the plain
     rule's non-dyadic path, which sums and pairs in full as the pop rule must) — and, for scale, the unweighted dyadic path.

Usage: python tools/popwalk_probe.py [--config C3] [--otf-walks 200000] [--reps 3]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node2vec-by-ecc_amd"))
import numpy as np
import torch

import node2vec
from n2v_hip import csr, synth


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return r, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--otf-walks", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-precomputed", action="store_true")
    a = ap.parse_args()
    cg, info = synth.make_config_graph(a.config)
    L = 80
    if not a.skip_precomputed:
        g = node2vec.Graph.from_csr(cg, 0.25, 4.0, device="cuda:0", rng="philox", seed=1)
        for name, pre in (("plain", g.preprocess_transition_probs), ("popularity", g.preprocess_transition_probs_popularity),
                          ("plain", g.preprocess_transition_probs), ("popularity", g.preprocess_transition_probs_popularity)):
            _, tp = timed(pre, 1)
            c, tw = timed(lambda: g.simulate_walks(2, L), a.reps)
            steps = float((c.lens.long() - 1).sum())
            print("%s precomputed %-10s preprocess %.3f s   walk %s steps/s (each of %d runs)" % (
                a.config, name, tp[0], " ".join("%.3e" % (steps / t) for t in tw), a.reps), flush=True)
            del c
        del g
        torch.cuda.empty_cache()
    rs = np.random.RandomState(1)
    wcg = csr.CsrGraph(cg.labels, cg.row_ptr, cg.col, None, cg.start_order, cg.directed)
    # symmetric fp64 weights in (0.25, 4.25): w(u, v) == w(v, u), from the unordered pair
    su = wcg.src_of().astype(np.int64)
    lo, hi = np.minimum(su, wcg.col), np.maximum(su, wcg.col)
    wcg.w = 0.25 + 4.0 * (((lo * 2654435761 + hi * 40503) % 1000003) / 1000003.0)
    for name, graph, pop in (("plain rule, fp64 weights (w != NULL)", wcg, False), ("pop rule,   fp64 weights (w != NULL)", wcg, True),
                             ("plain rule, unweighted (dyadic count)", cg, False), ("pop rule,   unweighted", cg, True)):
        eng = node2vec.WalkEngine(graph, 0.25, 4.0, device="cuda:0")
        sub = eng.start_order[:a.otf_walks].contiguous()
        (w, l), ts = timed(lambda: eng.walk_on_the_fly(sub, 1, L, rng="philox", seed=1, pop=pop), a.reps)
        steps = float((l.long() - 1).sum())
        print("%s on the fly, %s: %d walks x %d: %s steps/s" % (a.config, name, int(sub.numel()), L,
                                                               " ".join("%.3e" % (steps / t) for t in ts)), flush=True)
        del eng


if __name__ == "__main__":
    main()
