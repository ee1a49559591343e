"""Timing probe of the CBOW trainer (n2v_hip.cbow over a n2v_hip.corpus.SentenceCorpus).  Timing only: what the kernel
computes is the business of tests/test_gpu_cbow.py.

    python tools/cbow_probe.py [--shape 30music|small] [--rows N --items N --mean-length X] [--min-count 5]
                               [--size 100 --window 5 --negative 5] [--repeats 5]

A synthetic playlist corpus in the 30Music layout tools/eccstats_probe.py --shape 30music uses (3e7 events over 5e6
tracks, power-law track popularity 1 / rank^0.9) cut into playlists of geometric length (mean 11: 3e7 events in 2.7e6
sessions), at least 2 and at most 4096 tracks; pruned by --min-count like song2vec.  Prints one JSON line: the corpus
after pruning, and the median (min, max) in ms over `repeats` event-timed passes after two warm-up passes, with the
centres trained per second that the median implies.  The passes keep training the same tables (the timing does not
depend on their values).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "node2vec-by-ecc_amd")]

SHAPES = {"30music": dict(rows=30000000, items=5000000, mean_length=11.0),
          "small": dict(rows=3000000, items=500000, mean_length=11.0)}


def synthetic(rows, items, mean_length, seed, device):
    """-> (ids int64[T], offsets int64[S + 1]) on the device."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    pop = 1.0 / torch.arange(1, items + 1, dtype=torch.float64, device=device) ** 0.9
    cdf = torch.cumsum(pop, 0)
    ids = torch.searchsorted(cdf, torch.rand(rows, dtype=torch.float64, device=device, generator=g) * cdf[-1])
    ids = torch.clamp(ids, max=items - 1)
    n_sessions = int(rows / mean_length * 1.2) + 16
    p = 1.0 / max(mean_length - 1.0, 1.0)                     # length = 2 + Geometric(p): mean 2 + (1 - p) / p
    u = torch.rand(n_sessions, dtype=torch.float64, device=device, generator=g)
    lens = 2 + torch.floor(torch.log1p(-u) / np.log1p(-p)).long()
    lens = torch.clamp(lens, max=4096)
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=device), torch.cumsum(lens, 0)])
    off = off[off <= rows]
    return ids[:int(off[-1].item())], off


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30music", choices=sorted(SHAPES))
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--items", type=int, default=None)
    ap.add_argument("--mean-length", dest="mean_length", type=float, default=None)
    ap.add_argument("--min-count", dest="min_count", type=int, default=5)
    ap.add_argument("--size", type=int, default=100)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args(argv)
    shape = dict(SHAPES[a.shape])
    shape.update({k: getattr(a, k) for k in ("rows", "items", "mean_length") if getattr(a, k) is not None})
    import torch
    from n2v_hip import cbow
    from n2v_hip.corpus import SentenceCorpus
    dev = torch.device("cuda:0")
    ids, off = synthetic(seed=0, device=dev, **shape)
    corpus = SentenceCorpus.from_ids(np.arange(shape["items"]), ids, off, a.min_count)
    del ids
    model = cbow.CbowModel(len(corpus.labels), dim=a.size, window=a.window, negative=a.negative, device=dev)
    model.build_vocab(corpus.counts)
    S = corpus.n_sentences
    batch = cbow.default_alpha_batch(corpus)
    times, centres = [], []
    for n in range(2 + a.repeats):
        before = model.pairs_trained()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        model.train_pass(corpus, sentences_base=n * S, sentences_total=(2 + a.repeats) * S, sentence_id_base=n * S,
                         alpha_batch=batch)
        t1.record()
        torch.cuda.synchronize()
        if n >= 2:
            times.append(t0.elapsed_time(t1))
            centres.append(model.pairs_trained() - before)
    med = statistics.median(times)
    res = {"metric": "cbow_probe", "device": torch.cuda.get_device_name(0), "shape": a.shape, "events": shape["rows"],
           "sentences": S, "tokens_kept": corpus.n_tokens, "words_kept": len(corpus.labels), "max_len": corpus.max_len,
           "size": a.size, "window": a.window, "negative": a.negative, "repeats": a.repeats,
           "epoch_ms": [med, min(times), max(times)], "centres_per_epoch": int(statistics.median(centres)),
           "centres_per_s": statistics.median(centres) / (med * 1e-3)}
    assert torch.isfinite(model.syn0).all()
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
