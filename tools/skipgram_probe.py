"""Timing probe of the ragged skip-gram trainer (n2v_hip.skipgram over a n2v_hip.corpus.SentenceCorpus).  Timing only:
what the kernel computes is the business of tests/test_gpu_sgcsr.py.

    python tools/skipgram_probe.py [--shape 30music|small] [--tail 64] [--chunks 0,64,256,1024] [--min-count 5]
                                   [--size 100 --window 5 --negative 5] [--repeats 5]

The corpus is tools/cbow_probe.py's synthetic playlist corpus (30Music layout, playlists of geometric length with mean
11) with a planted tail: --tail sentences of 4 096 tokens drawn from the same track popularity, spread over the corpus.
For every chunk (0 = one wavefront per whole sentence, LDS slot max_len) one JSON line: the median (min, max) in ms
over `repeats` event-timed passes after two warm-up passes, the pairs per epoch and per second.  A last line names the
best chunk, the spread seen and whether "auto" (n2v_hip.skipgram.AUTO_CHUNK) is within that spread of it.  The passes
keep training the same tables (the timing does not depend on their values).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "node2vec-by-ecc_amd"), os.path.join(ROOT, "tools")]


def with_tail(ids, off, n_tail, items, seed, device):
    """Append n_tail sentences of 4 096 tokens, then move them to evenly spaced places among the others."""
    import torch
    if n_tail <= 0:
        return ids, off
    g = torch.Generator(device=device)
    g.manual_seed(seed + 1)
    pop = 1.0 / torch.arange(1, items + 1, dtype=torch.float64, device=device) ** 0.9
    cdf = torch.cumsum(pop, 0)
    extra = torch.searchsorted(cdf, torch.rand(n_tail * 4096, dtype=torch.float64, device=device, generator=g) * cdf[-1])
    extra = torch.clamp(extra, max=items - 1)
    lens = off[1:] - off[:-1]
    S = int(lens.numel())
    where = torch.linspace(0, S, n_tail + 2, device=device)[1:-1].long()         # the tail sentence k goes before `where[k]`
    all_lens = torch.cat([lens, torch.full((n_tail,), 4096, dtype=torch.int64, device=device)])
    key = torch.cat([torch.arange(S, device=device) * 2 + 1, where * 2])
    order = torch.argsort(key, stable=True)
    src_off = torch.cat([off[:-1], off[-1] + torch.arange(n_tail, device=device) * 4096])
    new_lens = all_lens[order]
    new_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=device), torch.cumsum(new_lens, 0)])
    flat = torch.cat([ids, extra])
    owner = torch.repeat_interleave(torch.arange(order.numel(), device=device), new_lens)
    pos = torch.arange(int(new_off[-1].item()), device=device) - new_off[:-1][owner]
    return flat[src_off[order][owner] + pos], new_off


def main(argv=None):
    from cbow_probe import SHAPES, synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="30music", choices=sorted(SHAPES))
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--items", type=int, default=None)
    ap.add_argument("--mean-length", dest="mean_length", type=float, default=None)
    ap.add_argument("--tail", type=int, default=64, help="planted sentences of 4 096 tokens")
    ap.add_argument("--chunks", default="0,64,256,1024")
    ap.add_argument("--min-count", dest="min_count", type=int, default=5)
    ap.add_argument("--size", type=int, default=100)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args(argv)
    shape = dict(SHAPES[a.shape])
    shape.update({k: getattr(a, k) for k in ("rows", "items", "mean_length") if getattr(a, k) is not None})
    chunks = [int(x) for x in a.chunks.split(",")]
    import torch
    from n2v_hip import skipgram
    from n2v_hip.corpus import SentenceCorpus
    dev = torch.device("cuda:0")
    ids, off = synthetic(seed=0, device=dev, **shape)
    ids, off = with_tail(ids, off, a.tail, shape["items"], 0, dev)
    corpus = SentenceCorpus.from_ids(np.arange(shape["items"]), ids, off, a.min_count)
    del ids
    model = skipgram.SkipGramModel(len(corpus.labels), dim=a.size, window=a.window, negative=a.negative, device=dev)
    model.build_vocab(corpus.counts)
    S = corpus.n_sentences
    batch = skipgram.default_alpha_batch(corpus)
    lens = corpus.offsets[1:] - corpus.offsets[:-1]
    common = {"metric": "skipgram_probe", "device": torch.cuda.get_device_name(0), "shape": a.shape, "events": shape["rows"],
              "tail": a.tail, "sentences": S, "tokens_kept": corpus.n_tokens, "words_kept": len(corpus.labels),
              "max_len": corpus.max_len, "sentences_over_256": int((lens > 256).sum().item()), "size": a.size,
              "window": a.window, "negative": a.negative, "repeats": a.repeats}
    medians, spreads = {}, {}
    n_pass = 0
    total = len(chunks) * (2 + a.repeats)
    for chunk in chunks:
        times, pairs = [], []
        for n in range(2 + a.repeats):
            before = model.pairs_trained()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            model.train_pass(corpus, sentences_base=n_pass * S, sentences_total=total * S, sentence_id_base=n_pass * S,
                             alpha_batch=batch, chunk=chunk)
            t1.record()
            torch.cuda.synchronize()
            n_pass += 1
            if n >= 2:
                times.append(t0.elapsed_time(t1))
                pairs.append(model.pairs_trained() - before)
        med = statistics.median(times)
        medians[chunk], spreads[chunk] = med, (max(times) - min(times)) / med
        print(json.dumps(dict(common, chunk=chunk, items=skipgram.n_items(corpus, chunk), epoch_ms=[med, min(times), max(times)],
                              pairs_per_epoch=int(statistics.median(pairs)), pairs_per_s=statistics.median(pairs) / (med * 1e-3))),
              flush=True)
    assert torch.isfinite(model.syn0).all()
    best = min(medians, key=medians.get)
    spread = max(spreads.values())
    auto = skipgram.resolve_chunk(corpus, "auto")
    res = {"metric": "skipgram_probe_summary", "best_chunk": best, "best_ms": medians[best], "auto_chunk": auto,
           "auto_ms": medians.get(auto), "largest_relative_spread": spread,
           "auto_within_spread_of_best": (None if auto not in medians else medians[auto] <= medians[best] * (1 + spread))}
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
