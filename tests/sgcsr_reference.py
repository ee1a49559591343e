"""TEST INFRASTRUCTURE — numpy restatement of the ragged skip-gram kernel of csrc/n2v_sgns_csr.hip (``sgns_csr_kernel``),
built from the primitives of tests/sgns_reference.py (imported unchanged): ``effective_sentence``, ``centre_window``,
``lcg_seed`` / ``lcg_skip``, ``_update``, ``walk_alpha``.  It trains a CSR corpus ITEM BY ITEM in float64, as the kernel
deals it out: with ``chunk == 0`` an item is a sentence; with ``chunk >= 1`` sentence s of n_s raw tokens has
S_s = ceil(n_s / chunk) items and item sp trains the effective centres [sp * n_eff / S_s, (sp + 1) * n_eff / S_s) from a
STAGED copy of the effective tokens [i_begin - window, i_end + window) & [0, n_eff), with the sentence's LCG skipped by
pairs_before * negative.  Items trained in order are the whole sentence trained by ``sgns_reference.train``, bit for bit
(tests/test_sgcsr_host.py).  The product never imports this file.

The `variant` argument plants ONE deliberate error of the kind the chunked design invites."""
import numpy as np

import sgns_reference as R

VARIANTS = ("clip_context", "skip_without_negative", "raw_split_bounds", "alpha_per_item")


def item_table(offsets, chunk):
    """Brute force: the items of a corpus in order, as (sentence, split, splits of the sentence)."""
    out = []
    for s in range(len(offsets) - 1):
        n = int(offsets[s + 1] - offsets[s])
        S = 1 if chunk == 0 else -(-n // chunk)
        out.extend((s, sp, S) for sp in range(S))
    return out


def item_bounds(n_eff, sp, S):
    return sp * n_eff // S, (sp + 1) * n_eff // S


def train_item(syn0, syn1neg, raw, s, sp, S, item, *, window, negative, alpha, min_alpha, sample_int, cum, seed,
               sentence_id_base, sentences_base, sentences_step, sentences_total, alpha_batch, stats, variant=None):
    """Item (s, sp) of S of the sentence with raw tokens `raw`; `item` is its number in the corpus (only the planted
    alpha error looks at it)."""
    sid = sentence_id_base + s
    sent = R.effective_sentence(raw, len(raw), sample_int, seed, sid)
    n_eff = len(sent)
    i_begin, i_end = item_bounds(n_eff, sp, S)
    if variant == "raw_split_bounds":
        i_begin, i_end = (min(n_eff, x) for x in item_bounds(len(raw), sp, S))
    a = R.walk_alpha(alpha, min_alpha, sentences_base, sentences_step, sentences_total, alpha_batch,
                     item if variant == "alpha_per_item" else s)
    pairs_before = 0
    for i in range(i_begin):
        win = R.centre_window(seed, sid, i, n_eff, window)
        if win is not None:
            pairs_before += win[1] - win[0] - 1
    lcg = R.lcg_skip(R.lcg_seed(seed, sid), pairs_before * (1 if variant == "skip_without_negative" else negative))
    # the wave's LDS slot: only these tokens exist for the item
    w_lo, w_hi = max(0, i_begin - window), min(n_eff, i_end + window)
    staged = sent[w_lo:w_hi]
    for i in range(i_begin, i_end):
        win = R.centre_window(seed, sid, i, n_eff, window)
        if win is None:
            continue
        lo, hi = win
        if variant == "clip_context":
            lo, hi = max(lo, i_begin), min(hi, i_end)
        ci = staged[i - w_lo]
        for j in range(lo, hi):
            if j == i:
                continue
            xj = staged[j - w_lo]
            h = syn0[xj].copy()
            work = np.zeros_like(h)
            R._update(syn1neg[ci], h, 1.0, a, work, stats)
            group = [ci]
            for d in range(1, negative + 1):
                t = R.draw(lcg, cum)
                lcg = R.lcg_step(lcg)
                if t != ci:
                    R._update(syn1neg[t], h, 0.0, a, work, stats)
                group.append(t if t != ci else -1)
                if d % 8 == 7 or d == negative:      # the kernel's groups: slots 0..7, 8..15, ...
                    live = [x for x in group if x >= 0]
                    stats.groups += 1
                    stats.repeat_groups += len(set(live)) < len(live)
                    group = []
            if negative == 0:
                stats.groups += 1
            syn0[xj] += work
            stats.pairs += 1


def train(syn0, syn1neg, tokens, offsets, chunk, *, window, negative, alpha, min_alpha, sample_int, cum_table, seed,
          sentence_id_base, sentences_base, sentences_step, sentences_total, alpha_batch, first_item=0, n_items=None,
          stats=None, variant=None):
    """The items [first_item, first_item + n_items) of the CSR corpus (default: all), in order, on float64 syn0 /
    syn1neg in place.  Sentence s has id sentence_id_base + s and job s // alpha_batch.  -> (pairs trained, Stats)."""
    assert variant is None or variant in VARIANTS
    stats = stats or R.Stats()
    tokens, offsets = np.asarray(tokens), np.asarray(offsets)
    cum = [int(c) for c in np.asarray(cum_table)] if cum_table is not None else []
    seed &= R.M64
    items = item_table(offsets, chunk)
    last = len(items) if n_items is None else first_item + n_items
    for item in range(first_item, last):
        s, sp, S = items[item]
        train_item(syn0, syn1neg, tokens[offsets[s]:offsets[s + 1]], s, sp, S, item, window=window, negative=negative,
                   alpha=alpha, min_alpha=min_alpha, sample_int=sample_int, cum=cum, seed=seed,
                   sentence_id_base=sentence_id_base, sentences_base=sentences_base, sentences_step=sentences_step,
                   sentences_total=sentences_total, alpha_batch=alpha_batch, stats=stats, variant=variant)
    return stats.pairs, stats
