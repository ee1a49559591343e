"""TEST INFRASTRUCTURE — numpy restatement of the CBOW kernel of csrc/n2v_cbow.hip (``cbow_kernel``), driven by the
kernel's own deterministic schedule, which is the skip-gram kernel's: hash32 sub-sampling and window shrink, the
per-sentence 48-bit LCG of the negative draws and the job-wise learning rate (tests/sgns_reference.py).  Rows are
float64, every target of a centre is applied in order; the sigmoid-table bin and the gradient are evaluated in float32
exactly as the kernel does.  ``near_edge`` counts sigmoid evaluations whose f lies within rel_delta * |neu1| . |row| of
a point where the float32 bin changes.

One sentence on one wavefront runs this algorithm exactly, so tests/test_gpu_cbow.py pins the kernel to it at fp32
rounding.  The product never imports this file.

The `variant` argument plants ONE deliberate error (tests/test_cbow_host.py measures how far each moves the tables,
to show that the GPU tolerance separates a correct kernel from each of them)."""
import numpy as np

from sgns_reference import (M64, Stats, _gradient, centre_window, draw, effective_sentence, exp_table, hash32,  # noqa: F401
                            lcg_seed, lcg_skip, lcg_step, mix64, walk_alpha)

VARIANTS = ("reversed_sum", "no_inv", "inv_wrong_branch", "stale_repeat", "dup_once", "window_off_by_one",
            "draw_without_context")


def train(syn0, syn1neg, tokens, offsets, *, window, negative, cbow_mean, alpha, min_alpha, sample_int, cum_table, seed,
          sentence_id_base, sentences_base, sentences_step, sentences_total, alpha_batch, stats=None, variant=None):
    """One launch over the CSR corpus on float64 syn0 / syn1neg, in place.  Sentence s has id sentence_id_base + s and
    hashes its tokens by their position in the sentence.  -> (centres trained, Stats)."""
    assert variant is None or variant in VARIANTS
    stats = stats or Stats()
    tokens, offsets = np.asarray(tokens), np.asarray(offsets)
    cum = [int(c) for c in np.asarray(cum_table)] if cum_table is not None else []
    seed &= M64
    for s in range(len(offsets) - 1):
        raw = tokens[offsets[s]:offsets[s + 1]]
        sid = sentence_id_base + s
        sent = effective_sentence(raw, len(raw), sample_int, seed, sid)
        a = walk_alpha(alpha, min_alpha, sentences_base, sentences_step, sentences_total, alpha_batch, s)
        lcg = lcg_seed(seed, sid)
        for i in range(len(sent)):
            win = centre_window(seed, sid, i, len(sent), window + (variant == "window_off_by_one"))
            if win is None:
                if variant == "draw_without_context":
                    for _ in range(negative):
                        lcg = lcg_step(lcg)
                continue
            lo, hi = win
            ci = sent[i]
            ctx = [sent[m] for m in range(lo, hi) if m != i]
            inv = float(np.float32(1.0) / np.float32(len(ctx)))
            neu1 = np.zeros(syn0.shape[1])
            for x in (reversed(ctx) if variant == "reversed_sum" else ctx):
                neu1 += syn0[x]
            mean_branch = bool(cbow_mean) != (variant == "inv_wrong_branch")
            if mean_branch and variant != "no_inv":
                neu1 *= inv
            work = np.zeros_like(neu1)
            group, seen = [ci], {}
            for d in range(negative + 1):
                if d == 0:
                    t, label = ci, 1.0
                else:
                    t, label = draw(lcg, cum), 0.0
                    lcg = lcg_step(lcg)
                    group.append(t if t != ci else -1)
                    if d % 8 == 7 or d == negative:      # the kernel's groups: slots 0..7, 8..15, ...
                        live = [x for x in group if x >= 0]
                        stats.groups += 1
                        stats.repeat_groups += len(set(live)) < len(live)
                        group = []
                    if t == ci:
                        stats.centre_draws = getattr(stats, "centre_draws", 0) + 1
                        continue
                row = syn1neg[t]
                if variant == "stale_repeat":            # every draw of a centre sees the row as the centre found it
                    row = seen.setdefault(t, syn1neg[t].copy())
                f = float(np.dot(neu1, row))
                g = _gradient(f, float(np.abs(neu1) @ np.abs(row)), label, a, stats)
                if g != 0.0:
                    work += g * row
                    syn1neg[t] += g * neu1
            if negative == 0:
                stats.groups += 1
            if not mean_branch and variant != "no_inv":
                work *= inv
            for x in (set(ctx) if variant == "dup_once" else ctx):
                syn0[x] += work
            stats.pairs += 1
    return stats.pairs, stats
