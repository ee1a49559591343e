"""TEST INFRASTRUCTURE — the counting tables and corpora of tests/test_gpu_w2v_ledger.py, shared with
tests/test_ledger_host.py, which proves the instrument on the CPU before a GPU sees it.

Racing wavefronts (many sentences on shared rows, walk_splits > 1, chunk > 0) leave tables that depend on the order the
hardware happened to run, so the tables cannot be pinned.  The multiset of trained EVENTS can: start the tables so that
every gradient is a constant and every update lands in a cell of its own, and the result is a sum, which has no order.

Counting tables, n_words <= dim - 1, all fp32:

    syn0[x]    = A * e_{dim-1}                  for every word x
    syn1neg[t] = C * e_t + B * e_{dim-1}

A * B = 0.006 ~ 0.5 / 83 is the middle of bin 498 of the sigmoid table (f in [0, 1/83)), and the learning rate is so
small (2^-16 ... 2^-17) that f never leaves it.  Every (context x, target t, label) event of skip-gram then adds
(label - table[498]) * alpha_sentence * C to the cell syn0[x][t]; in CBOW every context of the centre receives it
(divided by the context count with cbow_mean=0, where the bin is a function of that count).  The order of the events
changes a cell only at second order, through the slow drift of column dim-1.  The block syn0[:, :n_words] is therefore
a LEDGER of what was trained, with which draws and at which sentence's learning rate, whichever wavefront did it.  The
sequential restatements (sgns_reference.train, sgcsr_reference.train, cbow_reference.train) are the reference as they
stand.  Column dim-1 and syn1neg are order-dependent at the 1 % ... 80 %-of-an-event level and are not compared.

TOLERANCE, in events per ledger cell, absolute.  event_size = table[498] * min_alpha * C is the smallest change one
skip-gram event can make (a negative draw at the last job's learning rate; a positive one is 0.506 / 0.494 of it).
  * a missing, extra or misplaced skip-gram or cbow_mean=1 event moves a cell by >= 1 event; with cbow_mean=0 by
    >= 1 / (2 * window) = 0.1 event;
  * fp32 accumulation of N adds into a cell of at most N * (alpha / min_alpha) events errs by at most
    N^2 * 2^-24 * alpha / min_alpha events: <= 2^-9 event under the conditions below;
  * the order dependence (second order) is measured on the CPU at <= 3e-6 event (tests/test_ledger_host.py holds it
    below 2^-10).
TOL_EVENTS = 2^-6: derived, not measured — 64 times below a whole event, 6 times below a cbow_mean=0 event, 8 times
above the rounding bound.  CONDITIONS, computed from the reference alone and asserted by both test files
(`conditions`): the largest ledger cell of the reference holds <= 128 events, alpha / min_alpha <= 2, near_edge == 0.
Positive and negative events cancel in a cell, so tests/test_ledger_host.py also counts the ADDS of every cell (the
restatement run with a constant gradient): 23 at most.

The product never imports this file; it imports torch (through n2v_hip.sgns.vocab_tables) only when a case is built."""
import numpy as np

import cbow_reference as C_
import sgcsr_reference as G
import sgns_reference as R

A, B, C = 0.1, 0.06, 2.0 ** -4
ALPHA, MIN_ALPHA = 2.0 ** -16, 2.0 ** -17
WINDOW, SEED, ID_BASE, STEP = 5, 21, 1000, 3
WORDS_PER_JOB = 400          # the walk-matrix tests shrink sgns.MAX_WORDS_IN_BATCH to this: several jobs per launch
BIN = 498
TOL_EVENTS = 2.0 ** -6
MAX_CELL_EVENTS = 128
MAX_ALPHA_RATIO = 2.0


def counting_tables(n_words, dim, stride=None):
    """-> (syn0, syn1neg) float32 [n_words, stride]; columns >= dim are zero."""
    assert n_words <= dim - 1
    stride = dim if stride is None else stride
    s0 = np.zeros((n_words, stride), np.float32)
    s1 = np.zeros((n_words, stride), np.float32)
    s0[:, dim - 1] = A
    s1[:, dim - 1] = B
    s1[np.arange(n_words), np.arange(n_words)] = C
    return s0, s1


def ledger(syn0, n_words):
    return np.asarray(syn0, dtype=np.float64)[:, :n_words]


def event_size(min_alpha=MIN_ALPHA, c=C):
    """The smallest change one skip-gram event makes to a ledger cell."""
    return float(R.exp_table()[BIN]) * min_alpha * c


def deviation_events(syn0, ref_ledger):
    """Largest |ledger - reference| over the cells, in events."""
    return float(np.abs(ledger(syn0, ref_ledger.shape[1]) - ref_ledger).max() / event_size())


def conditions(ref):
    """The three conditions of the tolerance, from a reference result alone -> (largest cell in events, alpha ratio,
    near_edge); raises when one fails."""
    cell = float(np.abs(ref["ledger"]).max() / event_size())
    ratio = ALPHA / MIN_ALPHA
    assert cell <= MAX_CELL_EVENTS, (ref["name"], "largest cell", cell)
    assert ratio <= MAX_ALPHA_RATIO and MAX_CELL_EVENTS ** 2 * 2.0 ** -24 * ratio <= 2.0 ** -9
    assert ref["stats"].near_edge == 0, (ref["name"], "sigmoid evaluations on a bin edge", ref["stats"].near_edge)
    assert ref["stats"].pairs > 0
    return cell, ratio, ref["stats"].near_edge


# ---- corpora -----------------------------------------------------------------------------------------------------------

def _flat_counts(tokens, n_words):
    """Flat word counts: every word the corpus' mean count, so that no ledger cell collects the draws of a frequent word."""
    return np.full(n_words, max(1, int((np.asarray(tokens) >= 0).sum()) // n_words), np.int64)


def walk_matrix(n_words, n_walks=24, L=80, seed=5):
    """24 walks x 80 over one vocabulary; three walks are short, -1 padded."""
    rs = np.random.RandomState(seed + n_words)
    walks = rs.randint(0, n_words, (n_walks, L)).astype(np.int32)
    lens = np.full(n_walks, L, np.int32)
    lens[[3, 7, 20]] = [1, 41, 79]
    for w in range(n_walks):
        walks[w, lens[w]:] = -1
    return walks, lens


SPLIT_LENS = (1, 2, 63, 64, 65, 128, 130, 192, 200)


def split_matrix(n_words, minus1, L=200, seed=9):
    """The walk matrix of the walk_splits cases: with sample=0 the effective length is the raw one, so the splits begin
    on 64, 65 and 128, the 64-lane blocks of lcg_skip_to_centre; `minus1` puts -1 tokens inside the walks."""
    rs = np.random.RandomState(seed + n_words)
    walks = rs.randint(0, n_words, (len(SPLIT_LENS), L)).astype(np.int32)
    lens = np.array(SPLIT_LENS, np.int32)
    if minus1:
        walks[rs.random_sample(walks.shape) < 0.04] = -1
        walks[:, 60:63] = -1
    for w in range(len(lens)):
        walks[w, lens[w]:] = -1
    return walks, lens


RAGGED_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 130, 257)


def ragged_corpus(n_words, lens=RAGGED_LENS, seed=13):
    """-> (tokens int32, offsets int64) with -1 tokens inside the sentences."""
    rs = np.random.RandomState(seed + n_words)
    sents = [rs.randint(0, n_words, n).astype(np.int32) for n in lens]
    for s in sents:
        s[rs.random_sample(len(s)) < 0.03] = -1
    tokens = np.concatenate(sents).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int64)
    return tokens, offsets


def walks_as_csr(walks, lens):
    tokens = np.concatenate([walks[w, :lens[w]] for w in range(len(lens))]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return tokens, offsets


def vocab(counts, sample):
    from n2v_hip import sgns
    return sgns.vocab_tables(counts, sample)


# ---- cases -------------------------------------------------------------------------------------------------------------
# kind "walks": n2v_sgns_train over a walk matrix (racing wavefronts, walk_splits, shared negatives); "span": the six
# sub-interval launches of n2v_sgns_train_span; "csr": n2v_sgns_csr_train; "cbow": n2v_cbow_train.

def _c(kind, n_words, dim, negative=5, sample=1e-3, corpus="walks", share=False, minus1=False, cbow_mean=1):
    return dict(kind=kind, n_words=n_words, dim=dim, negative=negative, sample=sample, corpus=corpus, share=share,
                minus1=minus1, cbow_mean=cbow_mean)


CASES = {
    "walks-d128": _c("walks", 120, 128),
    "walks-d64": _c("walks", 60, 64),
    "walks-d128-n12": _c("walks", 120, 128, negative=12),
    "shared-d64": _c("walks", 60, 64, share=True),
    "shared-d128-n7": _c("walks", 120, 128, negative=7, share=True),
    "splits-s0-n5": _c("walks", 120, 128, sample=0, corpus="split"),
    "splits-s0-n12": _c("walks", 120, 128, negative=12, sample=0, corpus="split"),
    "splits-sub-n5": _c("walks", 120, 128, corpus="split", minus1=True),
    "splits-sub-n12": _c("walks", 120, 128, negative=12, corpus="split", minus1=True),
    "span-d64": _c("span", 60, 64),
    "csr-d64": _c("csr", 60, 64, corpus="ragged"),
    "csr-d100": _c("csr", 90, 100, corpus="ragged"),
    "cbow-mean1": _c("cbow", 60, 64, cbow_mean=1),
    "cbow-mean0": _c("cbow", 60, 64, cbow_mean=0),
}
SPAN_INTERVALS, SPAN_SUBS, SPAN_SHARD_OFFSET = 2, 3, 5000
CSR_BATCH, CBOW_BATCH = 2, 5

_DATA = {}


def case_data(name):
    """-> dict: the case's fields, counts, walks / lens or tokens / offsets, and the schedule both sides use."""
    if name in _DATA:
        return _DATA[name]
    c = dict(CASES[name], name=name)
    n = c["n_words"]
    if c["corpus"] == "ragged":
        c["tokens"], c["offsets"] = ragged_corpus(n)
        flat = c["tokens"]
    else:
        c["walks"], c["lens"] = split_matrix(n, c["minus1"]) if c["corpus"] == "split" else walk_matrix(n)
        flat = c["walks"]
        if c["kind"] == "cbow":
            c["tokens"], c["offsets"] = walks_as_csr(c["walks"], c["lens"])
    c["counts"] = _flat_counts(flat, n)
    n_sent = len(c["lens"]) if "lens" in c else len(c["offsets"]) - 1
    if c["kind"] == "walks":
        c["batch"] = max(1, WORDS_PER_JOB // c["walks"].shape[1])
    elif c["kind"] == "span":
        c["batch"] = max(1, WORDS_PER_JOB // c["walks"].shape[1])
        c["epoch_base"] = 2 * n_sent * STEP
    else:
        c["batch"] = CSR_BATCH if c["kind"] == "csr" else CBOW_BATCH
    c["sentences_total"] = (4 if c["kind"] == "span" else 1) * n_sent * STEP
    _DATA[name] = c
    return c


def ref_kwargs(c):
    sample_int, cum = vocab(c["counts"], c["sample"])
    return dict(window=WINDOW, negative=c["negative"], alpha=ALPHA, min_alpha=MIN_ALPHA, sample_int=sample_int,
                cum_table=cum, seed=SEED, sentences_step=STEP, sentences_total=c["sentences_total"], alpha_batch=c["batch"])


def start_tables(c):
    """float64 copies of the fp32 counting tables, for a restatement."""
    s0, s1 = counting_tables(c["n_words"], c["dim"])
    return s0.astype(np.float64), s1.astype(np.float64)


def run_reference(name, variant=None, order=None, splits=None):
    """The sequential restatement of a case -> dict(name, ledger, pairs, stats, syn0).

    variant: a planted error of sgcsr_reference / cbow_reference.  order: a permutation of the case's sentences (walks,
    cbow) or items (csr) — each keeps its id and its job's learning rate.  splits: for a walk-matrix case, S = walk_splits
    wavefronts per walk restated through sgcsr_reference.train_item (which is where its planted variants live)."""
    c = case_data(name)
    kw = ref_kwargs(c)
    r0, r1 = start_tables(c)
    stats = R.Stats()
    kind = c["kind"]
    if kind in ("walks", "span"):
        walks, lens = c["walks"], c["lens"]
        if kind == "span":
            assert variant is None and order is None and splits is None
            n = len(lens)
            k = SPAN_INTERVALS * SPAN_SUBS
            for s in range(k):
                b, e = s * n // k, (s + 1) * n // k
                R.train(r0, r1, walks[b:e], lens[b:e], walk_id_base=c["epoch_base"] + SPAN_SHARD_OFFSET + b,
                        sentences_base=c["epoch_base"] + b * STEP, stats=stats, share_negatives=c["share"], **kw)
        elif splits is not None:
            skw = dict(kw, cum=[int(x) for x in kw["cum_table"]])
            del skw["cum_table"]
            items = [(w, sp) for w in range(len(lens)) for sp in range(splits)]
            for item in (items if order is None else [items[i] for i in order]):
                w, sp = item
                G.train_item(r0, r1, walks[w, :lens[w]], w, sp, splits, w * splits + sp, sentence_id_base=ID_BASE,
                             sentences_base=0, stats=stats, variant=variant, **skw)
        else:
            assert variant is None
            if order is None:
                R.train(r0, r1, walks, lens, walk_id_base=ID_BASE, sentences_base=0, stats=stats,
                        share_negatives=c["share"], **kw)
            else:
                for w in order:
                    R.train(r0, r1, walks[w:w + 1], lens[w:w + 1], walk_id_base=ID_BASE + w,
                            sentences_base=(w // c["batch"]) * c["batch"] * STEP, stats=stats,
                            share_negatives=c["share"], **kw)
    elif kind == "csr":
        chunk = 16 if splits is None else splits          # the ledger does not depend on the chunk; the variants do
        if order is None:
            G.train(r0, r1, c["tokens"], c["offsets"], chunk, sentence_id_base=ID_BASE, sentences_base=0, stats=stats,
                    variant=variant, **kw)
        else:
            skw = dict(kw, cum=[int(x) for x in kw["cum_table"]])
            del skw["cum_table"]
            items = G.item_table(c["offsets"], chunk)
            for item in order:
                s, sp, S = items[item]
                G.train_item(r0, r1, c["tokens"][c["offsets"][s]:c["offsets"][s + 1]], s, sp, S, item,
                             sentence_id_base=ID_BASE, sentences_base=0, stats=stats, variant=variant, **skw)
    else:
        tokens, offsets = c["tokens"], c["offsets"]
        if order is None:
            C_.train(r0, r1, tokens, offsets, cbow_mean=c["cbow_mean"], sentence_id_base=ID_BASE, sentences_base=0,
                     stats=stats, variant=variant, **kw)
        else:
            for s in order:
                C_.train(r0, r1, tokens[offsets[s]:offsets[s + 1]], np.array([0, offsets[s + 1] - offsets[s]]),
                         cbow_mean=c["cbow_mean"], sentence_id_base=ID_BASE + s,
                         sentences_base=(s // c["batch"]) * c["batch"] * STEP, stats=stats, variant=variant, **kw)
    return dict(name=name, ledger=ledger(r0, c["n_words"]).copy(), pairs=stats.pairs, stats=stats, syn0=r0)


_CACHE = {}


def reference(name):
    """The unplanted, in-order restatement of a case, computed once per process and never modified by its users."""
    if name not in _CACHE:
        _CACHE[name] = run_reference(name)
    return _CACHE[name]
