"""GPU tests: WHICH events racing word2vec wavefronts train — the pairs, their negative draws and their learning rates —
pinned to the sequential float64 restatements through counting tables (tests/ledger_cases.py has the construction, the
derivation of the tolerance and its conditions; tests/test_ledger_host.py proves the instrument on the CPU, planted
errors included).

Every case starts from the counting tables, runs its launch(es) once in atomic mode, and asserts: the ledger block
syn0[:, :n_words] within TOL_EVENTS = 2^-6 event of the restatement's in every cell, pairs_trained() equal to the
restatement's, finite tables, zero padding columns.  Covered: many wavefronts on shared rows (n2v_sgns_train,
sgns_shared_kernel, n2v_cbow_train), walk_splits > 1 (n2v_sgns_train, n2v_sgns_train_span), chunk > 0
(n2v_sgns_csr_train: windowed staging, item bisection, lcg_skip_to_centre), on static-stride and counter grids.

Pinned here: the events, their draws and learning rates.  Not pinned, and not pinnable: the VALUES a race leaves (column
dim-1, syn1neg, real tables), and the lossy row modes under a race.

MEASURED on an MI355X: at most 2.2e-5 event over all cases (negative 12; 6.8e-6 with negative <= 7), 700 times inside
the tolerance; DESIGN.md §3 lists the figure of each group of cases."""
import numpy as np
import pytest

import ledger_cases as L

pytestmark = pytest.mark.gpu

GRIDS = [(1, False), (2, True), (7, True), (0, True)]      # (max_blocks, work counter); 0 = the default grid
GRID_IDS = ["1block-static", "2blocks-counter", "7blocks-counter", "default"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def refs():
    """The restatement of every case, computed once and never modified; the conditions of the tolerance hold."""
    out = {}
    for name in L.CASES:
        out[name] = L.reference(name)
        L.conditions(out[name])
    return out


@pytest.fixture()
def small_jobs(monkeypatch):
    """The walk-matrix trainer steps the learning rate once per job of MAX_WORDS_IN_BATCH words; at test size that is one
    job per launch.  Shrunk, a launch spans several jobs and a learning rate taken from the wrong walk shows."""
    from n2v_hip import sgns
    monkeypatch.setattr(sgns, "MAX_WORDS_IN_BATCH", L.WORDS_PER_JOB)


def _load_tables(torch, m, c):
    s0, s1 = L.counting_tables(c["n_words"], c["dim"], m.stride)
    m.syn0.copy_(torch.from_numpy(s0))
    m.syn1neg.copy_(torch.from_numpy(s1))


def _sgns_model(torch, c, counter=True):
    from n2v_hip import sgns
    m = sgns.SgnsModel(c["n_words"], dim=c["dim"], window=L.WINDOW, negative=c["negative"], alpha=L.ALPHA,
                       min_alpha=L.MIN_ALPHA, sample=c["sample"], seed=L.SEED, update_mode="atomic",
                       share_negatives=c["share"], allow_out_of_band=True)
    m.build_vocab(counts=c["counts"])
    _load_tables(torch, m, c)
    if not counter:
        m.work_counter = None
    return m


def _ragged_model(torch, c, counter=True):
    from n2v_hip import cbow, skipgram
    kw = dict(dim=c["dim"], window=L.WINDOW, negative=c["negative"], alpha=L.ALPHA, min_alpha=L.MIN_ALPHA,
              sample=c["sample"], seed=L.SEED)
    m = cbow.CbowModel(c["n_words"], cbow_mean=c["cbow_mean"], **kw) if c["kind"] == "cbow" else \
        skipgram.SkipGramModel(c["n_words"], **kw)
    m.build_vocab(c["counts"])
    _load_tables(torch, m, c)
    if not counter:
        m.work_counter = None
    return m


def _corpus(torch, c):
    from n2v_hip.corpus import SentenceCorpus
    n = c["n_words"]
    return SentenceCorpus(torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["offsets"]).cuda(), np.arange(n),
                          np.zeros(n, np.int64), max(1, int(np.diff(c["offsets"]).max())))


def _assert_ledger(torch, m, c, ref, what):
    torch.cuda.synchronize()
    g0, g1 = m.syn0.cpu().numpy(), m.syn1neg.cpu().numpy()
    dev = L.deviation_events(g0, ref["ledger"])
    pairs = m.pairs_trained()
    print("%s %s: %d pairs (restatement %d), largest ledger deviation %.3g event (tolerance %.3g)"
          % (c["name"], what, pairs, ref["pairs"], dev, L.TOL_EVENTS))
    assert np.isfinite(g0).all() and np.isfinite(g1).all(), what
    assert (g0[:, c["dim"]:] == 0).all() and (g1[:, c["dim"]:] == 0).all(), "padding columns moved"
    assert pairs == ref["pairs"], (c["name"], what, pairs, ref["pairs"])
    assert dev <= L.TOL_EVENTS, (c["name"], what, dev)
    return dev


def _train_walks(torch, c, blocks=0, counter=True, splits=1):
    m = _sgns_model(torch, c, counter)
    m.train_pass(torch.from_numpy(c["walks"]).cuda(), torch.from_numpy(c["lens"]).cuda(), sentences_base=0,
                 sentences_total=c["sentences_total"], walk_id_base=L.ID_BASE, sentences_step=L.STEP, max_blocks=blocks,
                 splits=splits)
    return m


# ---- 1: n2v_sgns_train, one wavefront per walk, walks racing on shared rows ---------------------------------------------------

@pytest.mark.parametrize("blocks,counter", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("name", ["walks-d128", "walks-d64", "walks-d128-n12"])
def test_racing_walks_train_the_restatements_events(torch_cuda, small_jobs, refs, name, blocks, counter):
    c = L.case_data(name)
    _assert_ledger(torch_cuda, _train_walks(torch_cuda, c, blocks, counter), c, refs[name], GRID_IDS[GRIDS.index((blocks, counter))])


# ---- 2: walk_splits ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [2, 3, 7, 200])
@pytest.mark.parametrize("name", ["splits-s0-n5", "splits-s0-n12", "splits-sub-n5", "splits-sub-n12"])
def test_split_walks_train_the_restatements_events(torch_cuda, small_jobs, refs, name, S):
    """S wavefronts per walk: each skips the walk's LCG to its first centre (lcg_skip_to_centre) and races the others on
    the walk's rows.  The restatement of the UNSPLIT walks is the reference, whatever S (tests/test_ledger_host.py)."""
    c = L.case_data(name)
    assert S <= c["walks"].shape[1]
    _assert_ledger(torch_cuda, _train_walks(torch_cuda, c, splits=S), c, refs[name], "S=%d" % S)
    if S in (3, 7):                                         # one workgroup on static stride; 7 blocks (S=7: off the counter)
        _assert_ledger(torch_cuda, _train_walks(torch_cuda, c, 1, False, S), c, refs[name], "S=%d, 1 block static" % S)
        _assert_ledger(torch_cuda, _train_walks(torch_cuda, c, 7, True, S), c, refs[name], "S=%d, 7 blocks counter" % S)


@pytest.mark.parametrize("predraw", ["0", "1"])
@pytest.mark.parametrize("name", ["splits-s0-n5", "splits-sub-n5"])
def test_split_walks_with_and_without_parallel_draws(torch_cuda, small_jobs, refs, monkeypatch, name, predraw):
    monkeypatch.setenv("N2V_SGNS_PREDRAW", predraw)
    c = L.case_data(name)
    _assert_ledger(torch_cuda, _train_walks(torch_cuda, c, splits=3), c, refs[name], "S=3 predraw=%s" % predraw)


# ---- 3: n2v_sgns_train_span with splits ---------------------------------------------------------------------------------------------

def test_span_launches_with_splits_train_the_restatements_events(torch_cuda, small_jobs, refs):
    torch = torch_cuda
    c = L.case_data("span-d64")
    m = _sgns_model(torch, c)
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    launch = m.span_launcher(torch.from_numpy(c["walks"]).cuda(), torch.from_numpy(c["lens"]).cuda(), c["sentences_total"],
                             L.STEP, state, subs_per_interval=L.SPAN_SUBS, n_sub_total=L.SPAN_INTERVALS * L.SPAN_SUBS,
                             shard_offset=L.SPAN_SHARD_OFFSET, splits=3)
    for interval in range(L.SPAN_INTERVALS):
        state.copy_(torch.tensor([interval, c["epoch_base"]]))
        for sub in range(L.SPAN_SUBS):
            launch(sub)
    _assert_ledger(torch, m, c, refs["span-d64"], "2 intervals x 3 sub-intervals, S=3")


# ---- 4: sgns_shared_kernel ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocks", [1, 2, 0], ids=["1block", "2blocks", "default"])
@pytest.mark.parametrize("name", ["shared-d64", "shared-d128-n7"])
def test_racing_walks_with_shared_negatives_train_the_restatements_events(torch_cuda, small_jobs, refs, name, blocks):
    c = L.case_data(name)
    assert c["share"] and c["negative"] <= 7
    _assert_ledger(torch_cuda, _train_walks(torch_cuda, c, blocks), c, refs[name], "%s blocks" % (blocks or "default"))


# ---- 5: n2v_sgns_csr_train, chunked -------------------------------------------------------------------------------------------

def _train_csr(torch, c, chunk, blocks=0, counter=True, cuts=None):
    from n2v_hip import skipgram
    m = _ragged_model(torch, c, counter)
    corpus = _corpus(torch, c)
    total = skipgram.n_items(corpus, chunk)
    bounds = [0] + list(cuts or []) + [total]
    for b, e in zip(bounds[:-1], bounds[1:]):
        m.train_pass(corpus, sentences_base=0, sentences_total=c["sentences_total"], sentence_id_base=L.ID_BASE,
                     sentences_step=L.STEP, alpha_batch=c["batch"], chunk=chunk, first_item=b, item_count=e - b,
                     max_blocks=blocks)
    return m, total


@pytest.mark.parametrize("chunk", [1, 4, 16, 64, 100])
@pytest.mark.parametrize("name", ["csr-d64", "csr-d100"])
def test_chunked_items_train_the_restatements_events(torch_cuda, refs, name, chunk):
    """The items of a sentence race on its rows; each stages only its window of the effective sentence and skips the
    sentence's LCG to its first centre.  The ledger of the whole sentences is the reference, whatever the chunk."""
    c = L.case_data(name)
    for blocks, counter in GRIDS:
        m, total = _train_csr(torch_cuda, c, chunk, blocks, counter)
        _assert_ledger(torch_cuda, m, c, refs[name], "chunk %d (%d items) %s" % (chunk, total, GRID_IDS[GRIDS.index((blocks, counter))]))


@pytest.mark.parametrize("name,chunk", [("csr-d64", 16), ("csr-d100", 4)])
def test_two_launches_over_an_item_range_sum_to_the_whole(torch_cuda, refs, name, chunk):
    from sgcsr_reference import item_table
    c = L.case_data(name)
    items = item_table(c["offsets"], chunk)
    k = max(i for i, (s, sp, S) in enumerate(items) if sp == 1)        # the cut falls inside the last sentence
    assert 0 < k < len(items) and items[k][0] == items[k - 1][0]
    m, total = _train_csr(torch_cuda, c, chunk, cuts=[k])
    assert total == len(items)
    _assert_ledger(torch_cuda, m, c, refs[name], "chunk %d, items [0, %d) then [%d, %d)" % (chunk, k, k, total))


# ---- 6: n2v_cbow_train ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocks,counter", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("name", ["cbow-mean1", "cbow-mean0"])
def test_racing_cbow_sentences_train_the_restatements_events(torch_cuda, refs, name, blocks, counter):
    c = L.case_data(name)
    m = _ragged_model(torch_cuda, c, counter)
    m.train_pass(_corpus(torch_cuda, c), sentences_base=0, sentences_total=c["sentences_total"], sentence_id_base=L.ID_BASE,
                 sentences_step=L.STEP, alpha_batch=c["batch"], max_blocks=blocks)
    _assert_ledger(torch_cuda, m, c, refs[name], GRID_IDS[GRIDS.index((blocks, counter))])
