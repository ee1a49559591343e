"""CPU tests of the counting-table instrument of tests/test_gpu_w2v_ledger.py (tests/ledger_cases.py), run on the
float64 restatements alone: the conditions its tolerance is derived under hold for every case the GPU file uses, the
ledger does not depend on the order of the events, and it does move — by half an event at least — under every planted
error that changes which events are trained, with which draws or at which learning rate."""
import numpy as np
import pytest

import cbow_reference as C
import ledger_cases as L
import sgcsr_reference as G
import sgns_reference as R

ORDER_TOL = 2.0 ** -10      # events: what a permutation of the items or sentences may move a cell by
SPLITS = (2, 3, 7, 200)
CHUNKS = (1, 4, 16, 64, 100)


def _moved(got, name):
    """Largest ledger difference from the case's unplanted in-order reference, in events."""
    return L.deviation_events(got["syn0"], L.reference(name)["ledger"])


@pytest.mark.parametrize("name", sorted(L.CASES))
def test_conditions_of_the_tolerance_hold(name):
    ref = L.reference(name)
    cell, ratio, near = L.conditions(ref)
    c = L.case_data(name)
    assert c["n_words"] <= c["dim"] - 1
    assert np.isfinite(ref["syn0"]).all()
    # the rounding bound the tolerance quotes, with the figures of this very case
    assert cell ** 2 * 2.0 ** -24 * ratio <= 2.0 ** -9 < L.TOL_EVENTS
    print("%s: %d pairs, largest cell %.1f events, alpha ratio %g, near_edge %d" % (name, ref["pairs"], cell, ratio, near))


@pytest.mark.parametrize("name", [n for n in sorted(L.CASES) if n != "cbow-mean0"])
def test_no_cell_collects_more_than_128_adds(monkeypatch, name):
    """|cell| undercounts the adds of a cell in which positive and negative events cancel, and the rounding bound speaks
    of adds.  With the gradient replaced by a constant every event adds the same amount, so the restatement itself
    counts the adds of every cell exactly (cbow-mean0 trains cbow-mean1's corpus: the same adds, each 1 / count as large)."""
    unit = 2.0 ** -20

    def constant(f, bound, label, alpha, stats):
        return unit
    monkeypatch.setattr(R, "_gradient", constant)
    monkeypatch.setattr(C, "_gradient", constant)
    got = L.run_reference(name)
    adds = got["ledger"] / (unit * L.C)
    assert np.abs(adds - np.round(adds)).max() < 1e-6 and adds.min() >= 0
    print("%s: %d adds in all, %d at most in one cell" % (name, round(adds.sum()), round(adds.max())))
    assert 0 < adds.max() <= L.MAX_CELL_EVENTS
    assert got["pairs"] == L.reference(name)["pairs"]
    a, b = L.case_data("cbow-mean0"), L.case_data("cbow-mean1")
    assert np.array_equal(a["tokens"], b["tokens"]) and np.array_equal(a["offsets"], b["offsets"])


def test_the_corpora_reach_the_edges_they_are_built_for():
    c = L.case_data("splits-s0-n5")
    assert tuple(c["lens"]) == L.SPLIT_LENS and c["batch"] == 2
    begins = {sp * int(n) // S for n in c["lens"] for S in SPLITS for sp in range(S)}
    assert {64, 65, 128} <= begins                          # sample=0: effective = raw positions
    assert any(int(n) < 200 for n in c["lens"])             # S = L leaves empty splits on the short walks
    sub = L.case_data("splits-sub-n5")
    kw = L.ref_kwargs(sub)
    eff = [len(R.effective_sentence(sub["walks"][w], sub["lens"][w], kw["sample_int"], L.SEED, L.ID_BASE + w))
           for w in range(len(sub["lens"]))]
    inside = sum(int((sub["walks"][w, :sub["lens"][w]] < 0).sum()) for w in range(len(sub["lens"])))
    assert inside > 0 and sum(eff) < int((sub["walks"] >= 0).sum())
    r = L.case_data("csr-d64")
    assert tuple(np.diff(r["offsets"])) == L.RAGGED_LENS and (r["tokens"] < 0).any()
    for chunk in CHUNKS:                                    # every chunk cuts some sentence into several items
        assert max(S for _, _, S in G.item_table(r["offsets"], chunk)) > 1
    # a decaying learning rate: the launch spans several jobs
    for name in L.CASES:
        d = L.case_data(name)
        n_sent = len(d["lens"]) if "lens" in d else len(d["offsets"]) - 1
        if d["kind"] != "span":
            assert n_sent > 2 * d["batch"], name


def _record_bins(monkeypatch):
    seen = []
    inner = R._gradient

    def recording(f, bound, label, alpha, stats):
        seen.append(f)
        return inner(f, bound, label, alpha, stats)
    monkeypatch.setattr(R, "_gradient", recording)
    monkeypatch.setattr(C, "_gradient", recording)
    return seen


def _bin(f):
    return int(np.float32(np.float32(np.float32(f) + np.float32(R.MAX_EXP)) * np.float32(83)))


@pytest.mark.parametrize("name", ["walks-d64", "shared-d64", "splits-sub-n12", "csr-d64"])
def test_skipgram_f_stays_in_bin_498(monkeypatch, name):
    seen = _record_bins(monkeypatch)
    L.run_reference(name)
    assert len(seen) > 1000 and {_bin(f) for f in seen} == {L.BIN}
    print("%s: f in [%.5f, %.5f]" % (name, min(seen), max(seen)))
    assert 0.5 * L.A * L.B < min(seen) and max(seen) < 1.5 * L.A * L.B


@pytest.mark.parametrize("name", ["cbow-mean1", "cbow-mean0"])
def test_cbow_bin_is_a_function_of_the_context_count(monkeypatch, name):
    seen = _record_bins(monkeypatch)
    L.run_reference(name)
    assert len(seen) > 1000
    ab = np.float64(np.float32(L.A)) * np.float64(np.float32(L.B))
    counts = set()
    for f in seen:
        k = int(round(f / ab)) if name == "cbow-mean0" else 1
        counts.add(k)
        assert 1 <= k <= 2 * L.WINDOW and abs(f / ab - k) < 0.05 * k, (f, k)
        assert _bin(f) == _bin(k * ab), (f, k)
    assert counts == ({1} if name == "cbow-mean1" else set(range(1, 2 * L.WINDOW + 1))), counts


@pytest.mark.parametrize("name", ["walks-d64", "shared-d64", "csr-d64", "cbow-mean1", "cbow-mean0"])
def test_order_of_items_or_sentences_moves_no_cell(name):
    c = L.case_data(name)
    n = len(G.item_table(c["offsets"], 16)) if c["kind"] == "csr" else len(c["lens"])
    order = np.random.RandomState(3).permutation(n).tolist()
    in_order = L.run_reference(name, order=list(range(n)))
    assert _moved(in_order, name) == 0.0 and in_order["pairs"] == L.reference(name)["pairs"]
    got = L.run_reference(name, order=order)
    d = _moved(got, name)
    print("%s: %d items or sentences permuted move a cell by %.3g event at most" % (name, n, d))
    assert got["pairs"] == L.reference(name)["pairs"] and d <= ORDER_TOL


@pytest.mark.parametrize("name", ["splits-s0-n5", "splits-sub-n12"])
def test_split_walks_restated_item_by_item_are_the_whole_walks(name):
    """walk_splits = S is sgcsr_reference.train_item with a fixed S per walk: in order it trains sgns_reference.train's
    events, and its items in a random order move no cell either — so sgns_reference.train IS the reference of a split launch."""
    want = L.reference(name)
    for S in SPLITS:
        got = L.run_reference(name, splits=S)
        order = np.random.RandomState(S).permutation(len(L.SPLIT_LENS) * S).tolist()
        mixed = L.run_reference(name, splits=S, order=order)
        d, dm = _moved(got, name), _moved(mixed, name)
        print("%s S=%d: in order %.3g, permuted %.3g event" % (name, S, d, dm))
        assert got["pairs"] == mixed["pairs"] == want["pairs"]
        assert d <= ORDER_TOL and dm <= ORDER_TOL


# ---- sensitivity: a planted error that changes the events moves some cell by half an event at least -----------------------

@pytest.mark.parametrize("variant", ["clip_context", "skip_without_negative", "alpha_per_item"])
@pytest.mark.parametrize("name", ["csr-d64", "csr-d100"])
def test_chunk_cases_fail_against_a_planted_expected_side(name, variant):
    want = L.reference(name)
    for chunk in CHUNKS:
        got = L.run_reference(name, variant=variant, splits=chunk)
        d = _moved(got, name)
        print("%s chunk %d %s: %.1f events, pairs %d vs %d" % (name, chunk, variant, d, got["pairs"], want["pairs"]))
        assert d >= 0.5 > L.TOL_EVENTS, (name, chunk, variant, d)
        if variant != "clip_context":
            assert got["pairs"] == want["pairs"]          # invisible to the pair count


@pytest.mark.parametrize("variant", ["clip_context", "skip_without_negative", "alpha_per_item"])
@pytest.mark.parametrize("name", ["splits-s0-n5", "splits-sub-n12"])
def test_splits_cases_fail_against_a_planted_expected_side(name, variant):
    want = L.reference(name)
    for S in SPLITS:
        got = L.run_reference(name, variant=variant, splits=S)
        d = _moved(got, name)
        print("%s S=%d %s: %.1f events, pairs %d vs %d" % (name, S, variant, d, got["pairs"], want["pairs"]))
        assert d >= 0.5 > L.TOL_EVENTS, (name, S, variant, d)
        if variant != "clip_context":
            assert got["pairs"] == want["pairs"]


@pytest.mark.parametrize("name,chunk", [("csr-d64", 4), ("csr-d64", 16), ("splits-sub-n12", 7)])
def test_raw_split_bounds_moves_nothing_and_rightly_so(name, chunk):
    """raw_split_bounds cuts a sentence at other centres, but its cuts still partition the sentence in order, each item
    skips the LCG to its own first centre and stages its own window: the SAME events, dealt to other items.  The ledger
    counts events, not who trained them, so it must not move — not a miss of the instrument."""
    got = L.run_reference(name, variant="raw_split_bounds", splits=chunk)
    assert got["pairs"] == L.reference(name)["pairs"]
    assert _moved(got, name) == 0.0


CBOW_EVENT_VARIANTS = ("window_off_by_one", "dup_once", "no_inv", "inv_wrong_branch")


@pytest.mark.parametrize("variant", CBOW_EVENT_VARIANTS)
@pytest.mark.parametrize("name", ["cbow-mean1", "cbow-mean0"])
def test_cbow_cases_fail_against_a_planted_expected_side(name, variant):
    got = L.run_reference(name, variant=variant)
    d = _moved(got, name)
    print("%s %s: %.2f events" % (name, variant, d))
    assert d >= 0.5 > L.TOL_EVENTS, (name, variant, d)


def test_draw_without_context_cannot_be_observed():
    """Planted as an error of the draws, but no corpus can show it (tests/test_cbow_host.py has the argument: a centre
    without context needs a one-word sentence, which has no later centre to see the LCG, and every sentence seeds its own).
    The corpus does hold a one-word sentence; the ledger must not move at all."""
    assert 1 in L.case_data("cbow-mean1")["lens"]
    for name in ("cbow-mean1", "cbow-mean0"):
        assert _moved(L.run_reference(name, variant="draw_without_context"), name) == 0.0


@pytest.mark.parametrize("variant", ["reversed_sum", "stale_repeat"])
def test_cbow_arithmetic_variants_are_not_the_ledgers_business(variant):
    """The order of the context sum and a stale row of a repeated draw change VALUES at fp32 rounding, not events: the
    ledger must not see them (tests/test_gpu_cbow.py pins them on one wavefront)."""
    got = L.run_reference("cbow-mean1", variant=variant)
    assert _moved(got, "cbow-mean1") <= ORDER_TOL
