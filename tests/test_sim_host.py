"""CPU tests of the test infrastructure around csrc/n2v_sim.hip: the float64 restatement tests/sim_reference.py against
the per-pair functions of oracle/augment_oracle.py, and the case tables of tests/test_gpu_sim_exact.py — that they run
every instantiation, hold every edge they are there for, and that every set / order comparison of that module is decided
by the reference alone (no comparison is left out for lack of a gap)."""
import itertools
import os
import re

import numpy as np
import pytest

import sim_reference as R
import test_gpu_sim_exact as G
from helpers import ROOT
from oracle import augment_oracle, linkpred_oracle


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_agrees_with_the_per_pair_oracle():
    rs = np.random.RandomState(8)
    n, d = 30, 37
    vec = rs.normal(size=(n, d)).astype(np.float32)
    vec[4] = 0.0                                            # unitvec: stays zero, similarity 0
    pos = (rs.random_sample((n, d)) + 0.01).astype(np.float32)
    pairs = [(0, 1), (2, 2), (5, 29), (17, 3), (4, 9), (9, 4), (28, 11)]
    emb, pemb = dict(enumerate(vec)), dict(enumerate(pos))
    S = {m: R.block(R.prepare(v, d, None, m), R.prepare(v, d, None, m), m) for m, v in (("cos", vec), ("pearson", vec), ("jsd", pos))}
    for i, j in pairs:
        # the oracle's cos is a float32 dot of float32 unit vectors: d products and sums, two normalisations of d terms
        assert abs(S["cos"][i, j] - augment_oracle.similarity(emb, i, j)) <= float(3 * R.gamma(d + 3))
        assert abs(S["cos"][i, j] - linkpred_oracle.similarity(emb, i, j)) <= float(3 * R.gamma(d + 3))
        if 4 not in (i, j):
            want = augment_oracle.get_similarity({k: v.astype(np.float64) for k, v in emb.items()}, i, j, "pearson")
            assert abs(S["pearson"][i, j] - want) < 1e-13
        assert abs(S["jsd"][i, j] - augment_oracle.js(pos[i].astype(np.float64), pos[j].astype(np.float64))) < 1e-13
    assert S["cos"][4, 9] == 0.0 and augment_oracle.similarity(emb, 4, 9) == 0.0 and linkpred_oracle.similarity(emb, 9, 4) == 0.0
    assert np.isnan(R.block(R.prepare(vec, d, None, "pearson"), R.prepare(vec, d, None, "pearson"), "pearson")[4]).all()


def test_rel_entr_case_split_is_scipys():
    from scipy.special import rel_entr
    v = [0.0, -0.0, 0.3, 1.0, -0.2, np.inf, np.nan, 1e-40]
    x, y = np.array(list(itertools.product(v, v))).T
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(R.rel_entr(x, y), rel_entr(x, y))


def test_stride_rows_and_padding_of_prepare():
    rs = np.random.RandomState(1)
    vec = rs.normal(size=(9, 12)).astype(np.float32)
    vec[:, 7:] = np.nan
    rows = np.array([3, 3, 8, 0])
    for m in ("cos", "pearson", "jsd"):
        P = R.prepare(vec, 7, rows, m)
        assert P.shape == (4, 32) and (P[:, 7:] == 0).all() and np.isfinite(P).all()
        assert np.array_equal(P, R.prepare(vec[rows][:, :7].copy(), 7, None, m))


def test_row_selection_restatement():
    sc = np.array([[0.5, np.nan, 0.5, -1.0, 2.0, -0.0, 0.0]], dtype=np.float32)
    assert R.rows_topk(sc, 7) == [[4, 0, 2, 5, 6, 3, 1]]
    assert R.rows_count(sc, 0.0).tolist() == [3]
    off, cols, vals = R.rows_fill(np.vstack([sc, sc]), 0.5)
    assert off.tolist() == [0, 1] and cols.tolist() == [4, 4] and vals.tolist() == [2.0, 2.0]
    assert R.order_key_select(sc[0], 4) == [0, 2, 4, 6] and sorted(R.rows_topk(sc, 4)[0]) == [0, 2, 4, 5]


# ------------------------------------------------------------------------------------------------ coverage of the tables
def test_every_instantiation_is_launched_and_named_as_in_the_source():
    assert set(G.INSTANTIATIONS) == set(itertools.product(("mfma", "vector", "jsd"), ("block", "scan")))
    assert set(G.FAMILIES) == {"mfma", "vector", "jsd"}
    src = open(os.path.join(ROOT, "node2vec-by-ecc_amd", "csrc", "n2v_sim.hip")).read()
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(sim_\w+<[^>]*>)", src))
    assert launched == set(G.INSTANTIATIONS.values())
    assert 'getenv("N2V_SIM_VECTOR")' in src


def test_block_table_covers_the_shapes_and_arguments_of_the_issue():
    t = G.BLOCK_CASES
    assert {(c[0], c[1]) for c in t} == set(G.BLOCK_SHAPES)
    assert {R.dpad_of(c[2]) for c in t} == {32, 64, 96, 160, 512} and all(c[2] % 32 for c in t)
    assert {c[3] for c in t} == {0, 1, 64, 100}
    assert {c[4] for c in t} == {3, 128}
    assert {c[5] for c in t} == {"off", "0", "5", "first", "last", "none"}
    assert {c[6] for c in t} == {"cos", "pearson"}
    seen = set()
    for i in range(len(t)):
        c = G.block_case(i)
        assert c["srcA"].shape[0] > c["row_begin"] + c["n_rows"] and c["ld"] > c["n_cols"]
        cols = c["row_begin"] + np.arange(c["n_rows"]) + c["zoff"]
        hit = cols[(cols < c["n_cols"])] if c["zoff"] >= 0 else cols[:0]
        if c["zero_kind"] == "first":
            assert 0 in hit
        if c["zero_kind"] == "last":
            assert c["n_cols"] - 1 in hit
        if c["zero_kind"] in ("0", "5"):
            assert len(hit) > 0
        if c["zero_kind"] in ("none", "off"):
            assert len(hit) == 0
        # integer operands: exact in fp32 whatever the order, rows distinct
        for M in (c["intA"], c["intB"]):
            assert np.array_equal(M, np.round(M)) and np.abs(M).max() <= 2 and M.shape[1] == c["dpad"] <= 512
            assert len({r.tobytes() for r in M}) == M.shape[0] or c["dpad"] == 32 and M.shape[0] > 200
        assert 4 * c["dpad"] < 2 ** 24
        sp = c["special"]
        seen |= set(sp)
        if "identical" in sp:
            assert np.array_equal(c["jsdA"][sp["identical"][0]], c["jsdB"][sp["identical"][1]])
        if "neg_row" in sp:
            assert (c["jsdA"][sp["neg_row"]] < 0).sum() == 1 and c["row_begin"] <= sp["neg_row"] < c["row_begin"] + c["n_rows"]
        if "neg_col" in sp:
            assert (c["jsdB"][sp["neg_col"]] < 0).sum() == 1
        if "zeros_row" in sp:
            assert (c["jsdA"][sp["zeros_row"]] == 0).any() and (c["jsdA"][sp["zeros_row"]] > 0).any()
        assert (np.delete(c["jsdA"], [sp.get("neg_row", 0)], axis=0) >= 0).all()
    assert seen == {"identical", "neg_row", "neg_col", "zeros_row", "zeros_col"}


def test_prepare_table_covers_the_issue():
    t = G.PREP_CASES
    for m in ("cos", "pearson", "jsd"):
        assert {c["dim"] for c in t if c["method"] == m} == set(G.PREP_DIMS) - ({1} if m == "pearson" else set())
    assert {c["stride_extra"] for c in t} == {0, 5} and {c["rows_mode"] for c in t} == {"none", "perm", "repeat"}
    assert {c["n_rows"] for c in t} == {1, 3, 4, 5, 257}
    seen = set()
    for i in range(len(t)):
        c = G.prepare_case(i)
        assert np.isnan(c["vec"][:, c["dim"]:]).all() and np.isfinite(c["vec"][:, :c["dim"]]).all()
        assert c["dpad"] % 32 == 0 and c["dpad"] >= c["dim"]
        x = c["vec"] if c["rows"] is None else c["vec"][c["rows"]]
        if c["rows_mode"] == "perm":
            assert sorted(c["rows"].tolist()) == list(range(c["n_rows"]))
        if c["rows_mode"] == "repeat":
            assert c["vec"].shape[0] > c["n_rows"]
            if c["n_rows"] >= 3:
                assert len(set(c["rows"].tolist())) < c["n_rows"]
        sp = c["special"]
        seen |= set(sp)
        if "zero_row" in sp:
            assert (x[0, :c["dim"]] == 0).all()
        if "const_row" in sp:
            assert (x[0, :c["dim"]] == 0.5).all() and 0.5 * c["dim"] < 2 ** 24
        if "ill_row" in sp:
            r = x[1, :c["dim"]].astype(np.float64)
            assert abs(r.mean()) * np.sqrt(c["dim"]) / np.linalg.norm(r - r.mean()) > 1000
            assert np.isfinite(R.prepare_bound(c["vec"], c["dim"], c["rows"], "pearson")[1]).all()
        if "zero_sum_row" in sp:
            assert x[0, :c["dim"]].astype(np.float64).sum() == 0 and (x[0, :c["dim"]] != 0).any()
    assert seen == {"zero_row", "const_row", "ill_row", "zero_sum_row"}


@pytest.mark.parametrize("fam", G.FAMILIES)
@pytest.mark.parametrize("upper", [0, 1])
def test_scan_table_holds_its_edges(fam, upper):
    A, B = G.scan_operands(fam, upper)
    n_cols = B.shape[0]
    S = R.block(A, B, G.family_method(fam))
    assert set(G.SCAN_RANGES) == {(0, 200), (64, 192), (1, 130), (130, 131)}
    assert [rb % 64 for rb, _ in G.SCAN_RANGES].count(0) < len(G.SCAN_RANGES)          # a row_begin off the tile grid
    for rb, re in G.SCAN_RANGES:
        Sr = S[rb:re]
        taus = {k: G.scan_tau(fam, k, Sr) for k in G.SCAN_TAUS}
        assert taus["-inf"] == -np.inf
        assert (Sr == taus["equal"]).any(), "tau 'equal' must be a score that occurs"
        assert (Sr > taus["between"]).any() and (Sr < taus["between"]).any() and not (Sr == taus["between"]).any()
        assert float(np.float32(taus["between"])) == taus["between"] and float(np.float32(taus["equal"])) == taus["equal"]
        for tk, tau in taus.items():
            full = R.topk_scan(Sr, tau, None, upper, rb)
            for ek in G.SCAN_EXCL:
                pairs = G.scan_excl_pairs(ek, rb, re, n_cols, upper, tau, Sr)
                assert all(rb <= r < re and 0 <= c < n_cols for r, c in pairs)
                hit = [(r, c) for r, c in pairs if (r, c, float(S[r, c])) in full]
                if ek == "one" and full:
                    assert len(pairs) == 1 and len(hit) == 1, "the excluded pair must be one that qualifies"
                if ek == "below_tau":
                    assert not hit and (tk != "between" or pairs or re - rb == 1)
                if ek == "first_last":
                    assert (rb, 0) in pairs and (re - 1, n_cols - 1) in pairs
                if ek == "corners64" and re - rb > 127:
                    assert len(pairs) == 4 and {(r - rb) % 64 for r, _ in pairs} == {0, 63} and {c % 64 for _, c in pairs} == {0, 63}
                if ek == "corners128" and re - rb > 127:
                    assert {(r - rb) % 128 for r, _ in pairs} == {0, 127} and {c % 128 for _, c in pairs} == {0, 127}
                if ek.startswith("corners") and tk == "-inf" and not upper and pairs:
                    assert hit, "corner keys must remove something"
        # the overflow case: more candidates than the capacity the GPU test gives it
        n_all = len(R.topk_scan(Sr, -np.inf, None, upper, rb))
        assert n_all >= 2 and n_all // 2 < n_all


def test_ties_cases_have_more_than_k_scores_equal_to_the_kth():
    for fam in G.FAMILIES:
        A = G.ties_case(fam)
        S = R.block(A, A, G.family_method(fam))
        for upper in ((True,) if fam == "jsd" else (False, True)):
            k, top = G.ties_k(S, upper)
            kth = top[k - 1][0]
            taken = sum(1 for t in top[:k] if t[0] == kth)
            assert sum(1 for t in top if t[0] == kth) > taken >= 2 and k < len(top)
    # the small buffer really overflows on the first row block of the dot cases
    assert 256 * G.ties_case("mfma").shape[0] > 2048


def test_threshold_cases_hold_a_score_equal_to_thre():
    for n_cols in G.SEL_NCOLS:
        cases = G.threshold_cases(n_cols)
        assert {s.shape[0] for s, _ in cases} == {1, 8, 300}
        assert sum(1 for s, t in cases if (s == np.float32(t)).any()) >= 6
        assert any(t == 0.0 and np.signbit(s[s == 0]).any() for s, t in cases), "+0.0 against -0.0 scores"
        assert any(np.isposinf(t) for _, t in cases) and any(np.isneginf(t) for _, t in cases)
        for s, t in cases:
            assert float(np.float32(t)) == t or np.isinf(t)
        p = G.padded(cases[0][0])
        assert p.shape[1] == n_cols + 7 and np.isposinf(p[:, n_cols]).all() and np.isnan(p[:, n_cols + 1]).all()
    rows = G.selection_rows(600)
    k = dict(zip(G.ROW_KINDS, rows))
    assert len(set(k["all_equal"].tolist())) == 1
    z = k["signed_zeros"]
    assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
    assert np.isposinf(k["with_inf"]).any() and np.isneginf(k["with_inf"]).any() and not np.isnan(k["with_inf"]).any()
    assert 1 < np.isnan(k["some_nan"]).sum() < 600 and not np.isinf(k["some_nan"]).any() and np.isnan(k["all_nan"]).all()
    d = k["denormals"]
    assert (np.abs(d[d != 0]) < np.finfo(np.float32).tiny).all() and (d > 0).any() and (d < 0).any()
    lb = np.unique(k["last_bit"]).view(np.uint32)
    assert len(lb) == 2 and lb[1] - lb[0] == 1


# ------------------------------------------------------------------------------------------------ nothing is left out
def test_no_selection_comparison_is_left_out_for_lack_of_a_gap():
    """Every set / order comparison of the GPU module must be decided by the reference: exact small-integer operands
    (every fp32 partial sum exact), scores that are the test's own inputs, or a float64 gap above twice the error bound.
    The share of comparisons that would have to be skipped or loosened is 0."""
    total = left_out = 0
    kinds = set()
    for name, kind, payload in G.selection_comparisons():
        total += 1
        kinds.add(kind)
        if kind == "exact":
            ok = all(np.array_equal(M, np.round(M)) and np.abs(M).max() <= 2 and 4 * M.shape[1] < 2 ** 24 for M in payload)
        elif kind == "given":
            ok = all(M.dtype == np.float32 for M in payload)
        else:
            margin, bound = payload
            ok = bool(np.all(margin > 2 * bound)) and np.isfinite(bound).all()
        if not ok:
            left_out += 1
            print("left out:", name)
    assert kinds == {"exact", "given", "gap"} and total >= 4 + 2 * len(G.SCAN_RANGES) * 2 + 3 + 2 + len(G.SEL_NCOLS)
    assert left_out == 0, "%d of %d comparisons are not decided by the reference" % (left_out, total)


# ------------------------------------------------------------------------------------------------ the signed zeros
def test_signed_zero_rows_separate_python_order_from_the_bit_key_order():
    """rows_topk's contract is Python's sort, for which -0.0 == +0.0 (column order decides); a key that puts every +0.0
    above every -0.0 selects another set.  On the signed-zero rows of the GPU test the two differ for some k, so that
    test fails on a kernel with the bit-key order."""
    for n_cols in G.SEL_NCOLS[1:]:
        row = G.selection_rows(n_cols)[G.ROW_KINDS.index("signed_zeros")]
        want = R.rows_topk(row[None, :], n_cols)[0]
        assert want == list(range(n_cols))
        differ = [k for k in range(n_cols + 1) if sorted(want[:k]) != R.order_key_select(row, k)]
        assert differ, n_cols
    # on rows without a -0.0 the two orders agree for every k
    for kind in ("all_equal", "with_inf", "some_nan", "all_nan", "denormals", "last_bit", "normals"):
        row = G.selection_rows(257)[G.ROW_KINDS.index(kind)]
        if (row == 0).any() and np.signbit(row[row == 0]).any():
            continue
        full = R.rows_topk(row[None, :], 257)[0]
        assert all(sorted(full[:k]) == R.order_key_select(row, k) for k in range(258)), kind
