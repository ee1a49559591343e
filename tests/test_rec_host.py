"""CPU tests of the top-N recommendation path: the vectorised restatement (tests/rec_reference.py) against the literal
transcription of src/bine_train.py:311-406, the host tables and builders of n2v_hip/recommend.py, and the proof that the
inputs of tests/test_gpu_rec.py are fit for an exact comparison."""
import math

import numpy as np
import pytest

import rec_reference as R


def _dict_case(seed, n_u=23, n_v=41, d=6, ties=True):
    """A small labelled problem: node lists as the reference holds them, test users / items with labels the model does
    not know on both sides, test items outside the item list, zero rows (exact ties) and a repeated score."""
    rs = np.random.RandomState(seed)
    emb_u = rs.normal(size=(n_u, d))
    emb_v = rs.normal(size=(n_v, d))
    if ties:
        emb_u[rs.choice(n_u, 3, replace=False)] = 0.0
        emb_v[rs.choice(n_v, 5, replace=False)] = 0.0
        emb_v[7] = emb_v[3]                                         # two items with the same score for every user
        emb_v[11] = -0.0 * np.ones(d)                               # scores of -0.0 against positive rows
    users = np.array(sorted("u%03d" % i for i in range(n_u)))
    items = np.array(sorted("i%03d" % i for i in range(n_v)))
    node_list_u = {l: {"embedding_vectors": emb_u[i:i + 1]} for i, l in enumerate(users)}
    node_list_v = {l: {"embedding_vectors": emb_v[i:i + 1]} for i, l in enumerate(items)}
    test_u = [str(x) for x in rs.permutation(users)[:15]] + ["nobody", "u999"]
    test_v = [str(x) for x in rs.permutation(items)[:30]] + ["i777", "zzz"]
    rs.shuffle(test_v)
    test_rate = {}
    for u in test_u:
        liked = [str(x) for x in rs.choice(test_v, rs.randint(1, 6), replace=False)]
        liked += ["elsewhere%d" % j for j in range(rs.randint(0, 3))]
        test_rate[u] = {x: float(rs.randint(1, 6)) for x in liked}
    return users, items, emb_u, emb_v, node_list_u, node_list_v, test_u, test_v, test_rate


def _index_form(users, items, emb_u, emb_v, test_u, test_v, test_rate):
    from n2v_hip import recommend as rec
    table = np.concatenate([emb_u, emb_v])
    u_idx = rec.label_index(users, test_u)
    v_idx = rec.label_index(items, test_v)
    v_idx = np.where(v_idx >= 0, v_idx + len(users), -1).astype(np.int32)
    return (table, u_idx, v_idx) + rec.truth_csr(test_u, test_v, test_rate)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("top_n", [1, 5, 10, 40])
def test_vectorised_restatement_equals_the_literal_transcription(seed, top_n):
    users, items, emb_u, emb_v, nlu, nlv, test_u, test_v, test_rate = _dict_case(seed)
    detail = {}
    want = R.top_N_literal(test_u, test_v, test_rate, nlu, nlv, top_n, detail)
    table, u_idx, v_idx, ptr, pos, lens = _index_form(users, items, emb_u, emb_v, test_u, test_v, test_rate)
    assert (u_idx[-2:] == -1).all() and (v_idx == -1).sum() == 2
    S = R.scores(table, table.shape[1], u_idx, v_idx)
    # numpy's matrix product and the reference's per-pair dot may round differently: take the per-pair values
    for i, u in enumerate(test_u):
        for j, v in enumerate(test_v):
            if u_idx[i] >= 0 and v_idx[j] >= 0:
                S[i, j] = float(np.array(nlu[u]["embedding_vectors"]).dot(np.array(nlv[v]["embedding_vectors"]).T)[0][0])
    ranked, _ = R.ranked_lists(S, top_n)
    assert [[test_v[j] for j in row] for row in ranked] == detail["lists"]
    per_user = R.user_metrics(ranked, ptr, pos, lens)
    assert per_user.tolist() == detail["per_user"]
    assert R.averages(per_user) == want


def test_ties_follow_the_item_list_and_signed_zeros_tie():
    """What the rule decides: an unknown user gets the first k items of the list; -0.0 and +0.0 are one score."""
    S = np.array([[0.0, -0.0, 0.0, -0.0, 1.0, -1.0], [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0], [np.nan, -np.inf, 0.0, np.nan, 2.0, 2.0]])
    ranked, _ = R.ranked_lists(S, 4)
    assert ranked.tolist() == [[4, 0, 1, 2], [0, 1, 2, 3], [4, 5, 2, 1]]
    lit = sorted({j: float(s) for j, s in enumerate(S[0])}.items(), key=lambda x: x[1], reverse=True)[:4]
    assert [j for j, _ in lit] == ranked[0].tolist()


def test_host_tables_equal_the_reference_functions_bit_for_bit():
    import bine_train as bt
    from n2v_hip import recommend as rec
    disc = rec.discount_table(300)
    idcg = rec.idcg_table(300)
    assert disc.tolist() == [1 / math.log(i + 2, 2) for i in range(300)] == R.discount_table(300)
    for n in range(301):
        assert idcg[n] == R.IDCG(n) == bt.IDCG(n)
    for n in (1, 2, 7, 64, 300):
        lst = list(range(n))
        assert bt.nDCG(lst, lst) == R.nDCG(lst, lst) == sum(disc[:n].tolist()) / idcg[n]
        # a single hit at rank i contributes exactly discount[i]
        assert bt.nDCG(lst, [n - 1]) == disc[n - 1] / idcg[1]


def test_label_index_and_truth_csr():
    from n2v_hip import recommend as rec
    labels = np.array(sorted(["a", "b", "d", "k10", "k9"]))
    assert rec.label_index(labels, ["d", "zz", "a", "", "k9", "c"]).tolist() == [2, -1, 0, -1, 4, -1]
    assert rec.label_index(np.array([3, 5, 9]), [9, 4, 3, 10, -1]).tolist() == [2, -1, 0, -1, -1]
    assert rec.label_index(np.array([3, 5, 9]), ["3", "5"]).tolist() == [-1, -1]       # '3' is not 3 as a dict key
    assert rec.label_index(labels, []).tolist() == [] and rec.label_index(np.array([], dtype=str), ["a"]).tolist() == [-1]
    test_u = ["u2", "ghost", "u1"]
    test_v = ["i5", "i1", "i9", "i3"]
    test_rate = {"u1": {"i3": 4.0, "i5": 1.0, "gone": 5.0}, "u2": {"i9": 2.0}, "ghost": {"away": 1.0, "i1": 3.0}, "unused": {}}
    ptr, pos, lens = rec.truth_csr(test_u, test_v, test_rate)
    assert ptr.tolist() == [0, 1, 2, 4] and pos.tolist() == [2, 1, 0, 3] and lens.tolist() == [1, 2, 3]
    assert ptr.dtype == np.int64 and pos.dtype == np.int32
    # no test item inside the list at all: the denominators stay
    ptr, pos, lens = rec.truth_csr(["u1"], ["q"], test_rate)
    assert ptr.tolist() == [0, 0] and pos.tolist() == [] and lens.tolist() == [3]
    with pytest.raises(KeyError):
        rec.truth_csr(["u1", "missing"], test_v, test_rate)
    with pytest.raises(ZeroDivisionError):
        rec.truth_csr(["u1", "unused"], test_v, test_rate)
    # a repeated item label is refused by the builder and collapsed to its first place by the callers, as the
    # reference's recommend_dict[u] does
    with pytest.raises(ValueError, match="repeats"):
        rec.truth_csr(["u1"], ["i5", "i1", "i5"], test_rate)
    assert rec.unique_in_order(["i5", "i1", "i5", "i3", "i1"]) == ["i5", "i1", "i3"]
    users, items, emb_u, emb_v, nlu, nlv, tu, tv, tr = _dict_case(7)
    tv2 = tv + tv[:4]
    assert R.top_N_literal(tu, tv2, tr, nlu, nlv, 10) == R.top_N_literal(tu, rec.unique_in_order(tv2), tr, nlu, nlv, 10)


def test_without_a_gpu_there_is_no_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from n2v_hip import recommend as rec
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rec.top_n_lists(torch.zeros((4, 4), dtype=torch.float64), 4, [0], [1], 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rec.evaluate(torch.zeros((4, 4), dtype=torch.float64), 4, [0], [1], [0, 1], [0], [1], 1)


def test_top_N_without_a_gpu_is_the_host_path_it_was():
    """The drop-in keeps its host path where no GPU is visible; on distinct scores it equals the restatement."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import bine_train as bt
    users, items, emb_u, emb_v, nlu, nlv, test_u, test_v, test_rate = _dict_case(3, ties=False)
    test_u, test_v = test_u[:-2], [v for v in test_v if v in nlv]
    got = bt.top_N(test_u, test_v, test_rate, nlu, nlv, 10)
    want = R.top_N_literal(test_u, test_v, test_rate, nlu, nlv, 10)
    assert got == pytest.approx(want, rel=0, abs=1e-12)


# ================================================================================================ the input condition
@pytest.mark.parametrize("case", range(len(R.REAL_CASES)))
def test_real_cases_are_fit_for_an_exact_comparison(case):
    """No user of the committed real-valued inputs has two neighbouring scores among its best k + 1 closer than the sum
    of their forward bounds: the share the GPU test would have to leave out is 0.  Every case still has exact ties
    (the zeroed users) that only the list-order rule decides."""
    users, items, d, top_n = R.REAL_CASES[case]
    for seed in R.REAL_SEEDS:
        table, u_idx, v_idx = R.real_case(users, items, d, seed)
        S = R.scores(table, d, u_idx, v_idx)
        B = R.score_bound(table, d, u_idx, v_idx)
        bad, min_gap, max_bound, tied = R.ambiguous_users(S, B, top_n)
        print("case %s seed %d: ambiguous %d, smallest gap %.3g, largest bound %.3g, users with exact ties %d"
              % (R.REAL_CASES[case], seed, len(bad), min_gap, max_bound, tied))
        assert len(bad) == 0
        assert min_gap > 100 * max_bound
        assert tied >= users // 20


def test_integer_case_is_exact_and_cuts_tie_groups():
    table, u_idx, v_idx = R.integer_case()
    assert np.array_equal(table, np.round(table)) and np.abs(table).max() <= 3
    S = R.scores(table, 64, u_idx, v_idx)
    assert np.abs(S).max() <= 9 * 64 < 2 ** 53 and np.array_equal(S, np.round(S))
    ranked, score = R.ranked_lists(S, 10)
    cut = sum(1 for u in range(S.shape[0]) if np.sort(S[u])[::-1][10] == score[u, 9])
    print("integer case: max |score| %d, users whose top-10 cut falls inside a tie group: %d" % (np.abs(S).max(), cut))
    assert cut >= 20
    for d in (1, 3, 4, 37, 100, 256, 512):
        t, _, _ = R.integer_case(40, 300, d, seed=d)
        assert 9 * d < 2 ** 53 and np.array_equal(t, np.round(t))
