"""CPU tests of the EccenKNN path: the restatement tests/eccknn_reference.py against itself and against the textbook
cosine, the Trainset bookkeeping, the error paths of n2v_hip.eccknn and the argument parser of main_rec.py."""
import numpy as np
import pytest

import eccknn_reference as E

SMALL = [  # (seed, n_x, n_y, n_ratings, kind, zeros)
    (1, 1, 1, 1, "int", 0),
    (2, 2, 3, 5, "int", 1),
    (3, 9, 7, 30, "int", 0),
    (4, 17, 12, 90, "half", 3),
    (5, 23, 11, 120, "fp64", 4),
    (6, 12, 30, 150, "fp64", 0),
]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "%dx%d-%s" % (c[1], c[2], c[4]))
@pytest.mark.parametrize("name", ["cosine", "msd"])
@pytest.mark.parametrize("min_support", [1, 3])
def test_numpy_form_equals_the_literal_loops(case, name, min_support):
    seed, n_x, n_y, n, kind, zeros = case
    x, y, r, w = E.make_case(seed, n_x, n_y, n, kind, zeros)
    assert (w < 0).any() or n_y < 3
    yr = E.build_yr(x, y, r)
    lit, fast = E.LITERAL[name](n_x, yr, min_support, w), E.NUMPY[name](n_x, yr, min_support, w)
    assert set(lit) == set(fast)
    for key in lit:
        assert E.canon(lit[key]) == E.canon(fast[key]), key
    assert np.array_equal(np.diag(lit["sim"]), np.ones(n_x))


def test_case_generator_gives_inner_ids_and_plants_its_edges():
    x, y, r, w = E.make_case(7, 20, 15, 100, "int", zeros=2)
    for v, n in ((x, 20), (y, 15)):
        inner, raw = E.inner_ids(v.tolist())
        assert np.array_equal(inner, v) and raw == list(range(len(raw))) and len(raw) <= n
    assert len(set(zip(x.tolist(), y.tolist()))) == len(x)
    assert (r == 0.0).sum() == 2
    yr = E.build_yr(x, y, r)
    single = [k for k, v in yr.items() if len(v) == 1]
    assert single, "no y with a single rater"
    freq = E.cosine_numpy(20, yr, 1, w)["freq"]
    off = freq - np.diag(np.diag(freq))
    assert ((off.sum(axis=1) == 0) & (np.diag(freq) > 0)).any(), "no x that shares nothing"


def test_cosine_with_unit_weights_is_the_textbook_cosine():
    x, y, r, _ = E.make_case(8, 30, 20, 250, "int")
    yr = E.build_yr(x, y, r)
    sim = E.cosine_numpy(30, yr, 1, np.ones(20))["sim"]
    dense = np.zeros((30, 20)); have = np.zeros((30, 20), bool)
    dense[x, y] = r; have[x, y] = True
    checked = 0
    for i in range(30):
        for j in range(i + 1, 30):
            co = have[i] & have[j]
            if not co.any():
                assert sim[i, j] == 0.0
                continue
            a, b = dense[i, co], dense[j, co]
            # integer ratings: every sum is exact, so the textbook formula is the same fp64 number
            want = float(np.dot(a, b)) / np.sqrt(float(np.dot(a, a)) * float(np.dot(b, b)))
            assert sim[i, j] == want == sim[j, i]
            checked += 1
    assert checked > 100


def test_estimate_rule_of_the_restatement():
    sim = np.array([[1.0, 0.5, 0.5, -0.0, np.nan, 0.25],
                    [0.5, 1.0, 0, 0, 0, 0], [0.5, 0, 1, 0, 0, 0], [-0.0, 0, 0, 1, 0, 0],
                    [np.nan, 0, 0, 0, 1, 0], [0.25, 0, 0, 0, 0, 1]])
    yr = {0: [(4, 5.0), (3, 1.0), (2, 2.0), (1, 4.0), (5, 3.0)]}
    # NaN last; the two 0.5 in list order (x=2 first); k = 1 keeps x=2 only
    assert E.estimate(sim, yr, 0, 0, 1, 1) == (2.0, {"actual_k": 1})
    est, d = E.estimate(sim, yr, 0, 0, 3, 1)
    assert d == {"actual_k": 3} and est == (0.5 * 2.0 + 0.5 * 4.0 + 0.25 * 3.0) / (0.5 + 0.5 + 0.25)
    assert E.estimate(sim, yr, 0, 0, 5, 1)[1] == {"actual_k": 3}
    with pytest.raises(E.PredictionImpossible):
        E.estimate(sim, yr, 0, 0, 5, 4)
    with pytest.raises(E.PredictionImpossible):
        E.estimate(sim, yr, -1, 0, 5, 1)
    with pytest.raises(E.PredictionImpossible):
        E.estimate(sim, yr, 0, 1, 5, 1)          # nobody rated y = 1


def test_trainset_ids_and_order():
    from n2v_hip import eccknn
    users = ["u9", "u2", "u9", "u5", "u2", "u5"]
    items = [70, 70, 30, 30, 10, 70]
    r = [4.0, 3.0, 0.5, 2.0, 5.0, 1.0]
    ts = eccknn.Trainset.from_ratings(users, items, r)
    assert ts.u.tolist() == [0, 1, 0, 2, 1, 2] and ts.i.tolist() == [0, 0, 1, 1, 2, 0]
    assert (ts.n_users, ts.n_items, ts.n_ratings) == (3, 3, 6)
    assert ts.to_inner_uid("u5") == 2 and ts.to_inner_iid(10) == 2
    with pytest.raises(ValueError):
        ts.to_inner_uid("nobody")
    assert ts.knows_user(2) and not ts.knows_user(3) and ts.knows_item(0) and not ts.knows_item(-1)
    ptr, other, rr = ts.ir                      # item 70: users u9, u2, u5 in training order
    assert ptr.tolist() == [0, 3, 5, 6] and other.tolist() == [0, 1, 2, 0, 2, 1] and rr.tolist() == [4.0, 3.0, 1.0, 0.5, 2.0, 5.0]
    ptr, other, rr = ts.ur
    assert ptr.tolist() == [0, 2, 4, 6] and other.tolist() == [0, 1, 0, 2, 1, 0]
    assert ts.global_mean == E.global_mean(r) and ts.rating_scale == (0.5, 5.0)
    assert ts.inner_uids(["u2", "zz"]).tolist() == [1, -1]
    # the restatement's first-appearance rule is the same one
    assert np.array_equal(E.inner_ids(users)[0], ts.u) and np.array_equal(E.inner_ids(items)[0], ts.i)
    rs = np.random.RandomState(3)
    big = rs.normal(size=5000) * 1e3
    ts2 = eccknn.Trainset.from_ratings(range(5000), [0] * 5000, big)
    assert ts2.global_mean == E.global_mean(big)


def test_trainset_takes_any_hashable_raw_id():
    """Raw ids are dictionary keys, as surprise's are: numbers, strings, tuples and None may share a column, 1 and "1" are
    two users, and nothing is coerced to a common type."""
    from n2v_hip import eccknn
    users = [1, "a", 2, (1, 2), None, "1", 1]
    items = ["x", "x", 7, (7,), 7, "7", 7]
    ts = eccknn.Trainset.from_ratings(users, items, [1.0, 2.0, 3.0, 4.0, 5.0, 1.5, 2.5])
    assert ts.u.tolist() == [0, 1, 2, 3, 4, 5, 0] and ts.i.tolist() == [0, 0, 1, 2, 1, 3, 1]
    assert (ts.n_users, ts.n_items) == (6, 4)
    assert ts.inner_uids([1, 2, (1, 2), None, "1", "2"]).tolist() == [0, 2, 3, 4, 5, -1]
    assert ts.to_inner_iid((7,)) == 2 and ts.to_inner_iid("7") == 3 and ts.to_inner_iid(7) == 1


def test_error_paths():
    from n2v_hip import eccknn
    with pytest.raises(NameError, match=r"Wrong sim name jaccard\. Allowed values are cosine, msd, pearson, pearson_baseline\."):
        eccknn.EccenKNN(sim_options={"name": "jaccard"})
    with pytest.raises(NameError, match="pearson"):
        eccknn.EccenKNN(sim_options={"name": "pearson"})
    for k in (0, eccknn.MAX_K + 1):
        with pytest.raises(ValueError, match="k %d outside" % k):
            eccknn.EccenKNN(k=k, sim_options={"name": "cosine"})
    with pytest.raises(ValueError, match="min_k"):
        eccknn.EccenKNN(min_k=0, sim_options={"name": "cosine"})
    with pytest.raises(ValueError, match="duplicate"):
        eccknn.Trainset.from_ratings([1, 2, 1], [5, 5, 5], [1.0, 2.0, 3.0])
    ts = eccknn.Trainset.from_ratings([1, 2, 1], [5, 5, 6], [1.0, 2.0, 3.0])
    algo = eccknn.EccenKNN(sim_options={"name": "cosine", "user_based": True})
    with pytest.raises(KeyError):
        algo.fit(ts, {5: 1.0})                  # item 6 has no weight: i_dict[y]
    with pytest.raises(ValueError, match="weights"):
        algo.fit(ts, np.ones(3))
    item_based = eccknn.EccenKNN(sim_options={"name": "msd", "user_based": False})
    with pytest.raises(KeyError):
        item_based.fit(ts, {1: 1.0})            # y are users here: user 2 has no weight


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from n2v_hip import eccknn
    ts = eccknn.Trainset.from_ratings([1, 2, 1], [5, 5, 6], [1.0, 2.0, 3.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eccknn.EccenKNN(sim_options={"name": "cosine"}).fit(ts, np.ones(2))


def test_main_rec_argument_parser_and_readers(tmp_path):
    import main_rec
    a = main_rec.parse_args(["-input", "r.csv"])
    assert (a.k, a.mink, a.sim, a.item_based, a.weights, a.test_ratio, a.seed, a.cv) == (40, 1, "cosine", False, None, 0.2, 0, 0)
    a = main_rec.parse_args("-input r.csv -k 20 -mink 2 -sim msd -item-based -weights w.csv -test-ratio 0.1 -cv 5".split())
    assert (a.k, a.mink, a.sim, a.item_based, a.weights, a.test_ratio, a.cv) == (20, 2, "msd", True, "w.csv", 0.1, 5)
    for bad in (["-k", "3"], ["-input", "r.csv", "-test-ratio", "1.5"], ["-input", "r.csv", "-cv", "1"]):
        with pytest.raises(SystemExit):
            main_rec.parse_args(bad)
    p = tmp_path / "r.csv"
    p.write_text("userId,movieId,rating,timestamp\n1,10,4.5,99\n2,10,3,98\n\n1,11,0,97\n")
    users, items, ratings = main_rec.read_ratings(str(p))
    assert users == ["1", "2", "1"] and items == ["10", "10", "11"] and ratings.tolist() == [4.5, 3.0, 0.0]
    q = tmp_path / "w.csv"
    q.write_text("id,weight\n10,0.25\n11,-1.5\n")
    assert main_rec.read_weights(str(q)) == {"10": 0.25, "11": -1.5}
    train, test = main_rec.split(10, 0.2, 0)
    assert len(test) == 2 and sorted(train.tolist() + test.tolist()) == list(range(10)) and train.tolist() == sorted(train.tolist())
    seen = []
    for tr, te in main_rec.folds(10, 3, 0):
        assert sorted(tr.tolist() + te.tolist()) == list(range(10))
        seen += te.tolist()
    assert sorted(seen) == list(range(10))
