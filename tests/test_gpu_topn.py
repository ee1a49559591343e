"""GPU tests of the fused top-N kernels of the rating predictors (n2v_eccknn_topn, n2v_svd_topn) and of what is built on
them (top_n_lists, recommend, ranking_metrics, main_rec.py -topn).

Everything is compared by equality: item ids with torch.equal / ==, scores by their bytes.  The fused lists are held to
  * the restatement tests/topn_reference.py (a per-owner loop over the anti-testset and Python's stable reversed sort), and
  * the stored path on the device: every (owner, item) pair through estimate_batch + predict, the seen pairs masked, and a
    stable sort per owner,
for every N and every segment count of the case table; the result may not depend on the segments.  The case
(topn_reference.make_case; its edges are asserted by tests/test_topn_host.py) is 70 users x 150 items."""
import numpy as np
import pytest
import torch

import eccknn_reference as E
import rec_reference as R
import topn_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (ratings, class, similarity, user_based, k, min_k): k in {1, 40, 64, 65, 256} and min_k in {1, 3} on both sides
KNN_CONFIGS = ([("int", "eccen", "cosine", True, k, m) for k, m in ((1, 1), (40, 1), (40, 3), (64, 3), (65, 1), (256, 3))] +
               [("int", "eccen", "cosine", False, k, m) for k, m in ((1, 3), (40, 1), (64, 1), (65, 3), (256, 1))] +
               [("int", "eccen", "msd", True, 40, 1), ("int", "eccen", "msd", False, 65, 3),
                ("int", "knn", "pearson", True, 40, 1), ("int", "knn", "pearson", False, 256, 3),
                ("fp64", "eccen", "cosine", True, 40, 1), ("fp64", "eccen", "msd", False, 40, 3)])
SVD_CONFIGS = [(nf, biased) for nf in (1, 64, 65, 256) for biased in (True, False)]


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)


@pytest.fixture(scope="module")
def world():
    """The two cases with their trainsets, the fitted k-NN models and the seen CSR, each built once."""
    from n2v_hip import eccknn
    out = {"fit": {}}
    for kind in ("int", "fp64"):
        case = T.make_case(kind)
        ts = eccknn.Trainset.from_ratings(case["raw_u"], case["raw_i"], case["r"], rating_scale=case["scale"])
        assert np.array_equal(ts.u, case["u"]) and np.array_equal(ts.i, case["i"]) and ts.global_mean == case["mean"]
        seen = eccknn.csr_by_x(dev(ts.u, torch.int32), dev(ts.i, torch.int32), dev(ts.r, torch.float64), ts.n_users, ts.n_items)
        out[kind] = (case, ts, seen)
    return out


def fitted(world, kind, cls, name, user_based):
    """The fitted model of one similarity and side, with NaN planted in the Pearson matrix; built once per module."""
    from n2v_hip import eccknn
    key = (kind, cls, name, user_based)
    if key not in world["fit"]:
        case, ts, _ = world[kind]
        opts = {"name": name, "user_based": user_based}
        w = case["w_items"] if user_based else case["w_users"]
        algo = (eccknn.EccenKNN(sim_options=opts, device=DEV) if cls == "eccen" else eccknn.KNNBasic(sim_options=opts, device=DEV))
        algo.fit(ts, w)
        if name == "pearson":                                     # NaN similarities: they rank below every neighbour
            n_x = algo.sim.shape[0]
            rs = np.random.RandomState(5)
            a, b = rs.randint(0, n_x, 200), rs.randint(0, n_x, 200)
            a, b = a[a != b], b[a != b]
            algo.sim[dev(a, torch.int64), dev(b, torch.int64)] = float("nan")
            algo.sim[dev(b, torch.int64), dev(a, torch.int64)] = float("nan")
            assert bool(torch.isnan(algo.sim).any())
        world["fit"][key] = algo
    return world["fit"][key]


def stored_path(pred, seen_mask, n_items):
    """The stored path's lists at n = 256 from the [n_owners][n_items] predictions: seen pairs masked to -inf (no
    prediction is: it was clipped to lo), a stable ascending sort of the negated rows, (-1, NaN) behind the candidates."""
    neg = torch.where(seen_mask, torch.full_like(pred, float("inf")), -pred)
    val, idx = torch.sort(neg, dim=1, stable=True)
    items = torch.where(torch.isinf(val), torch.full_like(idx, -1), idx).to(torch.int32)
    score = torch.where(torch.isinf(val), torch.full_like(val, float("nan")), torch.gather(pred, 1, idx))
    pad = 256 - n_items
    items = torch.cat([items, torch.full((items.shape[0], pad), -1, dtype=torch.int32, device=items.device)], 1)
    score = torch.cat([score, torch.full((score.shape[0], pad), float("nan"), dtype=torch.float64, device=score.device)], 1)
    return items, score


def seen_mask_of(case, owners):
    mask = np.zeros((len(owners), case["n_items"]), dtype=bool)
    for row, u in enumerate(owners):
        if 0 <= u < case["n_users"]:
            mask[row, sorted(case["seen"][u])] = True
    return dev(mask, torch.bool)


def assert_same(got, want, what):
    """Item ids equal; scores equal by their bytes wherever there is an item, NaN wherever there is none."""
    gi, gs = got
    wi, ws = want
    assert gi.dtype == torch.int32 and gs.dtype == torch.float64 and gi.shape == gs.shape == wi.shape, what
    assert torch.equal(gi, wi), what
    real = wi >= 0
    assert torch.equal(gs.view(torch.int64)[real], ws.view(torch.int64)[real]), what
    assert bool(torch.isnan(gs[~real]).all()), what


def check_all_n_and_segments(fused, ranked, stored, what):
    """fused(n, segments) against the restated rankings and the stored lists, for every N and S of the case table."""
    for n in T.NS:
        wi, ws = T.lists(ranked, n)
        want = (dev(wi, torch.int32), dev(ws, torch.float64))
        assert_same((stored[0][:, :n], stored[1][:, :n]), want, (what, n, "stored path vs restatement"))
        for S in T.SEGMENTS:
            got = fused(n, S)
            assert_same(got, want, (what, n, S, "fused vs restatement"))
            assert_same(got, (stored[0][:, :n].contiguous(), stored[1][:, :n].contiguous()), (what, n, S, "fused vs stored path"))


# ---- the kernels --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,cls,name,user_based,k,min_k", KNN_CONFIGS,
                         ids=["%s-%s-%s-%s-k%d-mink%d" % (c[0], c[1], c[2], "user" if c[3] else "item", c[4], c[5]) for c in KNN_CONFIGS])
def test_knn_fused_equals_restatement_and_stored_path(world, kind, cls, name, user_based, k, min_k):
    from n2v_hip import eccknn
    case, ts, seen = world[kind]
    algo = fitted(world, kind, cls, name, user_based)
    owners = T.owner_list(case)
    yr = T.side(case, user_based)[1]
    predict = T.knn_predictor(algo.sim.cpu().numpy(), yr, user_based, k, min_k, case["mean"], *case["scale"])
    ranked = T.rankings(case["seen"], case["n_items"], owners, predict)
    # the stored path: every pair, calls that exist without the fused kernel
    qu = dev(np.repeat(owners, case["n_items"]), torch.int32)
    qi = dev(np.tile(np.arange(case["n_items"]), len(owners)), torch.int32)
    qx, qy = (qu, qi) if user_based else (qi, qu)
    est, _, imp = eccknn.estimate_batch(algo.sim, algo.yr, qx, qy, k, min_k)
    pred = eccknn.predict(est, imp, case["mean"], case["scale"]).view(len(owners), case["n_items"])
    stored = stored_path(pred, seen_mask_of(case, owners), case["n_items"])
    fused = lambda n, S: eccknn.top_n(algo.sim, algo.yr, seen, user_based, k, min_k, case["mean"], case["scale"], n,
                                      dev(owners, torch.int32), S)
    check_all_n_and_segments(fused, ranked, stored, (kind, cls, name, user_based, k, min_k))
    # the rows the case plants: rated everything, all but three, unknown
    items, score = fused(10, None)
    full, almost = case["users"].index("full"), case["users"].index("almost")
    assert (items[full] == -1).all() and torch.isnan(score[full]).all()
    assert (items[almost][:3] >= 0).all() and (items[almost][3:] == -1).all()
    unknown = int(np.nonzero(owners == -1)[0][0])
    mean = min(case["scale"][1], max(case["scale"][0], case["mean"]))
    assert items[unknown].tolist() == list(range(10)) and score[unknown].tolist() == [mean] * 10
    # owners None is every user
    every = eccknn.top_n(algo.sim, algo.yr, seen, user_based, k, min_k, case["mean"], case["scale"], 10)
    assert torch.equal(every[0], items[:case["n_users"]])


@pytest.mark.parametrize("n_factors,biased", SVD_CONFIGS, ids=["f%d-%s" % (f, "biased" if b else "unbiased") for f, b in SVD_CONFIGS])
def test_svd_fused_equals_restatement_and_stored_path(world, n_factors, biased):
    from n2v_hip import eccknn, svd
    case, ts, seen = world["int"]
    lo, hi = (1.0, 5.0) if biased else (-1.0, 1.0)                # a scale the untrained model leaves on both ends
    model = T.svd_tables(case, n_factors)
    mu = model[0] if biased else 0.0
    model = (mu,) + model[1:]
    bu, bi, pu, qi = (dev(a, torch.float64) for a in model[1:])
    owners = T.owner_list(case)
    predict = T.svd_predictor(model, biased, case["mean"], lo, hi)
    ranked = T.rankings(case["seen"], case["n_items"], owners, predict)
    kinds = {("lo" if s == lo else "hi" if s == hi else "in") for lst in ranked for _, s in lst}
    assert kinds == {"lo", "hi", "in"}
    qu = dev(np.repeat(owners, case["n_items"]), torch.int32)
    qi_ids = dev(np.tile(np.arange(case["n_items"]), len(owners)), torch.int32)
    est, imp = svd.estimate_batch(mu, biased, bu, bi, pu, qi, qu, qi_ids)
    pred = eccknn.predict(est, imp, case["mean"], (lo, hi)).view(len(owners), case["n_items"])
    stored = stored_path(pred, seen_mask_of(case, owners), case["n_items"])
    fused = lambda n, S: svd.top_n(mu, biased, bu, bi, pu, qi, seen, case["mean"], (lo, hi), n, dev(owners, torch.int32), S)
    check_all_n_and_segments(fused, ranked, stored, (n_factors, biased))
    if not biased:                                                # 'User and item are unknown.': the training mean
        unknown = int(np.nonzero(owners == -1)[0][0])
        items, score = fused(10, None)
        assert items[unknown].tolist() == list(range(10)) and score[unknown].tolist() == [min(hi, case["mean"])] * 10


def test_malformed_seen_csr_is_a_value_error(world):
    from n2v_hip import eccknn, svd
    case, ts, seen = world["int"]
    algo = fitted(world, "int", "eccen", "cosine", True)
    ptr, items, r = seen
    swapped = items.clone()
    row = int(ptr[case["users"].index("full")])
    swapped[row], swapped[row + 1] = items[row + 1], items[row]  # one row no longer ascending
    repeated = items.clone()
    repeated[row + 1] = items[row]
    outside = items.clone()
    outside[row + 5] = case["n_items"]
    negative = items.clone()
    negative[0] = -1
    bad_ptr = ptr.clone()
    bad_ptr[3] = ptr[-1] + 7
    model = [dev(a, torch.float64) for a in T.svd_tables(case, 8)[1:]]
    for bad in ((ptr, swapped, r), (ptr, repeated, r), (ptr, outside, r), (ptr, negative, r), (bad_ptr, items, r),
                (ptr[:-1], items, r), (ptr.to(torch.int32), items, r)):
        with pytest.raises(ValueError, match="malformed CSR|rows for|seen must be"):
            eccknn.top_n(algo.sim, algo.yr, bad, True, 40, 1, case["mean"], case["scale"], 10)
        with pytest.raises(ValueError, match="malformed CSR|rows for|seen must be"):
            svd.top_n(case["mean"], True, *model, bad, case["mean"], case["scale"], 10)
    for bad_k, bad_min_k in ((0, 1), (257, 1), (40, 0)):
        with pytest.raises(ValueError):
            eccknn.top_n(algo.sim, algo.yr, seen, True, bad_k, bad_min_k, case["mean"], case["scale"], 10)
    with pytest.raises(ValueError, match="owners"):
        eccknn.top_n(algo.sim, algo.yr, seen, True, 40, 1, case["mean"], case["scale"], 10, owners=[])


# ---- the classes --------------------------------------------------------------------------------------------------------

def restated_truth(case, testset, threshold):
    """ranking_metrics' ground truth, restated: users with at least one (counted) test item in order of first appearance,
    the inner ids of the items the trainset knows ascending, and the count of all of them."""
    truth = {}
    for ru, ri, r in testset:
        truth.setdefault(ru, set())
        if threshold is None or r >= threshold:
            truth[ru].add(ri)
    users = [ru for ru in truth if truth[ru]]
    ptr, pos, lens = [0], [], []
    for ru in users:
        pos.extend(sorted(case["items"].index(ri) for ri in truth[ru] if ri in case["items"]))
        ptr.append(len(pos))
        lens.append(len(truth[ru]))
    return users, np.array(ptr, np.int64), np.array(pos, np.int32), np.array(lens, np.int64)


def make_testset(case, seed=3):
    """(raw user, raw item, rating) triples: unrated pairs of known users, items the trainset does not know, a user it
    does not know, and a user whose only test rating is low."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(300):
        u, i = int(rs.randint(case["n_users"])), int(rs.randint(case["n_items"]))
        if i not in case["seen"][u]:
            out.append((case["users"][u], case["items"][i], float(rs.randint(1, 6))))
    out += [(case["users"][4], "new-item", 5.0), ("stranger", case["items"][2], 4.0), ("stranger", "new-item", 5.0),
            ("low-only", case["items"][7], 1.0)]
    return out


@pytest.mark.parametrize("which", ["eccen-user", "eccen-item", "knn-pearson", "mf"])
def test_lists_recommend_and_ranking_metrics(world, which):
    from n2v_hip import eccknn, svd
    case, ts, seen = world["int"]
    if which == "mf":
        algo = svd.SVD(n_factors=8, n_epochs=3, n_strata=2, device=DEV).fit(ts)
        model = (algo.mu,) + tuple(t.cpu().numpy() for t in (algo.bu, algo.bi, algo.pu, algo.qi))
        predict = T.svd_predictor(model, True, case["mean"], *case["scale"])
    else:
        cls, name, user_based = {"eccen-user": ("eccen", "cosine", True), "eccen-item": ("eccen", "msd", False),
                                 "knn-pearson": ("knn", "pearson", True)}[which]
        algo = fitted(world, "int", cls, name, user_based)
        predict = T.knn_predictor(algo.sim.cpu().numpy(), T.side(case, user_based)[1], user_based, algo.k, algo.min_k,
                                  case["mean"], *case["scale"])
    every = T.rankings(case["seen"], case["n_items"], range(case["n_users"]), predict)
    # top_n_lists: raw users, unknown ones are owner -1, repeats allowed, segments free
    raw = ["almost", "stranger", case["users"][0], "full", case["users"][0]]
    inner = [case["users"].index(u) if u in case["users"] else -1 for u in raw]
    picked = T.rankings(case["seen"], case["n_items"], inner, predict)
    for n, S in ((10, None), (10, 7), (1, 3), (65, 64)):
        wi, ws = T.lists(picked, n)
        assert_same(algo.top_n_lists(n, raw, S), (dev(wi, torch.int32), dev(ws, torch.float64)), (which, n, S))
    wi, ws = T.lists(every, 10)
    assert_same(algo.top_n_lists(), (dev(wi, torch.int32), dev(ws, torch.float64)), which)
    # recommend: raw ids, fillers dropped
    recs = algo.recommend(5)
    assert list(recs) == case["users"]
    for u, ru in enumerate(case["users"]):
        assert recs[ru] == [(case["items"][i], s) for i, s in every[u][:5]], ru
    assert recs["full"] == [] and len(recs["almost"]) == 3
    some = algo.recommend(3, users=["stranger", "almost"])
    unknown = T.rankings(case["seen"], case["n_items"], [-1], predict)[0]
    assert list(some) == ["stranger", "almost"] and some["stranger"] == [(case["items"][i], s) for i, s in unknown[:3]]
    assert some["almost"] == recs["almost"]
    if which != "mf":                                             # every estimate impossible: items 0, 1, 2 at one score
        assert [i for i, _ in unknown[:3]] == [0, 1, 2] and len(set(s for _, s in unknown)) == 1
    # ranking_metrics against the restated metrics on the restated lists
    testset = make_testset(case)
    for n, threshold in ((10, None), (10, 4), (3, 4.5)):
        users, ptr, pos, lens = restated_truth(case, testset, threshold)
        assert "stranger" in users and ("low-only" in users) == (threshold is None)
        owners = [case["users"].index(u) if u in case["users"] else -1 for u in users]
        ranked_items = T.lists(T.rankings(case["seen"], case["n_items"], owners, predict), n)[0]
        per_user = R.user_metrics(ranked_items, ptr, pos, lens)
        f1, m_ap, mrr, ndcg, got = algo.ranking_metrics(testset, n, threshold)
        assert E.canon(got) == E.canon(per_user), (which, n, threshold)
        assert (f1, m_ap, mrr, ndcg) == R.averages(per_user)
    with pytest.raises(ValueError, match="no user"):
        algo.ranking_metrics([("low-only", case["items"][7], 1.0)], 10, threshold=2)


# ---- main_rec.py --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo_flags", [["-algo", "eccen", "-k", "20", "-sim", "msd"], ["-algo", "knn", "-sim", "pearson", "-item-based"],
                                        ["-algo", "mf", "-factors", "8", "-epochs", "3", "-strata", "2"]], ids=["eccen", "knn", "mf"])
def test_main_rec_topn_end_to_end(world, tmp_path, capsys, algo_flags):
    import main_rec
    case = world["int"][0]
    p = tmp_path / "ratings.csv"
    p.write_text("user,item,rating\n" + "".join("%s,%s,%r\n" % t for t in zip(case["raw_u"], case["raw_i"], case["r"].tolist())))
    base = ["-input", str(p), "-seed", "2"] + algo_flags
    plain = main_rec.main(base)
    assert isinstance(plain, float) and capsys.readouterr().out.strip() == "RMSE: %r" % plain
    recs_file = tmp_path / "recs.csv"
    rmse, metrics = main_rec.main(base + ["-topn", "5", "-threshold", "4", "-save-recs", str(recs_file)])
    out = capsys.readouterr().out.strip().split("\n")
    assert rmse == plain and out == ["RMSE: %r" % rmse, "F1 / MAP / MRR / NDCG @5: %r / %r / %r / %r" % tuple(metrics)]
    # the same split and model by hand
    args = main_rec.parse_args(base + ["-topn", "5", "-threshold", "4"])
    users, items, ratings = main_rec.read_ratings(str(p))
    train, test = main_rec.split(len(ratings), 0.2, 2)
    algo = main_rec.fit_split(args, users, items, ratings, None, train)
    testset = [(users[i], items[i], ratings[i]) for i in test]
    assert tuple(metrics) == algo.ranking_metrics(testset, 5, 4.0)[:4] and 0.0 <= min(metrics) and max(metrics) <= 1.0
    want = ["%s,%s,%r" % (u, i, s) for u, lst in algo.recommend(5).items() for i, s in lst]
    assert recs_file.read_text().split("\n")[:-1] == want and len(want) > 5 * 60
    # -cv: one file per fold, one metrics line per fold
    folds = main_rec.main(base + ["-cv", "2", "-topn", "3", "-save-recs", str(tmp_path / "cv.csv")])
    out = capsys.readouterr().out.strip().split("\n")
    assert len(folds) == 2 and all(len(f) == 2 and len(f[1]) == 4 for f in folds)
    assert [l.split(":")[0] for l in out] == ["RMSE", "F1 / MAP / MRR / NDCG @3"] * 2 + ["mean RMSE"]
    assert sorted(f.name for f in tmp_path.iterdir() if f.name.startswith("cv.csv")) == ["cv.csv.0", "cv.csv.1"]
