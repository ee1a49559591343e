"""GPU tests of the centred k-NN predictors: n2v_eccknn_row_moments, n2v_eccknn_estimate_centered, n2v_eccknn_topn_centered and
the classes KNNWithMeans / KNNWithZScore / KNNBaseline with main_rec.py's -algo knnmeans | knnzscore | knnbaseline on top.

Everything is compared by equality against the restatement tests/knn_centered_reference.py: ids and counts with ==, scores by
their bytes (eccknn_reference.canon: a NaN's sign and payload are not part of the contract, as everywhere in n2v_sim.h).
The case is topn_reference.make_case, 70 users x 150 items, with NaN planted in a Pearson matrix that has non-positive
entries of its own.  A malformed rating list is only ever shown to the host-side range check: no test launches an estimate
kernel on ids outside their range."""
import numpy as np
import pytest
import torch

import eccknn_pearson_reference as P
import eccknn_reference as E
import knn_centered_reference as C
import rec_reference as R
import topn_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_MIN_K = ((1, 1), (40, 1), (40, 3), (64, 3), (65, 1), (256, 3))
SIDES = (True, False)


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)


def classes():
    from n2v_hip import eccknn
    return {"means": eccknn.KNNWithMeans, "zscore": eccknn.KNNWithZScore, "baseline": eccknn.KNNBaseline}


@pytest.fixture(scope="module")
def world():
    """The two cases with their trainsets and seen CSRs, the restated ALS baselines, and the fitted models; each once."""
    from n2v_hip import eccknn
    out = {"fit": {}}
    for kind in ("int", "fp64"):
        case = T.make_case(kind)
        ts = eccknn.Trainset.from_ratings(case["raw_u"], case["raw_i"], case["r"], rating_scale=case["scale"])
        assert np.array_equal(ts.u, case["u"]) and np.array_equal(ts.i, case["i"]) and ts.global_mean == case["mean"]
        seen = eccknn.csr_by_x(dev(ts.u, torch.int32), dev(ts.i, torch.int32), dev(ts.r, torch.float64), ts.n_users, ts.n_items)
        ur, ir = P.rows_of(case["u"], case["i"], case["r"], ts.n_users), P.rows_of(case["i"], case["u"], case["r"], ts.n_items)
        case["bu"], case["bi"] = P.baselines_als(ur, ir, case["mean"])
        out[kind] = (case, ts, seen)
    return out


def fitted(world, kind, mode, user_based):
    """(fitted model, its similarity on the host, the restatement's tables and yr).  The similarity is Pearson with NaN
    planted the way tests/test_gpu_topn.py plants it; its own entries are negative for about every other pair."""
    key = (kind, mode, user_based)
    if key not in world["fit"]:
        case, ts, _ = world[kind]
        algo = classes()[mode](sim_options={"name": "pearson", "user_based": user_based}, device=DEV)
        algo.fit(ts, case["w_items"] if user_based else case["w_users"])
        n_x = algo.sim.shape[0]
        rs = np.random.RandomState(5)
        a, b = rs.randint(0, n_x, 200), rs.randint(0, n_x, 200)
        a, b = a[a != b], b[a != b]
        algo.sim[dev(a, torch.int64), dev(b, torch.int64)] = float("nan")
        algo.sim[dev(b, torch.int64), dev(a, torch.int64)] = float("nan")
        sim = algo.sim.cpu().numpy()
        assert np.isnan(sim).any() and (sim < 0).any() and (sim == 0).any()
        x, y = (case["u"], case["i"]) if user_based else (case["i"], case["u"])
        n_y = case["n_items"] if user_based else case["n_users"]
        tab = C.tables(mode, x, y, case["r"], n_x, n_y, user_based, case["mean"], case["bu"], case["bi"])
        world["fit"][key] = (algo, sim, tab, T.side(case, user_based)[1])
    return world["fit"][key]


def assert_tables(algo, tab):
    """The fit's tables are the restatement's, byte for byte."""
    c = algo.centering
    assert c.mode == tab["mode"] and bool(c.user_based) == tab["user_based"] and c.global_mean == tab["gm"]
    if tab["mode"] == "baseline":
        assert E.canon(c.tx.cpu().numpy()) == E.canon(tab["bx"]) and E.canon(c.by.cpu().numpy()) == E.canon(tab["by"])
        return
    assert E.canon(c.tx.cpu().numpy()) == E.canon(tab["mu"])
    if tab["mode"] == "zscore":
        assert E.canon(c.sd.cpu().numpy()) == E.canon(tab["sd"]) and algo.overall_sigma == tab["overall_sd"]


def queries(case, user_based):
    """All items of a few owners (the two long rows among them), then unknown user / item / both and ids past the end."""
    owners = [case["users"].index("full"), case["users"].index("almost"), 0, 7, 33]
    qu = np.repeat(owners, case["n_items"]).tolist() + [-1, -1, 3, 3, -1, case["n_users"], 2, case["n_users"] + 5]
    qi = np.tile(np.arange(case["n_items"]), len(owners)).tolist() + [0, 5, -1, case["n_items"], -1, 4, case["n_items"] + 9, -1]
    qu, qi = np.array(qu, dtype=np.int32), np.array(qi, dtype=np.int32)
    return (qu, qi) + ((qu, qi) if user_based else (qi, qu))


# ---- row moments --------------------------------------------------------------------------------------------------------

def test_row_moments_equal_the_restatement():
    from n2v_hip import eccknn
    rs = np.random.RandomState(11)
    rows = [rs.normal(size=n) * 3.0 + 2.0 for n in (0, 1, 63, 64, 65, 130)] + [np.full(70, 2.5), np.full(1, -0.0), rs.randint(1, 6, 97) * 1.0]
    ptr = dev(np.cumsum([0] + [len(r) for r in rows]), torch.int64)
    flat = dev(np.concatenate(rows), torch.float64)
    for zero_sigma in (None, 1.75, float("nan")):
        mu, sd = eccknn.row_moments(ptr, flat, zero_sigma)
        wmu, wsd = C.row_moments(rows, zero_sigma)
        assert mu.dtype == sd.dtype == torch.float64 and mu.shape == sd.shape == (len(rows),)
        assert E.canon(mu.cpu().numpy()) == E.canon(wmu) and E.canon(sd.cpu().numpy()) == E.canon(wsd), zero_sigma
        assert np.isnan(wmu[0]) and np.isnan(wsd[0]) and wsd[1] == (1.75 if zero_sigma == 1.75 else 0.0)
        assert wsd[6] == wsd[7] == (1.75 if zero_sigma == 1.75 else 0.0) and wmu[6] == 2.5
    # the overall form: every value as one row
    mu, sd = eccknn.row_moments(dev([0, flat.numel()], torch.int64), flat)
    want = C.moments(np.concatenate(rows))
    assert (float(mu.item()), float(sd.item())) == want and want[1] > 0
    # a pointer past the end is clamped (the last row simply ends with the data), and bad arguments are ValueErrors
    over = ptr.clone()
    over[-1] += 1000
    assert E.canon(eccknn.row_moments(over, flat)[0].cpu().numpy()) == E.canon(C.row_moments(rows)[0])
    for bad in ((ptr.to(torch.int32), flat), (ptr, flat.to(torch.float32)), (ptr[:1], flat)):
        with pytest.raises(ValueError, match="row_moments"):
            eccknn.row_moments(*bad)


# ---- the estimates --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("user_based", SIDES, ids=["user", "item"])
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("kind", ["int", "fp64"])
def test_estimates_equal_the_restatement(world, kind, mode, user_based):
    from n2v_hip import eccknn
    case, ts, _ = world[kind]
    algo, sim, tab, yr = fitted(world, kind, mode, user_based)
    assert_tables(algo, tab)
    qu, qi, qx, qy = queries(case, user_based)
    dqx, dqy = dev(qx, torch.int32), dev(qy, torch.int32)
    seen_kinds = set()
    for k, min_k in K_MIN_K:
        est, ak, imp = eccknn.estimate_batch_centered(algo.sim, algo.yr, dqx, dqy, k, min_k, algo.centering)
        west, wak, wimp = C.estimate_all(tab, sim, yr, qx, qy, k, min_k)
        assert est.dtype == torch.float64 and ak.dtype == torch.int32 and imp.dtype == torch.uint8
        assert np.array_equal(ak.cpu().numpy(), wak) and np.array_equal(imp.cpu().numpy(), wimp), (k, min_k)
        assert E.canon(est.cpu().numpy()) == E.canon(west), (k, min_k)
        seen_kinds |= {"none" if a == 0 else "few" if a < min_k else "enough" for a in wak[:-8]}
        assert wimp[:-8].sum() == 0 and wimp[-8:].sum() == (0 if mode == "baseline" else 8) and (wak[-8:] == 0).all()
        # the stored path's other half: the fallback and the clip, and the rmse over the same queries
        r_true = np.random.RandomState(k).randint(1, 6, len(qx)).astype(np.float64)
        pred, err = eccknn.predict(est, imp, case["mean"], case["scale"], dev(r_true, torch.float64))
        wpred = E.predict_all(west, wimp, case["mean"], *case["scale"])
        assert E.canon(pred.cpu().numpy()) == E.canon(wpred) and err == E.rmse(r_true, wpred)
    assert seen_kinds == {"none", "few", "enough"}
    # the class: estimate / test / rmse give the same numbers
    algo.k, algo.min_k = 40, 3
    west, wak, wimp = C.estimate_all(tab, sim, yr, qx, qy, 40, 3)
    for q in (0, 151, 400, len(qx) - 8, len(qx) - 6, len(qx) - 1):
        u, i = int(qu[q]), int(qi[q])
        if wimp[q]:
            with pytest.raises(eccknn.PredictionImpossible, match="unkown"):
                algo.estimate(u, i)
        else:
            got, details = algo.estimate(u, i)
            assert E.canon(np.array([got])) == E.canon(west[q:q + 1]) and details == {"actual_k": int(wak[q])}
    raw = lambda ids, names: [names[v] if 0 <= v < len(names) else "nobody-%d" % v for v in ids]
    testset = list(zip(raw(qu, case["users"]), raw(qi, case["items"]), r_true.tolist()))
    pred, ak, imp = algo.test(testset)
    wpred = E.predict_all(west, wimp, case["mean"], *case["scale"])
    assert E.canon(pred) == E.canon(wpred) and np.array_equal(ak, wak) and np.array_equal(imp, wimp.astype(bool))
    assert algo.rmse(testset) == E.rmse(r_true, wpred)


# ---- top-N ----------------------------------------------------------------------------------------------------------------

def stored_lists(pred, seen_mask, n_items):
    """The stored path's lists at n = 256: seen pairs masked, a stable sort of the negated rows, (-1, NaN) behind."""
    neg = torch.where(seen_mask, torch.full_like(pred, float("inf")), -pred)
    val, idx = torch.sort(neg, dim=1, stable=True)
    items = torch.where(torch.isinf(val), torch.full_like(idx, -1), idx).to(torch.int32)
    score = torch.where(torch.isinf(val), torch.full_like(val, float("nan")), torch.gather(pred, 1, idx))
    pad = 256 - n_items
    items = torch.cat([items, torch.full((items.shape[0], pad), -1, dtype=torch.int32, device=items.device)], 1)
    score = torch.cat([score, torch.full((score.shape[0], pad), float("nan"), dtype=torch.float64, device=score.device)], 1)
    return items, score


def assert_same(got, want, what):
    gi, gs = got
    wi, ws = want
    assert gi.dtype == torch.int32 and gs.dtype == torch.float64 and gi.shape == gs.shape == wi.shape, what
    assert torch.equal(gi, wi), what
    real = wi >= 0
    assert torch.equal(gs.view(torch.int64)[real], ws.view(torch.int64)[real]), what
    assert bool(torch.isnan(gs[~real]).all()), what


@pytest.mark.parametrize("user_based", SIDES, ids=["user", "item"])
@pytest.mark.parametrize("mode,kind,k,min_k", [("means", "int", 40, 3), ("zscore", "int", 65, 1), ("baseline", "int", 40, 1),
                                               ("baseline", "fp64", 256, 3)])
def test_fused_lists_equal_the_restatement_and_the_stored_path(world, mode, kind, k, min_k, user_based):
    from n2v_hip import eccknn
    case, ts, seen = world[kind]
    algo, sim, tab, yr = fitted(world, kind, mode, user_based)
    owners = T.owner_list(case)
    ranked = C.rankings(case, tab, sim, yr, owners, k, min_k)
    qu = dev(np.repeat(owners, case["n_items"]), torch.int32)
    qi = dev(np.tile(np.arange(case["n_items"]), len(owners)), torch.int32)
    qx, qy = (qu, qi) if user_based else (qi, qu)
    est, _, imp = eccknn.estimate_batch_centered(algo.sim, algo.yr, qx, qy, k, min_k, algo.centering)
    pred = eccknn.predict(est, imp, case["mean"], case["scale"]).view(len(owners), case["n_items"])
    mask = np.zeros((len(owners), case["n_items"]), dtype=bool)
    for row, u in enumerate(owners):
        if u >= 0:
            mask[row, sorted(case["seen"][u])] = True
    stored = stored_lists(pred, dev(mask, torch.bool), case["n_items"])
    d_owners = dev(owners, torch.int32)
    for n in T.NS:
        wi, ws = T.lists(ranked, n)
        want = (dev(wi, torch.int32), dev(ws, torch.float64))
        assert_same((stored[0][:, :n], stored[1][:, :n]), want, (n, "stored path vs restatement"))
        for S in T.SEGMENTS:
            got = eccknn.top_n_centered(algo.sim, algo.yr, seen, k, min_k, case["scale"], n, algo.centering, d_owners, S)
            assert_same(got, want, (n, S, "fused vs restatement"))
            assert_same(got, (stored[0][:, :n].contiguous(), stored[1][:, :n].contiguous()), (n, S, "fused vs stored path"))
    # the unknown owner: the clipped training mean for every item, or under the baseline mode the clipped gm + bi[i]
    unknown = ranked[int(np.nonzero(owners == -1)[0][0])]
    lo, hi = case["scale"]
    if mode == "baseline":
        want = sorted(((i, min(hi, max(lo, case["mean"] + float(case["bi"][i])))) for i in range(case["n_items"])),
                      key=lambda t: t[1], reverse=True)
        assert unknown == want and len({s for _, s in unknown}) > 10
    else:
        assert unknown == [(i, min(hi, max(lo, case["mean"]))) for i in range(case["n_items"])]
    # the class: raw users in, the same lists out; recommend and ranking_metrics run on them
    algo.k, algo.min_k = k, min_k
    raw = ["almost", "stranger", case["users"][0], "full"]
    picked = C.rankings(case, tab, sim, yr, [case["users"].index(u) if u in case["users"] else -1 for u in raw], k, min_k)
    wi, ws = T.lists(picked, 10)
    assert_same(algo.top_n_lists(10, raw, 7), (dev(wi, torch.int32), dev(ws, torch.float64)), "top_n_lists")
    recs = algo.recommend(3, users=["stranger", "almost"])
    assert recs["stranger"] == [(case["items"][i], s) for i, s in picked[1][:3]]
    assert recs["almost"] == [(case["items"][i], s) for i, s in picked[0][:3]]
    f1, m_ap, mrr, ndcg, per_user = algo.ranking_metrics([("almost", case["items"][picked[0][0][0]], 5.0), ("stranger", case["items"][0], 4.0)], 10)
    assert per_user.shape[0] == 2 and 0.0 < mrr <= 1.0


def test_malformed_rating_lists_are_value_errors_on_the_host(world):
    from n2v_hip import eccknn
    case, ts, seen = world["int"]
    algo = fitted(world, "int", "means", True)[0]
    ptr, xs, rs = algo.yr
    q = dev([0], torch.int32)
    past, negative = xs.clone(), xs.clone()
    past[17] = case["n_users"]
    negative[-1] = -1
    bad_ptr, short_ptr = ptr.clone(), ptr.clone()
    bad_ptr[4] = ptr[5] + 3
    short_ptr[-1] -= 1
    for bad in ((ptr, past, rs), (ptr, negative, rs), (bad_ptr, xs, rs), (short_ptr, xs, rs), (ptr, xs, rs[:-1]),
                (ptr, xs.to(torch.int64), rs), (ptr.to(torch.int32), xs, rs)):
        with pytest.raises(ValueError, match="yr"):
            eccknn.estimate_batch_centered(algo.sim, bad, q, q, 40, 1, algo.centering)
        with pytest.raises(ValueError, match="yr"):
            eccknn.top_n_centered(algo.sim, bad, seen, 40, 1, case["scale"], 10, algo.centering)
    eccknn.yr_check(algo.yr, case["n_users"])
    short = eccknn.Centering("zscore", True, case["mean"], algo.centering.tx, algo.centering.tx[:-1], None)
    for c in (short, algo.centering._replace(mode="baseline"), algo.centering._replace(tx=None)):
        with pytest.raises(ValueError, match="centering"):
            eccknn.estimate_batch_centered(algo.sim, algo.yr, q, q, 40, 1, c)
    for k, min_k in ((0, 1), (257, 1), (40, 0)):
        with pytest.raises(ValueError):
            eccknn.estimate_batch_centered(algo.sim, algo.yr, q, q, k, min_k, algo.centering)


# ---- KNNBaseline under pearson_baseline: one pair of baselines -----------------------------------------------------------------

def test_pearson_baseline_shares_the_baselines_of_the_fit(world, monkeypatch):
    from n2v_hip import eccknn
    case, ts, _ = world["int"]
    calls = []
    real = eccknn.baselines
    monkeypatch.setattr(eccknn, "baselines", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    for user_based in SIDES:
        del calls[:]
        algo = eccknn.KNNBaseline(k=40, min_k=2, sim_options={"name": "pearson_baseline", "user_based": user_based}, device=DEV).fit(ts)
        assert len(calls) == 1 and algo.centering.tx is algo.bx and algo.centering.by is algo.by
        plain = eccknn.KNNBasic(sim_options={"name": "pearson_baseline", "user_based": user_based}, device=DEV).fit(ts)
        assert len(calls) == 2 and torch.equal(plain.sim.view(torch.int64), algo.sim.view(torch.int64))
        x, y = (case["u"], case["i"]) if user_based else (case["i"], case["u"])
        n_x, n_y = (case["n_users"], case["n_items"]) if user_based else (case["n_items"], case["n_users"])
        tab = C.tables("baseline", x, y, case["r"], n_x, n_y, user_based, case["mean"], case["bu"], case["bi"])
        assert_tables(algo, tab)
        qu, qi, qx, qy = queries(case, user_based)
        est, ak, imp = eccknn.estimate_batch_centered(algo.sim, algo.yr, dev(qx, torch.int32), dev(qy, torch.int32), 40, 2, algo.centering)
        west, wak, wimp = C.estimate_all(tab, algo.sim.cpu().numpy(), T.side(case, user_based)[1], qx, qy, 40, 2)
        assert E.canon(est.cpu().numpy()) == E.canon(west) and np.array_equal(ak.cpu().numpy(), wak) and not imp.any()
        # estimate never raises, whatever the ids
        for u, i, q in ((-1, 5, len(qx) - 7), ("nobody", None, len(qx) - 4), (3, case["n_items"], len(qx) - 5)):
            assert algo.estimate(u, i) == (west[q], {"actual_k": 0})
        del calls[:]
        algo.fit(ts)                                              # a second fit computes them again, once
        assert len(calls) == 1


# ---- main_rec.py ----------------------------------------------------------------------------------------------------------

def small_csv(tmp_path):
    rs = np.random.RandomState(21)
    cells = rs.permutation(30 * 40)[:420]
    rows = [("u%02d" % (c // 40), "i%02d" % (c % 40), float(rs.randint(1, 6))) for c in cells]
    p = tmp_path / "ratings.csv"
    p.write_text("user,item,rating\n" + "".join("%s,%s,%r\n" % t for t in rows))
    return str(p), rows


def restated_split(mode, rows, train, test, scale, k, min_k, n, user_based=True):
    """(rmse, (f1, map, mrr, ndcg)) of one split, everything from the restatements: cosine similarity without weights,
    the tables, estimate_all over the test set, and the metrics of the restated rankings."""
    raw_u, raw_i, r = [rows[t][0] for t in train], [rows[t][1] for t in train], np.array([rows[t][2] for t in train])
    u, users = E.inner_ids(raw_u)
    i, items = E.inner_ids(raw_i)
    mean = E.global_mean(r)
    x, y, n_x, n_y = (u, i, len(users), len(items)) if user_based else (i, u, len(items), len(users))
    yr = E.build_yr(x, y, r)
    sim = E.NUMPY["cosine"](n_x, yr, 1, np.ones(n_y))["sim"]
    bu, bi = P.baselines_als(P.rows_of(u, i, r, len(users)), P.rows_of(i, u, r, len(items)), mean)
    tab = C.tables(mode, x, y, r, n_x, n_y, user_based, mean, bu, bi)
    tu = [users.index(rows[t][0]) if rows[t][0] in users else -1 for t in test]
    ti = [items.index(rows[t][1]) if rows[t][1] in items else -1 for t in test]
    est, _, imp = C.estimate_all(tab, sim, yr, *((tu, ti) if user_based else (ti, tu)), k, min_k)
    rmse = E.rmse([rows[t][2] for t in test], E.predict_all(est, imp, mean, *scale))
    truth = {}
    for t in test:
        truth.setdefault(rows[t][0], set()).add(rows[t][1])
    owners = list(truth)
    ptr, pos, lens = [0], [], []
    for ru in owners:
        pos.extend(sorted(items.index(ri) for ri in truth[ru] if ri in items))
        ptr.append(len(pos))
        lens.append(len(truth[ru]))
    case = dict(seen=T.seen_sets(u, i, len(users)), n_items=len(items), mean=mean, scale=scale)
    ranked = C.rankings(case, tab, sim, yr, [users.index(ru) if ru in users else -1 for ru in owners], k, min_k)
    per_user = R.user_metrics(T.lists(ranked, n)[0], np.array(ptr, np.int64), np.array(pos, np.int32), np.array(lens, np.int64))
    return rmse, R.averages(per_user)


@pytest.mark.parametrize("flag,mode", [("knnmeans", "means"), ("knnzscore", "zscore"), ("knnbaseline", "baseline")])
def test_main_rec_end_to_end(tmp_path, capsys, flag, mode):
    import main_rec
    path, rows = small_csv(tmp_path)
    base = ["-input", path, "-seed", "4", "-algo", flag, "-k", "5", "-mink", "2"]
    rmse, metrics = main_rec.main(base + ["-topn", "5"])
    out = capsys.readouterr().out.strip().split("\n")
    assert out == ["RMSE: %r" % rmse, "F1 / MAP / MRR / NDCG @5: %r / %r / %r / %r" % tuple(metrics)]
    train, test = main_rec.split(len(rows), 0.2, 4)
    assert (rmse, tuple(metrics)) == restated_split(mode, rows, train, test, (1.0, 5.0), 5, 2, 5)
    assert main_rec.main(base) == rmse
    capsys.readouterr()
    folds = main_rec.main(base + ["-cv", "2", "-topn", "3", "-item-based"])
    out = capsys.readouterr().out.strip().split("\n")
    assert [l.split(":")[0] for l in out] == ["RMSE", "F1 / MAP / MRR / NDCG @3"] * 2 + ["mean RMSE"]
    want = [restated_split(mode, rows, tr, te, (1.0, 5.0), 5, 2, 3, user_based=False) for tr, te in main_rec.folds(len(rows), 2, 4)]
    assert [(f[0], tuple(f[1])) for f in folds] == want


# ---- what was there before ------------------------------------------------------------------------------------------------

def test_knnbasic_is_unchanged(world):
    """estimate_batch / top_n of a KNNBasic fit still equal eccknn_reference and topn_reference (the existing suites are the
    real guard; this is the same check beside the new instantiations)."""
    from n2v_hip import eccknn
    case, ts, seen = world["int"]
    for user_based, k, min_k in ((True, 40, 3), (False, 65, 1)):
        algo = eccknn.KNNBasic(k=k, min_k=min_k, sim_options={"name": "cosine", "user_based": user_based}, device=DEV).fit(ts)
        sim, yr = algo.sim.cpu().numpy(), T.side(case, user_based)[1]
        qu, qi, qx, qy = queries(case, user_based)
        est, ak, imp = eccknn.estimate_batch(algo.sim, algo.yr, dev(qx, torch.int32), dev(qy, torch.int32), k, min_k)
        keep = (qx < sim.shape[0]) & (qy < len(yr))               # eccknn_reference takes -1 for unknown, nothing else
        west, wak, wimp = E.estimate_all(sim, yr, qx[keep], qy[keep], k, min_k)
        keep = dev(keep, torch.bool)
        assert E.canon(est[keep].cpu().numpy()) == E.canon(west) and np.array_equal(ak[keep].cpu().numpy(), wak)
        # impossible: the four unknown queries that were kept, and with min_k 3 the items with fewer raters ("lonely" has one)
        assert np.array_equal(imp[keep].cpu().numpy(), wimp) and wimp.sum() >= (4 if min_k == 1 else 5)
        owners = T.owner_list(case)
        ranked = T.rankings(case["seen"], case["n_items"], owners, T.knn_predictor(sim, yr, user_based, k, min_k, case["mean"], *case["scale"]))
        for n, S in ((10, None), (65, 3)):
            wi, ws = T.lists(ranked, n)
            got = eccknn.top_n(algo.sim, algo.yr, seen, user_based, k, min_k, case["mean"], case["scale"], n, dev(owners, torch.int32), S)
            assert_same(got, (dev(wi, torch.int32), dev(ws, torch.float64)), (user_based, n, S))
