"""GPU tests of the SlopeOne predictor: the deviation table in its dense and sparse forms (n2v_slopeone_dev,
n2v_slopeone_dev_sparse), the estimates (n2v_slopeone_estimate), the fused top-N lists (n2v_slopeone_topn) and what is built
on them (n2v_hip.slopeone.SlopeOne, main_rec.py -algo slopeone).

Everything is compared by equality with the restatement tests/slopeone_reference.py: integers with ==, fp64 values by their
bytes after eccknn_reference.canon (a NaN is compared as NaN, a zero by its sign bit).  The case table is
slopeone_reference.cases(); its edges are asserted by tests/test_slopeone_host.py.  Every case is a few hundred ratings."""
import numpy as np
import pytest
import torch

import eccknn_reference as E
import slopeone_reference as S
import topn_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 10, 256)
SEGMENTS = (None, 1, 2, 3, 64)


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)


def triples(case):
    return dev(case["i"], torch.int32), dev(case["u"], torch.int32), dev(case["r"], torch.float64)


def both_forms(case, accumulators=False):
    """(dense result, sparse result) of one case, each (dev, freq[, acc]) on the device."""
    from n2v_hip import eccknn, slopeone
    di, du, dr = triples(case)
    dense = slopeone.deviations(*eccknn.densify(di, du, dr, case["n_items"], case["n_users"]), accumulators=accumulators)
    xr = eccknn.csr_by_x(di, du, dr, case["n_items"], case["n_users"])
    return dense, slopeone.deviations_sparse(xr, case["n_users"], accumulators=accumulators)


def assert_table(got, model, what, acc=False):
    d, f = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert d.dtype == np.float64 and f.dtype == np.int32 and d.shape == f.shape == model["dev"].shape, what
    assert np.array_equal(f, model["freq"]), what
    assert E.canon(d) == E.canon(model["dev"]), what
    assert np.array_equal(np.signbit(d), np.signbit(np.where(np.isnan(model["dev"]), d, model["dev"]))), what
    if acc:
        assert E.canon(got[2].cpu().numpy()) == E.canon(model["acc"]), what


@pytest.fixture(scope="module")
def world():
    """The restated model of every case, and the device model of the cases the estimate and top-N tests use; built once."""
    from n2v_hip import eccknn, slopeone
    out = {}
    for name, case in S.cases():
        model = S.fit(case["u"], case["i"], case["r"], case["n_users"], case["n_items"])
        entry = dict(case=case, model=model)
        if not name.startswith("grid"):
            di, du, dr = triples(case)
            d, f = slopeone.deviations(*eccknn.densify(di, du, dr, case["n_items"], case["n_users"]))
            ptr = np.zeros(case["n_users"] + 1, dtype=np.int64)
            np.cumsum([len(lst) for lst in model["ur"]], out=ptr[1:])
            ur = (dev(ptr, torch.int64), dev([j for lst in model["ur"] for (j, _) in lst], torch.int32),
                  dev([r for lst in model["ur"] for (_, r) in lst], torch.float64))
            mu = eccknn.row_moments(ur[0], ur[2])[0]
            seen = eccknn.csr_by_x(du, di, dr, case["n_users"], case["n_items"])
            entry.update(dev=d, freq=f, ur=ur, mu=mu, seen=seen)
        out[name] = entry
    return out


# ---- the table ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_users", S.N_USERS)
@pytest.mark.parametrize("n_items", S.N_ITEMS)
def test_table_dense_and_sparse_equal_the_restatement(world, n_items, n_users):
    w = world["grid-%d-%d" % (n_items, n_users)]
    dense, sparse = both_forms(w["case"], accumulators=True)
    assert_table(dense, w["model"], ("dense", n_items, n_users), acc=True)
    assert_table(sparse, w["model"], ("sparse", n_items, n_users), acc=True)
    for a, b in zip(dense, sparse):                                # one form against the other, NaN payloads included
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)


def test_table_edges_of_the_main_case(world):
    from n2v_hip import _lib
    w = world["main"]
    assert int(_lib.load().n2v_eccknn_sparse_chunk()) == S.SC
    dense, sparse = both_forms(w["case"], accumulators=True)
    for form, got in (("dense", dense), ("sparse", sparse)):
        assert_table(got, w["model"], form, acc=True)
        d, f = got[0].cpu().numpy(), got[1].cpu().numpy()
        for a, b in ((3, 7), (3, 100), (7, 100)):                  # alike in one diagonal tile and across two tiles
            assert f[a, b] > 0 and d[a, b] == 0.0 and not np.signbit(d[a, b]) and np.signbit(d[b, a]), (form, a, b)
        assert not np.signbit(d.diagonal()).any() and (d.diagonal() == 0.0).all()
        assert f[129].max() == 0 and np.isnan(d[129, :129]).all() and np.isnan(d[:129, 129]).all()    # nobody co-rated
        assert f[10, 11] > 0 and np.isnan(d[10, 11]) and np.isnan(d[11, 10])                           # inf - inf
        assert f.diagonal()[[129, 20, 22, 23, 24]].tolist() == [0, 1, S.SC - 1, S.SC, S.SC + 1]
    assert torch.equal(dense[1], sparse[1]) and E.canon(dense[0].cpu().numpy()) == E.canon(sparse[0].cpu().numpy())
    # without the raw sums the same table
    plain = both_forms(w["case"])
    assert len(plain[0]) == 2 and torch.equal(plain[0][0].view(torch.int64), dense[0].view(torch.int64))
    assert torch.equal(plain[1][0].view(torch.int64), sparse[0].view(torch.int64))


def test_malformed_csr_and_table_limit_are_value_errors(world):
    from n2v_hip import eccknn, slopeone
    case = world["main"]["case"]
    di, du, dr = triples(case)
    ptr, ys, rs = eccknn.csr_by_x(di, du, dr, case["n_items"], case["n_users"])
    bad_y = ys.clone()
    bad_y[5] = case["n_users"]
    with pytest.raises(ValueError, match="malformed CSR.*outside"):
        slopeone.deviations_sparse((ptr, bad_y, rs), case["n_users"])
    unsorted = ys.clone()
    row = int((ptr[1:] - ptr[:-1]).argmax())
    b = int(ptr[row])
    unsorted[b], unsorted[b + 1] = ys[b + 1], ys[b]
    with pytest.raises(ValueError, match="malformed CSR.*ascending"):
        slopeone.deviations_sparse((ptr, unsorted, rs), case["n_users"])
    bad_ptr = ptr.clone()
    bad_ptr[3] = ys.numel() + 7
    with pytest.raises(ValueError, match="malformed CSR.*xr_ptr"):
        slopeone.deviations_sparse((bad_ptr, ys, rs), case["n_users"])
    # n_items^2 > 2^31: refused from the shapes alone (a meta tensor owns no memory)
    free = torch.cuda.mem_get_info()[0]
    wide = torch.empty((1, 46341), dtype=torch.float64, device="meta")
    with pytest.raises(ValueError, match="46341"):
        slopeone.deviations(wide, wide)
    wide_ptr = torch.empty(46342, dtype=torch.int64, device="meta")
    with pytest.raises(ValueError, match="46341"):
        slopeone.deviations_sparse((wide_ptr, ys, rs), case["n_users"])
    assert torch.cuda.mem_get_info()[0] >= free - (1 << 20)


# ---- the estimates ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["main", "small-63", "small-64", "small-65"])
def test_estimates_equal_the_restatement(world, name):
    from n2v_hip import slopeone
    w = world[name]
    case, model = w["case"], w["model"]
    assert E.canon(w["mu"].cpu().numpy()) == E.canon(model["mu"])
    qu, qi = S.all_pairs(case)
    want = S.estimate_all(model, qu, qi)
    clip = lambda q: dev(np.clip(q, -2 ** 31, 2 ** 31 - 1), torch.int32)
    est, nd, imp = slopeone.estimate_batch(w["dev"], w["freq"], w["ur"], w["mu"], clip(qu), clip(qi))
    assert E.canon(est.cpu().numpy()) == E.canon(want[0])
    assert np.array_equal(nd.cpu().numpy(), want[1]) and np.array_equal(imp.cpu().numpy(), want[2])
    assert want[2][-7:].all() and not want[2][:-7].any()             # unknown user, unknown item, ids out of range
    if name == "main":
        n_i = case["n_items"]
        at = lambda u, i: u * n_i + i
        assert tuple(len(model["ur"][u]) for u in range(6)) == S.LIST_LENS
        got_e, got_n = est.cpu().numpy(), nd.cpu().numpy()
        for u, ln in enumerate(S.LIST_LENS):                      # every entry of the long lists is usable for item 5
            assert got_n[at(u, 5)] == ln, (u, ln)
        assert got_n[at(9, 5)] == 0 and got_e[at(9, 5)].tobytes() == model["mu"][9].tobytes()    # nothing usable: the mean's bits
        assert got_n[at(9, 20)] == 1 and 20 in [j for j, _ in model["ur"][9]]                    # a rated item: the diagonal
        assert 0 < got_n[at(12, 5)] == len(model["ur"][12]) - 1
        assert np.isnan(got_e[at(5, 10)]) and got_n[at(5, 10)] == 130


def test_a_malformed_list_is_a_value_error_and_never_out_of_bounds(world):
    from n2v_hip import slopeone
    w = world["small-64"]
    ptr, ids, rs = w["ur"]
    q = dev([0, 1], torch.int32)
    bad = ids.clone()
    bad[3] = w["case"]["n_items"]
    with pytest.raises(ValueError, match="malformed lists: an x outside"):
        slopeone.estimate_batch(w["dev"], w["freq"], (ptr, bad, rs), w["mu"], q, q)
    bad_ptr = ptr.clone()
    bad_ptr[1] = ids.numel() + 5
    with pytest.raises(ValueError, match="malformed lists: ptr"):
        slopeone.estimate_batch(w["dev"], w["freq"], (bad_ptr, ids, rs), w["mu"], q, q)
    with pytest.raises(ValueError, match="malformed lists"):
        slopeone.top_n(w["dev"], w["freq"], (ptr, bad, rs), w["mu"], w["seen"], 3.0, (1.0, 5.0), 5)
    # unchecked, the kernels skip the entry that is no item and clamp the row: every other query keeps its bits
    model = w["model"]
    qu, qi = S.all_pairs(w["case"])
    qu, qi = qu[:-7], qi[:-7]
    est, nd, _ = slopeone.estimate_batch(w["dev"], w["freq"], (ptr, bad, rs), w["mu"], dev(qu, torch.int32), dev(qi, torch.int32),
                                         check=False)
    owner = int(np.searchsorted(ptr.cpu().numpy(), 3, side="right") - 1)
    pruned = dict(model, ur=[[e for k, e in enumerate(lst) if not (u == owner and k == 3 - int(ptr[owner]))]
                             for u, lst in enumerate(model["ur"])])
    want = S.estimate_all(pruned, qu, qi)
    assert E.canon(est.cpu().numpy()) == E.canon(want[0]) and np.array_equal(nd.cpu().numpy(), want[1])


def test_class_fit_test_and_rmse(world):
    from n2v_hip import eccknn, slopeone
    case = world["main"]["case"]
    raw_u, raw_i = ["u%d" % v for v in case["u"]], ["i%d" % v for v in case["i"]]
    ts = eccknn.Trainset.from_ratings(raw_u, raw_i, case["r"], rating_scale=case["scale"])
    model = S.fit(ts.u, ts.i, ts.r, ts.n_users, ts.n_items)
    fits = {form: slopeone.SlopeOne(sim_options={"form": form}, device=DEV).fit(ts) for form in ("auto", "dense", "sparse")}
    again = slopeone.SlopeOne(device=DEV).fit(ts)
    for form, algo in fits.items():
        assert_table((algo.dev, algo.freq), model, form)
        assert E.canon(algo.user_mean.cpu().numpy()) == E.canon(model["mu"])
        for a, b in ((algo.dev, again.dev), (algo.user_mean, again.user_mean)):      # two fits, either form: the same bytes
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), form
        assert torch.equal(algo.freq, again.freq)
    algo = fits["auto"]
    u5, i10, i3 = ts.to_inner_uid("u5"), ts.to_inner_iid("i10"), ts.to_inner_iid("i3")
    for u, i in ((u5, i3), (ts.to_inner_uid("u9"), i3), (ts.to_inner_uid("u9"), ts.to_inner_iid("i20")), (u5, i10)):
        got, want = algo.estimate(u, i), S.estimate(model, u, i)
        assert E.canon(np.array([got[0]])) == E.canon(np.array([want[0]])) and got[1] == {"n_deviations": want[1]}
    for u, i in ((-1, 0), (0, ts.n_items), ("u5", 0)):
        with pytest.raises(eccknn.PredictionImpossible):
            algo.estimate(u, i)
    rs = np.random.RandomState(3)
    testset = [("u%d" % rs.randint(40), "i%d" % rs.randint(133), float(rs.randint(1, 6))) for _ in range(200)]
    testset += [("stranger", "i3", 4.0), ("u5", "new-item", 2.0), ("stranger", "new-item", 5.0), ("u5", "i10", 3.0)]
    qu, qi = ts.inner_uids([t[0] for t in testset]), ts.inner_iids([t[1] for t in testset])
    est, nd, imp = S.estimate_all(model, qu, qi)
    pred = E.predict_all(est, imp, ts.global_mean, *ts.rating_scale)
    got = algo.test(testset)
    assert E.canon(got[0]) == E.canon(pred) and np.array_equal(got[1], nd) and np.array_equal(got[2], imp.astype(bool))
    assert imp.sum() >= 3 and np.isnan(est).any()
    assert algo.rmse(testset) == E.rmse([t[2] for t in testset], pred)


# ---- the top-N lists ----------------------------------------------------------------------------------------------------

def stored_path(pred, seen_mask, n_items):
    """The stored path's lists at n = 256 from the [n_owners][n_items] predictions: seen pairs masked to +inf of the negated
    rows (no prediction is -inf: it was clipped to lo), a stable ascending sort, (-1, NaN) behind the candidates."""
    neg = torch.where(seen_mask, torch.full_like(pred, float("inf")), -pred)
    val, idx = torch.sort(neg, dim=1, stable=True)
    items = torch.where(torch.isinf(val), torch.full_like(idx, -1), idx).to(torch.int32)
    score = torch.where(torch.isinf(val), torch.full_like(val, float("nan")), torch.gather(pred, 1, idx))
    pad = max(0, 256 - n_items)
    items = torch.cat([items, torch.full((items.shape[0], pad), -1, dtype=torch.int32, device=items.device)], 1)
    score = torch.cat([score, torch.full((score.shape[0], pad), float("nan"), dtype=torch.float64, device=score.device)], 1)
    return items, score


def assert_same(got, want, what):
    """Item ids equal; scores equal by their bytes wherever there is an item, NaN wherever there is none."""
    gi, gs = got
    wi, ws = want
    assert gi.dtype == torch.int32 and gs.dtype == torch.float64 and gi.shape == gs.shape == wi.shape, what
    assert torch.equal(gi, wi), what
    real = wi >= 0
    assert torch.equal(gs.view(torch.int64)[real], ws.view(torch.int64)[real]), what
    assert bool(torch.isnan(gs[~real]).all()), what


@pytest.mark.parametrize("name,scale", [("main", None), ("main", (-1.0, 1.0)), ("small-63", None), ("small-64", None),
                                        ("small-65", None)], ids=["main", "main-narrow", "small-63", "small-64", "small-65"])
def test_fused_lists_equal_the_restatement_and_the_stored_path(world, name, scale):
    from n2v_hip import eccknn, slopeone
    w = world[name]
    case = dict(w["case"], scale=scale or w["case"]["scale"])
    n_u, n_i = case["n_users"], case["n_items"]
    owners = np.array(list(range(n_u)) + [-1, 3, n_u - 1, 3, -1, n_u], dtype=np.int32)
    ranked = S.rankings(case, w["model"], owners)
    qu = dev(np.repeat(owners, n_i), torch.int32)
    qi = dev(np.tile(np.arange(n_i), len(owners)), torch.int32)
    est, _, imp = slopeone.estimate_batch(w["dev"], w["freq"], w["ur"], w["mu"], qu, qi)
    pred = eccknn.predict(est, imp, case["mean"], case["scale"]).view(len(owners), n_i)
    mask = np.zeros((len(owners), n_i), dtype=bool)
    for row, u in enumerate(owners):
        if 0 <= u < n_u:
            mask[row, sorted(case["seen"][u])] = True
    stored = stored_path(pred, dev(mask, torch.bool), n_i)
    for n in NS:
        wi, ws = T.lists(ranked, n)
        want = (dev(wi, torch.int32), dev(ws, torch.float64))
        assert_same((stored[0][:, :n], stored[1][:, :n]), want, (name, n, "stored path vs restatement"))
        for seg in SEGMENTS:
            got = slopeone.top_n(w["dev"], w["freq"], w["ur"], w["mu"], w["seen"], case["mean"], case["scale"], n,
                                 dev(owners, torch.int32), seg)
            assert_same(got, want, (name, n, seg, "fused vs restatement"))
            assert_same(got, (stored[0][:, :n].contiguous(), stored[1][:, :n].contiguous()), (name, n, seg, "fused vs stored path"))
    # what the cases plant
    items, score = slopeone.top_n(w["dev"], w["freq"], w["ur"], w["mu"], w["seen"], case["mean"], case["scale"], 256,
                                  dev(owners, torch.int32))
    items, score = items.cpu().numpy(), score.cpu().numpy()
    unknown = int(np.nonzero(owners == -1)[0][0])
    clipped_mean = min(case["scale"][1], max(case["scale"][0], case["mean"]))
    assert items[unknown][:min(n_i, 256)].tolist() == list(range(min(n_i, 256))) and (score[unknown][:n_i] == clipped_mean).all()
    assert np.array_equal(items[unknown], items[-1]) and np.array_equal(items[3], items[n_u + 1])     # owner n_users; repeats
    for u in range(n_u):                                          # N above the number of unseen items: (-1, NaN) behind them
        unseen = n_i - len(case["seen"][u])
        assert (items[u][:unseen] >= 0).all() and (items[u][unseen:] == -1).all() and np.isnan(score[u][unseen:]).all(), u
    if name.startswith("small"):
        assert (items[0] == -1).all()                             # user 0 rated every item
        assert sorted(items[1][:2].tolist()) == [0, n_i - 1] and (items[1][2:] == -1).all()
    if name.startswith("small") or scale:                         # many equal clipped scores: ranked by item id
        hi = case["scale"][1]
        ties = [row for row in range(n_u) if (score[row] == hi).sum() >= 5]
        assert ties
        for row in ties:
            at = items[row][score[row] == hi]
            assert (np.diff(at) > 0).all(), row


def test_segment_borders_fall_inside_lane_blocks():
    """The segments the lists above were cut into: at 2 and 3 segments a border lies inside a block of 64 candidates."""
    for n_i in (63, 64, 65, 133):
        for seg in (2, 3):
            borders = T.segment_borders(n_i, seg)
            assert borders and any(b % 64 for b in borders), (n_i, seg)


# ---- end to end ---------------------------------------------------------------------------------------------------------

def test_lists_recommend_and_metrics_of_the_class(world):
    from n2v_hip import eccknn, slopeone
    case = world["small-65"]["case"]
    raw_u, raw_i = ["u%d" % v for v in case["u"]], ["i%d" % v for v in case["i"]]
    ts = eccknn.Trainset.from_ratings(raw_u, raw_i, case["r"], rating_scale=case["scale"])
    algo = slopeone.SlopeOne(device=DEV).fit(ts)
    model = S.fit(ts.u, ts.i, ts.r, ts.n_users, ts.n_items)
    inner = dict(seen=T.seen_sets(ts.u, ts.i, ts.n_users), n_items=ts.n_items, mean=ts.global_mean, scale=ts.rating_scale)
    every = S.rankings(inner, model, range(ts.n_users))
    wi, ws = T.lists(every, 10)
    assert_same(algo.top_n_lists(), (dev(wi, torch.int32), dev(ws, torch.float64)), "every user")
    users, items = list(ts._raw2inner_u), list(ts._raw2inner_i)
    recs = algo.recommend(5)
    assert list(recs) == users
    for u, ru in enumerate(users):
        assert recs[ru] == [(items[i], s) for i, s in every[u][:5]], ru
    picked = algo.top_n_lists(3, ["stranger", users[4]], segments=2)
    wi, ws = T.lists(S.rankings(inner, model, [-1, 4]), 3)
    assert_same(picked, (dev(wi, torch.int32), dev(ws, torch.float64)), "raw users")
    k = next(u for u in range(ts.n_users) if len(every[u]) >= 5)
    f1, m_ap, mrr, ndcg, per_user = algo.ranking_metrics([(users[k], items[every[k][0][0]], 5.0), ("stranger", items[0], 4.0)], 5)
    assert per_user.shape == (2, 5) and mrr == 1.0 and 0.0 < f1 <= 1.0


def test_main_rec_slopeone_end_to_end(world, tmp_path, capsys):
    import main_rec
    case = world["small-65"]["case"]
    p = tmp_path / "ratings.csv"
    p.write_text("user,item,rating\n" + "".join("u%d,i%d,%r\n" % t for t in zip(case["u"], case["i"], case["r"].tolist())))
    base = ["-input", str(p), "-seed", "2", "-algo", "slopeone"]
    plain = main_rec.main(base)
    assert isinstance(plain, float) and capsys.readouterr().out.strip() == "RMSE: %r" % plain
    assert main_rec.main(base + ["-form", "sparse"]) == plain == main_rec.main(base + ["-form", "dense"])
    capsys.readouterr()
    recs_file = tmp_path / "recs.csv"
    rmse, metrics = main_rec.main(base + ["-topn", "5", "-save-recs", str(recs_file)])
    out = capsys.readouterr().out.strip().split("\n")
    assert rmse == plain and out == ["RMSE: %r" % rmse, "F1 / MAP / MRR / NDCG @5: %r / %r / %r / %r" % tuple(metrics)]
    # the same split and model by hand, against the restatement
    args = main_rec.parse_args(base + ["-topn", "5"])
    users, items, ratings = main_rec.read_ratings(str(p))
    train, test = main_rec.split(len(ratings), 0.2, 2)
    algo = main_rec.fit_split(args, users, items, ratings, None, train)
    ts = algo.trainset
    model = S.fit(ts.u, ts.i, ts.r, ts.n_users, ts.n_items)
    testset = [(users[k], items[k], ratings[k]) for k in test]
    est, _, imp = S.estimate_all(model, ts.inner_uids([t[0] for t in testset]), ts.inner_iids([t[1] for t in testset]))
    assert rmse == E.rmse([t[2] for t in testset], E.predict_all(est, imp, ts.global_mean, *ts.rating_scale))
    assert tuple(metrics) == algo.ranking_metrics(testset, 5)[:4] and 0.0 <= min(metrics) and max(metrics) <= 1.0
    inner = dict(seen=T.seen_sets(ts.u, ts.i, ts.n_users), n_items=ts.n_items, mean=ts.global_mean, scale=ts.rating_scale)
    raw_items = list(ts._raw2inner_i)
    want = ["%s,%s,%r" % (ru, raw_items[i], s) for ru, lst in zip(ts._raw2inner_u, S.rankings(inner, model, range(ts.n_users)))
            for i, s in lst[:5]]
    assert recs_file.read_text().split("\n")[:-1] == want and len(want) > 20
    # -cv: one file per fold, one metrics line per fold
    folds = main_rec.main(base + ["-cv", "2", "-topn", "3", "-save-recs", str(tmp_path / "cv.csv")])
    out = capsys.readouterr().out.strip().split("\n")
    assert len(folds) == 2 and all(len(f) == 2 and len(f[1]) == 4 for f in folds)
    assert [l.split(":")[0] for l in out] == ["RMSE", "F1 / MAP / MRR / NDCG @3"] * 2 + ["mean RMSE"]
    assert (tmp_path / "cv.csv.0").exists() and (tmp_path / "cv.csv.1").exists()
