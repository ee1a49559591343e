"""GPU tests of the CoClustering predictor: the averages (n2v_cocl_averages), the assignment passes (n2v_cocl_assign), the
estimates (n2v_cocl_estimate), the fused top-N lists (n2v_cocl_topn) and what is built on them
(n2v_hip.coclustering.CoClustering, main_rec.py -algo coclustering).

Everything is compared by equality with the restatement tests/coclustering_reference.py: integers with ==, fp64 values by
their bytes after eccknn_reference.canon (a NaN is compared as NaN).  The case tables are the restatement's; their edges are
asserted by tests/test_coclustering_host.py.  Every case is at most 1 500 ratings, but for the one list of 5 000 entries and
the chain over 2 100 users of one rating each."""
import numpy as np
import pytest
import torch

import coclustering_reference as C
import eccknn_reference as E
import topn_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 10, 256)
SEGMENTS = (None, 1, 64)


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)


def dev_list(lst):
    return dev(lst[0], torch.int64), dev(lst[1], torch.int32), dev(lst[2], torch.float64)


def host(t):
    return t.cpu().numpy()


def assert_avgs(got, want, what):
    for k, name in enumerate(("avg_cltr_u", "avg_cltr_i", "avg_cocltr")):
        g = host(got[k])
        assert g.dtype == np.float64 and g.shape == want[k].shape, (what, name)
        assert E.canon(g) == E.canon(want[k]), (what, name)
    assert np.array_equal(host(got[3]), want[3]), (what, "count_cocltr")


def problem(u, i, r, n_users, n_items):
    """The lists and means of one set of ratings on the host (the restatement's) and on the device."""
    from n2v_hip import eccknn
    ul, il = C.lists(u, i, r, n_users), C.lists(i, u, r, n_items)
    d_ul, d_il = dev_list(ul), dev_list(il)
    p = dict(ul=ul, il=il, mean=C.global_mean(r), um=C.mean_rows(ul), im=C.mean_rows(il), d_ul=d_ul, d_il=d_il,
             d_um=eccknn.row_moments(d_ul[0], d_ul[2])[0], d_im=eccknn.row_moments(d_il[0], d_il[2])[0])
    assert E.canon(host(p["d_um"])) == E.canon(p["um"]) and E.canon(host(p["d_im"])) == E.canon(p["im"])
    return p


def one_epoch_both(p, cu, ci, n_cu, n_ci, what, orders=((None, None),)):
    """One epoch from the explicit assignment (cu, ci) through the module functions under every row order, against the
    restatement's; returns the restatement's new assignment."""
    from n2v_hip import coclustering
    par = C.params(n_cltr_u=n_cu, n_cltr_i=n_ci)
    want_u, want_i, want_avgs = C.epoch(p["ul"], p["il"], cu, ci, par, p["mean"], p["um"], p["im"])
    for order in orders:
        d_cu, d_ci = dev(cu, torch.int32), dev(ci, torch.int32)
        got_avgs = coclustering.epoch(p["d_ul"], p["d_il"], d_cu, d_ci, n_cu, n_ci, p["mean"], p["d_um"], p["d_im"], order=order)
        assert_avgs(got_avgs, want_avgs, what)
        assert d_cu.dtype == torch.int32 and np.array_equal(host(d_cu), want_u), (what, "cltr_u")
        assert np.array_equal(host(d_ci), want_i), (what, "cltr_i")
    return want_u, want_i


# ---- whole fits, epoch by epoch -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fit", C.FITS, ids=["%dx%d" % (f[3], f[4]) for f in C.FITS])
def test_every_epoch_of_a_fit_equals_the_restatement(fit):
    from n2v_hip import coclustering
    n_u, n_i, n, n_cu, n_ci, n_epochs, kind = fit
    u, i, r = C.make_ratings(0, n_u, n_i, n, kind)
    par = C.params(n_cltr_u=n_cu, n_cltr_i=n_ci, n_epochs=n_epochs)
    p = problem(u, i, r, n_u, n_i)
    cu, ci = C.init(n_u, n_i, par)
    d_cu, d_ci = dev(cu, torch.int32), dev(ci, torch.int32)
    for e in range(n_epochs):
        cu, ci, want_avgs = C.epoch(p["ul"], p["il"], cu, ci, par, p["mean"], p["um"], p["im"])
        got_avgs = coclustering.epoch(p["d_ul"], p["d_il"], d_cu, d_ci, n_cu, n_ci, p["mean"], p["d_um"], p["d_im"])
        assert_avgs(got_avgs, want_avgs, (fit, e))
        assert np.array_equal(host(d_cu), cu) and np.array_equal(host(d_ci), ci), (fit, e)
    assert_avgs(coclustering.averages(p["d_ul"], n_i, d_cu, d_ci, n_cu, n_ci, p["mean"]),
                C.averages(p["ul"], cu, ci, n_cu, n_ci, p["mean"]), (fit, "final"))


# ---- lists of every length, chains of every length ------------------------------------------------------------------------

def test_lists_across_the_load_width_and_any_row_order():
    from n2v_hip import nmf
    u, i, r, n_u, n_i, cu, ci = C.list_case()
    p = problem(u, i, r, n_u, n_i)
    assert tuple(int(v) for v in np.diff(p["ul"][0])[:7]) == C.LIST_LENS
    rs = np.random.RandomState(1)
    orders = ((None, None), (nmf.row_order(p["d_ul"][0]), nmf.row_order(p["d_il"][0])),
              (dev(rs.permutation(n_u), torch.int32), dev(np.arange(n_i)[::-1], torch.int32)))
    cu2, ci2 = one_epoch_both(p, cu, ci, 5, 4, "lists 5x4", orders)
    assert not np.array_equal(cu2, cu) and not np.array_equal(ci2, ci)
    one_epoch_both(p, cu2, ci2, 5, 4, "lists 5x4, second epoch")
    rs = np.random.RandomState(2)
    one_epoch_both(p, rs.randint(64, size=n_u), rs.randint(64, size=n_i), 64, 64, "lists 64x64", orders[:2])


@pytest.mark.parametrize("n_users", C.CHAIN_USERS + (1023, 1024, 1025, 2100))
def test_chains_over_the_users(n_users):
    """The chains of the averages run over the users: the counts the issue names, and those around the 1 024 users the
    kernel compacts at a time."""
    from n2v_hip import coclustering
    rs = np.random.RandomState(n_users)
    n_i = 9
    u = np.repeat(np.arange(n_users), 1 if n_users > 500 else 3)  # every user has a partial sum, so every window adds some
    i = np.concatenate([rs.permutation(n_i)[:int(c)] for c in np.bincount(u)])
    r = rs.normal(size=len(u)) * 2.0 + 3.0
    p = problem(u, i, r, n_users, n_i)
    for n_cu, n_ci in ((1, 1), (3, 4), (64, 9)):
        cu, ci = rs.randint(n_cu, size=n_users), rs.randint(n_ci, size=n_i)
        got = coclustering.averages(p["d_ul"], n_i, dev(cu, torch.int32), dev(ci, torch.int32), n_cu, n_ci, p["mean"])
        assert_avgs(got, C.averages(p["ul"], cu, ci, n_cu, n_ci, p["mean"]), (n_users, n_cu, n_ci))


@pytest.mark.parametrize("clusters", [(2, 33), (4, 32), (5, 17), (8, 16), (9, 9), (16, 8), (17, 5), (32, 4), (33, 2)],
                         ids=lambda c: "%dx%d" % c)
def test_every_lane_grouping_of_the_assign_pass(clusters):
    """The assign kernel gives an entry 1, 2, 4, .. 64 lanes, by the candidate count of the side: both sides of every
    threshold, on user lists (16 x 150) and on item lists (150 x 16) that cross the 64 entries of a load."""
    n_cu, n_ci = clusters
    for n_u, n_i in ((16, 150), (150, 16)):
        u, i, r = C.make_ratings(4, n_u, n_i, 1500, "fp64")
        p = problem(u, i, r, n_u, n_i)
        assert max(np.diff(p["ul"][0]).max(), np.diff(p["il"][0]).max()) > 64
        rs = np.random.RandomState(n_cu * 100 + n_ci)
        one_epoch_both(p, rs.randint(n_cu, size=n_u), rs.randint(n_ci, size=n_i), n_cu, n_ci, (clusters, n_u, n_i))


@pytest.mark.parametrize("kind", ["tie", "inf", "huge"])
def test_arithmetic_edges(kind):
    u, i, r, n_u, n_i, cu, ci, n_cu, n_ci = C.edge_case(kind)
    p = problem(u, i, r, n_u, n_i)
    new_u, new_i = one_epoch_both(p, cu, ci, n_cu, n_ci, kind)
    one_epoch_both(p, new_u, new_i, n_cu, n_ci, kind + ", second epoch")


# ---- the class: fit, estimates -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fitted():
    """One trainset through the class and through the restatement, once: about 1 500 ratings of 70 users x 150 items."""
    from n2v_hip import coclustering, eccknn
    case = T.make_case("int")
    ts = eccknn.Trainset.from_ratings(case["raw_u"], case["raw_i"], case["r"], rating_scale=case["scale"])
    kw = dict(n_cltr_u=4, n_cltr_i=5, n_epochs=3, random_state=7)
    algo = coclustering.CoClustering(device=DEV, **kw).fit(ts)
    model = C.fit(ts.u, ts.i, ts.r, ts.n_users, ts.n_items, C.params(**kw))
    return dict(case=case, ts=ts, algo=algo, model=model, kw=kw)


def test_class_fit_equals_the_restatement_and_two_fits_give_the_same_bytes(fitted):
    from n2v_hip import coclustering
    algo, model, ts = fitted["algo"], fitted["model"], fitted["ts"]
    assert algo.cltr_u.dtype == algo.cltr_i.dtype == torch.int32
    assert np.array_equal(host(algo.cltr_u), model["cltr_u"]) and np.array_equal(host(algo.cltr_i), model["cltr_i"])
    for name in ("avg_cltr_u", "avg_cltr_i", "avg_cocltr", "user_mean", "item_mean"):
        assert E.canon(host(getattr(algo, name))) == E.canon(model[name]), name
    assert np.array_equal(host(algo.count_cocltr), model["count_cocltr"])
    again = coclustering.CoClustering(device=DEV, **fitted["kw"]).fit(ts)
    for name in ("avg_cltr_u", "avg_cltr_i", "avg_cocltr", "user_mean", "item_mean"):
        assert torch.equal(getattr(algo, name).view(torch.int64), getattr(again, name).view(torch.int64)), name
    assert torch.equal(algo.cltr_u, again.cltr_u) and torch.equal(algo.cltr_i, again.cltr_i)
    other = coclustering.CoClustering(device=DEV, **dict(fitted["kw"], random_state=8)).fit(ts)
    assert not torch.equal(algo.cltr_u, other.cltr_u)             # the seed reaches the first assignment


def test_estimates_for_known_and_unknown_ids(fitted):
    algo, model, ts = fitted["algo"], fitted["model"], fitted["ts"]
    n_u, n_i = ts.n_users, ts.n_items
    qu = np.concatenate([np.repeat(np.arange(n_u), n_i), [-1, -1, 3, n_u, 2, -1, -7]]).astype(np.int32)
    qi = np.concatenate([np.tile(np.arange(n_i), n_u), [4, -1, -1, 4, n_i, n_i, 2]]).astype(np.int32)
    want, _ = C.estimate_all(model, qu, qi)
    est, imp = algo._estimate_batch(dev(qu, torch.int32), dev(qi, torch.int32))
    assert E.canon(host(est)) == E.canon(want) and not host(imp).any()
    tail = host(est)[-7:]
    assert tail[0] == model["item_mean"][4] and tail[1] == model["mean"] and tail[2] == model["user_mean"][3]
    assert tail[3] == model["item_mean"][4] and tail[4] == model["user_mean"][2] and tail[5] == model["mean"]
    assert algo.estimate(3, 4) == C.estimate(model, 3, 4) and algo.estimate(-1, 4) == model["item_mean"][4]
    assert algo.estimate(3, "x") == model["user_mean"][3] and algo.estimate(n_u, n_i) == model["mean"]
    rs = np.random.RandomState(3)
    users, items = list(ts._raw2inner_u), list(ts._raw2inner_i)
    testset = [(users[rs.randint(n_u)], items[rs.randint(n_i)], float(rs.randint(1, 6))) for _ in range(200)]
    testset += [("stranger", items[3], 4.0), (users[5], "new-item", 2.0), ("stranger", "new-item", 5.0)]
    tu, ti = ts.inner_uids([t[0] for t in testset]), ts.inner_iids([t[1] for t in testset])
    est, imp = C.estimate_all(model, tu, ti)
    pred = E.predict_all(est, imp, ts.global_mean, *ts.rating_scale)
    got = algo.test(testset)
    assert len(got) == 2 and E.canon(got[0]) == E.canon(pred) and not got[1].any()
    assert (pred == ts.rating_scale[0]).any() or (pred == ts.rating_scale[1]).any()      # the clip is reached
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


@pytest.mark.parametrize("scale", [None, (2.5, 3.5)], ids=["scale", "narrow"])
def test_fused_lists_equal_the_restatement_and_the_stored_path(fitted, scale):
    from n2v_hip import coclustering, eccknn
    algo, model, ts = fitted["algo"], fitted["model"], fitted["ts"]
    scale = scale or ts.rating_scale
    n_u, n_i = ts.n_users, ts.n_items
    seen_sets = T.seen_sets(ts.u, ts.i, n_u)
    owners = np.array(list(range(n_u)) + [-1, 3, n_u - 1, 3, -1, n_u], dtype=np.int32)
    ranked = T.rankings(seen_sets, n_i, owners, C.predictor(model, *scale))
    avgs = tuple(dev(model[k], torch.float64) for k in ("avg_cltr_u", "avg_cltr_i", "avg_cocltr"))
    tables = (dev(model["cltr_u"], torch.int32), dev(model["cltr_i"], torch.int32), avgs, dev(model["user_mean"], torch.float64),
              dev(model["item_mean"], torch.float64))
    qu = dev(np.repeat(owners, n_i), torch.int32)
    qi = dev(np.tile(np.arange(n_i), len(owners)), torch.int32)
    est, imp = coclustering.estimate_batch(*tables, model["mean"], qu, qi)
    pred = eccknn.predict(est, imp, model["mean"], scale).view(len(owners), n_i)
    mask = np.zeros((len(owners), n_i), dtype=bool)
    for row, u in enumerate(owners):
        if 0 <= u < n_u:
            mask[row, sorted(seen_sets[u])] = True
    stored = stored_path(pred, dev(mask, torch.bool), n_i)
    seen = algo._seen()
    for n in NS:
        wi, ws = T.lists(ranked, n)
        want = (dev(wi, torch.int32), dev(ws, torch.float64))
        assert_same((stored[0][:, :n], stored[1][:, :n]), want, (n, "stored path vs restatement"))
        for seg in SEGMENTS:
            got = coclustering.top_n(*tables, seen, model["mean"], scale, n, dev(owners, torch.int32), seg)
            assert_same(got, want, (n, seg, "fused vs restatement"))
            assert_same(got, (stored[0][:, :n].contiguous(), stored[1][:, :n].contiguous()), (n, seg, "fused vs stored path"))
    # what the case plants
    items, score = (host(t) for t in coclustering.top_n(*tables, seen, model["mean"], scale, 256, dev(owners, torch.int32)))
    unknown = int(np.nonzero(owners == -1)[0][0])
    clipped = np.minimum(scale[1], np.maximum(scale[0], model["item_mean"]))
    assert sorted(items[unknown][:n_i].tolist()) == list(range(n_i))         # an unknown owner: every item, at its clipped mean
    assert np.array_equal(score[unknown][:n_i], clipped[items[unknown][:n_i]]) and len(set(score[unknown][:n_i].tolist())) > 1
    assert np.array_equal(items[unknown], items[-1]) and np.array_equal(items[3], items[n_u + 1])     # owner n_users; repeats
    full = ts.to_inner_uid("full")
    assert (items[full] == -1).all() and np.isnan(score[full]).all()         # rated every item
    for u in range(n_u):
        unseen = min(256, n_i - len(seen_sets[u]))
        assert (items[u][:unseen] >= 0).all() and (items[u][unseen:] == -1).all() and np.isnan(score[u][unseen:]).all(), u
    ties = [row for row in range(n_u) if (score[row] == scale[1]).sum() >= 5]
    if scale != ts.rating_scale:
        assert ties                                               # many equal clipped scores: ranked by item id
    for row in ties:
        assert (np.diff(items[row][score[row] == scale[1]]) > 0).all(), row


def test_lists_recommend_and_metrics_of_the_class(fitted):
    algo, model, ts = fitted["algo"], fitted["model"], fitted["ts"]
    seen_sets = T.seen_sets(ts.u, ts.i, ts.n_users)
    every = T.rankings(seen_sets, ts.n_items, range(ts.n_users), C.predictor(model, *ts.rating_scale))
    wi, ws = T.lists(every, 10)
    assert_same(algo.top_n_lists(), (dev(wi, torch.int32), dev(ws, torch.float64)), "every user")
    users, items = list(ts._raw2inner_u), list(ts._raw2inner_i)
    recs = algo.recommend(5)
    assert list(recs) == users
    for u, ru in enumerate(users):
        assert recs[ru] == [(items[i], s) for i, s in every[u][:5]], ru
    picked = algo.top_n_lists(3, ["stranger", users[4]], segments=2)
    wi, ws = T.lists(T.rankings(seen_sets, ts.n_items, [-1, 4], C.predictor(model, *ts.rating_scale)), 3)
    assert_same(picked, (dev(wi, torch.int32), dev(ws, torch.float64)), "raw users")
    k = next(u for u in range(ts.n_users) if len(every[u]) >= 5)
    f1, m_ap, mrr, ndcg, per_user = algo.ranking_metrics([(users[k], items[every[k][0][0]], 5.0), ("stranger", items[0], 4.0)], 5)
    assert per_user.shape == (2, 5) and mrr >= 0.5 and 0.0 < f1 <= 1.0


# ---- malformed inputs: a ValueError, never a launch -------------------------------------------------------------------------

def test_malformed_inputs_are_value_errors():
    from n2v_hip import coclustering
    u, i, r = C.make_ratings(0, 70, 50, 600, "half")
    p = problem(u, i, r, 70, 50)
    cu, ci = (dev(a, torch.int32) for a in C.init(70, 50, C.params()))
    avgs = coclustering.averages(p["d_ul"], 50, cu, ci, 3, 3, p["mean"])
    before = (cu.clone(), ci.clone())
    ptr, ids, rs = p["d_ul"]
    bad_ids = ids.clone()
    bad_ids[3] = 50
    bad_ptr = ptr.clone()
    bad_ptr[1] = ids.numel() + 5
    for lst, msg in (((ptr, bad_ids, rs), "malformed lists: an x outside"), ((bad_ptr, ids, rs), "malformed lists: ptr")):
        with pytest.raises(ValueError, match=msg):
            coclustering.averages(lst, 50, cu, ci, 3, 3, p["mean"])
        with pytest.raises(ValueError, match=msg):
            coclustering.assign(lst, True, cu, ci, avgs, p["d_um"], p["d_im"])
        with pytest.raises(ValueError, match=msg):
            coclustering.epoch(lst, p["d_il"], cu, ci, 3, 3, p["mean"], p["d_um"], p["d_im"])
    bad_il = (p["d_il"][0], p["d_il"][1].clone(), p["d_il"][2])
    bad_il[1][0] = -1
    with pytest.raises(ValueError, match="malformed lists: an x outside"):
        coclustering.assign(bad_il, False, cu, ci, avgs, p["d_um"], p["d_im"])
    for bad_value in (3, -1):
        bad_cu, bad_ci = cu.clone(), ci.clone()
        bad_cu[5] = bad_value
        bad_ci[7] = bad_value
        with pytest.raises(ValueError, match=r"cltr_u holds a cluster id outside \[0, 3\)"):
            coclustering.averages(p["d_ul"], 50, bad_cu, ci, 3, 3, p["mean"])
        with pytest.raises(ValueError, match=r"cltr_i holds a cluster id outside \[0, 3\)"):
            coclustering.averages(p["d_ul"], 50, cu, bad_ci, 3, 3, p["mean"])
        with pytest.raises(ValueError, match=r"cltr_i holds a cluster id outside"):
            coclustering.assign(p["d_ul"], True, cu, bad_ci, avgs, p["d_um"], p["d_im"])
        with pytest.raises(ValueError, match=r"cltr_u holds a cluster id outside"):
            coclustering.assign(p["d_il"], False, bad_cu, ci, avgs, p["d_um"], p["d_im"])
        with pytest.raises(ValueError, match=r"cltr_u holds a cluster id outside"):
            coclustering.estimate_batch(bad_cu, ci, avgs, p["d_um"], p["d_im"], p["mean"], cu[:2], cu[:2])
    for kw in (dict(n_cltr_u=0), dict(n_cltr_u=65), dict(n_cltr_i=65)):
        with pytest.raises(ValueError, match=r"outside \[1, 64\]"):
            coclustering.averages(p["d_ul"], 50, cu, ci, **dict(dict(n_cltr_u=3, n_cltr_i=3, global_mean=p["mean"]), **kw))
    # aliased buffers: both assignments inside one allocation, overlapping by one entry
    both = torch.zeros(70 + 50 - 1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="aliased buffers"):
        coclustering.assign(p["d_ul"], True, both[:70], both[69:], avgs, p["d_um"], p["d_im"])
    with pytest.raises(ValueError, match="aliased buffers"):
        coclustering.assign(p["d_il"], False, both[:70], both[69:], avgs, p["d_um"], p["d_im"])
    assert torch.equal(cu, before[0]) and torch.equal(ci, before[1])             # nothing was launched
    # unchecked, an entry that is no item adds nothing and the row range is clamped: every other row keeps its bits
    cu2, ci2 = cu.clone(), ci.clone()
    coclustering.assign((ptr, bad_ids, rs), True, cu2, ci2, avgs, p["d_um"], p["d_im"], check=False)
    owner = int(np.searchsorted(p["ul"][0], 3, side="right") - 1)
    want = C.assign_users(p["ul"], host(ci).astype(np.int64), 3, tuple(host(a) for a in avgs), p["um"], p["im"])
    rows = np.arange(70) != owner
    assert np.array_equal(host(cu2)[rows], want[rows]) and 0 <= int(cu2[owner]) < 3


# ---- end to end ---------------------------------------------------------------------------------------------------------

def test_main_rec_coclustering_end_to_end(fitted, tmp_path, capsys):
    import main_rec
    case = fitted["case"]
    p = tmp_path / "ratings.csv"
    p.write_text("user,item,rating\n" + "".join("%s,%s,%r\n" % t for t in zip(case["raw_u"], case["raw_i"], case["r"].tolist())))
    base = ["-input", str(p), "-seed", "2", "-algo", "coclustering", "-clusters-u", "4", "-clusters-i", "2", "-epochs", "3"]
    plain = main_rec.main(base)
    assert isinstance(plain, float) and capsys.readouterr().out.strip() == "RMSE: %r" % plain
    recs_file = tmp_path / "recs.csv"
    rmse, metrics = main_rec.main(base + ["-topn", "10", "-threshold", "3", "-save-recs", str(recs_file)])
    out = capsys.readouterr().out.strip().split("\n")
    assert rmse == plain and out == ["RMSE: %r" % rmse, "F1 / MAP / MRR / NDCG @10: %r / %r / %r / %r" % tuple(metrics)]
    # the same split and model by hand, against the restatement
    args = main_rec.parse_args(base + ["-topn", "10", "-threshold", "3"])
    users, items, ratings = main_rec.read_ratings(str(p))
    train, test = main_rec.split(len(ratings), 0.2, 2)
    algo = main_rec.fit_split(args, users, items, ratings, None, train)
    ts = algo.trainset
    model = C.fit(ts.u, ts.i, ts.r, ts.n_users, ts.n_items, C.params(n_cltr_u=4, n_cltr_i=2, n_epochs=3, random_state=2))
    assert np.array_equal(host(algo.cltr_u), model["cltr_u"]) and np.array_equal(host(algo.cltr_i), model["cltr_i"])
    testset = [(users[k], items[k], ratings[k]) for k in test]
    est, imp = C.estimate_all(model, ts.inner_uids([t[0] for t in testset]), ts.inner_iids([t[1] for t in testset]))
    assert rmse == E.rmse([t[2] for t in testset], E.predict_all(est, imp, ts.global_mean, *ts.rating_scale))
    assert tuple(metrics) == algo.ranking_metrics(testset, 10, 3.0)[:4] and 0.0 <= min(metrics) and max(metrics) <= 1.0
    raw_items = list(ts._raw2inner_i)
    ranked = T.rankings(T.seen_sets(ts.u, ts.i, ts.n_users), ts.n_items, range(ts.n_users), C.predictor(model, *ts.rating_scale))
    want = ["%s,%s,%r" % (ru, raw_items[i], s) for ru, lst in zip(ts._raw2inner_u, ranked) for i, s in lst[:10]]
    assert recs_file.read_text().split("\n")[:-1] == want and len(want) > 20
    # -cv: one file per fold, one metrics line per fold
    folds = main_rec.main(base + ["-cv", "2", "-topn", "3", "-save-recs", str(tmp_path / "cv.csv")])
    out = capsys.readouterr().out.strip().split("\n")
    assert len(folds) == 2 and all(len(f) == 2 and len(f[1]) == 4 for f in folds)
    assert [l.split(":")[0] for l in out] == ["RMSE", "F1 / MAP / MRR / NDCG @3"] * 2 + ["mean RMSE"]
    assert (tmp_path / "cv.csv.0").exists() and (tmp_path / "cv.csv.1").exists()
