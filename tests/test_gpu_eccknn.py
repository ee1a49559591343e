"""GPU tests: the EccenKNN kernels (csrc/n2v_eccknn.hip, C-ABI include/n2v_sim.h) against the restatement
tests/eccknn_reference.py, through the C-ABI unless a test says otherwise.

Exact comparisons only: fp64 arrays by their bytes (E.canon: a NaN's sign and payload are not part of the contract,
everything else is), integers with array_equal.  The reference side is the numpy form, which tests/test_eccknn_host.py
holds to the literal loops bit for bit.  No query and no pair is left out or masked.

Parity: unpinned, restated from the text (the reference needs `surprise` and its main() raises)."""
import numpy as np
import pytest

import eccknn_reference as E

pytestmark = pytest.mark.gpu

SENT = -12345.5
ISENT = -7


def _L():
    from n2v_hip import _lib as L
    return L


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def c_sim(x, y, r, w, n_x, n_y, name, min_support):
    """n2v_eccknn_densify + n2v_eccknn_sim; every output starts as a sentinel.  Returns numpy arrays."""
    import torch
    L = _L(); lib = L.load()
    dx, dy, dr, dw = _dev(x, np.int32), _dev(y, np.int32), _dev(r, np.float64), _dev(w, np.float64)
    dense = torch.full((n_y, n_x), SENT, dtype=torch.float64, device="cuda")
    mask = torch.full((n_y, n_x), 9, dtype=torch.uint8, device="cuda")
    st = L.stream_ptr(dense.device)
    L.check(lib.n2v_eccknn_densify(L.ptr(dx), L.ptr(dy), L.ptr(dr), len(r), n_x, n_y, L.ptr(dense), L.ptr(mask), st))
    f64 = lambda: torch.full((n_x, n_x), SENT, dtype=torch.float64, device="cuda")
    out = {"sim": f64(), "freq": torch.full((n_x, n_x), ISENT, dtype=torch.int32, device="cuda")}
    for nm in (("prods", "sqi", "sqj") if name == "cosine" else ("sq_diff",)):
        out[nm] = f64()
    g = lambda nm: L.ptr(out[nm]) if nm in out else None
    L.check(lib.n2v_eccknn_sim(L.ptr(dense), L.ptr(mask), n_x, n_y, L.ptr(dw), {"cosine": 0, "msd": 1}[name], min_support,
                               g("sim"), g("freq"), g("prods"), g("sqi"), g("sqj"), g("sq_diff"), st))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["_dense"], res["_mask"], res["_dsim"] = dense.cpu().numpy(), mask.cpu().numpy(), out["sim"]
    return res


def check_sim(x, y, r, w, n_x, n_y, name, min_support):
    want = E.NUMPY[name](n_x, E.build_yr(x, y, r), min_support, w)
    got = c_sim(x, y, r, w, n_x, n_y, name, min_support)
    for key in want:
        if key == "freq":
            assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key
        else:
            assert E.canon(got[key]) == E.canon(want[key]), (key, name, min_support, n_x, n_y)
    s = got["sim"]                                           # symmetry and diagonal, on every case
    assert E.canon(s) == E.canon(s.T) and np.array_equal(np.diag(s), np.ones(n_x))
    return want, got


def c_estimate(dsim, n_x, yr, n_y, qx, qy, k, min_k, expect_rc=0):
    """n2v_eccknn_estimate; dsim: device fp64 [n_x][n_x]; yr: the restatement's dict."""
    import torch
    L = _L(); lib = L.load()
    ptr = np.zeros(n_y + 1, np.int64)
    for yy, lst in yr.items():
        ptr[yy + 1] = len(lst)
    ptr = np.cumsum(ptr)
    xs = np.array([xx for yy in sorted(yr) for xx, _ in yr[yy]] or [0], dtype=np.int32)
    rs = np.array([rr for yy in sorted(yr) for _, rr in yr[yy]] or [0.0], dtype=np.float64)
    n_q = len(qx)
    est = torch.full((max(n_q, 1),), SENT, dtype=torch.float64, device="cuda")
    ak = torch.full((max(n_q, 1),), ISENT, dtype=torch.int32, device="cuda")
    imp = torch.full((max(n_q, 1),), 9, dtype=torch.uint8, device="cuda")
    dq = _dev(qx if n_q else [0], np.int32), _dev(qy if n_q else [0], np.int32)
    dp, dxs, drs = _dev(ptr, np.int64), _dev(xs, np.int32), _dev(rs, np.float64)
    rc = lib.n2v_eccknn_estimate(L.ptr(dsim), n_x, L.ptr(dp), L.ptr(dxs), L.ptr(drs), n_y, L.ptr(dq[0]), L.ptr(dq[1]), n_q,
                                 k, min_k, L.ptr(est), L.ptr(ak), L.ptr(imp), L.stream_ptr(est.device))
    torch.cuda.synchronize()
    res = est.cpu().numpy(), ak.cpu().numpy(), imp.cpu().numpy()
    if expect_rc:
        assert rc == expect_rc, rc
        return lib.n2v_last_error().decode(), res
    L.check(rc)
    return res, (est, imp)


def check_estimate(sim, dsim, n_x, yr, n_y, qx, qy, k, min_k):
    want = E.estimate_all(sim, yr, qx, qy, k, min_k)
    got, dev = c_estimate(dsim, n_x, yr, n_y, qx, qy, k, min_k)
    assert E.canon(got[0]) == E.canon(want[0]), np.nonzero(got[0] != want[0])[0][:10]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    return want, dev


# ---- 1 + 2: accumulators and sim ---------------------------------------------------------------------------------------

KINDS = ["int", "half", "fp64"]


@pytest.mark.parametrize("n_y", [1, 31, 32, 33, 100])
@pytest.mark.parametrize("n_x", [1, 2, 63, 64, 65, 130])
def test_sim_and_accumulators_bit_for_bit(n_x, n_y):
    """Both similarities, min_support 1 and 3, and both roles of the two sides (item-based is user-based with x and y
    swapped, so the swapped run also covers n_x in {1, 31, 32, 33, 100} against n_y in {1, 2, 63, 64, 65, 130})."""
    kind = KINDS[(n_x + n_y) % 3]
    n = max(1, int((0.3 if n_y <= 33 else 0.2) * n_x * n_y))
    x, y, r, w = E.make_case(1000 * n_x + n_y, n_x, n_y, n, kind, zeros=3 if n >= 6 else 0)
    w_swapped = np.random.RandomState(n_x * 7 + n_y).normal(size=n_x)
    big = n_x >= 63 and n_y >= 31
    if n >= 6:
        assert (r == 0.0).sum() == 3                         # 0.0 is a rating: the mask and the value are told apart
    for name in ("cosine", "msd"):
        for ms in (1, 3):
            want, got = check_sim(x, y, r, w, n_x, n_y, name, ms)
            if n >= 6:
                assert (got["_mask"][got["_dense"] == 0.0] == 1).sum() == 3
            if big:
                f = want["freq"]
                assert (f[np.triu_indices(n_x, 1)] == ms).any(), "no pair exactly at freq == min_support"
                assert (f[np.triu_indices(n_x, 1)] == ms - 1).any()
                single = [k for k, v in E.build_yr(x, y, r).items() if len(v) == 1]
                assert single, "no y with a single rater"
                off = f - np.diag(np.diag(f))
                assert ((off.sum(axis=1) == 0) & (np.diag(f) > 0)).any(), "no x that shares nothing"
            check_sim(y, x, r, w_swapped, n_y, n_x, name, ms)


@pytest.fixture(scope="module")
def real_case():
    x, y, r, w = E.make_case(77, 300, 200, 5999, "half")
    out = {}
    for name in ("cosine", "msd"):
        out[name] = check_sim(x, y, r, w, 300, 200, name, 1)
    return x, y, r, w, out


def test_real_case_is_nan_free_and_symmetric(real_case):
    x, y, r, w, out = real_case
    assert len(r) == 6000 and (w < 0).any()
    for name in ("cosine", "msd"):
        want, got = out[name]
        s = got["sim"]
        assert not np.isnan(s).any()
        assert s.tobytes() == want["sim"].tobytes()
        assert s.tobytes() == np.ascontiguousarray(s.T).tobytes() and (np.diag(s) == 1.0).all()
        assert (s[np.triu_indices(300, 1)] != 0).sum() > 10000


def test_dense_limit_is_an_error():
    import torch
    L = _L(); lib = L.load()
    lim = lib.n2v_eccknn_max_dense()
    assert lim == 1 << 31
    one = torch.zeros(8, dtype=torch.float64, device="cuda")
    rc = lib.n2v_eccknn_sim(L.ptr(one), L.ptr(one), 1 << 16, (1 << 15) + 1, L.ptr(one), 0, 1, L.ptr(one), None, None, None,
                            None, None, L.stream_ptr(one.device))
    assert rc != 0 and "dense limit" in lib.n2v_last_error().decode()
    rc = lib.n2v_eccknn_sim(L.ptr(one), L.ptr(one), 4, 2, L.ptr(one), 2, 1, L.ptr(one), None, None, None, None, None,
                            L.stream_ptr(one.device))
    assert rc != 0 and "method" in lib.n2v_last_error().decode()


# ---- 3: estimates ------------------------------------------------------------------------------------------------------

LENGTHS = [0, 1, 63, 64, 65, 200]


@pytest.fixture(scope="module")
def length_case():
    """210 users over 20 base items (integer ratings: equal sims are common), then one item per list length with exactly
    that many raters in a shuffled order; the item of length 0 exists only as an id."""
    rs = np.random.RandomState(5)
    n_u, base = 210, 20
    tr = [(u, i, float(rs.randint(1, 6))) for u in range(n_u) for i in range(base) if rs.random_sample() < 0.5 or i == u % base]
    raw_item = {}
    for L_ in LENGTHS[1:]:
        raw_item[L_] = base + len(raw_item)
        for u in rs.permutation(n_u)[:L_]:
            tr.append((int(u), raw_item[L_], float(rs.randint(1, 6))))
    x, xraw = E.inner_ids([t[0] for t in tr]); y, yraw = E.inner_ids([t[1] for t in tr])
    r = np.array([t[2] for t in tr])
    n_x, n_y = len(xraw), len(yraw) + 1                      # the last y has no rater
    item_of = {L_: yraw.index(v) for L_, v in raw_item.items()}
    item_of[0] = n_y - 1
    w = rs.normal(size=n_y)
    want, got = check_sim(x, y, r, w, n_x, n_y, "cosine", 1)
    yr = E.build_yr(x, y, r)
    assert n_x == n_u and [len(yr.get(item_of[L_], [])) for L_ in LENGTHS] == LENGTHS
    return n_x, n_y, yr, want["sim"], got["_dsim"], item_of


@pytest.mark.parametrize("min_k", [1, 5])
@pytest.mark.parametrize("k", [1, 20, 40, 256])
def test_estimates_bit_for_bit_over_list_lengths(length_case, k, min_k):
    n_x, n_y, yr, sim, dsim, item_of = length_case
    users = [0, 1, 2, 63, 64, 100, 209]
    qx = [u for u in users for _ in LENGTHS] + [-1, 5, -1]
    qy = [item_of[L_] for _ in users for L_ in LENGTHS] + [item_of[64], -1, -1]
    (est, ak, imp), _ = check_estimate(sim, dsim, n_x, yr, n_y, qx, qy, k, min_k)
    lens = np.array(LENGTHS * len(users))
    assert imp[-3:].tolist() == [1, 1, 1] and imp[:len(lens)][lens == 0].all()      # unknown user / item, empty list
    assert (lens[imp[:len(lens)] == 0] >= min_k).all()
    if k >= min_k:
        assert (imp == 0).sum() >= len(users) * 3
    assert (lens > k).any() or k == 256                      # k below and above the list length
    assert (lens[lens > 0] < k).any() or k == 1


@pytest.fixture(scope="module")
def crafted_case():
    """u0 and 30 users with one identical rating row (equal sims to u0), 5 others, all rating the target item in an order
    that reverses the ids of the identical users; nz shares only a 0.0-rated item with u0 (cosine: 0/0 = NaN); p0..p2 share
    nothing with u0 and alone rate the item yN."""
    rs = np.random.RandomState(11)
    tr = [("u0", "b%d" % i, float(v)) for i, v in enumerate([5, 1, 4, 2, 3, 5])] + [("u0", "yZ", 0.0)]
    for g in range(30):
        tr += [("g%d" % g, "b%d" % i, float(v)) for i, v in enumerate([3, 4, 2, 5, 1, 4])]
    for o in range(5):
        tr += [("o%d" % o, "b%d" % i, float(rs.randint(1, 6))) for i in range(6)]
    tr += [("nz", "yZ", 0.0)]
    order = ["o0"] + ["g%d" % g for g in range(29, 14, -1)] + ["o1", "nz", "o2"] + ["g%d" % g for g in range(14, -1, -1)] + ["o3", "o4"]
    tr += [(u, "yT", float(rs.randint(1, 6))) for u in order]
    for p in range(3):
        tr += [("p%d" % p, "yN", float(p + 1)), ("p%d" % p, "q%d" % p, 2.0)]
    x, xraw = E.inner_ids([t[0] for t in tr]); y, yraw = E.inner_ids([t[1] for t in tr])
    r = np.array([t[2] for t in tr])
    n_x, n_y = len(xraw), len(yraw)
    w = np.abs(np.random.RandomState(12).normal(size=n_y)) + 0.1
    want, got = check_sim(x, y, r, w, n_x, n_y, "cosine", 1)
    return n_x, n_y, E.build_yr(x, y, r), want["sim"], got["_dsim"], xraw, yraw


@pytest.mark.parametrize("k", [1, 20, 40, 256])
def test_equal_sims_straddle_rank_k_and_nan_ranks_last(crafted_case, k):
    n_x, n_y, yr, sim, dsim, xraw, yraw = crafted_case
    u0, yT, yN = xraw.index("u0"), yraw.index("yT"), yraw.index("yN")
    row = np.array([sim[u0, x2] for x2, _ in yr[yT]])
    g = np.array([xraw[x2].startswith("g") for x2, _ in yr[yT]])
    assert len(set(row[g].tolist())) == 1 and g.sum() == 30 and row[g][0] > 0
    assert np.isnan(sim[u0, xraw.index("nz")]) and np.isnan(row).sum() == 1
    above, not_below = int((row > row[g][0]).sum()), int((row >= row[g][0]).sum())
    if k == 20:
        assert above < k < not_below                         # rank k falls inside the group: list position decides
    gx = [x2 for x2, _ in yr[yT] if xraw[x2].startswith("g")]
    assert gx == sorted(gx, reverse=True)                    # ... and position order is not id order
    want, _ = check_estimate(sim, dsim, n_x, yr, n_y, [u0, u0], [yT, yN], k, 1)
    assert want[2].tolist() == [0, 1]                        # yN: an all-non-positive neighbourhood
    assert all(not sim[u0, x2] > 0 for x2, _ in yr[yN]) and want[1][1] == 0
    assert want[1][0] == min(k, int((row > 0).sum()))        # the NaN is never summed, also when k takes every entry
    if k == 20:                                              # the other tie rule would give another estimate
        sel = sorted(range(len(row)), key=lambda p: (-(row[p] if row[p] == row[p] else -np.inf), -p))[:k]
        other = sum(row[p] * yr[yT][p][1] for p in sel) / sum(row[p] for p in sel)
        assert abs(other - want[0][0]) > 1e-9


def test_negative_zero_ties_positive_zero_and_only_positive_sims_count():
    """A crafted sim matrix straight into n2v_eccknn_estimate: -0.0 and +0.0 tie (list position decides between them),
    and sim == 0 is not summed."""
    n_x = 8
    sim = np.eye(n_x)
    sim[0, 1:] = [-0.0, 0.0, -0.0, 0.5, 0.0, -1.0, np.nan]
    sim[1:, 0] = sim[0, 1:]
    yr = {0: [(6, 1.0), (1, 2.0), (2, 3.0), (3, 4.0), (5, 5.0), (7, 1.5), (4, 2.5)], 1: [(1, 2.0), (2, 3.0), (6, 1.0)]}
    assert np.signbit(sim[0, 1]) and not np.signbit(sim[0, 2])
    dsim = _dev(sim, np.float64)
    for k in (1, 2, 3, 4, 7, 256):
        for min_k in (1, 2):
            want, _ = check_estimate(sim, dsim, n_x, yr, 2, [0, 0], [0, 1], k, min_k)
            assert want[1].tolist() == [1, 0] and want[2].tolist() == [int(min_k > 1), 1]
            if min_k == 1:
                assert want[0][0] == 2.5
    # an over-large entry of the sim row and a huge rating: inf / inf is a NaN estimate, not impossible
    sim2 = np.eye(3); sim2[0, 1] = sim2[1, 0] = 1e308; sim2[0, 2] = sim2[2, 0] = 1e308
    want, _ = check_estimate(sim2, _dev(sim2, np.float64), 3, {0: [(1, 5.0), (2, 5.0)]}, 1, [0], [0], 40, 1)
    assert np.isnan(want[0][0]) and want[2][0] == 0


def test_estimate_argument_errors_launch_nothing(length_case):
    n_x, n_y, yr, sim, dsim, item_of = length_case
    L = _L(); lib = L.load()
    assert lib.n2v_eccknn_max_k() == 256
    for k, min_k, qx, word in ((257, 1, [0], "k 257"), (0, 1, [0], "k 0"), (20, 1, [], "n_q 0"), (20, 0, [0], "min_k 0")):
        msg, (est, ak, imp) = c_estimate(dsim, n_x, yr, n_y, qx, [item_of[64]] * len(qx), k, min_k, expect_rc=-1)
        assert word in msg, msg
        assert (est == SENT).all() and (ak == ISENT).all() and (imp == 9).all()


# ---- 4: predict and rmse -----------------------------------------------------------------------------------------------

def c_predict(est, imp, r_true, mean, lo, hi):
    import torch
    L = _L(); lib = L.load()
    de, di, dr = _dev(est, np.float64), _dev(imp, np.uint8), _dev(r_true, np.float64)
    pred = torch.full((len(est),), SENT, dtype=torch.float64, device="cuda")
    out = torch.full((1,), SENT, dtype=torch.float64, device="cuda")
    L.check(lib.n2v_eccknn_predict(L.ptr(de), L.ptr(di), L.ptr(dr), len(est), mean, lo, hi, L.ptr(pred), L.ptr(out),
                                   L.stream_ptr(pred.device)))
    torch.cuda.synchronize()
    return pred.cpu().numpy(), float(out.item())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_predict_falls_back_clips_and_sums_in_order(n):
    rs = np.random.RandomState(n)
    est = rs.normal(size=n) * 3 + 3                          # well outside [1, 5] on both sides
    imp = (rs.random_sample(n) < 0.2).astype(np.uint8)
    est[imp == 1] = 0.0
    if n >= 255:
        est[7] = np.nan; imp[7] = 0                          # min(hi, nan) is hi
        assert (est[imp == 0] < 1).any() and (est[imp == 0] > 5).any() and imp.any()
    r_true = rs.randint(1, 11, size=n) * 0.5 + rs.normal(size=n) * 1e-3
    mean = 3.0 + rs.normal() * 0.1
    want = E.predict_all(est, imp, mean, 1.0, 5.0)
    pred, err = c_predict(est, imp, r_true, mean, 1.0, 5.0)
    assert pred.tobytes() == want.tobytes()
    assert (pred[imp == 1] == mean).all() and pred.min() >= 1.0 and pred.max() <= 5.0
    assert err == E.rmse(r_true, want)
    # a mean outside the scale is clipped as well
    pred2, _ = c_predict(est, imp, r_true, 7.5, 1.0, 5.0)
    assert pred2.tobytes() == E.predict_all(est, imp, 7.5, 1.0, 5.0).tobytes()


# ---- 5: the Python surface ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def raw_case():
    rs = np.random.RandomState(21)
    cells = rs.permutation(90 * 70)[:1500]
    users = ["u%d" % (c // 70) for c in cells]
    items = [1000 + int(c % 70) for c in cells]
    r = rs.randint(1, 11, size=1500) * 0.5
    test = [("u%d" % rs.randint(0, 95), 1000 + int(rs.randint(0, 75)), float(rs.randint(1, 11) * 0.5)) for _ in range(400)]
    return users, items, r, test


@pytest.mark.parametrize("name", ["cosine", "msd"])
@pytest.mark.parametrize("user_based", [True, False])
def test_python_surface_agrees_with_the_c_abi_path(raw_case, name, user_based):
    from n2v_hip import eccknn
    users, items, r, test = raw_case
    ts = eccknn.Trainset.from_ratings(users, items, r, rating_scale=(2.5, 3.0))
    wd = {raw: float(np.sin(i) + 0.3) for i, raw in enumerate(dict.fromkeys(items if user_based else users))}
    algo = eccknn.EccenKNN(k=20, min_k=8, sim_options={"name": name, "user_based": user_based, "min_support": 3})
    assert algo.fit(ts, wd) is algo
    xs, ys = (ts.u, ts.i) if user_based else (ts.i, ts.u)
    n_x, n_y = (ts.n_users, ts.n_items) if user_based else (ts.n_items, ts.n_users)
    table = ts._raw2inner_i if user_based else ts._raw2inner_u
    w = np.empty(n_y)
    for raw, inner in table.items():
        w[inner] = wd[raw]
    want, got = check_sim(xs, ys, r, w, n_x, n_y, name, 3)
    assert algo.sim.dtype.is_floating_point and tuple(algo.sim.shape) == (n_x, n_x)
    assert E.canon(algo.sim.cpu().numpy()) == E.canon(got["sim"])
    yr = E.build_yr(xs, ys, r)
    qu, qi = ts.inner_uids([t[0] for t in test]), ts.inner_iids([t[1] for t in test])
    assert (qu < 0).any() and (qi < 0).any()
    qx, qy = (qu, qi) if user_based else (qi, qu)
    west, wak, wimp = E.estimate_all(want["sim"], yr, qx, qy, 20, 8)
    wpred = E.predict_all(west, wimp, E.global_mean(r), 2.5, 3.0)
    pred, ak, imp = algo.test(test)
    assert pred.tobytes() == wpred.tobytes() and np.array_equal(ak, wak) and np.array_equal(imp, wimp.astype(bool))
    assert 0 < imp.sum() < len(test) and (pred == 2.5).any() and (pred == 3.0).any()
    assert algo.rmse(test) == E.rmse([t[2] for t in test], wpred)
    known = (qu >= 0) & (qi >= 0)
    ok, bad = np.nonzero(known & (wimp == 0))[0][:3], np.nonzero(known & (wimp == 1))[0][:2]
    assert len(ok) == 3 and (len(bad) == 2 or name == "msd")     # msd sims are all positive: nothing known is impossible
    for q in ok:
        assert algo.estimate(int(qu[q]), int(qi[q])) == (west[q], {"actual_k": int(wak[q])})
    for q in bad:
        with pytest.raises(eccknn.PredictionImpossible):
            algo.estimate(int(qu[q]), int(qi[q]))
    with pytest.raises(eccknn.PredictionImpossible):
        algo.estimate(ts.n_users, 0)
    with pytest.raises(ValueError, match="empty"):
        algo.test([])


def test_item_based_equals_user_based_on_the_transposed_data(raw_case):
    from n2v_hip import eccknn
    users, items, r, test = raw_case
    w_items = np.cos(np.arange(len(set(items)))) + 0.2
    a = eccknn.EccenKNN(k=40, sim_options={"name": "cosine", "user_based": True}).fit(
        eccknn.Trainset.from_ratings(users, items, r), w_items)
    b = eccknn.EccenKNN(k=40, sim_options={"name": "cosine", "user_based": False}).fit(
        eccknn.Trainset.from_ratings(items, users, r), w_items)
    assert E.canon(a.sim.cpu().numpy()) == E.canon(b.sim.cpu().numpy())
    ra, rb = a.test(test), b.test([(i, u, t) for u, i, t in test])
    for va, vb in zip(ra, rb):
        assert va.tobytes() == vb.tobytes()
    assert a.rmse(test) == b.rmse([(i, u, t) for u, i, t in test])


def test_python_surface_argument_errors(raw_case):
    import torch
    from n2v_hip import eccknn
    sim = torch.eye(4, dtype=torch.float64, device="cuda")
    yr = (torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
          torch.zeros(1, dtype=torch.float64, device="cuda"))
    q = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in (0, eccknn.MAX_K + 1):
        with pytest.raises(ValueError, match="k %d outside" % k):
            eccknn.estimate_batch(sim, yr, q, q, k, 1)
    with pytest.raises(ValueError, match="nothing to estimate"):
        eccknn.estimate_batch(sim, yr, q[:0], q[:0], 20, 1)


def test_main_rec_prints_the_restatements_rmse(tmp_path, capsys):
    import main_rec
    rs = np.random.RandomState(31)
    cells = rs.permutation(40 * 30)[:500]
    lines = ["userId,movieId,rating,timestamp"] + ["%d,%d,%.1f,%d" % (c // 30 + 1, c % 30 + 100, rs.randint(1, 11) * 0.5, n)
                                                    for n, c in enumerate(cells)]
    p = tmp_path / "ratings.csv"
    p.write_text("\n".join(lines) + "\n")
    wl = ["%d,%r" % (i + 100, float(rs.normal())) for i in range(30)]
    q = tmp_path / "w.csv"
    q.write_text("\n".join(wl) + "\n")
    err = main_rec.main(["-input", str(p), "-k", "20", "-sim", "msd", "-weights", str(q), "-test-ratio", "0.25", "-seed", "4"])
    assert capsys.readouterr().out.strip() == "RMSE: %r" % err
    users, items, ratings = main_rec.read_ratings(str(p))
    wd = main_rec.read_weights(str(q))
    train, test = main_rec.split(500, 0.25, 4)
    x, xraw = E.inner_ids([users[i] for i in train]); y, yraw = E.inner_ids([items[i] for i in train])
    r = ratings[train]
    w = np.array([wd[v] for v in yraw])
    sim = E.msd_numpy(len(xraw), E.build_yr(x, y, r), 1, w)["sim"]
    qx = [xraw.index(users[i]) if users[i] in xraw else -1 for i in test]
    qy = [yraw.index(items[i]) if items[i] in yraw else -1 for i in test]
    est, _, imp = E.estimate_all(sim, E.build_yr(x, y, r), qx, qy, 20, 1)
    pred = E.predict_all(est, imp, E.global_mean(r), float(ratings.min()), float(ratings.max()))
    assert err == E.rmse(ratings[test], pred)
