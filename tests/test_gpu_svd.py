"""GPU tests of the matrix-factorisation kernels (n2v_svd_blocks_check, n2v_svd_epoch, n2v_svd_estimate;
csrc/n2v_svd.hip, C-ABI include/n2v_sim.h) against the restatement tests/svd_reference.py, through the C-ABI unless a
test says otherwise, then n2v_hip.svd and the driver.

Exact comparisons only: fp64 arrays by their bytes (E.canon: one canonical NaN), integers with array_equal."""
import functools

import numpy as np
import pytest

import eccknn_reference as E
import svd_reference as S

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 40, 30
EIGHT = dict(lr_bu=0.011, lr_bi=0.007, lr_pu=0.013, lr_qi=0.005, reg_bu=0.03, reg_bi=0.05, reg_pu=0.02, reg_qi=0.07)
FACTORS = [1, 63, 64, 65, 100, 128, 129, 256]                    # every edge of the four lane slots
STRATA = [1, 2, 3, 7, 64, 100]                                   # 64 and 100 exceed both sides: mostly empty blocks


def _L():
    from n2v_hip import _lib as L
    return L


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


@functools.lru_cache(maxsize=None)
def ratings():
    """400 ratings of 39 x 29 plus one: user 39 rates only item 29 and nobody else does, so that user and that item
    have ratings in one stratum only."""
    u, i, r = S.make_ratings(5, N_USERS - 1, N_ITEMS - 1, 400)
    u, i, r = np.append(u, N_USERS - 1), np.append(i, N_ITEMS - 1), np.append(r, 4.5)
    o = np.random.RandomState(6).permutation(len(r))
    return u[o], i[o], r[o]


@functools.lru_cache(maxsize=None)
def restated(nf, P, n_epochs, biased=True, lr_all=None):
    u, i, r = ratings()
    kw = dict(lr_all=lr_all) if lr_all is not None else EIGHT
    return S.fit(u, i, r, N_USERS, N_ITEMS, S.params(n_factors=nf, biased=biased, random_state=nf, **kw), P, n_epochs)


def host_blocks(u, i, r, n_users, n_items, P):
    """(blk_ptr, blk_u, blk_i, blk_r) on the host, by the restatement's block_order."""
    o = S.all_ratings_order(u)
    u, i, r = np.asarray(u)[o], np.asarray(i)[o], np.asarray(r, np.float64)[o]
    order, ptr = S.block_order(u, i, n_users, n_items, P)
    return ptr, u[order].astype(np.int32), i[order].astype(np.int32), r[order]


def status_of(ptr, bu, bi, P, n_users, n_items):
    import torch
    L = _L(); lib = L.load()
    d = _dev(ptr, np.int64), _dev(bu, np.int32), _dev(bi, np.int32)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(lib.n2v_svd_blocks_check(L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), P, n_users, n_items, len(bu), L.ptr(status),
                                     L.stream_ptr(status.device)))
    return int(status.item())


class CFit:
    """The raw C-ABI path: host block lists, checked, the restatement's initial model, then epochs on request."""

    def __init__(self, u, i, r, n_users, n_items, par, P):
        L = _L()
        blk = host_blocks(u, i, r, n_users, n_items, P)
        assert status_of(blk[0], blk[1], blk[2], P, n_users, n_items) == 0
        self.blk = _dev(blk[0], np.int64), _dev(blk[1], np.int32), _dev(blk[2], np.int32), _dev(blk[3], np.float64)
        self.model = [_dev(a, np.float64) for a in S.init(n_users, n_items, par)]
        self.mu = S.global_mean(r) if par["biased"] else 0.0
        self.head = [L.ptr(t) for t in self.blk] + [P, n_users, n_items, len(r), par["n_factors"], self.mu,
                                                    1 if par["biased"] else 0] + [par[k] for k in S.RATES]

    def epochs(self, n):
        import torch
        L = _L(); lib = L.load()
        for _ in range(n):
            L.check(lib.n2v_svd_epoch(*self.head, *[L.ptr(t) for t in self.model], L.stream_ptr(self.model[0].device)))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in self.model]


def assert_model(got, want, what):
    for name, g, w in zip(("bu", "bi", "pu", "qi"), got, want[1:]):
        assert g.shape == w.shape and E.canon(g) == E.canon(w), (name,) + what


# ---- 1: parity with the restatement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", STRATA)
@pytest.mark.parametrize("nf", FACTORS)
def test_model_bit_for_bit_after_one_and_three_epochs(nf, P):
    u, i, r = ratings()
    run = CFit(u, i, r, N_USERS, N_ITEMS, S.params(n_factors=nf, random_state=nf, **EIGHT), P)
    assert_model(run.epochs(1), restated(nf, P, 1), (nf, P, 1))
    got = run.epochs(2)
    assert_model(got, restated(nf, P, 3), (nf, P, 3))
    assert np.isfinite(got[2]).all() and (got[0] != 0).all() and (got[1] != 0).all()


def test_the_cases_cover_what_they_claim():
    u, i, r = ratings()
    assert len(r) == 401 and set(u) == set(range(N_USERS)) and (u == 39).sum() == 1 and (i == 29).sum() == 1
    for P in (3, 7):
        s, ub = S.block_keys(u, i, N_USERS, N_ITEMS, P)
        assert len(set(s[u == 5])) > 1 and len(set(zip(s, ub))) > P          # a user in several strata, many blocks
    ptr = host_blocks(u, i, r, N_USERS, N_ITEMS, 100)[0]
    assert (np.diff(ptr) == 0).mean() > 0.9 and 100 > N_USERS
    a, b = restated(100, 1, 1), restated(100, 7, 1)
    assert E.canon(a[3]) != E.canon(b[3])                        # the schedule is visible in the bytes
    # eight distinct rates: swapping any two changes the restatement
    base = S.params(n_factors=3, random_state=1, **EIGHT)
    ref = S.fit(u, i, r, N_USERS, N_ITEMS, base, 2, 1)
    for x in range(8):
        for y in range(x + 1, 8):
            kx, ky = S.RATES[x], S.RATES[y]
            swapped = S.fit(u, i, r, N_USERS, N_ITEMS, dict(base, **{kx: base[ky], ky: base[kx]}), 2, 1)
            assert any(E.canon(p) != E.canon(q) for p, q in zip(ref[1:], swapped[1:])), (kx, ky)


@pytest.mark.parametrize("P", [1, 3, 64])
@pytest.mark.parametrize("nf", [1, 65, 256])
def test_unbiased_bit_for_bit(nf, P):
    import torch
    u, i, r = ratings()
    run = CFit(u, i, r, N_USERS, N_ITEMS, S.params(n_factors=nf, biased=False, random_state=nf, **EIGHT), P)
    run.model[0].fill_(-7.5); run.model[1].fill_(-7.5)            # neither read nor written
    got = run.epochs(3)
    want = restated(nf, P, 3, biased=False)
    assert want[0] == 0.0 and E.canon(got[2]) == E.canon(want[3]) and E.canon(got[3]) == E.canon(want[4])
    assert (got[0] == -7.5).all() and (got[1] == -7.5).all()
    L = _L(); lib = L.load()                                      # a fourth epoch with NULL biases
    L.check(lib.n2v_svd_epoch(*run.head, None, None, L.ptr(run.model[2]), L.ptr(run.model[3]), L.stream_ptr(run.model[2].device)))
    torch.cuda.synchronize()
    assert E.canon(run.model[2].cpu().numpy()) == E.canon(restated(nf, P, 4, biased=False)[3])


@pytest.mark.parametrize("case", [(1, 1, 0, 0, 1), (1, 1, 0, 0, 3), (5, 4, 3, 2, 1), (5, 4, 3, 2, 2), (5, 4, 0, 3, 9)])
def test_single_rating_trainset(case):
    n_users, n_items, u, i, P = case
    for nf in (2, 70):
        par = S.params(n_factors=nf, random_state=3, **EIGHT)
        run = CFit([u], [i], [3.5], n_users, n_items, par, P)
        want = S.fit([u], [i], [3.5], n_users, n_items, par, P, 2)
        assert_model(run.epochs(2), want, case)
        init = S.init(n_users, n_items, par)
        assert (want[3][u] != init[2][u]).all() and np.array_equal(np.delete(want[3], u, 0), np.delete(init[2], u, 0))


@pytest.mark.parametrize("nf,P", [(65, 2), (100, 3), (256, 7)])
def test_overflow_reaches_the_same_positions(nf, P):
    """lr_all = 0.5 diverges: during the first epoch some factors pass 1e308 (inf), inf - inf and 0 * inf make NaN, and
    the rows that have not met them yet are still finite; after the second epoch everything that has a neighbour is
    NaN.  After every epoch the same entries are finite, inf, -inf and NaN as in the restatement, with the same bits."""
    u, i, r = ratings()
    run = CFit(u, i, r, N_USERS, N_ITEMS, S.params(n_factors=nf, random_state=nf, lr_all=0.5), P)
    for e in (1, 2, 3):
        got, want = run.epochs(1), restated(nf, P, e, lr_all=0.5)
        assert_model(got, want, (nf, P, e))
        for g, w in zip(got, want[1:]):
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isposinf(g), np.isposinf(w))
            assert np.array_equal(np.isneginf(g), np.isneginf(w))
        both = np.concatenate([want[3].ravel(), want[4].ravel()])
        if e == 1 and nf >= 100:                                  # 65 factors are still finite after one epoch
            assert np.isnan(both).any() and np.isinf(both).any() and np.isfinite(both).any() and np.isnan(want[1]).any()
    assert np.isnan(want[3][:39]).all() and np.isfinite(want[3][39]).all()       # user 39 met nobody


# ---- 2: estimates ------------------------------------------------------------------------------------------------------

def c_estimate(model, biased, qu, qi):
    import torch
    L = _L(); lib = L.load()
    mu, d = model[0], [_dev(a, np.float64) for a in model[1:]]
    dq = _dev(qu, np.int32), _dev(qi, np.int32)
    est = torch.full((len(qu),), -12345.5, dtype=torch.float64, device="cuda")
    imp = torch.full((len(qu),), 9, dtype=torch.uint8, device="cuda")
    L.check(lib.n2v_svd_estimate(*[L.ptr(t) for t in d], len(model[1]), len(model[2]), model[3].shape[1], float(mu),
                                 1 if biased else 0, L.ptr(dq[0]), L.ptr(dq[1]), len(qu), L.ptr(est), L.ptr(imp),
                                 L.stream_ptr(est.device)))
    torch.cuda.synchronize()
    return est, imp


@pytest.mark.parametrize("biased", [True, False])
@pytest.mark.parametrize("nf", FACTORS)
def test_estimates_and_rmse_bit_for_bit(nf, biased):
    from n2v_hip import eccknn
    model = restated(nf, 3, 1, biased=biased)
    rs = np.random.RandomState(nf)
    qu = np.concatenate([rs.randint(0, N_USERS, 150), [-1, 3, -1, N_USERS, 0, 39]])
    qi = np.concatenate([rs.randint(0, N_ITEMS, 150), [4, -1, -1, 2, N_ITEMS, 29]])
    qu[:150][rs.random_sample(150) < 0.15] = -1
    qi[:150][rs.random_sample(150) < 0.15] = -1
    r_true = rs.randint(1, 11, size=len(qu)) * 0.5
    est, imp = c_estimate(model, biased, qu, qi)
    west, wimp = S.estimate(model, [u if u < N_USERS else -1 for u in qu], [i if i < N_ITEMS else -1 for i in qi], biased)
    assert E.canon(est.cpu().numpy()) == E.canon(west) and np.array_equal(imp.cpu().numpy(), wimp)
    assert wimp.any() == (not biased) and (wimp == 0).sum() >= 60
    lo, hi = [float(v) for v in np.sort(west)[[len(west) // 4, 3 * len(west) // 4]]]     # both clips happen
    mean = (lo + hi) / 2
    pred, err = eccknn.predict(est, imp, mean, (lo, hi), _dev(r_true, np.float64))
    wpred = E.predict_all(west, wimp, mean, lo, hi)
    assert pred.cpu().numpy().tobytes() == wpred.tobytes() and err == E.rmse(r_true, wpred)
    assert (west < lo).any() and (west > hi).any() and lo < hi


# ---- 3: determinism and the Python surface -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def raw_case():
    rs = np.random.RandomState(21)
    cells = rs.permutation(45 * 35)[:450]
    users = ["u%d" % (c // 35) for c in cells]
    items = [1000 + int(c % 35) for c in cells]
    r = rs.randint(1, 11, size=450) * 0.5
    test = [("u%d" % rs.randint(0, 50), 1000 + int(rs.randint(0, 40)), float(rs.randint(1, 11) * 0.5)) for _ in range(200)]
    return users, items, r, test


@pytest.mark.parametrize("biased", [True, False])
def test_svd_class_equals_the_c_abi_path_and_repeats_itself(raw_case, biased):
    from n2v_hip import eccknn, svd
    users, items, r, test = raw_case
    ts = eccknn.Trainset.from_ratings(users, items, r, rating_scale=(1.0, 4.5))
    kw = dict(n_factors=70, n_epochs=3, biased=biased, random_state=11, **EIGHT)
    algo = svd.SVD(n_strata=5, **kw)
    assert algo.fit(ts) is algo and algo.n_strata_used == 5
    got = [t.cpu().numpy() for t in (algo.bu, algo.bi, algo.pu, algo.qi)]
    again = svd.SVD(n_strata=5, **kw).fit(ts)
    assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(got, (again.bu, again.bi, again.pu, again.qi)))
    par = S.params(**kw)
    raw = CFit(ts.u, ts.i, r, ts.n_users, ts.n_items, par, 5)
    twice = CFit(ts.u, ts.i, r, ts.n_users, ts.n_items, par, 5)
    m = raw.epochs(3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m, twice.epochs(3)))
    if not biased:
        assert not got[0].any() and not got[1].any()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, m))
    want = S.fit(ts.u, ts.i, r, ts.n_users, ts.n_items, par, 5)
    assert_model(got, want, ("class", biased))
    assert algo.mu == want[0] and (algo.mu == ts.global_mean) == biased
    # the block lists torch builds are the restatement's
    for a, b in zip((algo.blocks.ptr, algo.blocks.u, algo.blocks.i, algo.blocks.r), host_blocks(ts.u, ts.i, r, ts.n_users, ts.n_items, 5)):
        assert np.array_equal(a.cpu().numpy(), b) and a.cpu().numpy().dtype == b.dtype
    # test / rmse / estimate
    qu, qi = ts.inner_uids([t[0] for t in test]), ts.inner_iids([t[1] for t in test])
    west, wimp = S.estimate(want, qu, qi, biased)
    wpred = E.predict_all(west, wimp, E.global_mean(r), 1.0, 4.5)
    pred, imp = algo.test(test)
    assert pred.tobytes() == wpred.tobytes() and np.array_equal(imp, wimp.astype(bool)) and imp.any() == (not biased)
    assert algo.rmse(test) == E.rmse([t[2] for t in test], wpred)
    q = int(np.nonzero((qu >= 0) & (qi >= 0))[0][0])
    assert algo.estimate(int(qu[q]), int(qi[q])) == west[q]
    if biased:
        assert algo.estimate(10 ** 6, int(qi[q])) == want[0] + want[2][qi[q]] and algo.estimate("x", None) == want[0]
    else:
        with pytest.raises(eccknn.PredictionImpossible, match="User and item are unknown"):
            algo.estimate(10 ** 6, int(qi[q]))
    auto = svd.SVD(n_factors=4, n_epochs=1).fit(ts)
    assert auto.n_strata_used == svd.auto_strata(ts.n_users, ts.n_items, 450) == 4
    assert_model([t.cpu().numpy() for t in (auto.bu, auto.bi, auto.pu, auto.qi)],
                 S.fit(ts.u, ts.i, r, ts.n_users, ts.n_items, S.params(n_factors=4, n_epochs=1), 4), ("auto",))
    zero = svd.SVD(n_factors=4, n_epochs=0, n_strata=2).fit(ts)
    assert zero.pu.cpu().numpy().tobytes() == S.init(ts.n_users, ts.n_items, S.params(n_factors=4))[2].tobytes()


# ---- 4: the block check ------------------------------------------------------------------------------------------------

def test_blocks_check_names_the_cause():
    """Integers only: the check reads blk_ptr[0 .. P * P] and the n entries, whatever they hold.  None of these lists
    is given to n2v_svd_epoch."""
    import torch
    from n2v_hip import svd
    u, i, r = ratings()
    P = 3
    ptr, bu, bi, br = host_blocks(u, i, r, N_USERS, N_ITEMS, P)
    n = len(br)

    def blocks(ptr_=ptr, bu_=bu, bi_=bi):
        return svd.Blocks((_dev(ptr_, np.int64), _dev(bu_, np.int32), _dev(bi_, np.int32), _dev(br, np.float64)), N_USERS, N_ITEMS, P)

    ok = blocks()
    assert (ok.n, ok.n_strata) == (n, 3) and status_of(ptr, bu, bi, P, N_USERS, N_ITEMS) == 0
    sizes = np.diff(ptr)
    a, b = [int(k) for k in np.nonzero(sizes >= 2)[0][:2]]
    # a rating moved into a wrong block: the first entries of two blocks change places
    mu, mi = bu.copy(), bi.copy()
    ja, jb = int(ptr[a]), int(ptr[b])
    mu[[ja, jb]], mi[[ja, jb]] = bu[[jb, ja]], bi[[jb, ja]]
    assert status_of(ptr, mu, mi, P, N_USERS, N_ITEMS) & 8
    with pytest.raises(ValueError, match="outside the block"):
        blocks(bu_=mu, bi_=mi)
    # ids out of range
    for arr, val in ((0, N_USERS), (0, -1), (1, N_ITEMS), (1, -5), (0, 2 ** 31 - 1)):
        mu, mi = bu.copy(), bi.copy()
        (mu, mi)[arr][7] = val
        assert status_of(ptr, mu, mi, P, N_USERS, N_ITEMS) & 4
        with pytest.raises(ValueError, match="id out of range"):
            blocks(bu_=mu, bi_=mi)
    # blk_ptr not monotone / leaving [0, n] / not starting at 0
    for k, val in ((a + 1, int(ptr[a]) - 1 if ptr[a] else int(ptr[a + 2]) + 1), (4, -1), (4, n + 1), (4, 2 ** 62), (0, 1)):
        bad = ptr.copy(); bad[k] = val
        assert status_of(bad, bu, bi, P, N_USERS, N_ITEMS) & 1
        with pytest.raises(ValueError, match="not monotone"):
            blocks(ptr_=bad)
    # blk_ptr not ending at n
    bad = ptr.copy(); bad[-1] = n - 1
    assert status_of(bad, bu, bi, P, N_USERS, N_ITEMS) & 2
    with pytest.raises(ValueError, match="does not end at n"):
        blocks(ptr_=bad)
    # a block not ascending in u
    users = bu[ptr[a]:ptr[a + 1]]
    assert users[0] != users[-1]
    mu, mi = bu.copy(), bi.copy()
    mu[ptr[a]:ptr[a + 1]], mi[ptr[a]:ptr[a + 1]] = users[::-1], bi[ptr[a]:ptr[a + 1]][::-1]
    assert status_of(ptr, mu, mi, P, N_USERS, N_ITEMS) == 16
    with pytest.raises(ValueError, match="not ascending in u"):
        blocks(bu_=mu, bi_=mi)
    # shapes and types are refused on the host; epoch takes nothing but a checked Blocks
    with pytest.raises(ValueError, match="blk_ptr entries"):
        svd.Blocks((_dev(ptr[:-1], np.int64), _dev(bu, np.int32), _dev(bi, np.int32), _dev(br, np.float64)), N_USERS, N_ITEMS, P)
    with pytest.raises(ValueError, match="int64 blk_ptr"):
        svd.Blocks((_dev(ptr, np.int32), _dev(bu, np.int32), _dev(bi, np.int32), _dev(br, np.float64)), N_USERS, N_ITEMS, P)
    t = torch.zeros((N_USERS, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError, match="checked"):
        svd.epoch((ptr, bu, bi, br), 0.0, False, [0.0] * 8, None, None, t, t)
    with pytest.raises(ValueError, match="qi"):
        svd.epoch(ok, 0.0, False, [0.0] * 8, None, None, t, t)


def test_argument_errors_launch_nothing():
    import torch
    L = _L(); lib = L.load()
    u, i, r = ratings()
    run = CFit(u, i, r, N_USERS, N_ITEMS, S.params(n_factors=8, random_state=1), 2)
    before = [t.clone() for t in run.model]
    st = L.stream_ptr(before[0].device)
    ptrs = [L.ptr(t) for t in run.model]

    def call(**kw):
        head = list(run.head)
        names = ["blk_ptr", "blk_u", "blk_i", "blk_r", "P", "n_users", "n_items", "n", "nf"]
        for k, v in kw.items():
            head[names.index(k)] = v
        return lib.n2v_svd_epoch(*head, *ptrs, st)

    for kw, word in (({"nf": 0}, "n_factors 0"), ({"nf": 257}, "n_factors 257"), ({"P": 0}, "n_strata=0"),
                     ({"P": 32769}, "n_strata=32769"), ({"n": 0}, "n=0"), ({"n_users": 0}, "n_users=0"),
                     ({"n_items": 2 ** 31}, "n_items="), ({"blk_r": None}, "null")):
        assert call(**kw) != 0
        assert word in lib.n2v_last_error().decode() and "svd_epoch:" in lib.n2v_last_error().decode()
    assert lib.n2v_svd_estimate(*ptrs, N_USERS, N_ITEMS, 8, 0.0, 1, None, None, 1, None, None, st) != 0
    assert "svd_estimate: null" in lib.n2v_last_error().decode()
    assert lib.n2v_svd_estimate(*ptrs, N_USERS, N_ITEMS, 300, 0.0, 1, ptrs[0], ptrs[0], 1, ptrs[0], ptrs[0], st) != 0
    assert lib.n2v_svd_blocks_check(None, None, None, 2, N_USERS, N_ITEMS, 5, None, st) != 0
    assert "svd_blocks_check: null" in lib.n2v_last_error().decode()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, run.model))


# ---- 5: the driver -----------------------------------------------------------------------------------------------------

def test_main_rec_algo_mf_prints_the_restatements_rmse(tmp_path, capsys):
    import main_rec
    rs = np.random.RandomState(31)
    cells = rs.permutation(25 * 20)[:200]
    lines = ["userId,movieId,rating,timestamp"] + ["%d,%d,%.1f,%d" % (c // 20 + 1, c % 20 + 100, rs.randint(1, 11) * 0.5, n)
                                                    for n, c in enumerate(cells)]
    p = tmp_path / "ratings.csv"
    p.write_text("\n".join(lines) + "\n")
    err = main_rec.main(["-input", str(p), "-algo", "mf", "-factors", "8", "-epochs", "3", "-strata", "4"])
    assert capsys.readouterr().out.strip() == "RMSE: %r" % err
    users, items, ratings_ = main_rec.read_ratings(str(p))
    train, test = main_rec.split(200, 0.2, 0)
    x, xraw = E.inner_ids([users[k] for k in train]); y, yraw = E.inner_ids([items[k] for k in train])
    r = ratings_[train]
    model = S.fit(x, y, r, len(xraw), len(yraw), S.params(n_factors=8, n_epochs=3, random_state=0), 4)
    qx = [xraw.index(users[k]) if users[k] in xraw else -1 for k in test]
    qy = [yraw.index(items[k]) if items[k] in yraw else -1 for k in test]
    est, imp = S.estimate(model, qx, qy, True)
    pred = E.predict_all(est, imp, E.global_mean(r), float(ratings_.min()), float(ratings_.max()))
    assert err == E.rmse(ratings_[test], pred)
    errs = main_rec.main(["-input", str(p), "-algo", "mf", "-factors", "8", "-epochs", "1", "-cv", "2", "-seed", "3", "-unbiased"])
    assert len(errs) == 2 and all(np.isfinite(errs))
