"""CPU tests of the matrix-factorisation path: the restatement tests/svd_reference.py against hand values and against
itself (the schedule, the dot order, the literal loops), the host side of n2v_hip.svd (options, the auto rule, no CPU
fallback), the -algo mf flags of main_rec.py and the new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

import eccknn_reference as E
import svd_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGHT = dict(lr_bu=0.011, lr_bi=0.007, lr_pu=0.013, lr_qi=0.005, reg_bu=0.03, reg_bi=0.05, reg_pu=0.02, reg_qi=0.07)


def same(a, b):
    return all(E.canon(x) == E.canon(y) for x, y in zip(a, b))


# ---- the update --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fit", [S.fit, S.fit_literal])
@pytest.mark.parametrize("n_strata", [None, 1, 3])
def test_one_rating_by_hand(fit, n_strata):
    """pu = qi = (0.5, 0.5), r = mu = 4: dot = 0.5 and err = -0.5; every constant is a power of two, so the arithmetic
    below is exact."""
    par = S.params(n_factors=2, n_epochs=1, init_mean=0.5, init_std_dev=0, lr_bu=0.125, reg_bu=0.5, lr_bi=0.25,
                   reg_bi=0.125, lr_pu=0.5, reg_pu=0.25, lr_qi=0.25, reg_qi=0.5)
    mu, bu, bi, pu, qi = fit([0], [0], [4.0], 1, 1, par, n_strata)
    assert mu == 4.0
    assert bu.tolist() == [0.125 * -0.5] and bi.tolist() == [0.25 * -0.5]
    assert pu.tolist() == [[0.5 + 0.5 * (-0.5 * 0.5 - 0.25 * 0.5)] * 2] == [[0.3125, 0.3125]]
    # qi from the OLD pu (0.5): 0.375; from the new one (0.3125) it would be 0.3984375
    assert qi.tolist() == [[0.5 + 0.25 * (-0.5 * 0.5 - 0.5 * 0.5)] * 2] == [[0.375, 0.375]]
    assert 0.5 + 0.25 * (-0.5 * 0.3125 - 0.5 * 0.5) == 0.3984375
    # not biased: err = r - dot = 3.5, the biases stay zero
    mu, bu, bi, pu, qi = fit([0], [0], [4.0], 1, 1, dict(par, biased=False), n_strata)
    assert mu == 0.0 and bu.tolist() == [0.0] and bi.tolist() == [0.0]
    assert pu.tolist() == [[0.5 + 0.5 * (3.5 * 0.5 - 0.25 * 0.5)] * 2] and qi.tolist() == [[0.5 + 0.25 * (3.5 * 0.5 - 0.5 * 0.5)] * 2]


def test_params_fill_the_eight_rates():
    p = S.params(lr_all=0.25, reg_all=0.5, lr_qi=0.125, reg_bu=2)
    assert [p[k] for k in S.RATES] == [0.25, 0.25, 0.25, 0.125, 2.0, 0.5, 0.5, 0.5]
    assert (p["n_factors"], p["n_epochs"], p["biased"], p["init_std_dev"]) == (100, 20, True, 0.1)
    with pytest.raises(ValueError):
        S.params(bogus=1)


# ---- the schedule ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_users,n_items,n,P", [(40, 30, 400, 1), (40, 30, 400, 2), (40, 30, 400, 7), (41, 29, 500, 3),
                                                 (5, 9, 30, 64), (40, 30, 1, 4), (1, 1, 1, 5)])
def test_schedule_properties(n_users, n_items, n, P):
    u, i, r = S.make_ratings(7 * P + n, n_users, n_items, n)
    o = S.all_ratings_order(u)
    assert (np.diff(u[o]) >= 0).all() and all((np.diff(o[u[o] == k]) > 0).all() for k in range(n_users))
    su, si = u[o], i[o]
    order, ptr = S.block_order(su, si, n_users, n_items, P)
    assert sorted(order.tolist()) == list(range(n))              # every rating exactly once an epoch
    assert ptr[0] == 0 and ptr[-1] == n and len(ptr) == P * P + 1 and (np.diff(ptr) >= 0).all()
    s, ub = S.block_keys(su, si, n_users, n_items, P)
    assert ((0 <= s) & (s < P) & (0 <= ub) & (ub < P)).all()
    for st in range(P):
        users, items = set(), set()
        for b in range(P):
            part = order[ptr[st * P + b]:ptr[st * P + b + 1]]
            assert (s[part] == st).all() and (ub[part] == b).all()
            assert (np.diff(part) > 0).all()                     # all_ratings() order inside the block
            bu_, bi_ = set(su[part].tolist()), set(si[part].tolist())
            assert not (users & bu_) and not (items & bi_)       # no two blocks of a stratum share a row
            users |= bu_; items |= bi_
    if P == 1:
        assert order.tolist() == list(range(n))
    if P > n_users:
        assert (np.diff(ptr) == 0).sum() >= P * P - n
    seq = S.sequence(u, i, r, n_users, n_items, P)
    assert np.array_equal(seq[0], su[order]) and np.array_equal(seq[1], si[order]) and np.array_equal(seq[2], r[o][order])
    none = S.sequence(u, i, r, n_users, n_items, None)
    assert np.array_equal(none[0], su) and np.array_equal(none[2], r[o])


# ---- the dot -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf", [1, 63, 64, 65, 100, 256])
def test_lane_dot_leaves_all_lanes_equal(nf):
    rs = np.random.RandomState(nf)
    differs = 0
    for trial in range(20):
        q, p = rs.normal(size=nf) * 10.0 ** rs.randint(-3, 4), rs.normal(size=nf)
        v = S.lane_dot(q, p)
        assert v.shape == (64,) and len(set(v.view(np.uint64).tolist())) == 1
        assert S.dot_lanes(q, p).tobytes() == v[0].tobytes() == np.float64(S._dot_lanes_literal(q.tolist(), p.tolist())).tobytes()
        asc = S.dot_ascending(q, p)
        assert asc == S._dot_ascending_literal(q.tolist(), p.tolist())
        assert abs(asc - v[0]) <= 4 * nf * np.finfo(np.float64).eps * np.abs(q * p).sum()
        differs += asc != v[0]
    assert (differs > 0) == (nf > 2)                              # the order matters, so it is pinned


def test_lane_dot_hand_values():
    # lanes 0 and 32 meet first: (1 + 2^-53) rounds to 1, then + 2^-53 again rounds to 1; ascending order keeps neither
    q = np.zeros(64); p = np.ones(64)
    q[0], q[32], q[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert S.lane_dot(q, p)[0] == 1.0 == S.dot_lanes(q, p)
    q[0], q[32], q[1] = 2.0 ** -53, 2.0 ** -53, 1.0                # (2^-53 + 2^-53) + 1 = 1 + 2^-52
    assert S.lane_dot(q, p)[5] == 1.0 + 2.0 ** -52 and S.dot_ascending(q, p) == 1.0
    assert S.lane_dot([-0.0], [1.0])[0] == 0.0 and not np.signbit(S.lane_dot([-0.0], [1.0])).any()


# ---- the two forms -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_strata", [None, 1, 2, 5])
@pytest.mark.parametrize("nf,biased", [(3, True), (70, True), (5, False)])
def test_literal_loops_equal_the_row_form(nf, biased, n_strata):
    u, i, r = S.make_ratings(nf, 9, 7, 40)
    par = S.params(n_factors=nf, n_epochs=2, biased=biased, random_state=3, **EIGHT)
    lit = S.fit_literal(u, i, r, 9, 7, par, n_strata)
    fast = S.fit(u, i, r, 9, 7, par, n_strata)
    assert lit[0] == fast[0] and same(lit[1:], fast[1:])
    assert not np.array_equal(fast[3], S.init(9, 7, par)[2])
    if biased:
        assert fast[0] == E.global_mean(r) and (fast[1] != 0).any() and (fast[2] != 0).any()
    else:
        assert fast[0] == 0.0 and not fast[1].any() and not fast[2].any()


def test_one_stratum_is_the_sequential_order_with_another_dot():
    u, i, r = S.make_ratings(1, 12, 10, 60)
    one = S.fit(u, i, r, 12, 10, S.params(n_factors=2, n_epochs=2), 1)
    none = S.fit(u, i, r, 12, 10, S.params(n_factors=2, n_epochs=2), None)
    assert same(one[1:], none[1:])                               # two factors: one addition, no order to differ in
    one = S.fit(u, i, r, 12, 10, S.params(n_factors=70, n_epochs=2), 1)
    none = S.fit(u, i, r, 12, 10, S.params(n_factors=70, n_epochs=2), None)
    assert not same(one[1:], none[1:]) and np.allclose(one[3], none[3], rtol=0, atol=1e-12)
    three = S.fit(u, i, r, 12, 10, S.params(n_factors=2, n_epochs=2), 3)
    assert not same(three[1:], none[1:])                         # another permutation of the ratings


def test_estimate_restated():
    model = (3.0, np.array([0.5, -0.25]), np.array([1.0]), np.array([[1.0, 2.0], [0.5, 0.5]]), np.array([[0.25, 4.0]]))
    est, imp = S.estimate(model, [0, 1, -1, 0, -1, 2], [0, 0, 0, -1, -1, 1], True)
    assert est.tolist() == [3.0 + 0.5 + 1.0 + 8.25, 3.0 - 0.25 + 1.0 + 2.125, 4.0, 3.5, 3.0, 3.0] and not imp.any()
    est, imp = S.estimate(model, [0, 1, -1, 0, -1], [0, 0, 0, -1, -1], False)
    assert est.tolist() == [8.25, 2.125, 0.0, 0.0, 0.0] and imp.tolist() == [0, 0, 1, 1, 1]


# ---- the schedule does not change what is learnt -----------------------------------------------------------------------

def test_stratified_order_learns_what_the_sequential_order_learns():
    """Restatement against restatement: 120 x 90 at rank 4, 3 200 training and 800 test ratings, n_factors 10, 20 epochs,
    seeds 0-3 (one set of ratings, the seed draws the factors).  The mean test RMSE of P = 4 and of P = 16 must lie within
    the sequential order's own seed-to-seed standard deviation of its mean.
    Observed: RMSE(None) mean 0.59366, std 0.00127; P = 4 mean 0.59351 (0.00015 away), P = 16 mean 0.59380 (0.00014
    away); predicting the training mean gives 0.92025."""
    n_users, n_items = 120, 90
    u, i, r = S.make_ratings(2024, n_users, n_items, 4000)
    tr, te = slice(0, 3200), slice(3200, 4000)
    seeds = (0, 1, 2, 3)

    def rmse(model):
        known_u, known_i = set(u[tr].tolist()), set(i[tr].tolist())
        qu = [int(a) if int(a) in known_u else -1 for a in u[te]]
        qi = [int(b) if int(b) in known_i else -1 for b in i[te]]
        est, imp = S.estimate(model, qu, qi, True)
        return E.rmse(r[te], E.predict_all(est, imp, model[0], 1.0, 5.0))

    out = {}
    for P in (None, 4, 16):
        out[P] = [rmse(S.fit(u[tr], i[tr], r[tr], n_users, n_items, S.params(n_factors=10, n_epochs=20, random_state=sd), P))
                  for sd in seeds]
    mean, std = np.mean(out[None]), np.std(out[None])
    print("RMSE(None) mean %.5f std %.5f; P=4 mean %.5f; P=16 mean %.5f" % (mean, std, np.mean(out[4]), np.mean(out[16])))
    flat = E.rmse(r[te], np.full(800, E.global_mean(r[tr])))
    print("RMSE of the training mean %.5f" % flat)
    assert 0.0 < std and mean < flat                             # it learns: better than predicting the training mean
    for P in (4, 16):
        assert abs(np.mean(out[P]) - mean) <= std, (P, out[P], out[None])


# ---- n2v_hip.svd, host side --------------------------------------------------------------------------------------------

def test_auto_rule():
    from n2v_hip import svd
    assert svd.auto_strata(6040, 3706, 800000) == 256            # MovieLens-1M: 316^2 * 8 <= 8e5, the power of two below
    assert svd.auto_strata(40, 30, 400) == 4                     # 4 * 4 * 8 <= 400 < 8 * 8 * 8
    assert svd.auto_strata(40, 30, 7) == 1 and svd.auto_strata(1, 1, 1) == 1
    assert svd.auto_strata(3, 1000, 10 ** 6) == 3 and svd.auto_strata(1000, 5, 10 ** 6) == 5     # never above a side
    assert svd.auto_strata(10 ** 6, 5 * 10 ** 6, 3 * 10 ** 7) == svd.AUTO_MAX_STRATA == 256
    for n in (1, 31, 32, 127, 128, 511, 512, 10 ** 9):
        P = svd.auto_strata(10 ** 7, 10 ** 7, n)
        assert P & (P - 1) == 0 and (P == 1 or P * P * 8 <= n) and (P == 256 or 4 * P * P * 8 > n)
    with pytest.raises(ValueError):
        svd.auto_strata(0, 5, 5)
    assert isinstance(svd.auto_strata(np.int64(40), np.int64(30), np.int64(400)), int)


def test_option_errors_come_before_any_gpu_call():
    from n2v_hip import svd
    a = svd.SVD()
    assert (a.n_factors, a.n_epochs, a.biased, a.init_mean, a.init_std_dev, a.random_state, a.n_strata) == \
        (100, 20, True, 0.0, 0.1, 0, "auto")
    assert a.rates == [0.005] * 4 + [0.02] * 4
    a = svd.SVD(lr_all=0.25, reg_all=0.5, lr_qi=0.125, reg_bu=2, n_strata=7, n_factors=256, n_epochs=0)
    assert a.rates == [0.25, 0.25, 0.25, 0.125, 2.0, 0.5, 0.5, 0.5] and a.n_strata == 7 and a.reg_bu == 2.0
    for kw, word in (({"n_factors": 0}, "n_factors 0 outside"), ({"n_factors": 257}, "n_factors 257 outside"),
                     ({"n_epochs": -1}, "n_epochs -1"), ({"lr_all": float("nan")}, "lr_bu"),
                     ({"reg_all": float("inf")}, "reg_bu"), ({"lr_pu": float("inf")}, "lr_pu"),
                     ({"reg_qi": float("nan")}, "reg_qi"), ({"lr_bi": float("-inf")}, "lr_bi"),
                     ({"n_strata": 0}, "n_strata 0"), ({"n_strata": -3}, "n_strata -3"), ({"n_strata": "many"}, "n_strata"),
                     ({"n_strata": 2.5}, "n_strata"), ({"n_strata": 32769}, "n_strata 32769")):
        with pytest.raises(ValueError, match=word):
            svd.SVD(**kw)
    assert svd.MAX_FACTORS == 256 and svd.PredictionImpossible is __import__("n2v_hip.eccknn").eccknn.PredictionImpossible


def test_no_cpu_fallback():
    import torch
    from n2v_hip import eccknn, svd
    if torch.cuda.is_available():
        return                                                   # tests/test_gpu_svd.py runs the device path
    ts = eccknn.Trainset.from_ratings([1, 2, 1], [5, 5, 6], [1.0, 2.0, 3.0])
    with pytest.raises(RuntimeError) as e:
        svd.SVD(n_factors=2, n_epochs=1).fit(ts)
    with pytest.raises(RuntimeError) as want:
        eccknn._require_gpu()
    assert str(e.value) == str(want.value) and "no CPU fallback" in str(e.value)
    t = torch.zeros(3, dtype=torch.int64)
    for call in (lambda: svd.build_blocks(t, t, t.double(), 1, 1, 1), lambda: svd.Blocks((t, t, t, t), 1, 1, 1),
                 lambda: svd.epoch(None, 0.0, True, [0.0] * 8, t, t, t, t),
                 lambda: svd.estimate_batch(0.0, True, t, t, t, t, t, t)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the driver --------------------------------------------------------------------------------------------------------

def test_main_rec_mf_flags():
    import main_rec
    a = main_rec.parse_args("-input r.csv -algo mf".split())
    assert (a.algo, a.factors, a.epochs, a.lr, a.reg, a.strata, a.unbiased, a.seed) == ("mf", 100, 20, 0.005, 0.02, "auto", False, 0)
    a = main_rec.parse_args("-input r.csv -algo mf -factors 8 -epochs 3 -lr 0.01 -reg 0.1 -strata 4 -unbiased -seed 5 -cv 3".split())
    assert (a.factors, a.epochs, a.lr, a.reg, a.strata, a.unbiased, a.seed, a.cv) == (8, 3, 0.01, 0.1, 4, True, 5, 3)
    assert main_rec.parse_args("-input r.csv -algo mf -strata auto -test-ratio 0.3".split()).strata == "auto"
    for flag in ("-sim msd", "-k 10", "-mink 2", "-weights w.csv", "-mode ir", "-item-based", "-form sparse", "-sim cosine",
                 "-k 40", "-form auto"):
        with pytest.raises(SystemExit):
            main_rec.parse_args(("-input r.csv -algo mf " + flag).split())
    for bad in ("-algo svd", "-algo svd -factors 8", "-algo mf -factors 0", "-algo mf -factors 257", "-algo mf -epochs -1",
                "-algo mf -strata 0", "-algo mf -strata many", "-algo mf -lr nan", "-algo knn -factors 8", "-epochs 3",
                "-algo knn -strata 4", "-unbiased", "-algo bogus"):
        with pytest.raises(SystemExit):
            main_rec.parse_args(("-input r.csv " + bad).split())
    # the other two algorithms keep their defaults
    a = main_rec.parse_args("-input r.csv".split())
    assert (a.algo, a.k, a.mink, a.sim, a.form, a.item_based) == ("eccen", 40, 1, "cosine", "auto", False)


def test_algo_svd_points_to_mf(capsys):
    import main_rec
    with pytest.raises(SystemExit):
        main_rec.parse_args("-input r.csv -algo svd".split())
    msg = capsys.readouterr().err
    assert "-algo mf" in msg and "-strata 1" in msg and "not built" in msg


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_bound():
    from n2v_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    for macro, v in (("N2V_SVD_BAD_PTR", 1), ("N2V_SVD_BAD_END", 2), ("N2V_SVD_BAD_ID", 4), ("N2V_SVD_WRONG_BLOCK", 8),
                     ("N2V_SVD_UNSORTED", 16)):
        assert re.search(r"#define %s %d\b" % (macro, v), hdr)
    section = hdr[hdr.index("Matrix factorisation"):hdr.index("int32_t n2v_svd_max_factors")]
    assert "UNPINNED" in section
    assert re.search(r"#define N2V_ABI_VERSION 5\b", open(os.path.join(ROOT, "include", "n2v_hip.h")).read())
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(n2v_[a-z0-9_]+)\s*\(", hdr))
    new = {"n2v_svd_max_factors", "n2v_svd_max_strata", "n2v_svd_blocks_check", "n2v_svd_epoch", "n2v_svd_estimate"}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    # (that each binding has the header's parameters, type by type: tests/test_host_logic.py)
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in new)
    from n2v_hip import svd
    assert lib.n2v_svd_max_factors() == 256 == svd.MAX_FACTORS and lib.n2v_svd_max_strata() == svd.MAX_STRATA
    assert [b for b, _ in svd.BLOCKS_BAD] == [1, 2, 4, 8, 16]
    for doc in (svd.__doc__, S.__doc__):
        assert "UNPINNED" in doc
