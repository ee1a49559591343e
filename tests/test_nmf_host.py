"""CPU tests of the NMF path: the restatement tests/nmf_reference.py against a literal transcription of surprise's loop
and against deliberate errors, its properties, the host side of n2v_hip.nmf (options, no CPU fallback), the -algo nmf
flags of main_rec.py and the new C-ABI symbols."""
import functools
import os
import re

import numpy as np
import pytest

import eccknn_reference as E
import nmf_reference as N
import svd_reference as SV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    """Bit for bit, host against host: the very bytes, NaNs included."""
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() and np.asarray(x).shape == np.asarray(y).shape for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def case():
    """14 users x 11 items, 70 ratings in a shuffled training order, inner ids by first appearance (as Trainset numbers
    them); three planted lines in front: A rates Y, B rates X, A rates X, so ir[X] = [B, A] while all_ratings() has A
    first."""
    u, i, r = N.make_ratings(3, 13, 10, 67)
    users = ["A", "B", "A"] + ["u%d" % k for k in u]
    items = ["Y", "X", "X"] + ["i%d" % k for k in i]
    r = np.concatenate(([4.0, 2.0, 5.0], r))
    (x, xraw), (y, yraw) = E.inner_ids(users), E.inner_ids(items)
    return np.array(x, np.int64), np.array(y, np.int64), r, len(xraw), len(yraw)


# ---- the restatement against the literal loop --------------------------------------------------------------------------

def test_the_case_has_an_item_whose_ir_order_is_not_ascending():
    u, i, r, n_users, n_items = case()
    ptr, us, _ = N.item_lists_ir(u, i, r, n_items)
    aptr, aus, _ = N.item_lists(u, i, r, n_items)
    assert np.array_equal(ptr, aptr)
    assert us[ptr[1]:ptr[2]][:2].tolist() == [1, 0] and aus[aptr[1]:aptr[2]][:2].tolist() == [0, 1]      # item X = inner 1
    assert all((np.diff(aus[aptr[k]:aptr[k + 1]]) > 0).all() for k in range(n_items))
    assert sum(not (np.diff(us[ptr[k]:ptr[k + 1]]) > 0).all() for k in range(n_items)) >= 3
    from n2v_hip import eccknn
    ts = eccknn.Trainset.from_ratings(u.tolist(), i.tolist(), r)
    assert all(np.array_equal(a, b) for a, b in zip(ts.ir, N.item_lists_ir(u, i, r, n_items)))
    assert all(np.array_equal(a, b) for a, b in zip(ts.ur, N.user_lists(u, i, r, n_users)))


@pytest.mark.parametrize("nf", [1, 4, 65])
def test_row_form_equals_the_literal_loop(nf):
    u, i, r, n_users, n_items = case()
    par = N.params(n_factors=nf, random_state=nf)
    pu, qi = N.init(n_users, n_items, par)
    for n_epochs in (1, 2):
        pu, qi = N.epoch_literal(u, i, r, n_users, n_items, pu, qi, par)
        assert same((pu, qi), N.fit(u, i, r, n_users, n_items, par, n_epochs)), n_epochs
    assert not np.array_equal(pu, N.init(n_users, n_items, par)[0]) and np.isfinite(pu).all() and np.isfinite(qi).all()


def test_literal_loop_on_non_finite_tables():
    u, i, r, n_users, n_items = case()
    par = N.params(n_factors=3, random_state=1)
    pu, qi = N.init(n_users, n_items, par)
    pu[2] = 0.0; qi[1, 1] = np.inf
    lit = N.epoch_literal(u, i, r, n_users, n_items, pu, qi, par)
    assert same(lit, N.fit(u, i, r, n_users, n_items, par, 1, tables=(pu, qi)))
    assert np.isnan(lit[0][2]).all() and np.isnan(lit[1]).any() and np.isfinite(lit[0]).any()


# ---- deliberate errors are caught by the case --------------------------------------------------------------------------

def test_deliberate_errors_change_bits():
    u, i, r, n_users, n_items = case()
    par = N.params(n_factors=4, random_state=2)
    pu, qi = N.init(n_users, n_items, par)
    ul, il = N.user_lists(u, i, r, n_users), N.item_lists(u, i, r, n_items)
    want = N.epoch(ul, il, pu, qi, par)
    # item lists taken in ir order
    got = N.epoch(ul, N.item_lists_ir(u, i, r, n_items), pu, qi, par)
    assert same(got[:1], want[:1]) and not same(got[1:], want[1:])
    # the item pass reading the already-updated pu
    assert not same([N.half_pass(il, qi, want[0], par["reg_qi"])], want[1:])
    # reg * n * p in another association: n * (reg * p)

    def half_pass_assoc(lst, own, oth, reg):
        ptr, ids, rr = lst
        out = np.empty_like(own)
        for k in range(len(ptr) - 1):
            p = own[k]
            num, den = np.zeros(own.shape[1]), np.zeros(own.shape[1])
            for e in range(ptr[k], ptr[k + 1]):
                q = oth[ids[e]]
                est = SV.dot_lanes(q, p)
                num = num + q * rr[e]
                den = den + q * est
            den = den + int(ptr[k + 1] - ptr[k]) * (reg * p)
            out[k] = p * (num / den)
        return out

    assoc = half_pass_assoc(ul, pu, qi, par["reg_pu"]), half_pass_assoc(il, qi, pu, par["reg_qi"])
    assert not same(assoc, want) and all(np.allclose(a, w, rtol=1e-14, atol=0) for a, w in zip(assoc, want))
    # a pairwise np.dot in place of the lane dot at F = 65
    par = N.params(n_factors=65, random_state=2)
    pu, qi = N.init(n_users, n_items, par)
    want = N.epoch(ul, il, pu, qi, par)
    got = N.epoch(ul, il, pu, qi, par, dot_fn=np.dot)
    assert not same(got[:1], want[:1]) and not same(got[1:], want[1:]) and np.allclose(got[0], want[0], rtol=1e-12, atol=0)


# ---- properties --------------------------------------------------------------------------------------------------------

def test_non_negative_in_non_negative_out_and_all_zero_gives_nan():
    u, i, r, n_users, n_items = case()
    pu, qi = N.fit(u, i, r, n_users, n_items, N.params(n_factors=5, n_epochs=4, random_state=7))
    assert (pu >= 0).all() and (qi >= 0).all() and (pu > 0).any()
    pu, qi = N.fit(u, i, r, n_users, n_items, N.params(n_factors=5, n_epochs=1, init_low=0, init_high=0))
    assert np.isnan(pu).all() and np.isnan(qi).all()


def test_it_learns_better_than_the_training_mean():
    """60 x 40 with 666 ratings of a rank-3 non-negative model plus noise, rounded to 1 .. 5; F = 4, reg = 0.06.
    Observed: clipped training RMSE 1.93 at 0 epochs, 0.92 at 20, 0.44 at 50; the training mean scores 0.89."""
    u, i, r = N.make_ratings(11, 60, 40, 666)
    par = N.params(n_factors=4, random_state=0)

    def rmse(tables):
        est, imp = N.estimate(tables[0], tables[1], u.tolist(), i.tolist())
        assert not imp.any()
        return E.rmse(r, E.predict_all(est, imp, E.global_mean(r), 1.0, 5.0))

    ul, il = N.user_lists(u, i, r, 60), N.item_lists(u, i, r, 40)
    tables = N.init(60, 40, par)
    at = {0: rmse(tables)}
    for ep in range(1, 51):
        tables = N.epoch(ul, il, tables[0], tables[1], par)
        if ep in (20, 50):
            at[ep] = rmse(tables)
    flat = E.rmse(r, np.full(len(r), E.global_mean(r)))
    print("clipped training RMSE %r; the training mean %.4f" % (at, flat))
    assert (tables[0] > 0).all() and (tables[1] > 0).all()       # strictly positive, no NaN
    assert at[50] < at[20] < at[0] and at[50] < flat


# ---- n2v_hip.nmf, host side --------------------------------------------------------------------------------------------

def test_option_errors_come_before_any_gpu_call():
    from n2v_hip import nmf, svd
    a = nmf.NMF()
    assert (a.n_factors, a.n_epochs, a.biased, a.reg_pu, a.reg_qi, a.init_low, a.init_high, a.random_state, a.device) == \
        (15, 50, False, 0.06, 0.06, 0.0, 1.0, 0, "cuda:0")
    assert a.mu == 0.0 and isinstance(a, svd.SVD)
    a = nmf.NMF(n_factors=256, n_epochs=0, reg_pu=0.5, reg_qi=0, init_low=2, init_high=2)
    assert (a.n_factors, a.n_epochs, a.reg_pu, a.reg_qi, a.init_low, a.init_high) == (256, 0, 0.5, 0.0, 2.0, 2.0)
    for kw, word in (({"n_factors": 0}, "n_factors 0 outside"), ({"n_factors": 257}, "n_factors 257 outside"),
                     ({"n_epochs": -1}, "n_epochs -1"), ({"reg_pu": float("nan")}, "reg_pu"), ({"reg_qi": float("inf")}, "reg_qi"),
                     ({"init_low": 1, "init_high": 0.5}, "init_low"), ({"init_high": float("inf")}, "init_high"),
                     ({"init_low": float("nan")}, "init_low"), ({"biased": True}, "biased=True is not built")):
        with pytest.raises(ValueError, match=word):
            nmf.NMF(**kw)
    with pytest.raises(ValueError, match="biased"):
        N.params(biased=True)
    assert N.DEFAULTS == dict(n_factors=15, n_epochs=50, biased=False, reg_pu=0.06, reg_qi=0.06, init_low=0, init_high=1,
                              random_state=0)


def test_no_cpu_fallback():
    import torch
    from n2v_hip import eccknn, nmf
    if torch.cuda.is_available():
        return                                                   # tests/test_gpu_nmf.py runs the device path
    ts = eccknn.Trainset.from_ratings([1, 2, 1], [5, 5, 6], [1.0, 2.0, 3.0])
    with pytest.raises(RuntimeError) as e:
        nmf.NMF(n_factors=2, n_epochs=1).fit(ts)
    with pytest.raises(RuntimeError) as want:
        eccknn._require_gpu()
    assert str(e.value) == str(want.value) and "no CPU fallback" in str(e.value)
    t = torch.zeros(3, dtype=torch.int64)
    for call in (lambda: nmf.lists((t, t.int(), t.double()), 2, 2), lambda: nmf.item_major((t, t.int(), t.double()), 2),
                 lambda: nmf.epoch(None, 0.06, 0.06, t, t, t, t)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the driver --------------------------------------------------------------------------------------------------------

def test_main_rec_nmf_flags():
    import main_rec
    a = main_rec.parse_args("-input r.csv -algo nmf".split())
    assert (a.algo, a.factors, a.epochs, a.reg, a.seed, a.cv, a.topn, a.test_ratio) == ("nmf", 15, 50, 0.06, 0, 0, None, 0.2)
    a = main_rec.parse_args("-input r.csv -algo nmf -factors 8 -epochs 3 -reg 0.1 -seed 5 -cv 3 -topn 5 -threshold 4 -save-recs o.csv".split())
    assert (a.factors, a.epochs, a.reg, a.seed, a.cv, a.topn, a.threshold, a.save_recs) == (8, 3, 0.1, 5, 3, 5, 4.0, "o.csv")
    assert main_rec.parse_args("-input r.csv -algo nmf -test-ratio 0.3 -epochs 0".split()).epochs == 0
    for flag in ("-lr 0.01", "-strata 4", "-strata auto", "-unbiased", "-sim msd", "-k 10", "-mink 2", "-weights w.csv", "-mode ir",
                 "-item-based", "-form sparse", "-sim cosine", "-k 40", "-form auto"):
        with pytest.raises(SystemExit):
            main_rec.parse_args(("-input r.csv -algo nmf " + flag).split())
    for bad in ("-algo nmf -factors 0", "-algo nmf -factors 257", "-algo nmf -epochs -1", "-algo nmf -reg nan",
                "-algo nmf -threshold 3", "-algo nmf -cv 1"):
        with pytest.raises(SystemExit):
            main_rec.parse_args(("-input r.csv " + bad).split())


@pytest.mark.parametrize("flag", ["-lr 0.01", "-strata 4", "-unbiased", "-k 10", "-sim msd", "-item-based"])
def test_refused_flags_use_the_existing_wording(flag, capsys):
    import main_rec
    with pytest.raises(SystemExit):
        main_rec.parse_args(("-input r.csv -algo nmf " + flag).split())
    assert "%s does not go with -algo nmf" % flag.split()[0] in capsys.readouterr().err


def test_the_old_refusals_are_unchanged(capsys):
    import main_rec
    with pytest.raises(SystemExit):
        main_rec.parse_args("-input r.csv -algo svd".split())
    msg = capsys.readouterr().err
    assert "not built" in msg and "-algo mf" in msg and "-strata 1" in msg
    with pytest.raises(SystemExit):
        main_rec.parse_args("-input r.csv -algo bogus".split())
    msg = capsys.readouterr().err
    assert "-algo bogus" in msg and "nmf" in msg
    for bad, word in (("-algo knn -factors 8", "-factors does not go with -algo knn"), ("-epochs 3", "-epochs does not go with -algo eccen"),
                      ("-algo mf -k 10", "-k does not go with -algo mf")):
        with pytest.raises(SystemExit):
            main_rec.parse_args(("-input r.csv " + bad).split())
        assert word in capsys.readouterr().err
    a = main_rec.parse_args("-input r.csv -algo mf".split())      # mf keeps its own defaults
    assert (a.factors, a.epochs, a.lr, a.reg, a.strata) == (100, 20, 0.005, 0.02, "auto")
    a = main_rec.parse_args("-input r.csv".split())
    assert (a.algo, a.k, a.mink, a.sim, a.form) == ("eccen", 40, 1, "cosine", "auto")


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_bound():
    from n2v_hip import _lib, nmf
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    for macro, v in (("N2V_NMF_BAD_PTR", 1), ("N2V_NMF_BAD_END", 2), ("N2V_NMF_BAD_ID", 4), ("N2V_NMF_UNSORTED", 8),
                     ("N2V_NMF_BAD_COUNT", 16)):
        assert re.search(r"#define %s %d\b" % (macro, v), hdr)
    section = hdr[hdr.index("Non-negative matrix factorisation"):hdr.index("int32_t n2v_nmf_depth")]
    assert "UNPINNED" in section
    assert re.search(r"#define N2V_ABI_VERSION 5\b", open(os.path.join(ROOT, "include", "n2v_hip.h")).read())
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    new = {"n2v_nmf_depth": 0, "n2v_nmf_lists_check": 10, "n2v_nmf_epoch": 19}
    for name, count in new.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).strip()
        assert (0 if params == "void" else params.count(",") + 1) == count == len(_lib.SIGNATURES[name][1]), name
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in new)
    assert lib.n2v_abi_version() == 5
    assert 1 <= lib.n2v_nmf_depth() <= 64 and 64 % lib.n2v_nmf_depth() == 0
    assert [b for b, _ in nmf.LISTS_BAD] == [1, 2, 4, 8, 16]
    for doc in (nmf.__doc__, N.__doc__):
        assert "UNPINNED" in doc
