"""CPU tests of the CoClustering predictor: the restatement tests/coclustering_reference.py against a literal transcription
of surprise's loops (equal on half-star ratings, different on arbitrary doubles: the summation deviation is real and is
exact where the sums are), a table worked out by hand, the argmin rule, proof that the case tables of the GPU test are not
vacuous, the constructor, the -algo coclustering flags of main_rec.py, the "no CPU fallback" errors and the five new C-ABI
symbols.  No GPU."""
import os
import re

import numpy as np
import pytest

import coclustering_reference as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bytes(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


# ---- the restatement and surprise's own loops ----------------------------------------------------------------------------

@pytest.mark.parametrize("shape,clusters,n_epochs", [((70, 50, 600), (3, 3), 20), ((70, 50, 600), (8, 5), 20),
                                                     ((70, 50, 600), (17, 2), 20), ((70, 50, 600), (64, 64), 4),
                                                     ((130, 67, 1500), (3, 3), 20), ((130, 67, 1500), (17, 2), 6)])
def test_grouped_sums_equal_the_literal_loops_on_half_star_ratings(shape, clusters, n_epochs):
    u, i, r = C.make_ratings(0, *shape, "half")
    par = C.params(n_cltr_u=clusters[0], n_cltr_i=clusters[1], n_epochs=n_epochs)
    ta, tb = [], []
    a = C.fit(u, i, r, shape[0], shape[1], par, trace=ta)
    b = C.fit_literal(u, i, r, shape[0], shape[1], par, trace=tb)
    assert len(ta) == len(tb) == n_epochs
    for k, (x, y) in enumerate(zip(ta, tb)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), k
    for name in ("avg_cltr_u", "avg_cltr_i", "avg_cocltr"):
        assert same_bytes(a[name], b[name]), name
    assert np.array_equal(a["count_cocltr"], b["count_cocltr"])


def test_the_deviation_is_real_on_arbitrary_doubles():
    u, i, r = C.make_ratings(0, 70, 50, 600, "fp64")
    par = C.params(n_epochs=2)
    a, b = C.fit(u, i, r, 70, 50, par), C.fit_literal(u, i, r, 70, 50, par)
    assert not all(same_bytes(a[name], b[name]) for name in ("avg_cltr_u", "avg_cltr_i", "avg_cocltr"))
    for name in ("avg_cltr_u", "avg_cltr_i", "avg_cocltr"):       # in last bits only
        assert np.allclose(a[name], b[name], rtol=1e-13, atol=0.0), name
    ul = C.lists(u, i, r, 70)
    cu, ci = C.init(70, 50, par)
    g, l = C.sums(ul, cu, ci, 3, 3), C.sums_literal(ul, cu, ci, 3, 3)
    assert all(np.array_equal(x, y) for x, y in zip(g[:3], l[:3]))           # the counts are the same integers
    assert not all(same_bytes(x, y) for x, y in zip(g[3:], l[3:]))


# ---- by hand ---------------------------------------------------------------------------------------------------------------

def test_table_by_hand():
    """edge_case("tie"): users 0 and 1 rated items 0 .. 3 with 4, 4, 2, 1; user 2 rated items 2, 3 with 5, 3.  Users in
    clusters 0, 1, 2; items in clusters 0, 1, 2, 2.  Training mean 30 / 10."""
    u, i, r, n_u, n_i, cu, ci, n_cu, n_ci = C.edge_case("tie")
    ul, il = C.lists(u, i, r, n_u), C.lists(i, u, r, n_i)
    mean, um, im = C.global_mean(r), C.mean_rows(ul), C.mean_rows(il)
    assert mean == 3.0 and um.tolist() == [2.75, 2.75, 4.0] and im.tolist() == [4.0, 4.0, 3.0, 5.0 / 3.0]
    au, ai, acc, cc = C.averages(ul, cu, ci, n_cu, n_ci, mean)
    assert au.tolist() == [11.0 / 4.0, 11.0 / 4.0, 8.0 / 2.0]
    assert ai.tolist() == [8.0 / 2.0, 8.0 / 2.0, 14.0 / 6.0]
    assert acc.tolist() == [[4.0, 4.0, 1.5], [4.0, 4.0, 1.5], [3.0, 3.0, 4.0]]          # two empty co-clusters: the mean
    assert cc.tolist() == [[1, 1, 2], [1, 1, 2], [0, 0, 2]]
    keep = []
    new_u = C.assign_users(ul, ci, n_cu, (au, ai, acc), um, im, keep)
    # user 0, candidate 2, its four entries in list order
    e = 0.0
    for item, rating in ((0, 4.0), (1, 4.0), (2, 2.0), (3, 1.0)):
        est = (((acc[2][ci[item]] + 2.75) - 4.0) + im[item]) - ai[ci[item]]
        d = rating - est
        e = e + d * d
    assert keep[0][2] == e
    assert keep[0][0] == keep[0][1] and keep[1][0] == keep[1][1]             # equal averages: a tie, and the first wins
    assert new_u.tolist()[:2] == [0, 0] and cu.tolist()[:2] == [0, 1]
    keep = []
    new_i = C.assign_items(il, new_u, n_ci, (au, ai, acc), um, im, keep)
    assert all(k[0] == k[1] for k in keep) and new_i.tolist() == [C.argmin(k) for k in keep]
    m = dict(cltr_u=cu, cltr_i=ci, avg_cltr_u=au, avg_cltr_i=ai, avg_cocltr=acc, user_mean=um, item_mean=im, mean=mean,
             n_users=n_u, n_items=n_i)
    assert C.estimate(m, 2, 0) == (((3.0 + 4.0) - 4.0) + 4.0) - 4.0           # user 2 never rated item 0: an empty co-cluster
    assert C.estimate(m, 2, -1) == 4.0 and C.estimate(m, 3, 1) == 4.0 and C.estimate(m, -1, 4) == 3.0
    est, imp = C.estimate_all(m, [2, 2, 3, -1], [0, -1, 1, 4])
    assert est.tolist() == [3.0, 4.0, 4.0, 3.0] and not imp.any()


def test_argmin_rule():
    nan, inf = float("nan"), float("inf")
    for errors, want in (([3.0, 1.0, 1.0, 2.0], 1), ([0.0, 0.0], 0), ([inf, inf, inf], 0), ([2.0, nan, 1.0, nan], 1),
                         ([nan], 0), ([1.0, 0.0, -0.0], 1), ([5.0], 0), ([inf, 1e308], 1)):
        assert C.argmin(np.array(errors)) == want == int(np.argmin(np.array(errors))), errors


# ---- the GPU test's case tables are not vacuous ----------------------------------------------------------------------------

def test_case_tables_reach_their_edges():
    changed = empty_uc = empty_cc = False
    for n_u, n_i, n, n_cu, n_ci, n_epochs, kind in C.FITS:
        assert n_u <= 130 and n_i <= 67 and n <= 1500
        u, i, r = C.make_ratings(0, n_u, n_i, n, kind)
        assert len(set(u.tolist())) == n_u and len(set(i.tolist())) == n_i
        trace = []
        m = C.fit(u, i, r, n_u, n_i, C.params(n_cltr_u=n_cu, n_cltr_i=n_ci, n_epochs=n_epochs), trace=trace)
        first = C.init(n_u, n_i, C.params(n_cltr_u=n_cu, n_cltr_i=n_ci))
        changed |= any(not np.array_equal(a[0], b[0]) or not np.array_equal(a[1], b[1]) for a, b in zip([first] + trace, trace))
        if (n_u, n_i, n, n_cu, n_ci) == (70, 50, 600, 17, 2):
            for cu, ci in [first] + trace:
                empty_uc |= bool((np.bincount(cu, minlength=n_cu) == 0).any())
                cc = C.averages(m["ul"], cu, ci, n_cu, n_ci, m["mean"])[3]
                empty_cc |= bool((cc == 0).any())
    assert changed and empty_uc and empty_cc
    assert {(f[3], f[4]) for f in C.FITS} == {(1, 1), (2, 3), (3, 3), (17, 2), (63, 64), (64, 64)}
    # the planted lists
    u, i, r, n_u, n_i, cu, ci = C.list_case()
    assert tuple(np.bincount(u, minlength=n_u)[:7]) == C.LIST_LENS == (0, 1, 63, 64, 65, 129, 5000)
    assert len(set(i.tolist())) == n_i == 5000
    # the arithmetic edges
    seen = {}
    for kind in ("tie", "inf", "huge"):
        u, i, r, n_u, n_i, cu, ci, n_cu, n_ci = C.edge_case(kind)
        ul, il = C.lists(u, i, r, n_u), C.lists(i, u, r, n_i)
        mean, um, im = C.global_mean(r), C.mean_rows(ul), C.mean_rows(il)
        avgs = C.averages(ul, cu, ci, n_cu, n_ci, mean)
        keep = []
        new_u = C.assign_users(ul, ci, n_cu, avgs, um, im, keep)
        C.assign_items(il, new_u, n_ci, avgs, um, im, keep)
        seen[kind] = keep
    assert any(k[0] == k[1] and k[0] <= k.min() for k in seen["tie"])
    assert any(np.isnan(k).any() and not np.isnan(k[0]) for k in seen["inf"])            # a NaN that is not the first entry wins
    assert any(np.isnan(k).all() for k in seen["inf"])
    assert any(np.isinf(k).all() and len(k) > 1 for k in seen["huge"])                   # all +inf: a tie, the first index


# ---- the class and the flags ---------------------------------------------------------------------------------------------

def test_constructor_and_limits():
    from n2v_hip import coclustering, eccknn
    assert issubclass(coclustering.CoClustering, eccknn.Predictor) and coclustering.MAX_CLUSTERS == C.MAX_CLUSTERS == 64
    a = coclustering.CoClustering()
    assert (a.n_cltr_u, a.n_cltr_i, a.n_epochs, a.random_state) == (3, 3, 20, 0) == tuple(C.DEFAULTS[k] for k in
                                                                                         ("n_cltr_u", "n_cltr_i", "n_epochs", "random_state"))
    assert coclustering.CoClustering(n_cltr_u=64, n_cltr_i=1, n_epochs=0).n_cltr_u == 64
    for kw in (dict(n_cltr_u=0), dict(n_cltr_u=65), dict(n_cltr_i=0), dict(n_cltr_i=65), dict(n_cltr_i=-3)):
        with pytest.raises(ValueError, match=r"outside \[1, 64\]"):
            coclustering.CoClustering(**kw)
    with pytest.raises(ValueError, match="n_epochs"):
        coclustering.CoClustering(n_epochs=-1)
    for text in ("surprise", "UNPINNED", "tests/coclustering_reference.py", "no CPU fallback", "grouped by user row"):
        assert text in coclustering.__doc__
    assert "UNPINNED" in C.__doc__ and "DEVIATION" in C.__doc__


def test_no_cpu_fallback(monkeypatch):
    import torch
    from n2v_hip import coclustering, eccknn
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ts = eccknn.Trainset.from_ratings([0, 0, 1], [0, 1, 1], [3.0, 4.0, 5.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coclustering.CoClustering().fit(ts)
    ur, ir = (tuple(torch.as_tensor(a) for a in lst) for lst in (ts.ur, ts.ir))
    cu, ci = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    f = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    avgs = (f(1), f(1), f(1, 1))
    q = torch.zeros(1, dtype=torch.int32)
    for call in (lambda: coclustering.averages(ur, 2, cu, ci, 1, 1, 4.0),
                 lambda: coclustering.assign(ur, True, cu, ci, avgs, f(2), f(2)),
                 lambda: coclustering.epoch(ur, ir, cu, ci, 1, 1, 4.0, f(2), f(2)),
                 lambda: coclustering.estimate_batch(cu, ci, avgs, f(2), f(2), 4.0, q, q),
                 lambda: coclustering.top_n(cu, ci, avgs, f(2), f(2), None, 4.0, (1, 5), 10)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="outside"):              # the option checks still come first
        coclustering.top_n(cu, ci, avgs, f(2), f(2), None, 4.0, (1, 5), 257)


def test_main_rec_flags(capsys):
    import main_rec
    a = main_rec.parse_args("-input r.csv -algo coclustering".split())
    assert (a.algo, a.clusters_u, a.clusters_i, a.epochs, a.topn, a.cv, a.test_ratio, a.seed) == ("coclustering", 3, 3, 20, None, 0, 0.2, 0)
    a = main_rec.parse_args("-input r.csv -algo coclustering -clusters-u 17 -clusters-i 2 -epochs 5 -topn 10 -threshold 4 "
                            "-save-recs o.csv -cv 3 -test-ratio 0.3 -seed 7".split())
    assert (a.clusters_u, a.clusters_i, a.epochs, a.topn, a.threshold, a.save_recs, a.cv, a.test_ratio, a.seed) == \
        (17, 2, 5, 10, 4.0, "o.csv", 3, 0.3, 7)
    for flag in ("-k 20", "-mink 2", "-sim msd", "-shrinkage 50", "-weights w.csv", "-mode ir", "-item-based", "-form sparse",
                 "-factors 8", "-lr 0.1", "-reg 0.1", "-strata 2", "-unbiased"):
        with pytest.raises(SystemExit):
            main_rec.parse_args(("-input r.csv -algo coclustering %s" % flag).split())
        assert "%s does not go with -algo coclustering" % flag.split()[0] in capsys.readouterr().err, flag
    for flag in ("-clusters-u 0", "-clusters-i 65", "-epochs -1"):
        with pytest.raises(SystemExit):
            main_rec.parse_args(("-input r.csv -algo coclustering %s" % flag).split())
        assert "outside [1, 64]" in capsys.readouterr().err or flag.startswith("-epochs"), flag
    for algo in ("eccen", "knn", "knnbaseline", "mf", "nmf", "slopeone"):    # the cluster flags belong to coclustering alone
        with pytest.raises(SystemExit):
            main_rec.parse_args(("-input r.csv -algo %s -clusters-u 4" % algo).split())
        assert "-clusters-u does not go with -algo %s" % algo in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main_rec.parse_args("-input r.csv -algo bogus".split())
    err = capsys.readouterr().err
    assert "-algo bogus" in err and "coclustering" in err and "slopeone" in err and "-algo coclustering" in main_rec.__doc__
    # the other algorithms keep their defaults
    assert main_rec.parse_args("-input r.csv -algo nmf".split()).epochs == 50
    assert main_rec.parse_args("-input r.csv -algo mf".split()).epochs == 20


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------

NEW = {"n2v_cocl_max_clusters": 0, "n2v_cocl_averages": 17, "n2v_cocl_assign": 18, "n2v_cocl_estimate": 18, "n2v_cocl_topn": 26}


def test_symbols_are_declared_bound_and_exported():
    from n2v_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    section = hdr[hdr.index("Co-clustering: surprise's"):hdr.index("int32_t n2v_cocl_max_clusters(")]
    for text in ("UNPINNED", "tests/coclustering_reference.py", "DEVIATION", "argmin"):
        assert text in section, text
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(n2v_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SIGNATURES)
    for name, count in NEW.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1)
        assert len(_lib.SIGNATURES[name][1]) == (0 if params.strip() == "void" else params.count(",") + 1) == count, name
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW) and lib.n2v_cocl_max_clusters() == 64
    assert "n2v_cocl.hip" in open(os.path.join(ROOT, "node2vec-by-ecc_amd", "csrc", "Makefile")).read()


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Every call below returns before the first HIP call: no GPU is needed (and none is touched)."""
    from n2v_hip import _lib
    lib = _lib.load()
    one = 1 << 20   # a non-NULL "pointer" that is never dereferenced: each call fails its argument checks first

    def avg(n_users=5, n_items=7, n=4, n_cu=3, n_ci=3, ptr=one, part=one, count=one):
        return lib.n2v_cocl_averages(ptr, one, one, n_users, n_items, n, one, one, n_cu, n_ci, 3.0, part, one, one, one, count, None)

    def assign(n_users=5, n_items=7, n=4, n_cu=3, n_ci=3, ptr=one, cltr_u=one, cltr_i=one + 4096, side=1):
        return lib.n2v_cocl_assign(ptr, one, one, None, n_users, n_items, n, side, n_cu, n_ci, one, one, one, one, one, cltr_u,
                                   cltr_i, None)

    def est(n_users=5, n_items=7, n_cu=3, n_ci=3, n_q=3, table=one, out=one):
        return lib.n2v_cocl_estimate(one, one, one, one, table, one, one, n_users, n_items, n_cu, n_ci, 3.0, one, one, n_q, out, one,
                                     None)

    def top(n_users=5, n_items=7, n_cu=3, n_ci=3, n_owners=3, top_n=10, segments=0, table=one, items=one):
        return lib.n2v_cocl_topn(one, one, one, one, table, one, one, n_users, n_items, n_cu, n_ci, one, one, 4, one, n_owners, 3.0,
                                 1.0, 5.0, top_n, segments, one, one, items, one, None)

    for call, kw, msg in ((avg, dict(n_users=0), "n_users=0"), (avg, dict(n_items=1 << 31), "n_items"), (avg, dict(n=-1), "n=-1"),
                          (avg, dict(n_cu=0), "outside [1, 64]"), (avg, dict(n_ci=65), "outside [1, 64]"), (avg, dict(ptr=None), "null"),
                          (avg, dict(part=None), "null"), (avg, dict(count=None), "null"),
                          (assign, dict(n_items=0), "n_items=0"), (assign, dict(n_cu=65), "outside [1, 64]"),
                          (assign, dict(n_ci=0), "outside [1, 64]"), (assign, dict(ptr=None), "null"), (assign, dict(cltr_u=None), "null"),
                          (assign, dict(cltr_i=one), "overlap"), (assign, dict(cltr_i=one + 4 * 4), "overlap"),
                          (assign, dict(cltr_u=one + 4 * 6, cltr_i=one), "overlap"), (assign, dict(cltr_i=one, side=0), "overlap"),
                          (est, dict(n_q=0), "n_q"), (est, dict(n_users=0), "n_users=0"), (est, dict(n_cu=65), "outside [1, 64]"),
                          (est, dict(table=None), "null"), (est, dict(out=None), "null"),
                          (top, dict(n_items=0), "n_items=0"), (top, dict(n_ci=0), "outside [1, 64]"), (top, dict(n_owners=0), "n_owners"),
                          (top, dict(top_n=257), "top_n"), (top, dict(segments=65), "segments"), (top, dict(table=None), "null"),
                          (top, dict(items=None), "null")):
        assert call(**kw) != 0, (call.__name__, kw)
        assert msg in lib.n2v_last_error().decode(), (call.__name__, kw, lib.n2v_last_error())
