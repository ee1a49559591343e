"""GPU tests: the eccentricity-statistics kernels (csrc/n2v_eccstats.hip, C-ABI include/n2v_sim.h) against the
restatement tests/eccstats_reference.py, through the C-ABI unless a test says otherwise.

Exact comparisons only: fp64 arrays by their bytes (R.canon: a NaN's sign and payload are not part of the contract,
everything else is), integers with array_equal.  The reference side is the numpy form, which tests/test_eccstats_host.py
holds to the literal loops bit for bit and to output recorded from the reference within a measured bound.  Every output
buffer starts as a sentinel.  The sorts are torch calls (n2v_hip.eccstats.prepare), as in the module.

`ir == 0`: with the reference's z(x) = x - (mean / std) an item's ir is zero only if its mean of -log(count) equals
mean / std of all of them, a transcendental number against an algebraic one, so no data set reaches it other than by a
chance rounding.  The inf -> 0 rule is therefore driven where it lives, at n2v_eccstats_finish, with ir holding +0.0 and
-0.0 (test_quotient_inf_rule), and inside the chain by a case whose ie is infinite over a finite ir."""
import math
import os

import numpy as np
import pytest

import eccstats_reference as R

pytestmark = pytest.mark.gpu

SENT = -12345.5
ISENT = -7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eccstats")
CHAIN = ("irg", "irz", "irmean", "ws", "fs", "ue", "wi", "fi", "ir", "ie", "ire", "ier", "uer", "ier_", "q")


def _L():
    from n2v_hip import _lib as L
    return L


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _full(n, value, dtype):
    import torch
    return torch.full((n,), value, dtype=dtype, device="cuda")


def c_moments(x):
    import torch
    L = _L(); lib = L.load()
    scratch = _full(int(lib.n2v_eccstats_moments_scratch(x.numel())), SENT, torch.float64)
    stats = _full(8, SENT, torch.float64)
    L.check(lib.n2v_eccstats_moments(L.ptr(x), x.numel(), L.ptr(scratch), L.ptr(stats), L.stream_ptr(x.device)))
    return stats


def c_finish(op, a, b=None, stats=None):
    import torch
    L = _L(); lib = L.load()
    out = _full(a.numel(), SENT, torch.float64)
    L.check(lib.n2v_eccstats_finish(op, L.ptr(a), L.ptr(b), L.ptr(stats), a.numel(), L.ptr(out), L.stream_ptr(a.device)))
    return out


def c_segsum(seg_ptr, a, perm=None, idx=None, g=None, mean=False):
    import torch
    L = _L(); lib = L.load()
    n_seg = seg_ptr.numel() - 1
    scratch = _full(n_seg + 1, ISENT, torch.int32)
    out, wout = _full(n_seg, SENT, torch.float64), (_full(n_seg, SENT, torch.float64) if g is not None else None)
    L.check(lib.n2v_eccstats_segsum(L.ptr(seg_ptr), n_seg, L.ptr(perm), L.ptr(a), a.numel(), L.ptr(idx), L.ptr(g),
                                    g.numel() if g is not None else 0, int(mean), L.ptr(scratch), L.ptr(out), L.ptr(wout),
                                    L.stream_ptr(a.device)))
    return out, wout


def c_statistics(u, i, fb, tw, n_users, n_items):
    """The whole chain through the C-ABI on inner ids; numpy arrays keyed as the restatement's."""
    import torch
    from n2v_hip import eccstats as S
    L = _L(); lib = L.load()
    du, di, dfb = _dev(u, np.int64), _dev(i, np.int64), _dev(fb, np.float64)
    key_sorted, perm_g, n_tw, perm_u, perm_i = S.prepare(du, di, _dev(tw, np.int64), n_items)
    n = len(fb)
    st = L.stream_ptr(dfb.device)
    scratch = _full(int(lib.n2v_eccstats_groups_scratch(n)), ISENT, torch.int64)
    row_group, group_begin = _full(n, ISENT, torch.int32), _full(n + 1, ISENT, torch.int64)
    unum, item_gptr, counts = _full(n, ISENT, torch.int64), _full(n_items + 1, ISENT, torch.int64), _full(2, ISENT, torch.int64)
    L.check(lib.n2v_eccstats_groups(L.ptr(key_sorted), L.ptr(perm_g), n, n_tw, n_items, L.ptr(scratch), L.ptr(row_group),
                                    L.ptr(group_begin), L.ptr(unum), L.ptr(item_gptr), L.ptr(counts), st))
    n_groups, largest = counts.tolist()
    assert (unum[n_groups:] == ISENT).all() and (group_begin[n_groups + 1:] == ISENT).all()      # nothing past the end
    unum = unum[:n_groups].contiguous()
    table = S.log_table(largest + 1).cuda()
    irg, status = _full(n_groups, SENT, torch.float64), torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(lib.n2v_eccstats_irg(L.ptr(unum), n_groups, L.ptr(table), table.numel(), L.ptr(irg), L.ptr(status), st))
    z = lambda x: c_finish(S.Z, x, stats=c_moments(x))
    zo = lambda x: c_finish(S.ZERO_ONE, x, stats=c_moments(x))
    irmean, _ = c_segsum(item_gptr, irg, mean=True)
    ir, irz = z(irmean), z(irg)
    fs, ws = c_segsum(S._csr_ptr(du, n_users), dfb, perm=perm_u, idx=row_group, g=irz)
    uer = c_finish(S.DIV, ws, fs)
    ue = z(uer)
    fi, wi = c_segsum(S._csr_ptr(di, n_items), dfb, perm=perm_i, idx=du.to(torch.int32), g=ue)
    ier_ = c_finish(S.DIV, wi, fi)
    ie = z(ier_)
    ire = zo(c_finish(S.MUL, ie, ir))
    q = c_finish(S.DIV_INF0, ie, ir)
    ier = zo(q)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    loc = locals()
    out = {k: loc[k].cpu().numpy() for k in CHAIN + ("unum", "row_group", "item_gptr")}
    out["group_begin"], out["largest"] = group_begin[:n_groups + 1].cpu().numpy(), largest
    return out


def check(u, i, fb, tw):
    """Runs both sides on raw ids u, i; returns (restatement, device)."""
    want = R.statistics_numpy(u, i, fb, tw)
    iu, _ = R.first_appearance(u)
    ii, _ = R.first_appearance(i)
    got = c_statistics(iu, ii, fb, tw, len(want["users"]), len(want["items"]))
    assert got["unum"].dtype == np.int64 and np.array_equal(got["unum"], want["unum"])
    assert np.array_equal(got["row_group"], want["row_group"])
    assert np.array_equal(got["group_begin"], np.concatenate([[0], np.cumsum(want["unum"])]))
    assert np.array_equal(got["item_gptr"], np.searchsorted(want["group_item"], np.arange(len(want["items"]) + 1)))
    assert got["largest"] == want["unum"].max()
    assert R.canon(got["irg"]) == R.canon(np.array([-math.log(int(c)) for c in want["unum"]]))   # the host's math.log
    for k in CHAIN:
        assert got[k].shape == want[k].shape and R.canon(got[k]) == R.canon(want[k]), \
            (k, np.nonzero(got[k] != want[k])[0][:8])
    return want, got


# ---- the committed fixtures ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["syn400", "syn20000", "syn3000", "dup1500", "tw2500"])
def test_fixtures_bit_for_bit(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    want, _ = check([str(v) for v in d["uid"]], [str(v) for v in d["id"]], d["feedback"], d["timewindow"])
    assert np.isfinite(want["ier"]).all()
    counts = np.bincount(want["unum"])
    assert (counts > 1).any()                                   # a count that repeats: the table is hit more than once


# ---- segment lengths ----------------------------------------------------------------------------------------------------

SEG_LENS = [1, 2, 63, 64, 65, 127, 129, 64 * 78 + 1]


def test_segment_lengths_across_both_bins():
    """One item and one user of every length in SEG_LENS (lane path below 64, wavefront path from 64 on, the longest
    64 * 78 + 1 = 4993 rows: full chunks and a tail of one), feedback from a seeded uniform, and an item whose number of
    groups also passes 64 so the mean of irg takes the wavefront path too."""
    rs = np.random.RandomState(11)
    i = np.repeat(np.arange(len(SEG_LENS)), SEG_LENS)
    u = rs.permutation(i)
    fb = rs.uniform(0.1, 5.0, size=len(i))
    tw = 201001 + rs.randint(0, 3, size=len(i))
    tw[i == len(SEG_LENS) - 1] = 300000 + rs.randint(0, 150, size=SEG_LENS[-1])
    want, got = check(u, i, fb, tw)
    assert sorted(np.bincount(R.first_appearance(i)[0]).tolist()) == SEG_LENS
    assert sorted(np.bincount(R.first_appearance(u)[0]).tolist()) == SEG_LENS
    per_item = np.bincount(want["group_item"])
    assert per_item.max() >= 65 and per_item.min() == 1
    assert np.isfinite(want["ie"]).all() and np.isfinite(want["ue"]).all()
    assert (np.bincount(want["unum"]) > 1).any()


# ---- element counts of the chunked global sums -------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 4095, 4096, 4097, 8193])
def test_chunk_boundaries_of_the_global_sums(count):
    """`count` groups, items and users at once: one timewindow (a group is an item), 1 to 3 rows per item, every user at
    least one row."""
    rs = np.random.RandomState(count)
    i = rs.permutation(np.repeat(np.arange(count), 1 + np.arange(count) % 3))
    u = rs.permutation(np.arange(len(i)) % count)
    fb = rs.uniform(0.1, 5.0, size=len(i))
    want, _ = check(u, i, fb, np.full(len(i), 201001))
    assert len(want["unum"]) == len(want["items"]) == len(want["users"]) == count
    if count > 1:
        assert np.isfinite(want["ier"]).all() and len(np.unique(want["unum"])) == 3
    else:
        assert np.isnan(want["ie"]).all()


def test_single_user_zero_variance():
    """One user: std(uer) = 0, ue = -inf or +inf, ie NaN; equal to the restatement after canonicalisation."""
    want, got = check(*R.make_rows(7, 1, 9, 40))
    assert len(want["users"]) == 1 and np.isinf(want["ue"]).all() and np.isnan(want["ie"]).all() and np.isnan(got["ier"]).all()


def test_identical_item_profiles_infinite_ie_runs_the_inf_rule():
    """Every item is rated by the same three users with the same feedback in the same order, so wi / fi is one value:
    std = 0 and ie = x - (mean / 0) is infinite, while ir is finite and varies (the third user's window alternates, which
    changes the group counts).  q = ie / ir is then +-inf everywhere and must come out as 0.0 inside the chain."""
    u, i, fb, tw = [], [], [], []
    for j in range(6):
        u += [0, 1, 2]; i += [j] * 3; fb += [1.3, 2.7, 0.9]; tw += [1, 2, 1 if j % 2 == 0 else 3]
    want, got = check(np.array(u), np.array(i), np.array(fb), np.array(tw))
    assert np.isfinite(want["ue"]).all() and np.isfinite(want["ir"]).all() and (want["ir"] != 0).all()
    assert np.isinf(want["ie"]).all() and (got["q"] == 0.0).all() and not np.signbit(got["q"]).any()


# ---- the kernels on their own -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 8193, 64 * 4096 + 1])
def test_moments_order_and_min_max(n):
    rs = np.random.RandomState(n)
    x = rs.uniform(-3.0, 7.0, size=n) * 10.0 ** rs.randint(-3, 4, size=n)
    if n > 2:
        x[rs.randint(0, n)] = 0.0
        x[rs.randint(0, n)] = -0.0
    s = c_moments(_dev(x, np.float64)).cpu().numpy()
    m = np.float64(R.chunked_sum(x)) / np.float64(n)
    d = x - m
    ssd = np.float64(R.chunked_sum(d * d))
    lo, hi = R.min_max(x)
    want = np.array([R.chunked_sum(x), m, ssd, ssd / n, np.sqrt(ssd / n), lo, hi, n], dtype=np.float64)
    assert R.canon(s) == R.canon(want), (s, want)


def test_moments_zero_signs_and_nan():
    for x, lo, hi in (([0.0, -0.0], -0.0, 0.0), ([-0.0, -0.0], -0.0, -0.0), ([0.0, 0.0, 5.0], 0.0, 5.0),
                      ([-2.0, -0.0], -2.0, -0.0), ([-np.inf, np.inf, 1.0], -np.inf, np.inf)):
        s = c_moments(_dev(x, np.float64)).cpu().numpy()
        assert R.canon(s[5:7]) == R.canon(np.array([lo, hi])) == R.canon(np.array(R.min_max(np.array(x)))), x
    x = np.arange(5000, dtype=np.float64)
    x[4500] = np.nan
    s = c_moments(_dev(x, np.float64)).cpu().numpy()
    assert np.isnan(s[[0, 1, 2, 3, 4, 5, 6]]).all() and s[7] == 5000


def test_quotient_inf_rule():
    """ier's quotient with ir == +0.0 and -0.0: +-inf becomes +0.0, 0 / 0 stays NaN, everything else is the quotient."""
    from n2v_hip import eccstats as S
    ie = np.array([1.5, -1.5, 0.0, 2.0, -0.0, np.inf, 3.0, -7.25, 1e308, np.nan])
    ir = np.array([0.0, 0.0, 0.0, -0.0, -0.0, 2.0, 1.5, -0.5, 1e-308, 1.0])
    with np.errstate(all="ignore"):
        q = ie / ir
    want = np.where(np.isinf(q), 0.0, q)
    assert np.isinf(q).sum() == 5 and np.isnan(want).sum() == 3
    got = c_finish(S.DIV_INF0, _dev(ie, np.float64), _dev(ir, np.float64)).cpu().numpy()
    assert R.canon(got) == R.canon(want)
    plain = c_finish(S.DIV, _dev(ie, np.float64), _dev(ir, np.float64)).cpu().numpy()
    assert R.canon(plain) == R.canon(q)
    zo = c_finish(S.ZERO_ONE, _dev(want[[0, 1, 6, 7]], np.float64), stats=c_moments(_dev(want[[0, 1, 6, 7]], np.float64)))
    assert R.canon(zo.cpu().numpy()) == R.canon(R.zero_one(want[[0, 1, 6, 7]]))


def test_segsum_out_of_range_is_nan_not_a_fault():
    ptr = _dev([0, 2, 2, 5], np.int64)
    a = _dev([1.0, 2.0, 4.0, 8.0, 16.0], np.float64)
    g = _dev([10.0, 100.0], np.float64)
    idx = _dev([0, 1, 0, 7, -1], np.int32)
    perm = _dev([4, 3, 2, 9, 0], np.int64)
    s, w = c_segsum(ptr, a, perm=perm, idx=idx, g=g)
    s, w = s.cpu().numpy(), w.cpu().numpy()
    assert s[0] == 24.0 and s[1] == 0.0 and np.isnan(s[2]) and np.isnan(w[0]) and w[1] == 0.0 and np.isnan(w[2])
    s, w = c_segsum(ptr, a, idx=_dev([0, 1, 0, 1, 0], np.int32), g=g)
    assert s.cpu().numpy().tolist() == [3.0, 0.0, 28.0] and w.cpu().numpy().tolist() == [210.0, 0.0, 1000.0]
    L = _L(); lib = L.load()
    assert lib.n2v_eccstats_segsum(L.ptr(ptr), 0, None, L.ptr(a), 5, None, None, 0, 0, L.ptr(idx), L.ptr(s), None, None) != 0
    assert b"eccstats_segsum" in lib.n2v_last_error()


# ---- the module and main_rec ----------------------------------------------------------------------------------------------

def test_item_statistics_object():
    from n2v_hip import eccstats as S
    d = np.load(os.path.join(GOLDEN, "dup1500.npz"))
    uid, iid = [str(v) for v in d["uid"]], [str(v) for v in d["id"]]
    want = R.statistics_numpy(uid, iid, d["feedback"], d["timewindow"])
    st = S.item_statistics(uid, iid, d["feedback"], d["timewindow"], intermediates=True)
    assert st.items == want["items"] and st.users == want["users"]
    for k in S.MODES + ("ue",):
        assert R.canon(getattr(st, k)) == R.canon(want[k]), k
    for k in S.INTERMEDIATES:
        assert R.canon(st.intermediates[k]) == R.canon(want[k]), k
    w = st.weights("ire")
    assert list(w) == want["items"] and list(w.values()) == want["ire"].tolist()
    assert S.item_statistics(uid, iid, d["feedback"], d["timewindow"]).intermediates is None
    with pytest.raises(ValueError):
        st.weights("ue")


@pytest.fixture(scope="module")
def ratings_file(tmp_path_factory):
    """The rows of the syn400 fixture without repeated (uid, id) pairs (the k-NN trainset refuses them), as a csv."""
    d = np.load(os.path.join(GOLDEN, "syn400.npz"))
    seen, rows = set(), []
    for r in zip(d["uid"].tolist(), d["id"].tolist(), d["feedback"].tolist(), d["timestamp"].tolist()):
        if r[:2] not in seen:
            seen.add(r[:2])
            rows.append(r)
    path = tmp_path_factory.mktemp("eccstats") / "ratings.csv"
    path.write_text("".join("%d,%d,%r,%d\n" % r for r in rows))
    return str(path), rows


@pytest.mark.parametrize("mode", ["ir", "ie", "ire", "ier"])
def test_main_rec_mode_end_to_end(mode, ratings_file, tmp_path, capsys):
    import main_rec
    from n2v_hip import eccstats as S
    path, rows = ratings_file
    f = str(tmp_path / "w.csv")
    base = ["-input", path, "-k", "10", "-sim", "cosine"]
    err = main_rec.main(base + ["-mode", mode, "-save-weights", f])
    printed = capsys.readouterr().out
    st = S.item_statistics([str(r[0]) for r in rows], [str(r[1]) for r in rows], [r[2] for r in rows],
                           S.timewindow_utc([r[3] for r in rows]))
    want = st.weights(mode)
    saved = main_rec.read_weights(f)
    assert list(saved) == list(want) and R.canon(np.array(list(saved.values()))) == R.canon(np.array(list(want.values())))
    assert np.isfinite(list(want.values())).all()
    err2 = main_rec.main(base + ["-weights", f])
    assert capsys.readouterr().out == printed == "RMSE: %r\n" % err and err2 == err
    if mode == "ir":
        ones = main_rec.main(base)
        assert ones != err, "the weights are not used"
