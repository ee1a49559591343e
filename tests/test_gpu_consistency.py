"""GPU tests: the eccentricity-consistency kernels (csrc/n2v_ecccons.hip, C-ABI include/n2v_sim.h) and n2v_hip.consistency
against the restatement tests/consistency_reference.py and, end to end, against what the reference's septile_for_plot
returned (tests/golden/consistency/*.npz).

Everything is compared by equality, NaN positions included (every NaN canonical): integers with array_equal, fp64 by
bytes.  Output buffers handed to the C-ABI start as sentinels and what lies past the written part must still hold them."""
import os

import numpy as np
import pytest

import consistency_reference as R

pytestmark = pytest.mark.gpu

SENT = -12345.5
ISENT = -7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _L():
    from n2v_hip import _lib as L
    return L


def _C():
    from n2v_hip import consistency as C
    return C


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _full(n, value, dtype):
    import torch
    return torch.full((n,), value, dtype=dtype, device="cuda")


def tile():
    return int(_L().load().n2v_eccsplit_tile())


# ---- join ---------------------------------------------------------------------------------------------------------------

def c_join(v1, v2, c1, c2, min_count):
    import torch
    L = _L(); lib = L.load()
    n = len(v1)
    d = [_dev(v1, np.float64), _dev(v2, np.float64), _dev(c1, np.int64), _dev(c2, np.int64)]
    scratch = _full(int(lib.n2v_eccsplit_scratch(n)), ISENT, torch.int64)
    ids, count = _full(n + 2, ISENT, torch.int64), _full(1, ISENT, torch.int64)
    o1, o2 = _full(n + 2, SENT, torch.float64), _full(n + 2, SENT, torch.float64)
    L.check(lib.n2v_ecccons_join(L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), n, min_count, L.ptr(scratch), L.ptr(ids),
                                 L.ptr(o1), L.ptr(o2), L.ptr(count), L.stream_ptr(ids.device)))
    m = int(count.item())
    ids, o1, o2 = ids.cpu().numpy(), o1.cpu().numpy(), o2.cpu().numpy()
    assert 0 <= m <= n and (ids[m:] == ISENT).all() and (o1[m:] == SENT).all() and (o2[m:] == SENT).all()
    return ids[:m], o1[:m], o2[:m]


def test_join_cases():
    """m = 0, 1, n - 1, n, n + 1, 63 / 64 / 65, one tile - 1 / tile / tile + 1 and more than two tiles; disjoint periods;
    support exactly min_count and min_count + 1; values moved by their bytes."""
    cases = R.join_cases(tile())
    assert {"m0", "m1", "m6", "m7", "m8", "m63", "m64", "m65", "m%d" % (tile() - 1), "m%d" % tile(), "m%d" % (tile() + 1)} <= set(cases)
    for name, cs in cases.items():
        ids, o1, o2 = c_join(*cs)
        want = R.join(*cs)
        assert np.array_equal(ids, want[0]) and np.all(np.diff(ids) > 0), name
        assert o1.tobytes() == want[1].tobytes() and o2.tobytes() == want[2].tobytes(), name        # NaN payload and -0.0 kept
    assert len(c_join(*cases["disjoint"])[0]) == 0 and len(c_join(*cases["all"])[0]) == 300
    assert c_join(*cases["support_edge"])[0].tolist() == [1]
    assert c_join(*cases["special_values"])[0].tolist() == [0, 1, 2, 3, 4, 5]
    ids, _, _ = _C().join(*[_dev(a, t) for a, t in zip(cases["m65"][:4], (np.float64, np.float64, np.int64, np.int64))], 4)
    assert np.array_equal(ids.cpu().numpy(), R.join(*cases["m65"])[0])


# ---- crosstab -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 7, 10, 64, 65, 100, 256])
def test_crosstab_cases(n):
    """Every n that takes another path, one cell (maximum contention), a diagonal, an empty bins1 row, m over several
    workgroups, no element at all; two runs give identical bytes."""
    C = _C()
    cases = {k: v for k, v in R.crosstab_cases().items() if v[2] == n}
    assert len(cases) >= 3
    for name, (b1, b2, _) in cases.items():
        d1, d2 = _dev(b1, np.int32), _dev(b2, np.int32)
        runs = [[t.cpu().numpy() for t in C.crosstab(d1, d2, n)] for _ in range(2)]
        want = R.crosstab(b1, b2, n)
        for got, w in zip(runs[0], want):
            assert got.dtype == w.dtype and got.shape == w.shape and R.canon(got) == R.canon(w), name
        assert [a.tobytes() for a in runs[0]] == [a.tobytes() for a in runs[1]], name
        assert runs[0][0].sum() == len(b1)
    if n == 7:
        assert np.isnan(R.crosstab(*cases["emptyrow_n7"])[2][2]).all() and np.isnan(R.crosstab(*cases["empty_n7"])[2]).all()
        assert len(cases["random_n7"][0]) > 2 * 16384                                         # three workgroups


# ---- profile ------------------------------------------------------------------------------------------------------------

def c_profile(user, item, fb, item_bin, n_users, n_bins, weighted, bad=None):
    import torch
    from n2v_hip import eccstats
    du = _dev(user, np.int64)
    arg = dict(user_ptr=eccstats._csr_ptr(du, n_users), perm=torch.sort(du, stable=True)[1], item=_dev(item, np.int64),
               feedback=_dev(fb, np.float64), item_bin=_dev(item_bin, np.int32))
    for k, (pos, value) in (bad or {}).items():
        arg[k] = arg[k].clone()
        arg[k][pos] = value
    return _C().profile(arg["user_ptr"], arg["perm"], arg["item"], arg["feedback"], arg["item_bin"], n_bins, weighted).cpu().numpy()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_bins", [1, 100, 256])
def test_profile_cases(n_bins, weighted):
    """Users with 0 binned rows (NaN row), 1, 63 / 64 / 65 and 1000 rows; items of bin 0 skipped; the weighted sums in file
    order on feedback (1e16 next to 1.0) whose sum depends on it."""
    cs = R.profile_cases()["bins%d" % n_bins]
    got = c_profile(*cs, weighted)
    want = R.profile(*cs, weighted=weighted)
    assert got.shape == want.shape == (cs[4], n_bins) and R.canon(got) == R.canon(want)
    assert np.isnan(got[[0, 6, 7]]).all() and np.bincount(cs[0][cs[3][cs[1]] > 0], minlength=9).tolist()[:6] == [0, 1, 63, 64, 65, 1000]
    if weighted and n_bins > 1:
        assert R.canon(R.profile(cs[0][::-1], cs[1][::-1], cs[2][::-1], *cs[3:], weighted=True)) != R.canon(want)


# ---- features -----------------------------------------------------------------------------------------------------------

def _feature_case(n_bins, d, missing, seed=5):
    rs = np.random.RandomState(seed)
    n_users, n_items, n_rows = 13, 40, 700
    user, item = rs.randint(0, n_users, n_rows), rs.randint(0, n_items, n_rows)
    fb = rs.uniform(0.5, 5, n_rows)
    prof = rs.uniform(size=(n_users, n_bins))
    prof[3] = np.nan
    has = np.ones(n_items, dtype=bool)
    if missing == "first":
        has[item[0]] = False
    elif missing == "last":
        has[item[-1]] = False
    elif missing == "every":
        has[:] = False
    elif missing == "some":
        has[rs.randint(0, n_items, 15)] = False
    slot = np.where(has, np.cumsum(has) - 1, -1).astype(np.int32)
    vec = rs.normal(size=(max(int(has.sum()), 1), d)).astype(np.float32)
    return user, item, fb, prof, slot, vec


def _features_numpy(user, item, fb, prof, slot=None, vec=None, value=None):
    rows = np.arange(len(user)) if slot is None else np.nonzero(slot[item] >= 0)[0]
    tail = value[item[rows]][:, None] if slot is None else vec[slot[item[rows]]].astype(np.float64)
    return np.concatenate([prof[user[rows]], tail], axis=1), fb[rows], rows


@pytest.mark.parametrize("n_bins,d", [(100, 100), (100, 3), (7, 4), (6, 2), (256, 128)])
@pytest.mark.parametrize("missing", ["none", "first", "last", "every", "some"])
def test_features_with_vectors(n_bins, d, missing):
    """Row lengths 200 (16-byte path), 103 and 11 (odd), 8; rows dropped at the first, the last, every and some rows."""
    user, item, fb, prof, slot, vec = _feature_case(n_bins, d, missing)
    X, y, rows = _C().feature_rows(_dev(user, np.int64), _dev(item, np.int64), _dev(fb, np.float64), _dev(prof, np.float64),
                                   _dev(slot, np.int32), _dev(vec, np.float32))
    wX, wy, wrows = _features_numpy(user, item, fb, prof, slot, vec)
    assert np.array_equal(rows.cpu().numpy(), wrows) and y.cpu().numpy().tobytes() == wy.tobytes()
    assert tuple(X.shape) == (len(wrows), n_bins + d) and R.canon(X.cpu().numpy()) == R.canon(wX)
    assert (missing == "every") == (len(wrows) == 0) and (missing == "none") == (len(wrows) == len(user))


@pytest.mark.parametrize("n_bins", [100, 7, 1])
def test_features_without_vectors(n_bins):
    """Row length 101: profile ++ [the item's number]; every row kept."""
    user, item, fb, prof, _, _ = _feature_case(n_bins, 2, "none")
    value = np.arange(40, dtype=np.float64) * 3 + 1e9
    X, y, rows = _C().feature_rows(_dev(user, np.int64), _dev(item, np.int64), _dev(fb, np.float64), _dev(prof, np.float64),
                                   item_value=_dev(value, np.float64))
    wX, wy, wrows = _features_numpy(user, item, fb, prof, value=value)
    assert np.array_equal(rows.cpu().numpy(), wrows) and y.cpu().numpy().tobytes() == wy.tobytes()
    assert tuple(X.shape) == (len(user), n_bins + 1) and R.canon(X.cpu().numpy()) == R.canon(wX)


# ---- malformed inputs -----------------------------------------------------------------------------------------------------

def test_malformed_integer_inputs_are_value_errors():
    C = _C()
    ok = _dev([1, 2, 7, 3], np.int32)
    for bad in ([1, 0, 7, 3], [1, 8, 7, 3], [1, 2, 7, -5], [2 ** 31 - 1, 2, 7, 3], [-2 ** 31, 2, 7, 3]):
        with pytest.raises(ValueError):
            C.crosstab(_dev(bad, np.int32), ok, 7)
        with pytest.raises(ValueError):
            C.crosstab(ok, _dev(bad, np.int32), 7)
    for n in (0, 257, -1):
        with pytest.raises(ValueError):
            C.crosstab(ok, ok, n)
    cs = R.profile_cases()["bins100"]
    n_rows = len(cs[0])
    c_profile(*cs, False)                                                            # the case itself is fine
    for bad in (dict(user_ptr=(3, 10 ** 6)), dict(user_ptr=(0, 1)), dict(user_ptr=(-1, n_rows + 1)), dict(user_ptr=(4, -2)),
                dict(perm=(5, n_rows)), dict(perm=(0, -1)), dict(item=(7, 400)), dict(item=(n_rows - 1, -1)),
                dict(item_bin=(9, 101)), dict(item_bin=(0, -1))):
        with pytest.raises(ValueError):
            c_profile(*cs, False, bad=bad)
    user, item, fb, prof, slot, vec = _feature_case(6, 2, "some")
    dev = lambda u=user, i=item, s=slot: (_dev(u, np.int64), _dev(i, np.int64), _dev(fb, np.float64), _dev(prof, np.float64),
                                          _dev(s, np.int32), _dev(vec, np.float32))
    C.feature_rows(*dev())
    def changed(a, pos, value):
        b = a.copy()
        b[pos] = value
        return b
    for kw in (dict(u=changed(user, 0, 13)), dict(u=changed(user, 699, -1)), dict(i=changed(item, 5, 40)), dict(i=changed(item, 5, -3)),
               dict(s=changed(slot, 2, len(vec))), dict(s=changed(slot, 39, -2))):
        with pytest.raises(ValueError):
            C.feature_rows(*dev(**kw))


# ---- end to end -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.CASES)
def test_transitions_equal_the_restatement_and_the_recording(name):
    C = _C()
    c, want = R.case(GOLDEN, name), R.restated(GOLDEN, name)
    got = C.transitions(c.uid, c.iid, c.feedback, c.timewindow, c.first, c.second)
    for kind in R.KINDS:
        t = getattr(got, kind)
        assert R.same_table(t, want[kind])
        table, ratio = c.frame(kind)                                                 # what the reference returned
        f = got.frame(kind)
        assert np.array_equal(np.stack([f.bin1, f.bin2, f.count, f.count_sum], axis=1), table) and np.array_equal(f.ratio, ratio)
        assert {r: (int(a), int(b)) for r, a, b in zip(t.ids, t.bins1, t.bins2)} == {r: v[2:] for r, v in c.joined(kind).items()}


def test_transitions_other_n_support_and_empty_join():
    C = _C()
    c = R.case(GOLDEN, "dup3000")
    for n, min_count in ((10, 0), (3, 12), (7, 10 ** 6)):
        got = C.transitions(c.uid, c.iid, c.feedback, c.timewindow, c.first, c.second, n=n, min_count=min_count)
        want = R.transitions(c.uid, c.iid, c.feedback, c.timewindow, c.first, c.second, n=n, min_count=min_count)
        for kind in R.KINDS:
            assert R.same_table(getattr(got, kind), want[kind])
    assert got.ue.ids == [] and not got.ue.count.any() and np.isnan(got.ue.ratio).all() and len(got.frame("ue")) == 0


@pytest.mark.parametrize("name", ["ml3000", "dup3000", "seg3000"])
def test_profile_and_features_end_to_end(name):
    C = _C()
    c = R.case(GOLDEN, name)
    for n_bins, weighted in ((100, False), (7, True)):
        users, items, item_bin, want = R.user_ie_profile(c.uid, c.iid, c.feedback, c.timewindow, n_bins, weighted)
        got = C.user_ie_profile(c.uid, c.iid, c.feedback, c.timewindow, n_bins=n_bins, weighted=weighted)
        assert got.users == users and got.items == items and np.array_equal(got.item_bin, item_bin)
        assert got.profile.shape == (len(users), n_bins) and R.canon(got.profile) == R.canon(want)
    rs = np.random.RandomState(3)
    vectors = {r: rs.normal(size=16).astype(np.float32) for r in items[::2]}       # every other item has a vector
    for vec in (None, vectors):
        X, y, rows = C.features(got, c.uid, c.iid, c.feedback, item_vectors=vec)
        wX, wy, wrows = R.features(users, want, c.uid, c.iid, c.feedback, vec)
        assert np.array_equal(rows, wrows) and y.tobytes() == wy.tobytes() and X.shape == wX.shape and R.canon(X) == R.canon(wX)
    assert 0 < len(rows) < len(c.uid)


def test_cli_writes_the_reference_tables(tmp_path, capsys):
    import consistency as cli
    c = R.case(GOLDEN, "seg3000")
    path = tmp_path / "r.csv"
    path.write_text("uid,id,feedback,timewindow\n" + "".join("%s,%s,%r,%d\n" % r for r in zip(c.uid, c.iid, c.feedback.tolist(), c.timewindow.tolist())))
    out = tmp_path / "out"
    a = cli.parse_args(["-input", str(path), "-seg-point", str(c.seg_point), "-window-col", "timewindow", "-out", str(out),
                        "-profile", str(tmp_path / "p.npy"), "-bins", "10", "-features", str(tmp_path / "X.npy"), str(tmp_path / "Y.npy")])
    cli.main(a)
    text = capsys.readouterr().out
    assert all(("%s: " % k) in text for k in R.KINDS)
    for kind in R.KINDS:
        rows = [line.split(",") for line in (out / ("%s_septile.csv" % kind)).read_text().splitlines()[1:]]
        table, ratio = c.frame(kind)
        assert np.array_equal(np.array([[int(v) for v in r[:4]] for r in rows]), table)
        assert [float(r[4]) for r in rows] == ratio.tolist()
    users, _, _, want = R.user_ie_profile(c.uid, c.iid, c.feedback, c.timewindow, 10)
    assert R.canon(np.load(tmp_path / "p.npy")) == R.canon(want)
    assert (tmp_path / "p.npy.users.txt").read_text().split() == users
    wX, wy, _ = R.features(users, want, c.uid, c.iid, c.feedback)
    assert R.canon(np.load(tmp_path / "X.npy")) == R.canon(wX) and np.array_equal(np.load(tmp_path / "Y.npy"), wy)
