"""CPU tests of the eccentricity consistency analysis: the restatement tests/consistency_reference.py against what the
reference's own septile_for_plot returned (tests/golden/consistency/*.npz, written by
tests/golden/make_consistency_golden.py), the tie rule, and everything n2v_hip.consistency and consistency.py decide on the
host before a launch.  Profiles and features cannot be recorded (the reference's mark_100 calls DataFrame.sort, which
pandas 2 no longer has): they are defined by the restatement, which is held here to plain Python loops."""
import os
import re

import numpy as np
import pytest

import consistency_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_fixtures_present_and_meet_their_conditions():
    assert sorted(f[:-4] for f in os.listdir(os.path.join(GOLDEN, "consistency")) if f.endswith(".npz")) == sorted(R.CASES)
    for name in R.CASES:
        c = R.case(GOLDEN, name)                                       # re-asserts the border and 3 n conditions
        assert len(c.uid) in (3000, 20000) and c.seed >= 1
    d = R.case(GOLDEN, "dup3000")
    assert len(set(zip(d.uid, d.iid))) < len(d.uid)                    # repeated (uid, id) rows
    s = R.case(GOLDEN, "seg3000")
    assert s.prefix == "30" and s.first == (None, s.seg_point) and s.second == (s.seg_point + 1, None)
    assert R.case(GOLDEN, "ml3000").first == (201101, 201298) and R.case(GOLDEN, "ml3000").second == (201301, 201498)


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_equals_the_recording(name):
    """No case and no kind exempted: joined ids, both bin columns, counts and row sums exactly, ratios as fp64."""
    c, got = R.case(GOLDEN, name), R.restated(GOLDEN, name)
    for kind in R.KINDS:
        g, want = got[kind], c.joined(kind)
        assert set(g["ids"]) == set(want) and len(g["ids"]) == len(want) >= 21, kind
        assert {r: (int(a), int(b)) for r, a, b in zip(g["ids"], g["bins1"], g["bins2"])} == {r: v[2:] for r, v in want.items()}, kind
        for col, k in (("v1", 0), ("v2", 1)):                          # the values themselves: within the statistics' bound
            rec = np.array([want[r][k] for r in g["ids"]])
            assert np.abs(g[col] - rec).max() <= R.C_Z * np.abs(rec).max(), (kind, col)
        table, ratio = c.frame(kind)
        f = R.frame(g["count"], g["count_sum"], g["ratio"])
        mine = np.stack([f.bin1, f.bin2, f.count, f.count_sum], axis=1)
        assert np.array_equal(mine, table), kind                       # the reference's order too
        assert np.array_equal(f.ratio, ratio), kind
        assert g["count"].sum() == len(want) and np.array_equal(g["count"].sum(axis=1), g["count_sum"])


def test_tie_rule_on_ties_that_straddle_every_border():
    """14 items, two ir values (7 items each) in both periods, n = 7: every border but one cuts through a tie, which goes
    by ascending raw id as sorted() orders the strings ('10' before '2')."""
    uid, iid, fb, tw = [], [], [], []
    for item in range(1, 15):
        for period in (201200, 201300):
            for month in range(1, 6):
                for rep in range(1 if item <= 7 else 2):              # items 8 .. 14: two rows per (item, month)
                    uid.append(str(100 + len(uid) % 9)); iid.append(str(item)); fb.append(1.0 + (len(fb) % 4)); tw.append(period + month)
    got = R.transitions(uid, iid, fb, tw, (201101, 201298), (201301, 201498))["ir"]
    assert len(got["ids"]) == 14 and len(set(got["v1"].tolist())) == 2 and len(set(got["v2"].tolist())) == 2
    order = sorted(range(14), key=lambda k: (got["v1"][k], got["ids"][k]))          # value, then the id as a string
    want = np.empty(14, dtype=np.int64)
    want[order] = np.repeat(np.arange(1, 8), 2)
    assert got["bins1"].tolist() == want.tolist() == got["bins2"].tolist()
    by_id = dict(zip(got["ids"], got["bins1"].tolist()))
    rare, common = ("1 2 3 4 5 6 7".split(), "10 11 12 13 14 8 9".split())            # sorted() order inside each tie
    low, high = (common, rare) if got["v1"][got["ids"].index("8")] < got["v1"][got["ids"].index("1")] else (rare, common)
    assert [by_id[r] for r in low + high] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7]
    assert np.array_equal(got["count"], np.diag([2] * 7))


def test_crosstab_frame_and_empty_join():
    count, count_sum, ratio = R.crosstab([1, 1, 2, 4], [2, 2, 1, 4], 4)
    assert count.tolist() == [[0, 2, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]] and count_sum.tolist() == [2, 1, 0, 1]
    assert ratio[0].tolist() == [0.0, 1.0, 0.0, 0.0] and np.isnan(ratio[2]).all()
    f = R.frame(count, count_sum, ratio)
    assert [tuple(r) for r in f.tolist()] == [(1, 2, 2, 2, 1.0), (2, 1, 1, 1, 1.0), (4, 4, 1, 1, 1.0)]
    # nobody above the support: zero counts, NaN ratios; a period without rows: ValueError
    uid, iid, fb, tw = ["1", "2", "1", "2"], ["5", "5", "6", "6"], [1.0, 2.0, 3.0, 4.0], [201201, 201202, 201301, 201302]
    got = R.transitions(uid, iid, fb, tw, (201101, 201298), (201301, 201498))
    for kind in R.KINDS:
        assert got[kind]["ids"] == [] and not got[kind]["count"].any() and np.isnan(got[kind]["ratio"]).all()
    with pytest.raises(ValueError):
        R.transitions(uid, iid, fb, tw, (201101, 201298), (201401, 201498))


def test_profile_restatement_equals_plain_loops():
    """np.add.at against Python loops over Python floats in file order, and the count form against the reference's own
    expression x / sum(tmp) over the nan_to_num'd sizes."""
    for name, (user, item, fb, item_bin, n_users, n_bins) in R.profile_cases().items():
        cnt = [[0.0] * n_bins for _ in range(n_users)]
        part = [[0.0] * n_bins for _ in range(n_users)]
        total = [0.0] * n_users
        for u, i, f in zip(user.tolist(), item.tolist(), fb.tolist()):
            b = int(item_bin[i])
            if b:
                cnt[u][b - 1] += 1.0
                part[u][b - 1] = part[u][b - 1] + f
                total[u] = total[u] + f
        with np.errstate(all="ignore"):
            want_c = np.array([[np.float64(x) / np.float64(sum(tmp)) for x in tmp] for tmp in cnt])
            want_w = np.array([[np.float64(x) / np.float64(t) for x in row] for row, t in zip(part, total)])
        got_c = R.profile(user, item, fb, item_bin, n_users, n_bins)
        got_w = R.profile(user, item, fb, item_bin, n_users, n_bins, weighted=True)
        assert R.canon(got_c) == R.canon(want_c) and R.canon(got_w) == R.canon(want_w), name
        assert np.isnan(got_c[0]).all() and np.isnan(got_c[6]).all() and np.isnan(got_c[7]).all()      # no binned row
        assert np.allclose(np.nansum(got_c, axis=1)[[1, 2, 3, 4, 5, 8]], 1.0)
        # the order matters: the same rows summed backwards give other bits
        back = R.profile(user[::-1], item[::-1], fb[::-1], item_bin, n_users, n_bins, weighted=True)
        assert n_bins == 1 or R.canon(back) != R.canon(got_w), name      # one bin: x / x whatever the order


def test_each_deliberate_error_is_caught_by_a_case():
    # ">=" for ">": a recorded case has an entity with exactly min_count rows in a period
    assert any(any(R.transitions(c.uid, c.iid, c.feedback, c.timewindow, c.first, c.second, variant="ge")[k]["ids"]
                   != R.restated(GOLDEN, name)[k]["ids"] for k in R.KINDS)
               for name, c in ((n, R.case(GOLDEN, n)) for n in ("ml3000", "dup3000", "seg3000")))
    tile = 2048
    assert any(len(R.join(*cs)[0]) != len(R.join(*cs, variant="ge")[0]) for cs in R.join_cases(tile).values())
    # row sums over bins2: both columns of a join have the same bin sizes, so only a crosstab case can tell
    differ = [k for k, (a, b, n) in R.crosstab_cases().items()
              if R.canon(R.crosstab(a, b, n)[2]) != R.canon(R.crosstab(a, b, n, variant="sum_bins2")[2])]
    assert "skewed_n7" in differ and "emptyrow_n7" in differ
    # profile by sum where count is meant
    assert all(R.canon(R.profile(*cs)) != R.canon(R.profile(*cs, variant="profile_sum")) for cs in R.profile_cases().values() if cs[5] > 1)          # with one bin both give x / x


def test_features_restatement():
    users, prof = ["a", "b"], np.array([[0.25, 0.75], [np.nan, np.nan]])
    uid, iid, fb = ["b", "a", "a", "b"], ["7", "8", "9", "8"], [1.0, 2.0, 3.0, 4.0]
    X, y, rows = R.features(users, prof, uid, iid, fb)
    assert rows.tolist() == [0, 1, 2, 3] and y.tolist() == fb and X.shape == (4, 3)
    assert X[1].tolist() == [0.25, 0.75, 8.0] and np.isnan(X[0, :2]).all() and X[0, 2] == 7.0
    vec = {"8": np.array([0.1, 0.2, 0.3], np.float32), 9: np.array([1, 2, 3], np.float32)}       # 9: an int key never matches '9'
    X, y, rows = R.features(users, prof, uid, iid, fb, vec)
    assert rows.tolist() == [1, 3] and y.tolist() == [2.0, 4.0] and X.shape == (2, 5)
    assert X[0].tolist() == [0.25, 0.75] + [float(np.float32(v)) for v in (0.1, 0.2, 0.3)]


def test_intervals():
    from n2v_hip import consistency as C
    assert C.parse_interval("201101:201298") == (201101, 201298)
    assert C.parse_interval(":201407") == (None, 201407) and C.parse_interval("201408:") == (201408, None)
    assert C.parse_interval(" 5 : 5 ") == (5, 5)
    assert C.seg_point_intervals(201407) == ((None, 201407), (201408, None))
    for bad in ("201101", "a:b", ":", "3:2", "1:2:3", "1.5:2", ""):
        with pytest.raises(ValueError):
            C.parse_interval(bad)
    for bad in ((None, None), (3, 2), (1.0, 2), 5, (1, 2, 3), (True, 2)):
        with pytest.raises(ValueError):
            C.check_interval(bad)
    with pytest.raises(ValueError):
        C.seg_point_intervals(2014.5)


def test_every_value_error_comes_without_a_gpu(monkeypatch):
    import torch
    from n2v_hip import consistency as C
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    uid, iid, fb, tw = ["1", "2", "1"], ["5", "5", "6"], [1.0, 2.0, 3.0], [201201, 201301, 201302]
    ok = dict(uid=uid, id=iid, feedback=fb, timewindow=tw, first=(201101, 201298), second=(201301, 201498), n=7, min_count=4)
    for change in (dict(n=0), dict(n=257), dict(n=7.0), dict(n=True), dict(min_count=-1), dict(min_count=1.5),
                   dict(first=(None, None)), dict(first=(201298, 201101)), dict(second=(201401, 201498)),      # no rows in it
                   dict(first=(201001, 201012)), dict(feedback=[1.0]), dict(timewindow=[201201]),
                   dict(uid=[], id=[], feedback=[], timewindow=[])):
        with pytest.raises(ValueError):
            C.transitions(**dict(ok, **change))
    with pytest.raises(RuntimeError, match="no GPU"):
        C.transitions(**ok)
    for change in (dict(n_bins=0), dict(n_bins=257), dict(n_bins=2.0), dict(feedback=[1.0])):
        kw = dict(uid=uid, id=iid, feedback=fb, timewindow=tw, n_bins=2)
        with pytest.raises(ValueError):
            C.user_ie_profile(**dict(kw, **change))
    with pytest.raises(RuntimeError, match="no GPU"):
        C.user_ie_profile(uid, iid, fb, tw, n_bins=2)
    prof = C.ProfileResult(["1", "2"], ["5", "6"], np.zeros(2), np.array([1, 2], np.int32), np.array([[0.5, 0.5], [1.0, 0.0]]), 2, False)
    for kw in (dict(uid=["1", "3", "1"]), dict(id=["5", "x", "6"]), dict(feedback=[1.0]),
               dict(item_vectors={"5": [1.0, 2.0], "6": [1.0]})):
        with pytest.raises(ValueError):
            C.features(prof, **dict(dict(uid=uid, id=iid, feedback=fb), **kw))
    X, y, rows = C.features(prof, uid, iid, fb, item_vectors={"77": [1.0, 2.0]})                   # no row has a vector
    assert X.shape == (0, 2) and len(y) == 0 and len(rows) == 0
    with pytest.raises(RuntimeError, match="no GPU"):
        C.features(prof, uid, iid, fb)
    with pytest.raises(RuntimeError, match="no GPU"):
        C.features(prof, uid, iid, fb, item_vectors={"5": [1.0, 2.0]})


def test_cli_parse_args_and_text(capsys):
    import consistency as cli
    a = cli.parse_args(["-input", "r.csv", "-first", "201101:201298", "-second", "201301:201498"])
    assert a.periods == ((201101, 201298), (201301, 201498))
    assert (a.n, a.min_count, a.window_col, a.out, a.profile, a.bins, a.weighted, a.features, a.item_emb, a.device) == \
        (7, 4, "timestamp", None, None, 100, False, None, None, "cuda:0")
    a = cli.parse_args(["-input", "r.csv", "-seg-point", "201407", "-n", "10", "-min-count", "0", "-window-col", "timewindow", "-out", "o",
                        "-profile", "p.npy", "-bins", "50", "-weighted", "-features", "X.npy", "Y.npy", "-item-emb", "e.txt"])
    assert a.periods == ((None, 201407), (201408, None)) and (a.n, a.min_count, a.window_col, a.out) == (10, 0, "timewindow", "o")
    assert (a.profile, a.bins, a.weighted, a.features, a.item_emb) == ("p.npy", 50, True, ["X.npy", "Y.npy"], "e.txt")
    base = ["-input", "r.csv"]
    both = base + ["-first", "1:2", "-second", "3:4"]
    for argv in (base, base + ["-first", "1:2"], base + ["-second", "1:2"], both + ["-seg-point", "3"], ["-first", "1:2", "-second", "3:4"],
                 base + ["-first", "2:1", "-second", "3:4"], base + ["-first", "x", "-second", "3:4"], both + ["-n", "0"],
                 both + ["-n", "257"], both + ["-bins", "0"], both + ["-min-count", "-1"], both + ["-window-col", "month"],
                 both + ["-features", "X.npy", "Y.npy"], both + ["-profile", "p", "-item-emb", "e.txt"],
                 both + ["-profile", "p", "-features", "X.npy"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    capsys.readouterr()
    count, count_sum, ratio = R.crosstab([1, 1, 2], [2, 1, 2], 3)
    from n2v_hip import consistency as C
    t = C.Table(["a", "b", "c"], None, None, None, None, count, count_sum, ratio)
    assert cli.frame_text(t.frame()) == "bin1,bin2,count,count_sum,ratio\n1,1,1,2,0.5\n1,2,1,2,0.5\n2,2,1,1,1.0\n"
    assert cli.table_text("ir", t).splitlines()[1:] == ["  1   0.50  0.50  0.00", "  2   0.00  1.00  0.00", "  3    nan   nan   nan"]


def test_symbols_are_declared_bound_and_exported():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from n2v_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    assert re.search(r"#define N2V_ECCCONS_MAX_BINS 256\b", hdr) and re.search(r"#define N2V_ECCCONS_CELLS 4096\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(n2v_ecccons_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"n2v_ecccons_" + s for s in ("check_i32", "check_i64", "check_ptr", "join", "crosstab", "profile",
                                                      "feature_rows", "features")}
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in declared:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).strip()
        assert len(_lib.SIGNATURES[name][1]) == len(params.split(",")), name
        assert hasattr(lib, name), name
    assert _lib.load().n2v_abi_version() == 5
    from n2v_hip import consistency as C
    assert C.MAX_BINS == 256 and (C.BAD_RANGE, C.BAD_PTR) == (1, 2)
