"""Host tests of the eccentricity statistics: the restatement tests/eccstats_reference.py against output recorded from the
reference's own src/utils.py (tests/golden/eccstats/*.npz, written by tests/golden/make_eccstats_golden.py), the two
forms of the restatement against each other, timewindow_utc, and the argparse errors of main_rec.py.  No GPU.

The bound.  pandas sums pairwise / with Kahan, the restatement left to right, so they cannot agree bit for bit.  The
bound is measured: c = 100 x the worst ratio observed over the committed fixtures, where the ratio is
max|restatement - recorded| / max|recorded column| for the z-scored columns (ir, ue, ie) and max|restatement - recorded|
itself for the zero-one columns (ire, ier).  Observed (restatement as committed, fixtures as committed):

    fixture     ir        ue        ie        ire       ier
    syn400      1.01e-15  6.63e-16  3.98e-16  3.33e-16  1.11e-15
    syn20000    8.00e-16  6.10e-15  8.06e-15  2.22e-16  2.33e-13
    syn3000     1.24e-15  1.52e-14  1.89e-14  3.33e-16  2.75e-13
    dup1500     1.22e-15  1.29e-14  1.48e-14  2.22e-16  3.50e-15
    tw2500      2.23e-16  4.24e-15  5.79e-15  1.11e-16  2.33e-14

worst z-scored 1.89e-14, worst zero-one 2.75e-13.
"""
import glob
import os

import numpy as np
import pytest

import eccstats_reference as R

C_Z = 100 * 1.89e-14          # relative to the column's largest magnitude
C_ZO = 100 * 2.75e-13         # absolute; the column lies in [0, 1]

FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eccstats", "*.npz")))
NAMES = [os.path.basename(p)[:-4] for p in FIXTURES]
_cache = {}


def load(path):
    """(fixture, numpy-form restatement of it), computed once and shared."""
    if path not in _cache:
        d = np.load(path)
        uid, iid = [str(v) for v in d["uid"]], [str(v) for v in d["id"]]
        _cache[path] = (d, uid, iid, R.statistics_numpy(uid, iid, d["feedback"], d["timewindow"]))
    return _cache[path]


def test_fixtures_present():
    assert set(NAMES) == {"syn400", "syn20000", "syn3000", "dup1500", "tw2500"}
    d = np.load(FIXTURES[NAMES.index("dup1500")])
    assert len(set(zip(d["uid"].tolist(), d["id"].tolist()))) < len(d["uid"])          # repeated (uid, id) rows
    assert str(np.load(FIXTURES[NAMES.index("tw2500")])["layout"]) == "tw"


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_unum_equals_the_recorded_one(path):
    d, _, _, got = load(path)
    want = dict(zip(zip(d["unum_id"].tolist(), d["unum_tw"].tolist()), d["unum"].tolist()))
    mine = dict(zip(zip([int(got["items"][i]) for i in got["group_item"]], got["group_tw"].tolist()), got["unum"].tolist()))
    assert len(mine) == len(got["unum"]) == len(d["unum"]) and mine == want


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_columns_within_the_measured_bound(path):
    d, _, _, got = load(path)
    for col, key, ids in (("ir", "id", "items"), ("ue", "uid", "users"), ("ie", "id", "items"), ("ire", "id", "items"),
                          ("ier", "id", "items")):
        rid = d[col + "_" + key].tolist()
        mine_ids = [int(v) for v in got[ids]]
        assert len(rid) == len(mine_ids) == len(set(rid)) and set(rid) == set(mine_ids), col     # no id left out
        pos = {v: n for n, v in enumerate(mine_ids)}
        mine = got[col][[pos[v] for v in rid]]
        want = d[col]
        assert np.isfinite(want).all() and np.isfinite(mine).all()
        dev = float(np.abs(mine - want).max())
        bound = C_Z * float(np.abs(want).max()) if col in ("ir", "ue", "ie") else C_ZO
        print("%s %s: deviation %.3e bound %.3e" % (os.path.basename(path), col, dev, bound))
        assert dev <= bound, (col, dev, bound)


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_numpy_form_equals_the_loops_by_bytes(path):
    d, uid, iid, got = load(path)
    lit = R.statistics_literal(uid, iid, d["feedback"], d["timewindow"])
    assert lit["users"] == got["users"] and lit["items"] == got["items"]
    for k in ("group_item", "group_tw", "row_group"):
        assert np.array_equal(lit[k], got[k]), k
    for k in R.COLUMNS:
        assert lit[k].dtype == got[k].dtype and R.canon(lit[k]) == R.canon(got[k]), k


def test_forms_agree_across_a_chunk_boundary_and_on_degenerate_input():
    for seed, n_u, n_i, n in ((7, 1, 9, 40), (8, 50, 4200, 9000), (9, 4100, 30, 6000)):
        u, i, fb, tw = R.make_rows(seed, n_u, n_i, n)
        a, b = R.statistics_literal(u.tolist(), i.tolist(), fb, tw), R.statistics_numpy(u, i, fb, tw)
        for k in R.COLUMNS:
            assert R.canon(a[k]) == R.canon(b[k]), (seed, k)
    one = R.statistics_numpy(*R.make_rows(7, 1, 9, 40))
    assert not np.isfinite(one["ue"]).any() and np.isnan(one["ie"]).all()         # zero variance: the IEEE result stands


def test_zero_sign_rule_of_min_max():
    assert R.canon(np.array(R.min_max(np.array([0.0, -0.0, 1.0])))) == R.canon(np.array([-0.0, 1.0]))
    assert R.canon(np.array(R.min_max(np.array([-1.0, -0.0, 0.0])))) == R.canon(np.array([-1.0, 0.0]))
    assert R.canon(np.array(R.zero_one(np.array([0.0, -0.0, 2.0])))) == R.canon(np.array(R.zo_literal([0.0, -0.0, 2.0])))
    assert np.isnan(R.min_max(np.array([1.0, np.nan]))).all()


def test_timewindow_utc():
    from n2v_hip import eccstats
    stamps = [0, 951782399, 951782400, 951868800, 1709164800, 1709251199, 1709251200, -1, 1735689599, 1735689600, 978300760]
    want = [197001, 200002, 200002, 200003, 202402, 202402, 202403, 196912, 202412, 202501, 200012]
    #        epoch   28 Feb   29 Feb: leap day  1 Mar    29 Feb 2024       1 Mar    before the epoch  31 Dec / 1 Jan
    got = eccstats.timewindow_utc(stamps)
    assert got.dtype == np.int64 and got.tolist() == want
    assert R.timewindow_utc(stamps).tolist() == want
    assert eccstats.timewindow_utc(np.array([str(s) for s in stamps]).astype(np.int64)).tolist() == want
    for path in FIXTURES:
        d = np.load(path)
        if "timestamp" in d:                                  # the reference's mark_timewindow under TZ=UTC
            assert np.array_equal(eccstats.timewindow_utc(d["timestamp"]), d["timewindow"])


def test_first_appearance_matches_the_trainset_order():
    from n2v_hip import eccstats
    raw = ["b", "a", "b", "c", "a", "10", "9"]
    inner, table = eccstats.first_appearance(raw)
    want_inner, want_table = R.inner_ids(raw)
    assert inner.tolist() == want_inner.tolist() and table == want_table and all(type(v) is str for v in table)


def _csv(tmp_path, rows):
    p = tmp_path / "r.csv"
    p.write_text("".join(",".join(map(str, r)) + "\n" for r in rows))
    return str(p)


def test_main_rec_argparse_errors(tmp_path, capsys):
    import main_rec
    four = _csv(tmp_path, [(1, 10, 3.0, 978300760), (2, 10, 4.0, 978300761), (2, 11, 1.0, 981000000)])
    for extra, word in ((["-mode", "ir", "-weights", "w.csv"], "-weights"), (["-mode", "ie", "-item-based"], "-item-based"),
                        (["-save-weights", "w.csv"], "-save-weights"), (["-mode", "xx"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            main_rec.parse_args(["-input", four] + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err
    three = tmp_path / "t.csv"
    three.write_text("1,10,3.0\n2,10,4.0\n")
    with pytest.raises(SystemExit) as e:
        main_rec.parse_args(["-input", str(three), "-mode", "ire"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "4th column" in err and "timestamp" in err
    a = main_rec.parse_args(["-input", four, "-mode", "ier"])
    assert a.windows.tolist() == [200012, 200012, 200102] and a.window_col == "timestamp"
    a = main_rec.parse_args(["-input", four, "-mode", "ier", "-window-col", "timewindow"])
    assert a.windows.tolist() == [978300760, 978300761, 981000000]
    a = main_rec.parse_args(["-input", str(three)])                      # without -mode nothing changes
    assert a.mode is None and a.weights is None and not hasattr(a, "windows")


def test_weights_file_round_trip(tmp_path):
    import main_rec
    w = {"10": 0.1 + 0.2, "11": -1.0 / 3.0, "12": float("inf"), "13": 0.0}
    main_rec.write_weights(str(tmp_path / "w.csv"), w)
    assert main_rec.read_weights(str(tmp_path / "w.csv")) == w
