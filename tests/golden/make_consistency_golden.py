#!/usr/bin/env python3
"""Generate tests/golden/consistency/*.npz: the reference's septile transition tables, captured from the reference itself.

CPU only; runs ONLY where the reference tree is mounted (the build container) and pandas is installed.  It imports the
reference's ``src/utils.py`` without writing bytecode, with TZ=UTC, builds the frame as make_eccstats_golden.py does and
calls the reference's own ``septile_for_plot`` for both prefixes ('ml': the fixed ranges 201100 < tw < 201299 and
201300 < tw < 201499; '30': cut at seg_point).  seaborn and matplotlib.pyplot only draw and are not installed: inert
stand-ins are registered in sys.modules before the call, which runs in a temporary directory.  Data only is written:
inputs and expected outputs, no reference source text.

Per case: ``uid, id`` (int64; the frame holds their decimal strings), ``feedback``, ``timewindow`` (and ``timestamp`` in
the ml layout) per row, ``prefix``, ``seg_point``, ``first``, ``second`` (the inclusive ranges the prefix means, -1: open),
``seed``, and for kind in ir, ie, ue
  ``<kind>_frame``   the returned count frame: columns bin1, bin2, count, count_sum (int64[rows][4]) and ``<kind>_ratio``
  ``<kind>_ids / _v1 / _v2 / _bins1 / _bins2``   the joined frame: the reference's calculate_*_from_iu over the two period
                     frames (cut from the frame sorted as septile_for_plot sorts it), merged on the id with the support
                     filter, and ref.mark_septile called on those joined values.  The generator asserts that the
                     group-by of these bins is the returned count frame.

The reference is not tie-stable and sums the rows of a period in another order than the restatement.  So a case is kept
only if, for each of its six value columns, the two values on either side of every septile border differ by more than
the bound tests/test_eccstats_host.py holds the restatement to (C_Z x the column's largest magnitude), equal values
therefore lie strictly inside a bin, and at least 3 x 7 entities of each kind are joined.  Seeds are searched until both
hold; the seed is stored.  Re-run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_consistency_golden.py
"""
import os
import sys
import tempfile
import time
from unittest import mock

os.environ["TZ"] = "UTC"
time.tzset()
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference/src")
import utils as ref  # noqa: E402  (the reference module)
import eccstats_reference as R  # noqa: E402  (only its seeded row generator)
from make_eccstats_golden import frame  # noqa: E402  (the frame as the reference's readers build it)

OUT = os.path.join(HERE, "consistency")
N = 7
C_Z = 100 * 1.89e-14                    # tests/test_eccstats_host.py
T0, T1 = 1325376000, 1388534400         # 2012-01-01 .. 2014-01-01 UTC: 24 months, 12 in each of the ml ranges
KINDS = (("ir", "id"), ("ie", "id"), ("ue", "uid"))


def stand_ins():
    sns, plt = mock.MagicMock(), mock.MagicMock()
    ax = sns.heatmap.return_value
    ax.get_xlim.return_value = (0.0, 1.0)
    ax.get_ylim.return_value = (0.0, 1.0)
    mpl = mock.MagicMock()
    mpl.pyplot = plt
    return {"seaborn": sns, "matplotlib": mpl, "matplotlib.pyplot": plt}


def septile_tables(df, seg_point, prefix):
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp, mock.patch.dict(sys.modules, stand_ins()):
        os.chdir(tmp)
        try:
            return ref.septile_for_plot(df.copy(), seg_point, prefix)
        finally:
            os.chdir(here)


def ranges(prefix, seg_point):
    if prefix == "ml":
        return (201101, 201298), (201301, 201498)
    return (None, seg_point), (seg_point + 1, None)


def cut(df, rng):
    keep = pd.Series(True, index=df.index)
    if rng[0] is not None:
        keep &= df.timewindow >= rng[0]
    if rng[1] is not None:
        keep &= df.timewindow <= rng[1]
    return df[keep]


def joined(df, first, second, kind, key):
    """The joined frame of one kind, marked by the reference's mark_septile."""
    df = df.sort_values("timewindow", ascending=0)
    fn = getattr(ref, "calculate_%s_from_iu" % kind)
    both = None
    for p, rng in ((1, first), (2, second)):
        t = fn(cut(df, rng)).rename(columns={kind: "%s%d" % (kind, p)})
        both = t if both is None else pd.merge(both, t, on=[key], how="inner")
    for rng in (first, second):
        sup = cut(df, rng).groupby([key])["feedback"].size().reset_index(name="rows")
        both = pd.merge(both, sup[sup.rows > 4], on=[key], how="inner").drop(columns=["rows"])
    both = ref.mark_septile(both, kind + "1")
    return ref.mark_septile(both, kind + "2")


def borders_clear(values):
    """Every septile border of the ascending values is wider than the bound."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    repeat = len(v) // N
    if repeat < 3 or not np.isfinite(v).all():
        return False
    bound = C_Z * float(np.abs(v).max())
    return all(v[k * repeat] - v[k * repeat - 1] > bound for k in range(1, N))


def capture(uid, iid, fb, fourth, layout, prefix, seg_point):
    """The arrays of one case, or None when a condition fails."""
    df = frame(uid, iid, fb, fourth, layout)
    first, second = ranges(prefix, seg_point)
    if len(cut(df, first)) == 0 or len(cut(df, second)) == 0:
        return None
    out = {"uid": np.asarray(uid, np.int64), "id": np.asarray(iid, np.int64), "feedback": np.asarray(fb, np.float64),
           "timewindow": np.asarray(df["timewindow"], np.int64), "prefix": np.array(prefix), "seg_point": np.int64(seg_point),
           "first": np.array([-1 if v is None else v for v in first], np.int64),
           "second": np.array([-1 if v is None else v for v in second], np.int64)}
    if layout == "ml":
        out["timestamp"] = np.asarray(fourth, np.int64)
    frames = {}
    for kind, key in KINDS:
        j = joined(df, first, second, kind, key)
        if len(j) < 3 * N or not (borders_clear(j[kind + "1"]) and borders_clear(j[kind + "2"])):
            return None
        frames[kind] = j
    tables = dict(zip(("ir", "ie", "ue"), septile_tables(df, seg_point, prefix)))
    for kind, key in KINDS:
        j, t = frames[kind], tables[kind]
        c1, c2 = kind + "1_7", kind + "2_7"
        mine = j.groupby([c1, c2])[key].size().reset_index(name="count")
        assert np.array_equal(mine.values, t[[c1, c2, "count"]].values), kind          # the joined frame is the reference's
        out[kind + "_frame"] = np.asarray(t[[c1, c2, "count", "count_sum"]].values, np.int64)
        out[kind + "_ratio"] = np.asarray(t["ratio"], np.float64)
        out[kind + "_ids"] = np.asarray(j[key].astype(int), np.int64)
        out[kind + "_v1"], out[kind + "_v2"] = np.asarray(j[kind + "1"], np.float64), np.asarray(j[kind + "2"], np.float64)
        out[kind + "_bins1"], out[kind + "_bins2"] = np.asarray(j[c1], np.int64), np.asarray(j[c2], np.int64)
    return out


def rows_of(seed, n_users, n_items, n, layout, uniform):
    u, i, fb, _ = R.make_rows(seed, n_users, n_items, n, uniform_feedback=uniform, item_power=0.6)
    rs = np.random.RandomState(seed + 1000)
    if layout == "ml":
        return u + 1, i + 1, fb, rs.randint(T0, T1, size=n)
    m = 1 + rs.randint(0, 24, size=n)                                    # 2014-02 .. 2016-01: 24 months
    return u + 1, i + 1, fb, (2014 + m // 12) * 100 + m % 12 + 1


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, n_users, n_items, n, layout, prefix, seg_point, uniform in (
            ("ml3000", 70, 110, 3000, "ml", "ml", 0, False), ("ml20000", 400, 150, 20000, "ml", "ml", 0, False),
            ("dup3000", 40, 60, 3000, "ml", "ml", 0, True), ("seg3000", 70, 80, 3000, "tw", "30", 201501, False)):
        for seed in range(1, 400):
            u, i, fb, fourth = rows_of(seed, n_users, n_items, n, layout, uniform)
            out = capture(u, i, fb, fourth, layout, prefix, seg_point)
            if out is not None:
                break
        else:
            raise SystemExit("%s: no seed meets the conditions" % name)
        if name == "dup3000":
            assert len(set(zip(u.tolist(), i.tolist()))) < n
        out["seed"] = np.int64(seed)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, "seed", seed, n, "rows", {k: len(out[k + "_ids"]) for k, _ in KINDS}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
