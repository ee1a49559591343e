#!/usr/bin/env python3
"""Generate tests/golden/eccstats/*.npz: the reference's eccentricity statistics, captured from the reference itself.

CPU only; runs ONLY where the reference tree is mounted (the build container) and pandas is installed.  It imports the
reference's ``src/utils.py`` without writing bytecode, with TZ=UTC (mark_timewindow uses time.localtime), builds the
frame exactly as src/main_rec.py:217-220 does (import_ml from a csv: string columns; mark_timewindow; feedback as float)
or, for the 30Music layout (:215), with the 4th column already a timewindow, and records the input rows and every output
table.  Data only is written: inputs and expected outputs, no reference source text.

Per case: ``uid, id`` (int64; the frame holds their decimal strings), ``feedback``, ``timestamp`` (ml layout only),
``timewindow`` (int64) per row, and
  ``unum_id / unum_tw / unum``   df_iu.groupby(["id", "timewindow"]).size()  (src/utils.py:96)
  ``ir_id / ir``, ``ue_uid / ue``, ``ie_id / ie``, ``ire_id / ire``, ``ier_id / ier``   calculate_*_from_iu
The 30Music layout: the reference leaves the timewindow column a string there, and pandas >= 2 refuses the mean over
it in calculate_ir_from_iu; the generator converts that column to int, which is what the arithmetic assumes.
Re-run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eccstats_golden.py
"""
import os
import sys
import tempfile
import time

os.environ["TZ"] = "UTC"
time.tzset()
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/src")
import utils as ref  # noqa: E402  (the reference module)
import eccstats_reference as R  # noqa: E402  (only its seeded row generator)

OUT = os.path.join(HERE, "eccstats")
T0, T1 = 946684800, 1041379200          # 2000-01-01 .. 2003-01-01 UTC: 36 months


def frame(uid, iid, fb, fourth, layout):
    with tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False) as f:
        for row in zip(uid, iid, fb, fourth):
            f.write("%d,%d,%s,%d\n" % (row[0], row[1], repr(float(row[2])), row[3]))
        path = f.name
    try:
        if layout == "ml":                                       # src/main_rec.py:217-220
            df = ref.import_ml(path, headercol=["uid", "id", "feedback", "timestamp"])
            df = ref.mark_timewindow(df)
            df.columns = ["uid", "id", "feedback", "timestamp", "timewindow"]
        else:                                                    # src/main_rec.py:215
            df = ref.import_ml(path, headercol=["uid", "id", "feedback", "timewindow"])
            df["timewindow"] = df["timewindow"].astype(int)
        df.feedback = df.feedback.astype(float)
    finally:
        os.unlink(path)
    return df


def dump(name, uid, iid, fb, fourth, layout="ml"):
    df = frame(uid, iid, fb, fourth, layout)
    out = {"uid": np.asarray(uid, np.int64), "id": np.asarray(iid, np.int64), "feedback": np.asarray(fb, np.float64),
           "timewindow": np.asarray(df["timewindow"], np.int64), "layout": np.array(layout)}
    if layout == "ml":
        out["timestamp"] = np.asarray(fourth, np.int64)
    assert np.array_equal(out["feedback"], np.asarray(df["feedback"], np.float64))
    size = df.groupby(["id", "timewindow"]).size().reset_index(name="unum")
    out["unum_id"] = np.asarray(size["id"].astype(int), np.int64)
    out["unum_tw"] = np.asarray(size["timewindow"], np.int64)
    out["unum"] = np.asarray(size["unum"], np.int64)
    for fn, key, col in (("calculate_ir_from_iu", "id", "ir"), ("calculate_ue_from_iu", "uid", "ue"),
                         ("calculate_ie_from_iu", "id", "ie"), ("calculate_ire_from_iu", "id", "ire"),
                         ("calculate_ier_from_iu", "id", "ier")):
        t = getattr(ref, fn)(df.copy())
        out["%s_%s" % (col, key)] = np.asarray(t[key].astype(int), np.int64)
        out[col] = np.asarray(t[col], np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, len(uid), "rows", len(out["unum"]), "groups", os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")


def stamps(seed, n):
    return np.random.RandomState(seed).randint(T0, T1, size=n)


def main():
    for name, seed, n_u, n_i, n in (("syn400", 1, 40, 60, 400), ("syn20000", 2, 600, 900, 20000),
                                    ("syn3000", 3, 150, 500, 3000)):
        u, i, fb, _ = R.make_rows(seed, n_u, n_i, n, uniform_feedback=False)
        dump(name, u + 1, i + 1, fb, stamps(seed, n))
    # repeated plays: duplicate (uid, id) rows, feedback that is not exactly representable
    u, i, fb, _ = R.make_rows(4, 30, 40, 1500, uniform_feedback=True)
    assert len(set(zip(u.tolist(), i.tolist()))) < 1200
    dump("dup1500", u + 1, i + 1, fb, stamps(4, 1500))
    # the 30Music layout: the 4th column is the timewindow
    u, i, fb, tw = R.make_rows(5, 80, 300, 2500, n_windows=12, uniform_feedback=False)
    dump("tw2500", u + 1, i + 1, fb, tw, layout="tw")


if __name__ == "__main__":
    main()
