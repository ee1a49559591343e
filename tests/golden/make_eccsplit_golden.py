#!/usr/bin/env python3
"""Generate tests/golden/eccsplit/*.npz: the reference's eccentricity split, captured from the reference itself.

CPU only; runs ONLY where the reference tree is mounted (the build container) and pandas is installed.  The rows are
those of tests/golden/eccstats/<case>.npz and the frame is built as make_eccstats_golden.py builds it (string id
columns, feedback as float).  Per case the reference's calculate_ue_from_iu gives df_ue; for n in 3, 7, 10 and
n_users + 5 its mark_n marks the bins and its save_edgelist / split_and_save_edgelist write the files into a temporary
directory.  Data only is written: expected outputs, no reference source text.

Per case:
  ``ue_uid / ue``      df_ue in its own order (ascending uid STRING), equal to the eccstats recording
  ``ns``               the values of n
  ``bins_<n>``         the ue_<n> column of mark_n's frame, put back into df_ue's order (int32)
  ``file_all``         the bytes of ue.edgelist (the same for every n)
  ``files_<n>`` / ``files_<n>_off``   the bytes of ue_1.edgelist .. ue_<n>.edgelist one after the other, and where each begins

pandas sorts with an unstable quicksort, so equal ue are in no promised order there; the rule stated here is the stable
sort over df_ue's order.  The generator asserts that the recording agrees with that rule and with the closed form of the
bins (tests/eccsplit_reference.py), and fails loudly when a future pandas disagrees.
Re-run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eccsplit_golden.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_eccstats_golden as G  # noqa: E402  (sets TZ, puts the reference and tests/ on the path)
import eccsplit_reference as R  # noqa: E402

ref = G.ref
OUT = os.path.join(HERE, "eccsplit")
CASES = ("syn400", "syn3000", "dup1500", "tw2500")


def dump(name):
    z = np.load(os.path.join(HERE, "eccstats", name + ".npz"))
    layout = str(z["layout"])
    df = G.frame(z["uid"], z["id"], z["feedback"], z["timestamp"] if layout == "ml" else z["timewindow"], layout)
    df_ue = ref.calculate_ue_from_iu(df.copy())
    uid = list(df_ue["uid"])
    assert uid == sorted(uid), "df_ue is no longer in ascending order of the uid strings"
    out = {"ue_uid": np.asarray([int(x) for x in uid], np.int64), "ue": np.asarray(df_ue["ue"], np.float64)}
    assert np.array_equal(out["ue_uid"], z["ue_uid"]) and out["ue"].tobytes() == z["ue"].tobytes()
    n_users = len(uid)
    ns = [3, 7, 10, n_users + 5]
    out["ns"] = np.asarray(ns, np.int64)
    user_of = {x: k for k, x in enumerate(uid)}
    row_user = np.array([user_of[x] for x in df["uid"]])
    names_u = np.asarray([int(x) for x in df["uid"]], np.int64)
    names_i = np.asarray([R.item_name(x) for x in df["id"]], np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        ref.save_edgelist(df, tmp + "/", "")
        out["file_all"] = np.frombuffer(open(os.path.join(tmp, "ue.edgelist"), "rb").read(), np.uint8)
    assert out["file_all"].tobytes() == R.text(names_u, names_i, z["feedback"]).encode()
    for n in ns:
        marked = ref.mark_n(df_ue.copy(), "ue", n)
        bins = np.asarray(marked.sort_index()["ue_%d" % n], np.int32)
        assert list(marked.sort_index()["uid"]) == uid
        # the stated rule: stable over df_ue's order, closed-form bins
        assert np.array_equal(bins, R.mark_n(out["ue"], n)), "%s n=%d: pandas broke a tie against the stable rule" % (name, n)
        assert np.array_equal(R.mark_literal(n_users, n), R.mark_by_rank(n_users, n))
        out["bins_%d" % n] = bins
        with tempfile.TemporaryDirectory() as tmp:
            ref.split_and_save_edgelist(df, marked, n, tmp + "/", "")
            blobs = [open(os.path.join(tmp, "ue_%d.edgelist" % k), "rb").read() for k in range(1, n + 1)]
            assert len(os.listdir(tmp)) == n
        for k, blob in enumerate(blobs, 1):
            r = R.rows_of_bin(row_user, bins, k)
            assert blob == R.text(names_u[r], names_i[r], z["feedback"][r]).encode(), (name, n, k)
        out["files_%d" % n] = np.frombuffer(b"".join(blobs), np.uint8)
        out["files_%d_off" % n] = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    limit = max(os.path.getsize(os.path.join(HERE, "eccstats", f)) for f in os.listdir(os.path.join(HERE, "eccstats")))
    assert size <= limit, (name, size, limit)
    print(name, n_users, "users", len(z["uid"]), "rows", size, "bytes")


if __name__ == "__main__":
    for case in CASES:
        dump(case)
