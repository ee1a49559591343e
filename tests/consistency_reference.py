"""The eccentricity consistency analysis restated in numpy: what n2v_hip.consistency and csrc/n2v_ecccons.hip are held to.

Reference: src/utils.py:163-226 (septile_for_plot, everything before the drawing), :272-279 (mark_septile), :326-379
(calculate_uie_dist, calculate_uvec, make_data, calculate_iu_uvec).  Builds on tests/eccstats_reference.py (the
statistics of a frame) and tests/eccsplit_reference.py (the rank bins).

    period      the rows whose timewindow lies in an inclusive (lo, hi) range (None: open), in file order.  The reference
                sorts the frame by timewindow first (an unstable sort); here the rows keep file order, which moves the
                last bits of a sum and nothing else (the golden cases keep every septile border wider than that)
    statistics  eccstats_reference.statistics_numpy over the period's rows alone: its own inner ids, its own z-scores
    support     rows of the item (ir, ie) or of the user (ue) inside the period; kept when > min_count in BOTH periods
    join        entities with a value in both periods and the support in both, ascending inner id of the whole file
    bins        eccsplit_reference.mark_n of each joined column on its own, n bins.  THE ONE DELIBERATE DEFINITION: the
                reference's quicksort leaves ties open; here equal values rank by ascending raw id as Python's sorted
                orders the ids (the order of the reference's frames), for the first and for the second column alike
    crosstab    count[a - 1][b - 1] = entities in bin a of the first and bin b of the second period; count_sum[a - 1] =
                the sum of row a - 1 (the reference's groupby(['x1_7'])['count'].sum()); ratio = count * 1.0 / count_sum,
                NaN (0 / 0) in a row no entity is in
    frame       the reference's long table: (bin1, bin2, count, count_sum, ratio) of the non-empty cells, ascending
                (bin1, bin2)
    profile     per user, over the user's rows in file order whose item has a bin (item_bin 0: skipped): the rows per bin
                divided by their number (the reference keeps .size()); weighted: the feedback per bin divided by the
                feedback of all those rows, every sum from +0.0 adding one row after the other in file order.  0 / 0 = NaN
    features    X[t] = profile[user of row k] ++ the item's vector widened to fp64, rows whose item has no vector
                dropped; without vectors ++ [float(int(raw id))].  y = feedback of the kept rows

`variant` switches on one deliberate error ("ge": support >= min_count; "sum_bins2": row sums over the second column;
"profile_sum": the feedback sum where the count is meant) so that tests can show the cases tell them apart."""
import numpy as np

import eccsplit_reference as E
import eccstats_reference as S

KINDS = ("ir", "ie", "ue")


def in_period(timewindow, rng):
    tw = np.asarray(timewindow, dtype=np.int64)
    lo, hi = rng
    keep = np.ones(len(tw), dtype=bool)
    if lo is not None:
        keep &= tw >= lo
    if hi is not None:
        keep &= tw <= hi
    return np.nonzero(keep)[0]


def crosstab(bins1, bins2, n, variant=None):
    """(count int64[n][n], count_sum int64[n], ratio fp64[n][n])."""
    b1, b2 = np.asarray(bins1, dtype=np.int64), np.asarray(bins2, dtype=np.int64)
    count = np.zeros((n, n), dtype=np.int64)
    np.add.at(count, (b1 - 1, b2 - 1), 1)
    count_sum = count.sum(axis=0 if variant == "sum_bins2" else 1)
    with np.errstate(all="ignore"):
        ratio = count.astype(np.float64) * 1.0 / count_sum.astype(np.float64)[:, None]
    return count, count_sum, ratio


def frame(count, count_sum, ratio):
    a, b = np.nonzero(count)
    return np.rec.fromarrays([a + 1, b + 1, count[a, b], count_sum[a], ratio[a, b]], names="bin1,bin2,count,count_sum,ratio")


def join(v1, v2, c1, c2, min_count, variant=None):
    """(ids ascending, values 1, values 2) of the entities with both counts above the support."""
    c1, c2 = np.asarray(c1), np.asarray(c2)
    if variant == "ge":
        keep = (c1 > 0) & (c2 > 0) & (c1 >= min_count) & (c2 >= min_count)
    else:
        keep = (c1 > 0) & (c2 > 0) & (c1 > min_count) & (c2 > min_count)
    ids = np.nonzero(keep)[0]
    return ids, np.asarray(v1)[ids], np.asarray(v2)[ids]


def _period_columns(uid, iid, fb, tw, rows, u, i, n_users, n_items):
    """Values and supports of one period over the inner ids of the whole file (NaN / 0 where absent)."""
    st = S.statistics_numpy([uid[k] for k in rows], [iid[k] for k in rows], fb[rows], tw[rows])
    cols = {k: np.full(n_items if k != "ue" else n_users, np.nan) for k in KINDS}
    lu, li = S.first_appearance(u[rows])[1], S.first_appearance(i[rows])[1]       # whole-file inner id of every local id
    cols["ir"][li], cols["ie"][li], cols["ue"][lu] = st["ir"], st["ie"], st["ue"]
    return cols, np.bincount(u[rows], minlength=n_users), np.bincount(i[rows], minlength=n_items)


def transitions(uid, iid, feedback, timewindow, first, second, n=7, min_count=4, variant=None):
    """{kind: dict(ids raw, v1, v2, bins1, bins2, count, count_sum, ratio)}; ValueError for a period without rows."""
    uid, iid = list(uid), list(iid)
    fb, tw = np.asarray(feedback, dtype=np.float64), np.asarray(timewindow, dtype=np.int64)
    u, users = S.first_appearance(uid)
    i, items = S.first_appearance(iid)
    per = []
    for rng in (first, second):
        rows = in_period(tw, rng)
        if len(rows) == 0:
            raise ValueError("a period without rows")
        per.append(_period_columns(uid, iid, fb, tw, rows, u, i, len(users), len(items)))
    out = {}
    for kind in KINDS:
        names, sup = (users, 1) if kind == "ue" else (items, 2)
        ids, v1, v2 = join(per[0][0][kind], per[1][0][kind], per[0][sup], per[1][sup], min_count, variant)
        raw = [names[k] for k in ids]
        if len(ids):
            tr = E.tie_rank_of(raw)
            b1, b2 = E.mark_n(v1, n, tr), E.mark_n(v2, n, tr)
        else:
            b1 = b2 = np.zeros(0, dtype=np.int32)
        count, count_sum, ratio = crosstab(b1, b2, n, variant)
        out[kind] = dict(ids=raw, v1=v1, v2=v2, bins1=b1, bins2=b2, count=count, count_sum=count_sum, ratio=ratio)
    return out


def profile(user, item, feedback, item_bin, n_users, n_bins, weighted=False, variant=None):
    """fp64[n_users][n_bins] from inner ids; rows in the order given (file order)."""
    user, item = np.asarray(user, dtype=np.int64), np.asarray(item, dtype=np.int64)
    b = np.asarray(item_bin, dtype=np.int64)[item]
    keep = b > 0
    u, b, f = user[keep], b[keep] - 1, np.asarray(feedback, dtype=np.float64)[keep]
    with np.errstate(all="ignore"):
        if weighted or variant == "profile_sum":
            part, total = np.zeros((n_users, n_bins)), np.zeros(n_users)
            np.add.at(part, (u, b), f)                                   # unbuffered: one row after the other
            np.add.at(total, u, f)
            return part / total[:, None]
        cnt = np.zeros((n_users, n_bins), dtype=np.int64)
        np.add.at(cnt, (u, b), 1)
        return cnt.astype(np.float64) / cnt.sum(axis=1).astype(np.float64)[:, None]


def user_ie_profile(uid, iid, feedback, timewindow, n_bins=100, weighted=False, variant=None):
    """(users raw by inner id, items raw, item_bin int32 by inner item id, profile)."""
    st = S.statistics_numpy(list(uid), list(iid), feedback, timewindow)
    u, users = S.first_appearance(list(uid))
    i, items = S.first_appearance(list(iid))
    item_bin = E.mark_n(st["ie"], n_bins, E.tie_rank_of(items))
    return users, items, item_bin, profile(u, i, feedback, item_bin, len(users), n_bins, weighted, variant)


def vector_of(item_vectors, raw):
    """The vector of a raw id, or None: the key itself, else its str (the keys of a KeyedVectors)."""
    for key in (raw, str(raw)):
        try:
            if key in item_vectors:
                return np.asarray(item_vectors[key], dtype=np.float32)
        except TypeError:
            pass
    return None


def features(users, prof, uid, iid, feedback, item_vectors=None):
    """(X fp64, y fp64, kept row numbers)."""
    pos = {r: k for k, r in enumerate(users)}
    fb = np.asarray(feedback, dtype=np.float64)
    X, kept = [], []
    for k, (ru, ri) in enumerate(zip(uid, iid)):
        if item_vectors is None:
            tail = np.array([float(int(ri))])
        else:
            tail = vector_of(item_vectors, ri)
            if tail is None:
                continue
            tail = tail.astype(np.float64)
        X.append(np.concatenate([prof[pos[ru]], tail]))
        kept.append(k)
    kept = np.array(kept, dtype=np.int64)
    width = prof.shape[1] + (1 if item_vectors is None else len(next(iter(_values(item_vectors)))))
    return (np.array(X, dtype=np.float64).reshape(len(kept), width), fb[kept], kept)


def _values(item_vectors):
    if hasattr(item_vectors, "values"):
        return item_vectors.values()
    return item_vectors.vectors


def canon(a):
    return S.canon(a)


CASES = ("ml3000", "ml20000", "dup3000", "seg3000")
C_Z = 100 * 1.89e-14          # the bound tests/test_eccstats_host.py holds the statistics to, relative to the column's largest magnitude
_cases, _restated = {}, {}


class Case:
    """A recorded case of tests/golden/consistency/<name>.npz (tests/golden/make_consistency_golden.py): the rows (raw ids
    as the decimal strings the reference's frame holds) and what the reference's septile_for_plot returned."""

    def __init__(self, golden_dir, name):
        import os
        z = np.load(os.path.join(golden_dir, "consistency", name + ".npz"))
        self.name, self._z = name, z
        self.uid, self.iid = [str(x) for x in z["uid"]], [str(x) for x in z["id"]]
        self.feedback, self.timewindow = z["feedback"], z["timewindow"]
        self.first, self.second = (tuple(None if v < 0 else int(v) for v in z[k]) for k in ("first", "second"))
        self.prefix, self.seg_point, self.seed = str(z["prefix"]), int(z["seg_point"]), int(z["seed"])

    def frame(self, kind):
        """(int64[rows][4]: bin1, bin2, count, count_sum; ratio fp64[rows]) as the reference returned them."""
        return self._z[kind + "_frame"], self._z[kind + "_ratio"]

    def joined(self, kind):
        """{raw id: (value 1, value 2, bin 1, bin 2)} of the reference's joined frame."""
        z = self._z
        cols = [z[kind + s].tolist() for s in ("_v1", "_v2", "_bins1", "_bins2")]
        return dict(zip([str(v) for v in z[kind + "_ids"]], zip(*cols)))

    def check_conditions(self, n=7):
        """What the generator asserted: at least 3 n joined, every septile border wider than the bound."""
        for kind in KINDS:
            for col in ("_v1", "_v2"):
                v = np.sort(self._z[kind + col])
                repeat = len(v) // n
                assert repeat >= 3 and np.isfinite(v).all(), (self.name, kind)
                bound = C_Z * float(np.abs(v).max())
                assert all(v[k * repeat] - v[k * repeat - 1] > bound for k in range(1, n)), (self.name, kind, col)


def case(golden_dir, name):
    if name not in _cases:
        _cases[name] = Case(golden_dir, name)
        _cases[name].check_conditions()
    return _cases[name]


def restated(golden_dir, name):
    """transitions() of a recorded case, computed once and shared."""
    if name not in _restated:
        c = case(golden_dir, name)
        _restated[name] = transitions(c.uid, c.iid, c.feedback, c.timewindow, c.first, c.second)
    return _restated[name]


def same_table(got, want):
    """got: an object or dict with ids, bins1, bins2, count, count_sum, ratio; exact, NaN positions included."""
    g = got if isinstance(got, dict) else vars(got)
    assert list(g["ids"]) == list(want["ids"])
    for k in ("bins1", "bins2", "count", "count_sum"):
        assert np.array_equal(np.asarray(g[k]), np.asarray(want[k])), k
    for k in ("v1", "v2", "ratio"):
        assert canon(np.asarray(g[k], dtype=np.float64)) == canon(want[k]), k
    return True


# ---- the case tables the host and the GPU tests share -----------------------------------------------------------------

def crosstab_cases():
    """{name: (bins1, bins2, n)}: one cell, a diagonal, an empty bins1 row, several workgroups, every n that takes another
    path (n <= 64: one stripe; 65, 100, 256: stripes of 63, 40 and 16 values of bins1)."""
    rs = np.random.RandomState(11)
    cases = {}
    for n in (1, 2, 7, 10, 64, 65, 100, 256):
        m = 40000 if n in (7, 256) else 3000                             # 40000: three workgroups
        cases["random_n%d" % n] = (rs.randint(1, n + 1, m), rs.randint(1, n + 1, m), n)
        cases["onecell_n%d" % n] = (np.full(20000, n), np.full(20000, max(n - 1, 1)), n)
        cases["diagonal_n%d" % n] = (np.arange(5 * n) % n + 1, np.arange(5 * n) % n + 1, n)
    b1 = rs.randint(1, 8, 500)
    b1[b1 == 3] = 4                                                      # nobody in bin 3 of the first column
    cases["emptyrow_n7"] = (b1, rs.randint(1, 8, 500), 7)
    cases["skewed_n7"] = (np.minimum(rs.randint(1, 12, 2000), 7), rs.randint(1, 8, 2000), 7)      # row sums != column sums
    cases["empty_n7"] = (np.zeros(0, np.int64), np.zeros(0, np.int64), 7)
    return {k: (np.asarray(a, np.int32), np.asarray(b, np.int32), n) for k, (a, b, n) in cases.items()}


def join_cases(tile, n=7, min_count=4):
    """{name: (v1, v2, c1, c2, min_count)}."""
    rs = np.random.RandomState(12)
    cases = {}
    for m in sorted({0, 1, n - 1, n, n + 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 5}):
        c1, c2 = rs.randint(0, 9, m), rs.randint(0, 9, m)
        cases["m%d" % m] = (rs.normal(size=m), rs.normal(size=m), c1, c2, min_count)
    m = 300
    half = np.arange(m) < m // 2
    cases["disjoint"] = (rs.normal(size=m), rs.normal(size=m), np.where(half, 9, 0), np.where(half, 0, 9), min_count)
    cases["all"] = (rs.normal(size=m), rs.normal(size=m), np.full(m, 9), np.full(m, 9), min_count)
    edge = np.array([min_count, min_count + 1, min_count + 1, min_count, 0, min_count + 1])
    other = np.array([min_count + 1, min_count + 1, min_count, min_count, min_count + 1, 0])
    cases["support_edge"] = (np.arange(6.0), -np.arange(6.0), edge, other, min_count)
    special = np.array([np.nan, -0.0, np.inf, -np.inf, 1e-310, 0.0])
    cases["special_values"] = (special, special[::-1].copy(), np.full(6, 7), np.full(6, 7), 0)
    return {k: (np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.int64), np.asarray(d, np.int64), mc)
            for k, (a, b, c, d, mc) in cases.items()}


def profile_cases():
    """{name: (user, item, feedback, item_bin, n_users, n_bins)}: users with 0, 1, 63, 64, 65 and 1000 binned rows, items
    of bin 0, feedback whose sum depends on the order (1e16 and 1.0 next to each other)."""
    rs = np.random.RandomState(13)
    cases = {}
    for n_bins in (1, 100, 256):
        n_items = 400
        item_bin = rs.randint(1, n_bins + 1, n_items)
        item_bin[:3] = 0                                                 # items 0 .. 2: no bin
        lens = [0, 1, 63, 64, 65, 1000, 0, 0, 130]                       # binned rows per user
        user = np.repeat(np.arange(len(lens)), lens)
        item = rs.randint(3, n_items, len(user))
        skipped = np.repeat([3, 5, 6, 8], [4, 7, 5, 2])                  # rows of unbinned items on top; user 6 has only such
        user, item = np.concatenate([user, skipped]), np.concatenate([item, rs.randint(0, 3, len(skipped))])
        fb = rs.choice([1e16, 1.0, -1e16, 0.1, 3.0], size=len(user))
        order = rs.permutation(len(user))                                # file order mixes the users
        cases["bins%d" % n_bins] = (user[order], item[order], fb[order], item_bin, len(lens), n_bins)
    return {k: (np.asarray(u, np.int64), np.asarray(i, np.int64), np.asarray(f, np.float64), np.asarray(b, np.int32), nu, nb)
            for k, (u, i, f, b, nu, nb) in cases.items()}
