"""The eccentricity split restated in numpy: what n2v_hip.eccsplit and csrc/n2v_eccsplit.hip are held to.

Reference: src/utils.py:305-312 (mark_n), :382-405 (split_and_save_edgelist, save_edgelist).  Graphs are not restated
here: csr.from_edges (held to networkx by tests/test_host_logic.py) over a bin's rows in file order is the yardstick.

    sort_key       the order of ue: ascending, -0.0 == +0.0, every NaN after +inf (pandas na_position='last')
    sort_order     users at rank 0, 1, ..: the stable sort by (ue, tie rank); the reference's quicksort leaves ties
                   unpinned, the stated rule is ascending raw uid as Python's sorted orders the ids (the order of df_ue)
    mark_literal   the array construction of :308-310, element for element
    mark_n         the same in closed form: bin = n if repeat == 0 else min(r // repeat + 1, n)
    rows_of_bin    the rows whose user is in the bin, in file order (:386-387); bin 0: every row
    names          int(raw uid), int('9999999' + raw id) (:392)
    text           "\\n".join("%d %d %s"), the weight as str(float) (:393-396); no trailing newline
"""
import math

import numpy as np

ITEM_PREFIX = "9999999"
INT64_MAX = np.int64(2 ** 63 - 1)


def sort_key(ue):
    """int64 keys that order as the rule orders ue (the bit trick the device uses, stated on the host)."""
    ue = np.ascontiguousarray(ue, dtype=np.float64)
    b = ue.view(np.int64)
    key = np.where(b >= 0, b, b ^ INT64_MAX)
    key = np.where(ue == 0.0, np.int64(0), key)
    return np.where(np.isnan(ue), INT64_MAX, key)


def tie_rank_of(users):
    order = sorted(range(len(users)), key=users.__getitem__)
    rank = np.empty(len(users), dtype=np.int64)
    rank[order] = np.arange(len(users))
    return rank


def sort_order(ue, tie_rank=None):
    """order[r] = the user at rank r."""
    ue = np.asarray(ue, dtype=np.float64)
    tr = np.arange(len(ue)) if tie_rank is None else np.asarray(tie_rank)
    order0 = np.argsort(tr, kind="stable")
    return order0[np.argsort(sort_key(ue[order0]), kind="stable")]


def sort_order_python(ue, tie_rank=None):
    """The same by Python's own stable sort and float comparisons: no bit tricks."""
    tr = list(range(len(ue))) if tie_rank is None else list(tie_rank)
    order0 = sorted(range(len(ue)), key=tr.__getitem__)
    nan_last = sorted(order0, key=lambda u: math.isnan(ue[u]))                   # stable: NaN after the rest
    import functools
    def cmp(a, b):
        x, y = ue[a], ue[b]
        if math.isnan(x) or math.isnan(y):
            return 0
        return -1 if x < y else (1 if x > y else 0)                               # -0.0 == 0.0
    return np.array(sorted(nan_last, key=functools.cmp_to_key(cmp)), dtype=np.int64)


def mark_literal(n_users, n):
    """ue_n by rank, as :308-310 build it."""
    repeat = int(math.floor(n_users / n))
    array = [i for i in range(1, n + 1) for _ in range(repeat)]
    array = array + [n for i in range(n_users - len(array))]
    return np.array(array, dtype=np.int64)


def mark_by_rank(n_users, n):
    r = np.arange(n_users, dtype=np.int64)
    repeat = n_users // n
    if repeat == 0:
        return np.full(n_users, n, dtype=np.int64)
    return np.minimum(r // repeat + 1, n)


def mark_n(ue, n, tie_rank=None):
    """bin[u], int32 in 1 .. n."""
    order = sort_order(ue, tie_rank)
    bins = np.empty(len(order), dtype=np.int32)
    bins[order] = mark_by_rank(len(order), n)
    return bins


def rows_of_bin(user, bins, which):
    user = np.asarray(user)
    return np.arange(len(user)) if which == 0 else np.nonzero(np.asarray(bins)[user] == which)[0]


def user_name(raw):
    return int(raw)


def item_name(raw):
    return int(ITEM_PREFIX + str(raw))


def text(user_names, item_names, feedback):
    return "\n".join("%d %d %s" % (int(u), int(i), str(float(f))) for u, i, f in zip(user_names, item_names, feedback))


def first_appearance(raw):
    raw = np.asarray(raw)
    uniq, first, inv = np.unique(raw, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    return rank[inv.reshape(-1)], uniq[order].tolist()


def split(uid, iid, feedback, ue_by_user, n):
    """(bins by inner user id, users, [text of graph 0 .. n], [(src, dst, w) of graph 0 .. n]) for raw ids that are
    ints or decimal strings (ties follow sorted() of whichever they are); ue_by_user: ue in order of first appearance."""
    u, users = first_appearance(uid)
    i, items = first_appearance(iid)
    un = np.array([user_name(r) for r in users], dtype=np.int64)
    it = np.array([item_name(r) for r in items], dtype=np.int64)
    fb = np.asarray(feedback, dtype=np.float64)
    bins = mark_n(ue_by_user, n, tie_rank_of(users))
    texts, edges = [], []
    for k in range(n + 1):
        r = rows_of_bin(u, bins, k)
        texts.append(text(un[u[r]], it[i[r]], fb[r]))
        edges.append((un[u[r]], it[i[r]], fb[r]))
    return bins, users, texts, edges


def wbytes(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def same_graph(a, b):
    """Exact: integers by value, weights by their bytes."""
    assert np.array_equal(a.labels, b.labels)
    assert np.array_equal(a.row_ptr, b.row_ptr)
    assert np.array_equal(a.col, b.col)
    assert np.array_equal(a.start_order, b.start_order)
    assert (a.w is None) == (b.w is None)
    if a.w is not None:
        assert a.w.dtype == np.float64 and wbytes(a.w) == wbytes(b.w)
    assert a.directed == b.directed and a.n_nodes == b.n_nodes and a.nnz == b.nnz
    return True


class Case:
    """A recorded case: the rows of tests/golden/eccstats/<name>.npz (raw ids as the decimal strings the reference's
    frame holds) and the reference's bins and files from tests/golden/eccsplit/<name>.npz."""

    def __init__(self, golden_dir, name):
        import os
        z = np.load(os.path.join(golden_dir, "eccstats", name + ".npz"))
        s = np.load(os.path.join(golden_dir, "eccsplit", name + ".npz"))
        self.name = name
        self.uid, self.iid = [str(x) for x in z["uid"]], [str(x) for x in z["id"]]
        self.feedback, self.timewindow = z["feedback"], z["timewindow"]
        self.ue_uid = [str(x) for x in s["ue_uid"]]                       # df_ue's order: ascending uid string
        self.ue = dict(zip(self.ue_uid, s["ue"].tolist()))
        self.ns = [int(x) for x in s["ns"]]
        self._s = s

    def bins(self, n):
        """{raw uid: recorded bin}"""
        return dict(zip(self.ue_uid, self._s["bins_%d" % n].tolist()))

    def files(self, n):
        """[bytes of ue.edgelist, ue_1.edgelist, .. ue_n.edgelist]"""
        blob, off = self._s["files_%d" % n].tobytes(), self._s["files_%d_off" % n]
        return [self._s["file_all"].tobytes()] + [blob[off[k]:off[k + 1]] for k in range(n)]
