"""Eccentricity split on the device: ue -> n equal bins of users -> one bipartite user-item graph per bin plus one for
everybody (csrc/n2v_eccsplit.hip, C-ABI include/n2v_sim.h).

Reference: src/utils.py:305-312 (mark_n), :382-405 (split_and_save_edgelist, save_edgelist), src/main_ecc.py:112-117,
and the read-back of every file by src/main.py:66-80.  Here the rows never become text: the bins and the n + 1 CSR
graphs are built on the device and each graph is downloaded once.  Files are the optional path (Split.write).

    bin     users sorted ascending by ue, rank r (0-based), repeat = n_users // n:
            bin = n if repeat == 0 else min(r // repeat + 1, n); the last bin takes the remainder
    ties    the sort is stable over ascending raw uid as Python's sorted orders the ids (strings lexicographically,
            the order of the reference's df_ue); the reference's own quicksort leaves ties unpinned.  -0.0 ties with
            +0.0; NaN sorts after +inf
    names   user: int(raw uid); item: int('9999999' + raw id)
    graph   graph 0: every row; graph k: the rows whose user is in bin k, in file order.  It is the graph
            csr.from_edges(user name, item name, feedback, directed=False) builds: a repeated (uid, id) row keeps its
            LAST weight, w is always an array.  A bin without users is csr.from_edges([], [], []).
    text    "%d %d %s" % (user name, item name, str(float(feedback))) per row, joined by "\\n", no trailing newline

The sorts are torch calls; everything between them is HIP.  Two host readbacks per graph (node count, pair count).
There is no CPU fallback.
"""
import os
import re

import numpy as np
import torch

from . import _lib
from . import csr as _csr
from . import eccstats as _eccstats

ITEM_PREFIX = "9999999"
LIMIT = 2 ** 31 - 1
NONE = 2 ** 63 - 1          # N2V_ECCSPLIT_NONE
_UID = re.compile(r"[+-]?[0-9]+\Z")
_IID = re.compile(r"[0-9]+\Z")
# every sort and every download of a graph goes through these two names (tools/eccsplit_probe.py times them apart)
_sort = torch.sort
_download = lambda t: t.cpu().numpy()


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("n2v_hip.eccsplit: no GPU visible (torch.cuda.is_available() is False); no CPU fallback")


# ---- host checks (every ValueError comes before any launch) -----------------------------------------------------------

def _digits(raw, pattern, what):
    if isinstance(raw, (bool, np.bool_)):
        raise ValueError("eccsplit: %s %r is not an integer" % (what, raw))
    if isinstance(raw, (int, np.integer)):
        s = str(int(raw))
    elif isinstance(raw, (str, np.str_)):
        s = str(raw)
    else:
        raise ValueError("eccsplit: %s %r is not an integer" % (what, raw))
    if not pattern.match(s):
        raise ValueError("eccsplit: %s %r is not an integer" % (what, raw))
    return s


def user_name(raw):
    """int(raw uid); ValueError unless it is an integer that fits int64."""
    v = int(_digits(raw, _UID, "uid"))
    if not -2 ** 63 <= v < 2 ** 63:
        raise ValueError("eccsplit: uid %r does not fit int64" % (raw,))
    return v


def item_name(raw):
    """int('9999999' + raw id); ValueError unless the id is a run of digits and the result fits int64."""
    v = int(ITEM_PREFIX + _digits(raw, _IID, "id"))
    if v >= 2 ** 63:
        raise ValueError("eccsplit: item %r: %d does not fit int64" % (raw, v))
    return v


def names_of(users, items):
    """(user names int64[n_users], item names int64[n_items]) of raw ids; ValueError for a name both sides share (the
    reference would merge the two nodes)."""
    un = np.array([user_name(r) for r in users], dtype=np.int64)
    it = np.array([item_name(r) for r in items], dtype=np.int64)
    _check_names(un, it)
    return un, it


def _check_names(un, it):
    for side, a in (("user", un), ("item", it)):
        if len(np.unique(a)) != len(a):
            raise ValueError("eccsplit: two %ss share one name" % side)
    both = np.intersect1d(un, it)
    if len(both):
        raise ValueError("eccsplit: %d is the name of a user and of an item" % int(both[0]))


def tie_rank_of(users):
    """tie_rank[u] = position of raw uid users[u] in sorted(users): the order of the reference's df_ue."""
    order = sorted(range(len(users)), key=users.__getitem__)
    rank = np.empty(len(users), dtype=np.int64)
    rank[order] = np.arange(len(users), dtype=np.int64)
    return rank


def bin_sizes(n_users, n):
    """Users per bin 1 .. n (host arithmetic; what tells an empty bin without asking the device)."""
    repeat = n_users // n
    if repeat == 0:
        return [0] * (n - 1) + [n_users]
    return [repeat] * (n - 1) + [n_users - repeat * (n - 1)]


def _check_mark(n_users, n, tie_rank):
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= LIMIT:
        raise ValueError("eccsplit: n = %r bins, expected an integer in 1 .. 2^31 - 1" % (n,))
    if not 1 <= n_users <= LIMIT:
        raise ValueError("eccsplit: %d users, expected 1 .. 2^31 - 1" % n_users)
    if tie_rank is None:
        return np.arange(n_users, dtype=np.int64)
    tr = np.asarray(tie_rank)
    if tr.dtype.kind not in "iu" or tr.shape != (n_users,) or not np.array_equal(np.sort(tr), np.arange(n_users)):
        raise ValueError("eccsplit: tie_rank must be a permutation of 0 .. n_users - 1")
    return tr.astype(np.int64)


# ---- C-ABI wrappers (device tensors in, device tensors out) -----------------------------------------------------------

def _mark_device(ue_dev, n, tie_rank_host):
    """int32[n_users] device: the bin of every user."""
    lib = _lib.load()
    dev, n_users = ue_dev.device, ue_dev.numel()
    with torch.cuda.device(dev):
        order0 = torch.from_numpy(np.argsort(tie_rank_host, kind="stable")).to(dev)      # users in tie order
        key = torch.empty(n_users, dtype=torch.int64, device=dev)
        _lib.check(lib.n2v_eccsplit_sort_key(_lib.ptr(ue_dev), n_users, _lib.ptr(key), _lib.stream_ptr(dev)))
        perm = _sort(key[order0], stable=True)[1]
        order = order0[perm].contiguous()
        bins = torch.empty(n_users, dtype=torch.int32, device=dev)
        _lib.check(lib.n2v_eccsplit_mark(_lib.ptr(order), n_users, int(n), _lib.ptr(bins), _lib.stream_ptr(dev)))
    return bins


def mark_n(ue, n, tie_rank=None, device="cuda:0"):
    """Bins (int32 numpy, 1 .. n) of users with eccentricity ue[u].  tie_rank: a permutation, the order among equal ue
    (None: the index)."""
    ue = np.ascontiguousarray(ue, dtype=np.float64).reshape(-1)
    tr = _check_mark(len(ue), n, tie_rank)
    _require_gpu()
    dev = torch.device(device)
    return _mark_device(torch.from_numpy(ue).to(dev), int(n), tr).cpu().numpy()


def _select(user, bins, which, counts):
    """rows int64[n_rows] device, ascending, the first counts[0] of them valid; counts[0] is written on the device."""
    lib = _lib.load()
    dev, n_rows = user.device, user.numel()
    scratch = torch.empty(int(lib.n2v_eccsplit_scratch(n_rows)), dtype=torch.int64, device=dev)
    rows = torch.empty(n_rows, dtype=torch.int64, device=dev)
    _lib.check(lib.n2v_eccsplit_select(_lib.ptr(user), n_rows, _lib.ptr(bins), bins.numel(), int(which), _lib.ptr(scratch),
                                       _lib.ptr(rows), _lib.ptr(counts), _lib.stream_ptr(dev)))
    return rows


def _empty_graph():
    return _csr.from_edges([], [], [])


def _graph(user, item, w, user_names, item_names, rows, cap, counts):
    """The graph of rows[0 .. counts[0]) (rows None: all).  counts: int64[3] device, [0] = selected rows (already
    there), [1] = nodes, [2] = pairs.  Two readbacks: counts[:2], then counts[2]."""
    lib = _lib.load()
    dev = user.device
    st = _lib.stream_ptr(dev)
    n_rows, n_users, n_items = user.numel(), user_names.numel(), item_names.numel()
    n_all = n_users + n_items
    i64 = lambda m: torch.empty(m, dtype=torch.int64, device=dev)
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)
    first = torch.full((n_all,), NONE, dtype=torch.int64, device=dev)
    _lib.check(lib.n2v_eccsplit_first(_lib.ptr(rows), _lib.ptr(counts), cap, _lib.ptr(user), _lib.ptr(item), n_rows, n_users,
                                      n_items, _lib.ptr(first), st))
    node_name, node_first, slot_of = i64(n_all), i64(n_all), i32(n_all)
    scratch = i64(int(lib.n2v_eccsplit_scratch(n_all)))
    _lib.check(lib.n2v_eccsplit_nodes(_lib.ptr(first), n_users, n_items, _lib.ptr(user_names), _lib.ptr(item_names),
                                      _lib.ptr(scratch), _lib.ptr(node_name), _lib.ptr(node_first), _lib.ptr(slot_of),
                                      _lib.ptr(counts[1:]), st))
    n_sel, n_nodes = counts[:2].tolist()                                  # readback 1
    if n_sel == 0 or n_nodes == 0:
        return _empty_graph()
    if 2 * n_sel > LIMIT:
        raise ValueError("eccsplit: %d rows in one graph, at most 2^30 - 1" % n_sel)
    names, perm_name = _sort(node_name[:n_nodes])
    perm_first = _sort(node_first[:n_nodes])[1]
    rank, start_order = i32(n_nodes), i32(n_nodes)
    _lib.check(lib.n2v_eccsplit_ranks(_lib.ptr(perm_name), _lib.ptr(perm_first), n_nodes, _lib.ptr(rank), _lib.ptr(start_order), st))
    key = i64(n_sel)
    _lib.check(lib.n2v_eccsplit_keys(_lib.ptr(rows), n_sel, _lib.ptr(user), _lib.ptr(item), n_rows, n_users, n_items,
                                     _lib.ptr(slot_of), _lib.ptr(rank), n_nodes, _lib.ptr(key), st))
    key_sorted, perm = _sort(key, stable=True)
    ekey, ew = i64(2 * n_sel), torch.empty(2 * n_sel, dtype=torch.float64, device=dev)
    scratch = i64(int(lib.n2v_eccsplit_scratch(n_sel)))
    _lib.check(lib.n2v_eccsplit_pairs(_lib.ptr(key_sorted), _lib.ptr(perm), n_sel, _lib.ptr(rows), _lib.ptr(w), n_rows, n_nodes,
                                      _lib.ptr(scratch), _lib.ptr(ekey), _lib.ptr(ew), _lib.ptr(counts[2:]), st))
    nnz = 2 * int(counts[2].item())                                       # readback 2
    ekey_sorted, perm_e = _sort(ekey[:nnz])
    row_ptr, col, wout = i64(n_nodes + 1), i32(nnz), torch.empty(nnz, dtype=torch.float64, device=dev)
    _lib.check(lib.n2v_eccsplit_fill(_lib.ptr(ekey_sorted), _lib.ptr(perm_e), nnz, _lib.ptr(ew), n_nodes, _lib.ptr(row_ptr),
                                     _lib.ptr(col), _lib.ptr(wout), st))
    return _csr.CsrGraph(_download(names), _download(row_ptr), _download(col), _download(wout), _download(start_order), False)


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def graph_from_ratings(user, item, w, user_labels, item_labels, rows=None, device="cuda:0"):
    """CsrGraph of the bipartite line list (user_labels[user[k]], item_labels[item[k]], w[k]) for k in rows (ascending
    row numbers; None: every row), as csr.from_edges(..., directed=False) builds it.  user / item: inner ids; the two
    sides must share no label.  Everything is checked on the host before the first launch."""
    u, i = _host(user, np.int64), _host(item, np.int64)
    wv = _host(w, np.float64)
    un, it = _host(user_labels, np.int64), _host(item_labels, np.int64)
    if not len(u) == len(i) == len(wv):
        raise ValueError("graph_from_ratings: %d user, %d item, %d w" % (len(u), len(i), len(wv)))
    if len(u) > LIMIT or len(un) + len(it) > LIMIT:
        raise ValueError("graph_from_ratings: %d rows, %d nodes: at most 2^31 - 1 each" % (len(u), len(un) + len(it)))
    if len(u) and (u.min() < 0 or u.max() >= len(un) or i.min() < 0 or i.max() >= len(it)):
        raise ValueError("graph_from_ratings: an id outside its labels")
    _check_names(un, it)
    r = None
    if rows is not None:
        r = _host(rows, np.int64)
        if len(r) and (r[0] < 0 or r[-1] >= len(u) or np.any(r[1:] <= r[:-1])):
            raise ValueError("graph_from_ratings: rows must ascend inside 0 .. n_rows - 1")
    _require_gpu()
    n_sel = len(u) if r is None else len(r)
    if n_sel == 0:
        return _empty_graph()
    dev = torch.device(device)
    to = lambda a: torch.from_numpy(a).to(dev)
    with torch.cuda.device(dev):
        counts = torch.tensor([n_sel, 0, 0], dtype=torch.int64).to(dev)
        return _graph(to(u), to(i), to(wv), to(un), to(it), None if r is None else to(r), n_sel, counts)


# ---- the split ----------------------------------------------------------------------------------------------------------

def edgelist_text(user_names, item_names, feedback):
    """The reference's file text of rows (src/utils.py:389-396): no trailing newline."""
    return "\n".join("%d %d %s" % (u, i, str(float(f))) for u, i, f in zip(user_names.tolist(), item_names.tolist(), feedback.tolist()))


class Split:
    """bins: {raw uid: bin}; graphs: [all rows, bin 1, .. bin n] (CsrGraph); users / items: raw ids by inner id;
    ue: the eccentricities used, by inner user id."""

    def __init__(self, n, users, items, ue, user_bin, graphs, row_user, row_item, feedback, user_names, item_names):
        self.n, self.users, self.items, self.ue, self.graphs = n, users, items, ue, graphs
        self.user_bin = user_bin
        self.bins = dict(zip(users, user_bin.tolist()))
        self._u, self._i, self._fb, self._un, self._in = row_user, row_item, feedback, user_names, item_names

    def rows_of(self, k):
        """Row numbers of graph k, ascending (0: every row)."""
        if not 0 <= k <= self.n:
            raise ValueError("eccsplit: graph %r, expected 0 .. %d" % (k, self.n))
        return np.arange(len(self._u)) if k == 0 else np.nonzero(self.user_bin[self._u] == k)[0]

    def rows_of_users(self, uids):
        """Row numbers, ascending, of the users named by the raw uids given (compared as user_name does: by integer
        value; a uid the split does not know selects nothing)."""
        sel = np.isin(self._un, np.array([user_name(r) for r in uids], dtype=np.int64))
        return np.nonzero(sel[self._u])[0]

    def edgelist_text(self, k=None, rows=None):
        """The reference's file text of graph k, or of the given row numbers."""
        r = self.rows_of(k) if rows is None else np.asarray(rows, dtype=np.int64)
        return edgelist_text(self._un[self._u[r]], self._in[self._i[r]], self._fb[r])

    def graph_of_rows(self, rows, device="cuda:0"):
        """The CsrGraph of the given row numbers (ascending), as graph_from_ratings builds it."""
        return graph_from_ratings(self._u, self._i, self._fb, self._un, self._in, rows=rows, device=device)

    def file_names(self, prefix=""):
        return [prefix + "ue.edgelist"] + [prefix + "ue_%d.edgelist" % k for k in range(1, self.n + 1)]

    def write(self, directory, prefix=""):
        """<prefix>ue.edgelist and <prefix>ue_1.edgelist .. ue_n.edgelist, the reference's bytes; returns the paths."""
        os.makedirs(directory, exist_ok=True)
        paths = [os.path.join(directory, f) for f in self.file_names(prefix)]
        for k, path in enumerate(paths):
            with open(path, "w") as f:
                f.write(self.edgelist_text(k))
        return paths


def _ue_array(ue, users):
    if hasattr(ue, "keys"):
        try:
            return np.array([ue[r] for r in users], dtype=np.float64)
        except KeyError as e:
            raise ValueError("eccsplit: no ue for uid %r" % (e.args[0],))
    a = np.ascontiguousarray(ue, dtype=np.float64).reshape(-1)
    if len(a) != len(users):
        raise ValueError("eccsplit: %d ue for %d users (give them in order of first appearance, or a dict)" % (len(a), len(users)))
    return a


def split(uid, id, feedback, timewindow=None, ue=None, n=10, device="cuda:0"):
    """Rows (uid[k], id[k], feedback[k]) -> Split.  ue: {raw uid: eccentricity} or an array over the users in order of
    first appearance; None: eccstats.item_statistics over the rows, which needs timewindow."""
    fb = np.ascontiguousarray(feedback, dtype=np.float64).reshape(-1)
    if not len(uid) == len(id) == len(fb) or len(fb) == 0:
        raise ValueError("eccsplit: %d uid, %d id, %d feedback" % (len(uid), len(id), len(fb)))
    if len(fb) > LIMIT // 2:
        raise ValueError("eccsplit: %d rows, at most 2^30 - 1" % len(fb))
    if ue is None and timewindow is None:
        raise ValueError("eccsplit: without ue the timewindow of every row is needed")
    u, users = _eccstats.first_appearance(uid)
    i, items = _eccstats.first_appearance(id)
    un, it = names_of(users, items)
    tr = _check_mark(len(users), n, tie_rank_of(users))
    n = int(n)
    ue_host = None if ue is None else _ue_array(ue, users)
    _require_gpu()
    if ue_host is None:
        stats = _eccstats.item_statistics(uid, id, fb, timewindow, device=device)
        assert stats.users == users
        ue_host = stats.ue
    dev = torch.device(device)
    to = lambda a: torch.from_numpy(a).to(dev)
    sizes = [len(users)] + bin_sizes(len(users), n)
    with torch.cuda.device(dev):
        du, di, dw, dun, dit = to(u), to(i), to(fb), to(un), to(it)
        bins = _mark_device(to(ue_host), n, tr)
        graphs = []
        for k in range(n + 1):
            if sizes[k] == 0:                                             # a bin without users: nothing is launched
                graphs.append(_empty_graph())
                continue
            counts = torch.zeros(3, dtype=torch.int64, device=dev)
            rows = _select(du, bins, k, counts)
            graphs.append(_graph(du, di, dw, dun, dit, rows, len(fb), counts))
        user_bin = bins.cpu().numpy()
    return Split(n, users, items, ue_host, user_bin, graphs, u, i, fb, un, it)
