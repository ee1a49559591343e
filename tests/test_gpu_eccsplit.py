"""GPU tests: the eccentricity-split kernels (csrc/n2v_eccsplit.hip, C-ABI include/n2v_sim.h) against the restatement
tests/eccsplit_reference.py, through the C-ABI unless a test says otherwise.

Exact comparisons only: integers with array_equal, weights by their bytes.  Every output buffer starts as a sentinel and
what lies past the written part must still hold it.  The graphs are held to csr.from_edges over the same rows (which
tests/test_host_logic.py holds to networkx and tests/test_eccsplit_host.py to the files the reference wrote); bins and
file bytes to the recording tests/golden/eccsplit/*.npz.  The sorts are torch calls, as in n2v_hip.eccsplit.

Malformed input is tested in tests/test_eccsplit_host.py, at the wrapper: no kernel here is handed a bad index."""
import math
import os

import numpy as np
import pytest

import eccsplit_reference as R

pytestmark = pytest.mark.gpu

SENT = -12345.5
ISENT = -7
NONE = 2 ** 63 - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = R.Case(GOLDEN, name)
    return _cases[name]


def _L():
    from n2v_hip import _lib as L
    return L


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _full(n, value, dtype):
    import torch
    return torch.full((n,), value, dtype=dtype, device="cuda")


def tile():
    return int(_L().load().n2v_eccsplit_tile())


# ---- C-ABI drivers -------------------------------------------------------------------------------------------------------

def c_sort_key(ue):
    import torch
    L = _L(); lib = L.load()
    d = _dev(ue, np.float64)
    key = _full(len(ue), ISENT, torch.int64)
    L.check(lib.n2v_eccsplit_sort_key(L.ptr(d), len(ue), L.ptr(key), L.stream_ptr(d.device)))
    return key


def c_mark(ue, n, tie_rank=None):
    import torch
    L = _L(); lib = L.load()
    n_users = len(ue)
    tr = np.arange(n_users) if tie_rank is None else np.asarray(tie_rank)
    order0 = _dev(np.argsort(tr, kind="stable"), np.int64)
    key = c_sort_key(ue)
    order = order0[torch.sort(key[order0], stable=True)[1]].contiguous()
    bins = _full(n_users + 3, ISENT, torch.int32)
    L.check(lib.n2v_eccsplit_mark(L.ptr(order), n_users, n, L.ptr(bins), L.stream_ptr(bins.device)))
    out = bins.cpu().numpy()
    assert (out[n_users:] == ISENT).all()
    return out[:n_users]


def c_select(user, bins, which, pad=0):
    """pad: sentinel words kept behind the scratch the call is told about; they must come back untouched."""
    import torch
    L = _L(); lib = L.load()
    du, db = _dev(user, np.int64), _dev(bins, np.int32)
    n_rows = len(user)
    n_scratch = int(lib.n2v_eccsplit_scratch(n_rows))
    scratch = _full(n_scratch + pad, ISENT, torch.int64)
    rows, count = _full(n_rows, ISENT, torch.int64), _full(1, ISENT, torch.int64)
    L.check(lib.n2v_eccsplit_select(L.ptr(du), n_rows, L.ptr(db), len(bins), which, L.ptr(scratch), L.ptr(rows), L.ptr(count),
                                    L.stream_ptr(du.device)))
    c = int(count.item())
    assert (scratch[n_scratch:] == ISENT).all()
    rows = rows.cpu().numpy()
    assert 0 <= c <= n_rows and (rows[c:] == ISENT).all()
    return rows[:c]


def c_first(user, item, n_users, n_items, rows=None, n_sel=None):
    import torch
    L = _L(); lib = L.load()
    du, di = _dev(user, np.int64), _dev(item, np.int64)
    first = _full(n_users + n_items, NONE, torch.int64)
    drows = None if rows is None else _dev(rows, np.int64)
    dn = None if n_sel is None else _dev([n_sel], np.int64)
    cap = len(user) if rows is None else len(rows)
    L.check(lib.n2v_eccsplit_first(L.ptr(drows), L.ptr(dn), cap, L.ptr(du), L.ptr(di), len(user), n_users, n_items, L.ptr(first),
                                   L.stream_ptr(du.device)))
    return first.cpu().numpy()


def first_numpy(user, item, n_users, n_items, rows=None):
    first = np.full(n_users + n_items, NONE, dtype=np.int64)
    k = np.arange(len(user)) if rows is None else np.asarray(rows, dtype=np.int64)
    np.minimum.at(first, user[k], 2 * k)
    np.minimum.at(first, n_users + item[k], 2 * k + 1)
    return first


def c_nodes(first, user_names, item_names):
    import torch
    L = _L(); lib = L.load()
    n_users, n_items = len(user_names), len(item_names)
    n_all = n_users + n_items
    df, dun, dit = _dev(first, np.int64), _dev(user_names, np.int64), _dev(item_names, np.int64)
    scratch = _full(int(lib.n2v_eccsplit_scratch(n_all)), ISENT, torch.int64)
    name, nfirst, slot_of = _full(n_all, ISENT, torch.int64), _full(n_all, ISENT, torch.int64), _full(n_all, ISENT, torch.int32)
    count = _full(1, ISENT, torch.int64)
    L.check(lib.n2v_eccsplit_nodes(L.ptr(df), n_users, n_items, L.ptr(dun), L.ptr(dit), L.ptr(scratch), L.ptr(name), L.ptr(nfirst),
                                   L.ptr(slot_of), L.ptr(count), L.stream_ptr(df.device)))
    c = int(count.item())
    name, nfirst = name.cpu().numpy(), nfirst.cpu().numpy()
    assert (name[c:] == ISENT).all() and (nfirst[c:] == ISENT).all()
    return name[:c], nfirst[:c], slot_of.cpu().numpy()


def nodes_numpy(first, user_names, item_names):
    seen = np.nonzero(first != NONE)[0]
    names = np.concatenate([user_names, item_names]).astype(np.int64)
    slot_of = np.full(len(first), -1, dtype=np.int32)
    slot_of[seen] = np.arange(len(seen))
    return names[seen], first[seen], slot_of


def c_pairs(key, w, n_nodes, rows=None, n_rows=None):
    """key: unsorted, one per selected row; w: by ROW.  Returns (ekey, ew) of the 2 * pairs entries."""
    import torch
    L = _L(); lib = L.load()
    n_sel = len(key)
    n_rows = n_sel if n_rows is None else n_rows
    key_sorted, perm = torch.sort(_dev(key, np.int64), stable=True)
    dw = _dev(w, np.float64)
    drows = None if rows is None else _dev(rows, np.int64)
    scratch = _full(int(lib.n2v_eccsplit_scratch(n_sel)), ISENT, torch.int64)
    ekey, ew, count = _full(2 * n_sel, ISENT, torch.int64), _full(2 * n_sel, SENT, torch.float64), _full(1, ISENT, torch.int64)
    L.check(lib.n2v_eccsplit_pairs(L.ptr(key_sorted), L.ptr(perm), n_sel, L.ptr(drows), L.ptr(dw), n_rows, n_nodes, L.ptr(scratch),
                                   L.ptr(ekey), L.ptr(ew), L.ptr(count), L.stream_ptr(dw.device)))
    p = int(count.item())
    ekey, ew = ekey.cpu().numpy(), ew.cpu().numpy()
    assert (ekey[2 * p:] == ISENT).all() and (ew[2 * p:] == SENT).all()
    return ekey[:2 * p], ew[:2 * p]


def pairs_numpy(key, w, n_nodes, rows=None):
    key = np.asarray(key, dtype=np.int64)
    perm = np.argsort(key, kind="stable")
    ks = key[perm]
    last = np.nonzero(np.append(ks[1:] != ks[:-1], True))[0]
    row = perm[last] if rows is None else np.asarray(rows)[perm[last]]
    a, b = ks[last] // n_nodes, ks[last] % n_nodes
    ekey = np.empty(2 * len(last), dtype=np.int64)
    ekey[0::2], ekey[1::2] = ks[last], b * n_nodes + a
    return ekey, np.repeat(np.asarray(w, dtype=np.float64)[row], 2)


def c_graph(user, item, w, user_names, item_names, rows=None):
    """The whole chain through the C-ABI, every buffer a sentinel first; a CsrGraph."""
    import torch
    from n2v_hip import csr
    L = _L(); lib = L.load()
    n_rows, n_users, n_items = len(user), len(user_names), len(item_names)
    sel = np.arange(n_rows) if rows is None else np.asarray(rows)
    n_sel = len(sel)
    first = c_first(user, item, n_users, n_items, rows=None if rows is None else sel)
    name, nfirst, slot_of = c_nodes(first, user_names, item_names)
    n_nodes = len(name)
    names, perm_name = torch.sort(_dev(name, np.int64))
    perm_first = torch.sort(_dev(nfirst, np.int64))[1]
    rank, start_order = _full(n_nodes + 2, ISENT, torch.int32), _full(n_nodes + 2, ISENT, torch.int32)
    st = L.stream_ptr(names.device)
    L.check(lib.n2v_eccsplit_ranks(L.ptr(perm_name), L.ptr(perm_first), n_nodes, L.ptr(rank), L.ptr(start_order), st))
    assert (rank[n_nodes:] == ISENT).all() and (start_order[n_nodes:] == ISENT).all()
    du, di, dslot = _dev(user, np.int64), _dev(item, np.int64), _dev(slot_of, np.int32)
    drows = None if rows is None else _dev(sel, np.int64)
    key = _full(n_sel + 2, ISENT, torch.int64)
    L.check(lib.n2v_eccsplit_keys(L.ptr(drows), n_sel, L.ptr(du), L.ptr(di), n_rows, n_users, n_items, L.ptr(dslot), L.ptr(rank),
                                  n_nodes, L.ptr(key), st))
    assert (key[n_sel:] == ISENT).all()
    ekey, ew = c_pairs(key[:n_sel].cpu().numpy(), w, n_nodes, rows=None if rows is None else sel, n_rows=n_rows)
    nnz = len(ekey)
    ekey_sorted, perm_e = torch.sort(_dev(ekey, np.int64))
    row_ptr, col, wout = _full(n_nodes + 3, ISENT, torch.int64), _full(nnz + 2, ISENT, torch.int32), _full(nnz + 2, SENT, torch.float64)
    dew = _dev(ew, np.float64)
    L.check(lib.n2v_eccsplit_fill(L.ptr(ekey_sorted), L.ptr(perm_e), nnz, L.ptr(dew), n_nodes, L.ptr(row_ptr), L.ptr(col), L.ptr(wout), st))
    assert (row_ptr[n_nodes + 1:] == ISENT).all() and (col[nnz:] == ISENT).all() and (wout[nnz:] == SENT).all()
    return csr.CsrGraph(names.cpu().numpy(), row_ptr[:n_nodes + 1].cpu().numpy(), col[:nnz].cpu().numpy(), wout[:nnz].cpu().numpy(),
                        start_order[:n_nodes].cpu().numpy(), False)


# ---- mark -------------------------------------------------------------------------------------------------------------------

POOL = np.array([-math.inf, -2.5, -0.0, 0.0, 0.25, 0.25, 1.0, math.inf, math.nan, -math.nan])


def special_ue(rs, n_users):
    """Ties, NaN of both signs, +-inf and +-0.0 among a few plain values."""
    ue = POOL[rs.randint(0, len(POOL), size=n_users)].copy()
    plain = rs.random_sample(n_users) < 0.3
    ue[plain] = rs.normal(size=int(plain.sum()))
    return ue


def test_sort_key_is_the_stated_order():
    ue = np.concatenate([POOL, [5e-324, -5e-324, 1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0]])
    assert np.array_equal(c_sort_key(ue).cpu().numpy(), R.sort_key(ue))


def test_mark_every_size():
    """n_users x n: one bin, repeat == 0 (n > n_users), a remainder in the last bin, n == n_users; ue with ties, NaN,
    +-inf and +-0.0; the tie rank both as the index and as a random permutation."""
    rs = np.random.RandomState(11)
    for n_users in (1, 2, 63, 64, 65, 257):
        for n in (1, 2, 7, n_users, n_users + 1, 1024):
            ue = special_ue(rs, n_users)
            got = c_mark(ue, n)
            assert got.min() >= 1 and got.max() <= n
            assert np.array_equal(got, R.mark_n(ue, n)), (n_users, n)
            tr = rs.permutation(n_users)
            assert np.array_equal(c_mark(ue, n, tr), R.mark_n(ue, n, tr)), (n_users, n)
    assert c_mark(np.arange(10.0), 3).tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 3, 3]       # the remainder goes to the last bin
    assert c_mark(np.zeros(4), 9).tolist() == [9, 9, 9, 9]                             # repeat == 0
    assert c_mark(np.array([0.0, -0.0, 0.0, -0.0]), 2).tolist() == [1, 1, 2, 2]        # a four-way tie keeps the index order


def test_mark_n_wrapper():
    from n2v_hip import eccsplit
    rs = np.random.RandomState(12)
    ue = special_ue(rs, 65)
    tr = rs.permutation(65)
    got = eccsplit.mark_n(ue, 7, tie_rank=tr)
    assert got.dtype == np.int32 and np.array_equal(got, R.mark_n(ue, 7, tr))


# ---- select -----------------------------------------------------------------------------------------------------------------

def test_select_shapes():
    T = tile()
    rs = np.random.RandomState(13)
    n_users = 9
    bins = np.array([1, 2, 3, 1, 2, 3, 5, 5, 1], dtype=np.int32)                      # bin 4: no user at all
    for n_rows in (1, T - 1, T, T + 1, 2 * T + 1):
        k = np.arange(n_rows)
        patterns = {
            "random": rs.randint(0, n_users, size=n_rows),
            "one bin": np.full(n_rows, 7),                                            # every row in bin 5
            "alternating": np.where(k % 2 == 0, 0, 1),                                # bins 1, 2, 1, 2, ..
            "last tile": np.where(k >= (n_rows - 1) // T * T, 2, 0),                  # bin 3 only in the last tile
            "last row": np.where(k == n_rows - 1, 2, 0),
        }
        for what, user in patterns.items():
            for which in (0, 1, 2, 3, 4, 5):
                got = c_select(user, bins, which)
                assert np.array_equal(got, R.rows_of_bin(user, bins, which)), (n_rows, what, which)
        assert len(c_select(patterns["one bin"], bins, 5)) == n_rows and len(c_select(patterns["one bin"], bins, 1)) == 0
        assert len(c_select(patterns["random"], bins, 4)) == 0 and len(c_select(patterns["random"], bins, 0)) == n_rows


# ---- first appearance ---------------------------------------------------------------------------------------------------------

def test_first_appearance():
    T = tile()
    rs = np.random.RandomState(14)
    n_rows, n_users, n_items = 2 * T + 1500, 40, 61
    user = rs.randint(0, n_users - 2, size=n_rows)
    item = rs.randint(0, n_items - 3, size=n_rows)
    item[rs.choice(n_rows - 1, 5000, replace=False)] = n_items - 3      # one item on 5 000 rows
    user[n_rows - 1], item[n_rows - 1] = n_users - 2, n_items - 2    # a user and an item seen only in the last row
    user[user == 5] = 6
    user[3], user[n_rows - 7] = 5, 5                                 # a user in the first and in the last tile only
    assert (item == n_items - 3).sum() >= 5000 and n_rows - 7 >= 2 * T
    want = first_numpy(user, item, n_users, n_items)
    assert want[n_users - 1] == NONE and want[n_users + n_items - 1] == NONE and want[5] == 6 and want[n_users - 2] == 2 * (n_rows - 1)
    assert np.array_equal(c_first(user, item, n_users, n_items), want)
    # a selection: what lies past the device's count is not read (row 0 there would lower two words)
    sel = np.sort(rs.choice(np.arange(1, n_rows), T + 3, replace=False))
    rows = np.concatenate([sel, np.zeros(50, dtype=np.int64)])
    assert np.array_equal(c_first(user, item, n_users, n_items, rows=rows, n_sel=len(sel)), first_numpy(user, item, n_users, n_items, sel))
    assert np.array_equal(c_first(user, item, n_users, n_items, rows=sel), first_numpy(user, item, n_users, n_items, sel))


# ---- nodes ------------------------------------------------------------------------------------------------------------------

def test_nodes():
    T = tile()
    rs = np.random.RandomState(15)
    n_users, n_items = T + 5, 2 * T - 3                              # the compaction crosses tile borders on both sides
    item_names = np.array([R.item_name(i) for i in range(1, n_items + 1)], dtype=np.int64)
    for what, user_names in (("above", 10 ** 17 + rs.permutation(n_users).astype(np.int64)),
                             ("interleaved", R.item_name(1) + 10 + 10 * rs.permutation(n_users).astype(np.int64))):
        assert len(np.intersect1d(user_names, item_names)) == 0
        if what == "above":
            assert user_names.min() > item_names.max()
        else:
            assert item_names.min() < user_names.min() < item_names.max()
        first = np.full(n_users + n_items, NONE, dtype=np.int64)
        seen = rs.random_sample(n_users + n_items) < 0.6
        seen[[0, n_users - 1, n_users, n_users + n_items - 1]] = [True, False, False, True]
        first[seen] = rs.permutation(4 * (n_users + n_items))[:int(seen.sum())]
        got, want = c_nodes(first, user_names, item_names), nodes_numpy(first, user_names, item_names)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), what
    none = c_nodes(np.full(n_users + n_items, NONE, dtype=np.int64), user_names, item_names)
    assert len(none[0]) == 0 and (none[2] == -1).all()


# ---- pairs ------------------------------------------------------------------------------------------------------------------

def test_pairs_last_of_every_run_wins():
    """Runs of 1, 65 and 4 097 equal keys laid across tile borders, the rows in a random order, every weight distinct:
    the weight of the LAST row of a run survives; NaN (with a payload), inf and -0.0 travel by their bytes."""
    T = tile()
    rs = np.random.RandomState(16)
    runs = [1] * (T - 30) + [65] + [1] * 10 + [4097] + [1, 65, 1, 1]
    assert sum(runs[:T - 30]) < T < sum(runs[:T - 29]) and 4097 > 2 * T
    n_nodes = len(runs) + 7
    a = np.arange(len(runs), dtype=np.int64)
    b = (a * 7 + 3) % n_nodes
    key_sorted = np.repeat(a * n_nodes + b, runs)
    n_sel = len(key_sorted)
    shuffle = rs.permutation(n_sel)
    key = key_sorted[shuffle]
    w = rs.permutation(n_sel).astype(np.float64) + 0.5
    # the winners of the three long runs carry the special values
    winners = [int(np.nonzero(key == a[j] * n_nodes + b[j])[0].max()) for j in (T - 30, T - 19, len(runs) - 3)]
    w[winners[0]] = np.frombuffer(np.array([0x7ff8dead0000beef], dtype=np.uint64).tobytes(), dtype=np.float64)[0]
    w[winners[1]], w[winners[2]] = -math.inf, -0.0
    want_key, want_w = pairs_numpy(key, w, n_nodes)
    got_key, got_w = c_pairs(key, w, n_nodes)
    assert len(got_key) == 2 * len(runs) and np.array_equal(got_key, want_key)
    assert got_w.tobytes() == want_w.tobytes()
    assert np.array([0x7ff8dead0000beef], dtype=np.uint64).tobytes() in got_w.tobytes() and np.signbit(got_w[got_w == 0.0]).all()
    # through a row selection: w is by row, rows[perm] picks it
    rows = np.sort(rs.choice(3 * n_sel, n_sel, replace=False))
    w_rows = rs.random_sample(3 * n_sel)
    got_key, got_w = c_pairs(key, w_rows, n_nodes, rows=rows, n_rows=3 * n_sel)
    want_key, want_w = pairs_numpy(key, w_rows, n_nodes, rows=rows)
    assert np.array_equal(got_key, want_key) and got_w.tobytes() == want_w.tobytes()


# ---- graphs -----------------------------------------------------------------------------------------------------------------

def inner(c):
    u, users = R.first_appearance(c.uid)
    i, items = R.first_appearance(c.iid)
    un = np.array([R.user_name(r) for r in users], dtype=np.int64)
    it = np.array([R.item_name(r) for r in items], dtype=np.int64)
    return u, i, un, it, users


def random_rows():
    rs = np.random.RandomState(17)
    u, i = rs.randint(0, 50, size=5000), rs.randint(0, 200, size=5000)
    w = rs.randint(1, 11, size=5000) * 0.5
    w[rs.choice(5000, 40, replace=False)] = [math.nan, math.inf, -0.0, 1.0] * 10
    un = rs.permutation(50).astype(np.int64) * 3 + 10 ** 9                    # between the 9- and the 10-digit item names
    it = np.array([R.item_name(x) for x in rs.permutation(200)], dtype=np.int64)
    assert len(np.intersect1d(un, it)) == 0 and it.min() < un.min() < it.max()
    return u, i, w, un, it, R.mark_n(rs.normal(size=50), 7)


def test_graph_through_the_abi_on_random_rows():
    from n2v_hip import csr
    u, i, w, un, it, bins = random_rows()
    for which in range(8):
        r = R.rows_of_bin(u, bins, which)
        got = c_graph(u, i, w, un, it, rows=None if which == 0 else r)
        assert R.same_graph(got, csr.from_edges(un[u[r]], it[i[r]], w[r], directed=False)), which


def test_graph_from_ratings_on_random_rows():
    from n2v_hip import csr, eccsplit
    u, i, w, un, it, bins = random_rows()
    assert len(set(zip(u.tolist(), i.tolist()))) < 5000                       # repeated pairs: the last weight wins
    for which in range(8):
        r = R.rows_of_bin(u, bins, which)
        got = eccsplit.graph_from_ratings(u, i, w, un, it, rows=None if which == 0 else r)
        assert R.same_graph(got, csr.from_edges(un[u[r]], it[i[r]], w[r], directed=False)), which
        assert got.w is not None


@pytest.mark.parametrize("name", ["dup1500", "tw2500"])
def test_graph_from_ratings_on_recorded_rows(name):
    from n2v_hip import csr, eccsplit
    c = case(name)
    u, i, un, it, users = inner(c)
    fb = np.asarray(c.feedback, np.float64)
    rec = c.bins(3)
    bins = np.array([rec[r] for r in users])
    for which in range(4):
        r = R.rows_of_bin(u, bins, which)
        got = eccsplit.graph_from_ratings(u, i, fb, un, it, rows=None if which == 0 else r)
        assert R.same_graph(got, csr.from_edges(un[u[r]], it[i[r]], fb[r], directed=False)), which


def test_graph_of_one_row_and_of_no_row():
    from n2v_hip import csr, eccsplit
    u, i, w = np.array([1, 0, 1]), np.array([0, 1, 1]), np.array([2.5, 1.0, 1.0])
    un, it = np.array([30, 10]), np.array([20, 99999991])
    one = eccsplit.graph_from_ratings(u, i, w, un, it, rows=[1])
    assert R.same_graph(one, csr.from_edges([30], [99999991], [1.0]))
    assert one.labels.tolist() == [30, 99999991] and one.w.tolist() == [1.0, 1.0] and one.start_order.tolist() == [0, 1]
    assert R.same_graph(eccsplit.graph_from_ratings(u[:1], i[:1], w[:1], un, it), csr.from_edges([10], [20], [2.5]))
    empty = csr.from_edges([], [], [])
    assert R.same_graph(eccsplit.graph_from_ratings(u, i, w, un, it, rows=[]), empty)
    assert R.same_graph(eccsplit.graph_from_ratings([], [], [], un, it), empty)


# ---- end to end -------------------------------------------------------------------------------------------------------------

def check_split(c, s, n):
    from n2v_hip import csr
    assert s.bins == c.bins(n)
    files = c.files(n)
    assert [s.edgelist_text(k).encode() for k in range(n + 1)] == files
    assert len(s.graphs) == n + 1
    u, i, un, it, users = inner(c)
    assert users == s.users
    fb = np.asarray(c.feedback, np.float64)
    for k, g in enumerate(s.graphs):
        r = R.rows_of_bin(u, s.user_bin, k)
        assert (len(r) == 0) == (files[k] == b"")
        assert R.same_graph(g, csr.from_edges(un[u[r]], it[i[r]], fb[r], directed=False)), (n, k)


@pytest.mark.parametrize("name", ["syn3000", "dup1500", "tw2500"])
def test_split_end_to_end_equals_the_recording(name):
    """ue from the device's own statistics (these cases have no two ue closer than 3.3e-6, and the device's ue is within
    3.5e-14 of the reference's, so the bins cannot flip): bins, file bytes and graphs, for every recorded n."""
    from n2v_hip import eccsplit
    c = case(name)
    for n in c.ns:
        check_split(c, eccsplit.split(c.uid, c.iid, c.feedback, c.timewindow, n=n), n)


def test_split_with_the_recorded_ue():
    """syn400 holds an exact tie and a gap of one ulp: only with the recorded ue handed in."""
    from n2v_hip import eccsplit
    c = case("syn400")
    u, users = R.first_appearance(c.uid)
    for n in c.ns:
        check_split(c, eccsplit.split(c.uid, c.iid, c.feedback, ue=c.ue, n=n), n)
    s = eccsplit.split(c.uid, c.iid, c.feedback, ue=[c.ue[r] for r in users], n=3)       # the array form
    check_split(c, s, 3)


# ---- main_ecc ---------------------------------------------------------------------------------------------------------------

def write_csv(path, rows):
    with open(path, "w") as f:
        f.write("uid,id,feedback,timewindow\n")
        for r in rows:
            f.write("%s,%s,%r,%d\n" % r)


def test_main_ecc_writes_the_files_of_the_restatement(tmp_path):
    import main_ecc
    c = case("tw2500")
    rows = list(zip(c.uid, c.iid, c.feedback.tolist(), c.timewindow.tolist()))[:700]
    csv = str(tmp_path / "ratings.csv")
    write_csv(csv, rows)
    out = tmp_path / "graph"
    s = main_ecc.main(main_ecc.parse_args(["-input", csv, "-split-n", "4", "-out", str(out), "-prefix", "tw_", "-window-col", "timewindow",
                                           "-save-bins", str(tmp_path / "bins.csv")]))
    uid, iid, fb = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    bins, users, texts, _ = R.split(uid, iid, fb, s.ue, 4)
    assert users == s.users and s.bins == dict(zip(users, bins.tolist()))
    names = ["tw_ue.edgelist"] + ["tw_ue_%d.edgelist" % k for k in range(1, 5)]
    assert sorted(os.listdir(out)) == sorted(names)
    assert [open(out / f, "rb").read() for f in names] == [t.encode() for t in texts]
    lines = open(tmp_path / "bins.csv").read().splitlines()
    assert len(lines) == len(users) and lines[0] == "%s,%r,%d" % (users[0], float(s.ue[0]), bins[0])


def test_main_ecc_embed(tmp_path):
    import main_ecc
    c = case("tw2500")
    rows = list(zip(c.uid, c.iid, c.feedback.tolist(), c.timewindow.tolist()))[:60]
    csv = str(tmp_path / "ratings.csv")
    write_csv(csv, rows)
    emb = tmp_path / "emb"
    n_users = len(set(r[0] for r in rows))
    s = main_ecc.main(main_ecc.parse_args(["-input", csv, "-split-n", str(n_users + 1), "-embed", str(emb), "-window-col", "timewindow",
                                           "--num-walks", "2", "--walk-length", "10", "--dimensions", "16"]))
    # repeat == 0: only ue.emb and the last bin's file, which hold the same graph
    assert sorted(os.listdir(emb)) == ["ue.emb", "ue_%d.emb" % (n_users + 1)]
    for f, g in (("ue.emb", s.graphs[0]), ("ue_%d.emb" % (n_users + 1), s.graphs[-1])):
        lines = open(emb / f).read().splitlines()
        assert lines[0] == "%d 16" % g.n_nodes and len(lines) == g.n_nodes + 1
        assert sorted(int(x.split()[0]) for x in lines[1:]) == g.labels.tolist()
