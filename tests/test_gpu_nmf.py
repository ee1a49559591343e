"""GPU tests of the NMF kernels (n2v_nmf_lists_check, n2v_nmf_epoch; csrc/n2v_nmf.hip, C-ABI include/n2v_sim.h) against
the restatement tests/nmf_reference.py, through the low-level wrappers nmf.lists / nmf.epoch, then nmf.NMF and the driver.

Exact comparisons only, no tolerance: fp64 tables by torch.equal on their int64 view, so every bit counts and a NaN must
sit where the restatement has one.  Which NaN it is does not count (bits): IEEE 754 leaves a NaN's sign and payload to the
implementation, 0/0 is negative on x86 hosts and positive on the device, and include/n2v_sim.h keeps them out of the
contract."""
import functools

import numpy as np
import pytest
import torch

import eccknn_reference as E
import nmf_reference as N
import rec_reference as R
import topn_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTORS = [1, 2, 15, 63, 64, 65, 127, 128, 129, 192, 193, 256]   # the lane and NS borders
SENTINEL = -7.5


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)


def bits(t):
    """The int64 view of an fp64 tensor or array, every NaN replaced by the one canonical NaN."""
    t = torch.as_tensor(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t.detach().cpu().contiguous()
    assert t.dtype == torch.float64
    return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).view(torch.int64)


def same(got, want):
    return got.shape == want.shape and torch.equal(bits(got), bits(want))


def nmf():
    from n2v_hip import nmf as module
    return module


def depth():
    """Rows the pass kernel fetches ahead of the entry it works on (DEPTH of csrc/n2v_nmf.hip): 4."""
    from n2v_hip import _lib
    return int(_lib.load().n2v_nmf_depth())


# ---- the base data -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def base():
    """70 users x 50 items, about 900 ratings in a shuffled file order, inner ids by first appearance.  Planted (raw ids):
    user "full" rated every item; item "all" is rated by every user; users "one0" .. "one2" rated nothing else and items
    "solo0" .. "solo2" have "full" as their only rater (rows of length 1 on both sides)."""
    rs = np.random.RandomState(17)
    cells = {(int(c) // 46, int(c) % 46) for c in rs.permutation(66 * 46)[:790]}
    rows = [("u%d" % a, "i%d" % b) for a, b in sorted(cells)]
    items = ["i%d" % b for b in range(46)] + ["all", "solo0", "solo1", "solo2"]
    users = ["u%d" % a for a in range(66)] + ["full", "one0", "one1", "one2"]
    rows += [("full", it) for it in items] + [(us, "all") for us in users if us != "full"]
    rows = [rows[k] for k in rs.permutation(len(rows))]
    r = rs.randint(1, 6, size=len(rows)).astype(np.float64)
    (u, uraw), (i, iraw) = E.inner_ids([a for a, _ in rows]), E.inner_ids([b for _, b in rows])
    return dict(u=np.array(u, np.int64), i=np.array(i, np.int64), r=r, users=uraw, items=iraw, n_users=len(uraw), n_items=len(iraw),
                raw=rows)


def test_the_base_data_is_what_it_claims():
    b = base()
    u, i, r = b["u"], b["i"], b["r"]
    assert (b["n_users"], b["n_items"]) == (70, 50) and 880 <= len(r) <= 920
    ul, il, ir = N.user_lists(u, i, r, 70), N.item_lists(u, i, r, 50), N.item_lists_ir(u, i, r, 50)
    ulen, ilen = np.diff(ul[0]), np.diff(il[0])
    assert ulen.max() == 50 and ilen.max() == 70 and (ulen == 1).sum() >= 3 and (ilen == 1).sum() >= 3
    assert all((np.diff(il[1][il[0][k]:il[0][k + 1]]) > 0).all() for k in range(50))
    assert sum(not (np.diff(ir[1][ir[0][k]:ir[0][k + 1]]) > 0).all() for k in range(50)) > 25      # ir order != ascending u
    assert not np.array_equal(ir[1], il[1])


@functools.lru_cache(maxsize=None)
def restated(nf, n_epochs, what="plain"):
    """The restatement's (pu, qi) after every epoch 0 .. n_epochs, from the initial tables of `what`."""
    b = base()
    par = N.params(n_factors=nf, random_state=nf)
    pu, qi = N.init(b["n_users"], b["n_items"], par)
    r = b["r"]
    if what == "zero":
        pu, qi = np.zeros_like(pu), np.zeros_like(qi)
    elif what == "zero_row":
        pu[5] = 0.0
    elif what == "huge":                                          # factors up to 4: q * 1e308 overflows for q > 1.8
        pu, qi, r = 4.0 * pu, 4.0 * qi, r.copy()
        r[40] = 1e308
    ul, il = N.user_lists(b["u"], b["i"], r, b["n_users"]), N.item_lists(b["u"], b["i"], r, b["n_items"])
    out = [(pu, qi)]
    for _ in range(n_epochs):
        out.append(N.epoch(ul, il, out[-1][0], out[-1][1], par))
    return par, r, out


class Run:
    """The low-level path: device lists through nmf.lists, tables between sentinel rows, epochs on request."""

    def __init__(self, ul, n_users, n_items, tables, order="descending", ir=None):
        m = nmf()
        self.ur = dev(ul[0], torch.int64), dev(ul[1], torch.int32), dev(ul[2], torch.float64)
        self.lists = m.lists(self.ur, n_users, n_items, ir=ir, order=order)
        nf = tables[0].shape[1]
        self.buf = [[torch.full((rows + 2, nf), SENTINEL, dtype=torch.float64, device=DEV) for rows in (n_users, n_items)]
                    for _ in range(2)]
        self.cur = 0
        self.buf[0][0][1:-1] = dev(tables[0], torch.float64)
        self.buf[0][1][1:-1] = dev(tables[1], torch.float64)

    def tables(self, which=None):
        return [t[1:-1] for t in self.buf[self.cur if which is None else which]]

    def epoch(self, reg_pu, reg_qi):
        pu, qi = self.tables()
        pu_out, qi_out = self.tables(1 - self.cur)
        nmf().epoch(self.lists, reg_pu, reg_qi, pu, qi, pu_out, qi_out)
        self.cur = 1 - self.cur
        torch.cuda.synchronize()
        for pair in self.buf:
            for t in pair:
                assert (t[0] == SENTINEL).all() and (t[-1] == SENTINEL).all(), "a sentinel row was written"
        return self.tables()


def run_base(nf, n_epochs, what="plain", order="descending"):
    b = base()
    par, r, want = restated(nf, n_epochs, what)
    run = Run(N.user_lists(b["u"], b["i"], r, b["n_users"]), b["n_users"], b["n_items"], want[0], order)
    got = []
    for ep in range(1, n_epochs + 1):
        pu, qi = run.epoch(par["reg_pu"], par["reg_qi"])
        assert same(pu, want[ep][0]) and same(qi, want[ep][1]), (nf, what, ep)
        got.append((pu.clone(), qi.clone()))
    return got, want


# ---- 1: the epoch kernels against the restatement ----------------------------------------------------------------------

@pytest.mark.parametrize("nf", FACTORS)
def test_tables_bit_for_bit_after_each_of_three_epochs(nf):
    got, want = run_base(nf, 3)
    assert np.isfinite(want[3][0]).all() and (want[3][0] > 0).all() and not np.array_equal(want[3][1], want[2][1])


def test_item_major_list_is_the_all_ratings_order():
    b = base()
    ul = N.user_lists(b["u"], b["i"], b["r"], b["n_users"])
    ur = dev(ul[0], torch.int64), dev(ul[1], torch.int32), dev(ul[2], torch.float64)
    got = nmf().item_major(ur, b["n_items"])
    want = N.item_lists(b["u"], b["i"], b["r"], b["n_items"])
    assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.float64]
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    order = nmf().row_order(ur[0]).cpu().numpy()
    lens = np.diff(ul[0])
    assert sorted(order.tolist()) == list(range(b["n_users"])) and (np.diff(lens[order]) <= 0).all() and lens[order[0]] == 50
    assert order.tolist() != list(range(b["n_users"]))


# ---- 2: list lengths around the look-ahead -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ragged():
    """Hand-made user rows of length 0, 1, 2, depth - 1, depth, depth + 1, the edges of the 64-entry chunks the ids
    arrive in, and 5 000; 5 001 items, the last one unrated (an empty item row)."""
    D = 4
    lengths = [0, 1, 2, D - 1, D, D + 1, 63, 64, 65, 64 + D - 1, 64 + D, 127, 128, 129, 5000]
    rs = np.random.RandomState(23)
    u = np.concatenate([np.full(n, k, np.int64) for k, n in enumerate(lengths)])
    i = np.concatenate([rs.permutation(5000)[:n] for n in lengths]).astype(np.int64)
    r = rs.randint(1, 6, size=len(u)).astype(np.float64)
    return lengths, u, i, r


def test_list_lengths_around_the_look_ahead():
    assert depth() == 4                                          # ragged() is built around it
    lengths, u, i, r = ragged()
    n_users, n_items = len(lengths), 5001
    par = N.params(n_factors=3, random_state=4)
    pu, qi = N.init(n_users, n_items, par)
    ul, il = N.user_lists(u, i, r, n_users), N.item_lists(u, i, r, n_items)
    assert np.diff(ul[0]).tolist() == lengths and np.diff(il[0])[-1] == 0
    want = N.epoch(ul, il, pu, qi, par)
    for order in ("descending", "identity"):
        run = Run(ul, n_users, n_items, (pu, qi), order)
        gpu, gqi = run.epoch(par["reg_pu"], par["reg_qi"])
        assert same(gpu, want[0]) and same(gqi, want[1]), order
    assert np.isnan(want[0][0]).all() and np.isnan(want[1][-1]).all()            # the empty rows: 0 / 0
    assert torch.isnan(gpu[0]).all() and torch.isnan(gqi[-1]).all() and np.isfinite(want[0][1:]).all()


# ---- 3: non-finite cases ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["zero", "zero_row", "huge"])
def test_non_finite_cases_follow_the_arithmetic(what):
    got, want = run_base(5, 3, what)
    last = want[3]
    if what == "zero":
        assert np.isnan(want[1][0]).all() and np.isnan(want[1][1]).all()
    elif what == "zero_row":
        assert np.isnan(want[1][0][5]).all() and np.isfinite(want[1][0][:5]).all() and np.isnan(last[1]).any()
    else:
        assert np.isinf(want[1][0]).any() and np.isfinite(want[1][0]).any() and np.isnan(last[0]).any()


# ---- 4: determinism -----------------------------------------------------------------------------------------------------

def test_two_fits_and_both_row_orders_give_the_same_bytes():
    from n2v_hip import eccknn
    b = base()
    ts = eccknn.Trainset.from_ratings([a for a, _ in b["raw"]], [c for _, c in b["raw"]], b["r"])
    fits = [nmf().NMF(n_factors=15, n_epochs=5, random_state=3, device=DEV).fit(ts) for _ in range(2)]
    assert torch.equal(fits[0].pu.view(torch.int64), fits[1].pu.view(torch.int64))
    assert torch.equal(fits[0].qi.view(torch.int64), fits[1].qi.view(torch.int64))
    a, _ = run_base(65, 3, order="descending")
    c, _ = run_base(65, 3, order="identity")
    assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for ea, ec in zip(a, c) for x, y in zip(ea, ec))
    perm = tuple(dev(np.random.RandomState(k).permutation(n), torch.int32) for k, n in ((1, b["n_users"]), (2, b["n_items"])))
    d, _ = run_base(65, 3, order=perm)
    assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for ea, ed in zip(a, d) for x, y in zip(ea, ed))


# ---- 5: malformed lists -------------------------------------------------------------------------------------------------

def test_malformed_lists_are_named_and_reach_no_pass_kernel():
    from n2v_hip import _lib
    m = nmf()
    b = base()
    n_users, n_items = b["n_users"], b["n_items"]
    ul, il = N.user_lists(b["u"], b["i"], b["r"], n_users), N.item_lists(b["u"], b["i"], b["r"], n_items)
    n = len(b["r"])

    def make(ul_=ul, il_=il):
        ur = dev(ul_[0], torch.int64), dev(ul_[1], torch.int32), dev(ul_[2], torch.float64)
        ir = dev(il_[0], torch.int64), dev(il_[1], torch.int32), dev(il_[2], torch.float64)
        return m.lists(ur, n_users, n_items, ir=ir)

    ok = make()
    assert (ok.n, ok.n_users, ok.n_items) == (n, n_users, n_items)

    def edit(lst, part, pos, val):
        out = [a.copy() for a in lst]
        out[part][pos] = val
        return tuple(out)

    # a ptr not monotone / leaving [0, n] / not starting at 0, on either side
    for k, val in ((3, int(ul[0][4]) + 1), (3, -1), (3, n + 1), (3, 2 ** 62), (0, 1)):
        with pytest.raises(ValueError, match="not monotone"):
            make(ul_=edit(ul, 0, k, val))
        with pytest.raises(ValueError, match="not monotone"):
            make(il_=edit(il, 0, k, val if val != int(ul[0][4]) + 1 else int(il[0][4]) + 1))
    with pytest.raises(ValueError, match="does not end at n"):
        make(ul_=edit(ul, 0, -1, n - 1))
    # an id out of range
    for val in (n_items, -1, 2 ** 31 - 1):
        with pytest.raises(ValueError, match="id out of range"):
            make(ul_=edit(ul, 1, 7, val))
    for val in (n_users, -3):
        with pytest.raises(ValueError, match="id out of range"):
            make(il_=edit(il, 1, 7, val))
    # an item row not ascending in user: Trainset.ir itself, the same ratings in training order
    with pytest.raises(ValueError) as e:
        make(il_=N.item_lists_ir(b["u"], b["i"], b["r"], n_items))
    assert "not strictly ascending in u" in str(e.value) and "same ratings" not in str(e.value)
    # not the same ratings: one item of a user's list swapped for another, every id still in range
    pos = int(ul[0][b["users"].index("u3")])
    other = next(v for v in range(n_items) if v not in ul[1][ul[0][b["users"].index("u3")]:ul[0][b["users"].index("u3") + 1]])
    with pytest.raises(ValueError, match="do not hold the same ratings"):
        make(ul_=edit(ul, 1, pos, other))
    # mismatched n
    short = (np.append(il[0][:-1], n - 1), il[1][:-1], il[2][:-1])
    with pytest.raises(ValueError, match="mismatched n"):
        make(il_=short)
    # shapes and types are refused on the host; epoch takes nothing but checked Lists
    with pytest.raises(ValueError, match="int64 ptr"):
        m.lists((dev(ul[0], torch.int32), dev(ul[1], torch.int32), dev(ul[2], torch.float64)), n_users, n_items)
    with pytest.raises(ValueError, match="user ptr entries"):
        m.lists((dev(ul[0][:-1], torch.int64), dev(ul[1], torch.int32), dev(ul[2], torch.float64)), n_users, n_items)
    t = torch.full((n_users, 4), SENTINEL, dtype=torch.float64, device=DEV)
    q = torch.full((n_items, 4), SENTINEL, dtype=torch.float64, device=DEV)
    t2, q2 = t.clone(), q.clone()
    with pytest.raises(TypeError, match="checked"):
        m.epoch((ul, il), 0.06, 0.06, t, q, t2, q2)
    with pytest.raises(ValueError, match="qi"):
        m.epoch(ok, 0.06, 0.06, t, t, t2, q2)
    # aliased in / out tables: refused by the wrapper and by the C-ABI, before any launch
    both = torch.full((n_users + n_items, 4), SENTINEL, dtype=torch.float64, device=DEV)
    shared_row = (t, q, both[:n_users], both[n_users - 1:n_users - 1 + n_items])      # the two outputs share a row
    aliased = ((t, q, t, q2), (t, q, t2, q), (both[:n_users], q, t2, both[n_users - 1:n_users - 1 + n_items]), shared_row)
    for tables in aliased:
        with pytest.raises(ValueError, match="aliased tables"):
            m.epoch(ok, 0.06, 0.06, *tables)
    lib = _lib.load()
    # u_ptr u_i u_r i_ptr i_u i_r u_order i_order | n_users n_items n n_factors reg_pu reg_qi
    head = [_lib.ptr(x) for x in ok.ur + ok.ir + ok.order] + [n_users, n_items, n, 4, 0.06, 0.06]
    st = _lib.stream_ptr(t.device)
    for tables in aliased:
        assert lib.n2v_nmf_epoch(*head, *[_lib.ptr(x) for x in tables], st) != 0
        assert "nmf_epoch:" in lib.n2v_last_error().decode() and "overlaps" in lib.n2v_last_error().decode()
    for k, v, word in ((8, 0, "n_users=0"), (9, 2 ** 31, "n_items="), (10, 0, "n=0"), (11, 0, "n_factors 0"),
                       (11, 257, "n_factors 257"), (2, None, "null"), (3, None, "null")):
        bad = list(head)
        bad[k] = v
        assert lib.n2v_nmf_epoch(*bad, *[_lib.ptr(x) for x in (t, q, t2, q2)], st) != 0
        assert word in lib.n2v_last_error().decode(), word
    assert lib.n2v_nmf_lists_check(None, None, None, None, n_users, n_items, n, None, None, st) != 0
    assert "nmf_lists_check: null" in lib.n2v_last_error().decode()
    torch.cuda.synchronize()
    assert all((x == SENTINEL).all() for x in (t, q, t2, q2, both))


# ---- 6: end to end ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fitted():
    """NMF() at its defaults on the base data, and the restatement's tables for the same."""
    from n2v_hip import eccknn
    b = base()
    ts = eccknn.Trainset.from_ratings([a for a, _ in b["raw"]], [c for _, c in b["raw"]], b["r"])
    algo = nmf().NMF(device=DEV).fit(ts)
    want = N.fit(b["u"], b["i"], b["r"], b["n_users"], b["n_items"], N.params())
    return ts, algo, want


def test_fit_at_the_defaults_equals_the_restatement():
    ts, algo, (pu, qi) = fitted()
    assert (algo.n_factors, algo.n_epochs, algo.biased, algo.mu) == (15, 50, False, 0.0)
    assert same(algo.pu, pu) and same(algo.qi, qi) and np.isfinite(pu).all() and (pu >= 0).all() and (qi >= 0).all()
    zero = nmf().NMF(n_epochs=0, random_state=4, device=DEV).fit(ts)
    init = N.init(ts.n_users, ts.n_items, N.params(random_state=4))
    assert same(zero.pu, init[0]) and same(zero.qi, init[1])


def test_estimate_test_and_rmse_equal_the_restatement():
    from n2v_hip import eccknn
    b = base()
    ts, algo, (pu, qi) = fitted()
    rs = np.random.RandomState(8)
    testset = [(b["users"][a], b["items"][c], float(rs.randint(1, 6))) for a, c in zip(rs.randint(0, 70, 60), rs.randint(0, 50, 60))]
    testset += [("stranger", "all", 3.0), ("full", "unseen", 4.0), ("stranger", "unseen", 1.0)]
    qu = [b["users"].index(a) if a in b["users"] else -1 for a, _, _ in testset]
    qi_ids = [b["items"].index(c) if c in b["items"] else -1 for _, c, _ in testset]
    est, imp = N.estimate(pu, qi, qu, qi_ids)
    assert imp.tolist() == [0] * 60 + [1, 1, 1]
    mean = E.global_mean(b["r"])
    pred = E.predict_all(est, imp, mean, 1.0, 5.0)
    got, got_imp = algo.test(testset)
    assert same(got, pred) and np.array_equal(got_imp, imp.astype(bool))
    assert algo.rmse(testset) == E.rmse([t[2] for t in testset], pred)
    for k in (0, 17, 59):
        assert np.float64(algo.estimate(qu[k], qi_ids[k])).tobytes() == est[k].tobytes()
    for a, c in ((-1, 3), (2, -1), (70, 0), (0, 50), ("full", 0)):
        with pytest.raises(eccknn.PredictionImpossible, match="User and item are unknown."):
            algo.estimate(a, c)
    assert pred.min() >= 1.0 and pred.max() <= 5.0 and len(set(pred.tolist())) > 20


@pytest.mark.parametrize("n", [1, 10])
def test_top_n_lists_equal_the_restatement(n):
    b = base()
    ts, algo, (pu, qi) = fitted()
    raw = b["users"] + ["stranger", "full", "one1"]
    owners = [b["users"].index(a) if a in b["users"] else -1 for a in raw]
    predict = T.svd_predictor(N.model(pu, qi), False, E.global_mean(b["r"]), 1.0, 5.0)
    ranked = T.rankings(T.seen_sets(b["u"], b["i"], b["n_users"]), b["n_items"], owners, predict)
    wi, ws = T.lists(ranked, n)
    gi, gs = algo.top_n_lists(n, raw)
    assert gi.dtype == torch.int32 and torch.equal(gi.cpu(), torch.from_numpy(wi))
    real = torch.from_numpy(wi >= 0)
    assert torch.equal(bits(gs)[real], bits(ws)[real])
    assert (wi[b["users"].index("full")] == -1).all() and (wi[:, 0] >= 0).sum() == len(raw) - 2      # "full" has seen everything


def small_csv(tmp_path):
    rs = np.random.RandomState(21)
    cells = rs.permutation(30 * 40)[:420]
    rows = [("u%02d" % (c // 40), "i%02d" % (c % 40), float(rs.randint(1, 6))) for c in cells]
    p = tmp_path / "ratings.csv"
    p.write_text("user,item,rating\n" + "".join("%s,%s,%r\n" % t for t in rows))
    return str(p), rows


def restated_split(rows, train, test, scale, nf, n_epochs, seed, n=None):
    """rmse, or (rmse, (f1, map, mrr, ndcg)) with n, of one split, everything from the restatements."""
    raw_u, raw_i, r = [rows[t][0] for t in train], [rows[t][1] for t in train], np.array([rows[t][2] for t in train])
    u, users = E.inner_ids(raw_u)
    i, items = E.inner_ids(raw_i)
    mean = E.global_mean(r)
    pu, qi = N.fit(u, i, r, len(users), len(items), N.params(n_factors=nf, n_epochs=n_epochs, random_state=seed))
    tu = [users.index(rows[t][0]) if rows[t][0] in users else -1 for t in test]
    ti = [items.index(rows[t][1]) if rows[t][1] in items else -1 for t in test]
    est, imp = N.estimate(pu, qi, tu, ti)
    rmse = E.rmse([rows[t][2] for t in test], E.predict_all(est, imp, mean, *scale))
    if n is None:
        return rmse
    truth = {}
    for t in test:
        truth.setdefault(rows[t][0], set()).add(rows[t][1])
    owners = list(truth)
    ptr, pos, lens = [0], [], []
    for ru in owners:
        pos.extend(sorted(items.index(ri) for ri in truth[ru] if ri in items))
        ptr.append(len(pos))
        lens.append(len(truth[ru]))
    ranked = T.rankings(T.seen_sets(u, i, len(users)), len(items), [users.index(ru) if ru in users else -1 for ru in owners],
                        T.svd_predictor(N.model(pu, qi), False, mean, *scale))
    per_user = R.user_metrics(T.lists(ranked, n)[0], np.array(ptr, np.int64), np.array(pos, np.int32), np.array(lens, np.int64))
    return rmse, R.averages(per_user)


def test_main_rec_algo_nmf_returns_what_the_restatement_gives(tmp_path, capsys):
    import main_rec
    path, rows = small_csv(tmp_path)
    base_args = ["-input", path, "-algo", "nmf", "-factors", "8", "-epochs", "3"]
    err = main_rec.main(base_args)
    assert capsys.readouterr().out.strip() == "RMSE: %r" % err
    train, test = main_rec.split(len(rows), 0.2, 0)
    assert err == restated_split(rows, train, test, (1.0, 5.0), 8, 3, 0)
    folds = main_rec.main(base_args + ["-cv", "2", "-topn", "5"])
    out = capsys.readouterr().out.strip().split("\n")
    assert [l.split(":")[0] for l in out] == ["RMSE", "F1 / MAP / MRR / NDCG @5"] * 2 + ["mean RMSE"]
    want = [restated_split(rows, tr, te, (1.0, 5.0), 8, 3, 0, 5) for tr, te in main_rec.folds(len(rows), 2, 0)]
    assert [(f[0], tuple(f[1])) for f in folds] == want
    recs = tmp_path / "recs.csv"
    main_rec.main(base_args + ["-topn", "3", "-save-recs", str(recs), "-seed", "2", "-test-ratio", "0.3"])
    lines = recs.read_text().strip().split("\n")
    assert len(lines) > 30 and all(len(l.split(",")) == 3 for l in lines)
