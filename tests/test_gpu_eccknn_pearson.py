"""GPU tests of the KNNBasic baseline: the Pearson similarities (n2v_eccknn_pearson, n2v_eccknn_pearson_sparse) and the
ALS baselines (n2v_eccknn_baselines; csrc/n2v_eccknn.hip, C-ABI include/n2v_sim.h) against the restatement
tests/eccknn_pearson_reference.py, through the C-ABI unless a test says otherwise, then the Python surface.

Exact comparisons only, as in tests/test_gpu_eccknn.py: fp64 arrays by their bytes (E.canon: one canonical NaN),
integers with array_equal.  Every output buffer starts as a sentinel."""
import numpy as np
import pytest

import eccknn_reference as E
import eccknn_pearson_reference as P

pytestmark = pytest.mark.gpu

SENT = -12345.5
ISENT = -7
KIND = {"pearson": 0, "pearson_baseline": 1}
NAMES = ("pearson", "pearson_baseline")


def _L():
    from n2v_hip import _lib as L
    return L


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host_csr(major, minor, r, n_major, by_minor=True):
    """CSR of (major, minor, r): rows ascending in minor (what the similarity reads) or in training order (ur / ir)."""
    major, minor, r = np.asarray(major, np.int64), np.asarray(minor, np.int64), np.asarray(r, np.float64)
    order = np.lexsort((minor, major)) if by_minor else np.argsort(major, kind="stable")
    ptr = np.zeros(n_major + 1, np.int64)
    np.cumsum(np.bincount(major, minlength=n_major), out=ptr[1:])
    return ptr, minor[order].astype(np.int32), r[order]


def _outputs(n_x, name):
    import torch
    out = {"sim": None, "freq": torch.full((n_x, n_x), ISENT, dtype=torch.int32, device="cuda")}
    for nm in ("sim",) + P.ACCUMULATORS[name]:
        out[nm] = torch.full((n_x, n_x), SENT, dtype=torch.float64, device="cuda")
    return out


def _out_ptrs(out, name):
    L = _L()
    a = [L.ptr(out[nm]) for nm in P.ACCUMULATORS[name][1:]] + [None, None]
    return [L.ptr(out["sim"]), L.ptr(out["freq"]), L.ptr(out["prods"])] + a[:4]


def baseline_inputs(seed, n_x, n_y):
    """(global_mean, bx, by) of a seed: what pearson_baseline reads beside the ratings."""
    rs = np.random.RandomState(seed)
    return 3.0 + rs.normal(), rs.normal(size=n_x), rs.normal(size=n_y)


def c_pearson(form, x, y, r, w, n_x, n_y, name, min_support, bl=None, shrinkage=100.0):
    """n2v_eccknn_densify + n2v_eccknn_pearson, or a checked host CSR + n2v_eccknn_pearson_sparse; numpy arrays out.
    w None: NULL.  bl = (global_mean, bx, by) for pearson_baseline."""
    import torch
    L = _L(); lib = L.load()
    dw = None if w is None else _dev(w, np.float64)
    gm, dbx, dby = (0.0, None, None) if bl is None else (float(bl[0]), _dev(bl[1], np.float64), _dev(bl[2], np.float64))
    out = _outputs(n_x, name)
    st = L.stream_ptr(out["sim"].device)
    tail = [L.ptr(dw), KIND[name], min_support, gm, L.ptr(dbx), L.ptr(dby), float(shrinkage)] + _out_ptrs(out, name) + [st]
    if form == "dense":
        dx, dy, dr = _dev(x, np.int32), _dev(y, np.int32), _dev(r, np.float64)
        dense = torch.full((n_y, n_x), SENT, dtype=torch.float64, device="cuda")
        mask = torch.full((n_y, n_x), 9, dtype=torch.uint8, device="cuda")
        L.check(lib.n2v_eccknn_densify(L.ptr(dx), L.ptr(dy), L.ptr(dr), len(r), n_x, n_y, L.ptr(dense), L.ptr(mask), st))
        L.check(lib.n2v_eccknn_pearson(L.ptr(dense), L.ptr(mask), n_x, n_y, *tail))
    else:
        ptr, ys, rs = host_csr(x, y, r, n_x)
        dp, dy, dr = _dev(ptr, np.int64), _dev(ys, np.int32), _dev(rs, np.float64)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.check(lib.n2v_eccknn_csr_check(L.ptr(dp), L.ptr(dy), n_x, n_y, len(rs), L.ptr(status), st))
        assert int(status.item()) == 0
        L.check(lib.n2v_eccknn_pearson_sparse(L.ptr(dp), L.ptr(dy), L.ptr(dr), n_x, n_y, len(rs), *tail))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def restatement(x, y, r, w, n_x, name, min_support, bl=None, shrinkage=100.0):
    yr = E.build_yr(x, y, r)
    if name == "pearson":
        return P.pearson_numpy(n_x, yr, min_support, w)
    return P.pearson_baseline_numpy(n_x, yr, min_support, bl[0], bl[1], bl[2], shrinkage, w)


def assert_same(got, want, what):
    assert set(got) == set(want), what
    for key in want:
        if key == "freq":
            assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (key,) + what
        else:
            assert E.canon(got[key]) == E.canon(want[key]), (key,) + what


def check_both(x, y, r, w, n_x, n_y, name, min_support, bl=None, shrinkage=100.0):
    """dense == sparse == restatement, every array; returns the restatement's arrays."""
    want = restatement(x, y, r, w, n_x, name, min_support, bl, shrinkage)
    what = (name, min_support, n_x, n_y, w is None)
    dense = c_pearson("dense", x, y, r, w, n_x, n_y, name, min_support, bl, shrinkage)
    sparse = c_pearson("sparse", x, y, r, w, n_x, n_y, name, min_support, bl, shrinkage)
    assert_same(dense, want, what + ("dense",))
    assert_same(sparse, want, what + ("sparse",))
    for key in dense:                                            # bytewise, NaN payloads included
        assert dense[key].tobytes() == sparse[key].tobytes(), (key,) + what
    s = dense["sim"]
    assert E.canon(s) == E.canon(s.T) and np.array_equal(np.diag(s), np.ones(n_x))
    return want


# ---- 1: the grid of the cosine / msd tests -----------------------------------------------------------------------------

KINDS = ["int", "half", "fp64"]


@pytest.mark.parametrize("n_y", [1, 31, 32, 33, 100])
@pytest.mark.parametrize("n_x", [1, 2, 63, 64, 65, 130])
def test_sim_and_accumulators_bit_for_bit_dense_and_sparse(n_x, n_y):
    kind = KINDS[(n_x + n_y) % 3]
    n = max(1, int((0.3 if n_y <= 33 else 0.2) * n_x * n_y))
    x, y, r, w = E.make_case(1000 * n_x + n_y, n_x, n_y, n, kind, zeros=3 if n >= 6 else 0)
    if n >= 6:
        assert (r == 0.0).sum() == 3                             # a 0.0 rating is a rating: mask and value differ
    bl = baseline_inputs(n_x * 31 + n_y, n_x, n_y)
    for name in NAMES:
        for ms, shrinkage in ((1, 100.0), (3, 7.5)):
            for weights in (None, w):
                want = check_both(x, y, r, weights, n_x, n_y, name, ms, bl if name == "pearson_baseline" else None, shrinkage)
                assert want["freq"].trace() == len(r)            # every rating, the zeros too, is on its row's diagonal
    if n_x >= 63 and n_y >= 31:
        assert (want["freq"][np.triu_indices(n_x, 1)] >= 3).any() and (want["sim"] == 0.0).any()


# ---- 2: sparse row lengths around the staging chunk --------------------------------------------------------------------

def test_row_lengths_around_the_staging_chunk():
    C = int(_L().load().n2v_eccknn_sparse_chunk())
    assert C == 16
    lengths = [0, 1, C - 1, C, C + 1, 2 * C + 1]                 # {0, 1, 15, 16, 17, 33}
    n_x, n_y = 70, 12 * C
    rs = np.random.RandomState(4321)
    rows = [sorted(rs.permutation(n_y)[:lengths[i % 6]].tolist()) for i in range(n_x)]
    rows[8] = list(range(0, 2 * (2 * C + 1), 2))                 # two interleaved rows: no common y, many rounds
    rows[11] = list(range(1, 2 * (2 * C + 1), 2))
    rows[10] = rows[5][:C]                                       # a subset of a longer row
    assert set(len(v) for v in rows[:64]) == set(lengths) == set(len(v) for v in rows[64:])
    x = np.array([i for i, v in enumerate(rows) for _ in v])
    y = np.array([yy for v in rows for yy in v])
    order = rs.permutation(len(x))
    x, y = x[order], y[order]
    r = rs.normal(size=len(x)) * 3.0 + rs.random_sample(len(x))
    w = rs.normal(size=n_y)
    bl = baseline_inputs(77, n_x, n_y)
    for name in NAMES:
        for weights in (None, w):
            want = check_both(x, y, r, weights, n_x, n_y, name, 1, bl if name == "pearson_baseline" else None)
        f = want["freq"]
        assert f[8, 11] == 0 and f[5, 10] == C and f[0].sum() == 0 and f[5, 5] == 2 * C + 1


# ---- 3: degenerate data ------------------------------------------------------------------------------------------------

def test_constant_row_gives_zero_not_nan():
    n_x, n_y = 5, 6
    x = np.repeat(np.arange(n_x), n_y); y = np.tile(np.arange(n_y), n_x)
    r = np.random.RandomState(3).randint(1, 6, size=n_x * n_y).astype(np.float64)
    r[x == 0] = 3.0
    want = check_both(x, y, r, None, n_x, n_y, "pearson", 1)
    assert (want["freq"] == n_y).all() and (want["sim"][0, 1:] == 0.0).all() and not np.isnan(want["sim"]).any()
    assert (want["sim"][1:, 1:] != 0.0).all()


def test_cancellation_below_zero_keeps_the_nan():
    """Ratings 1e6 + small: n*sqi - si*si is a difference of numbers near 1e13 whose true value is far below their
    rounding error, so its sign is noise; where exactly one of the two factors is negative the sqrt is NaN."""
    n_x, n_y = 24, 12
    rs = np.random.RandomState(5)
    x = np.repeat(np.arange(n_x), n_y); y = np.tile(np.arange(n_y), n_x)
    r = 1e6 + rs.normal(size=n_x * n_y) * 1e-6
    keep = rs.random_sample(len(r)) < 0.8
    x, y, r = x[keep], y[keep], r[keep]
    w = rs.normal(size=n_y)
    for weights in (None, w):
        want = check_both(x, y, r, weights, n_x, n_y, "pearson", 2)
        n = want["freq"].astype(np.double)
        assert ((n * want["sqi"] - want["si"] * want["si"]) < 0).any()       # the restatement really goes below zero
        nan = np.isnan(want["sim"])
        assert nan.any() and not nan.all() and not nan[np.arange(n_x), np.arange(n_x)].any()


def test_baseline_zero_sq_diff_keeps_nan_and_inf():
    """global_mean = by = bx = 0, so the deviations are the ratings: a row of 0.0 ratings has sq_diff 0 and prods 0
    (0/0: NaN); 1e-200 against 1e100 has prods 1e-100 and a sq_diff_i that underflows to 0 (x/0: inf)."""
    n_x, n_y = 5, 4
    x = np.repeat(np.arange(n_x), n_y); y = np.tile(np.arange(n_y), n_x)
    r = np.random.RandomState(6).randint(1, 6, size=n_x * n_y).astype(np.float64)
    r[x == 0] = 0.0
    r[x == 2] = 1e-200
    r[x == 3] = 1e100
    bl = (0.0, np.zeros(n_x), np.zeros(n_y))
    for weights in (None, np.array([1.0, 2.0, -1.0, 0.5])):
        want = check_both(x, y, r, weights, n_x, n_y, "pearson_baseline", 1, bl)
        s = want["sim"]
        assert want["sq_diff_i"][0, 1] == 0.0 and np.isnan(s[0, 1]) and np.isnan(s[1, 0])
        assert want["sq_diff_i"][2, 3] == 0.0 and want["prods"][2, 3] != 0.0 and np.isinf(s[2, 3]) and np.isinf(s[3, 2])
        assert np.isfinite(s[1, 4]) and s[1, 4] != 0.0 and want["freq"][0, 0] == n_y


# ---- 4: baselines ------------------------------------------------------------------------------------------------------

def c_baselines(ur, ir, n_users, n_items, mean, n_epochs, reg_u, reg_i):
    import torch
    L = _L(); lib = L.load()
    d = [_dev(a, t) for a, t in zip(ur + ir, (np.int64, np.int32, np.float64) * 2)]
    bu = torch.full((n_users,), SENT, dtype=torch.float64, device="cuda")
    bi = torch.full((n_items,), SENT, dtype=torch.float64, device="cuda")
    L.check(lib.n2v_eccknn_baselines(L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), n_users, L.ptr(d[3]), L.ptr(d[4]), L.ptr(d[5]),
                                     n_items, float(mean), n_epochs, float(reg_u), float(reg_i), L.ptr(bu), L.ptr(bi),
                                     L.stream_ptr(bu.device)))
    torch.cuda.synchronize()
    return bu.cpu().numpy(), bi.cpu().numpy()


@pytest.fixture(scope="module")
def length_case():
    """Users 0..4 rate 1, 63, 64, 65, 200 of the items 0..199; items 200..204 are rated by as many of the users 5..204.
    Training order is shuffled, so every list's order is its own."""
    lengths = [1, 63, 64, 65, 200]
    rs = np.random.RandomState(11)
    u = [k for k, n in enumerate(lengths) for _ in range(n)] + [int(v) for n in lengths for v in 5 + rs.permutation(200)[:n]]
    i = [int(v) for n in lengths for v in rs.permutation(200)[:n]] + [200 + k for k, n in enumerate(lengths) for _ in range(n)]
    order = rs.permutation(len(u))
    u, i = np.array(u)[order], np.array(i)[order]
    r = rs.normal(size=len(u)) * 1.5 + 3.0
    n_users, n_items = 205, 205
    ur, ir = host_csr(u, i, r, n_users, by_minor=False), host_csr(i, u, r, n_items, by_minor=False)
    assert np.diff(ur[0])[:5].tolist() == lengths and np.diff(ir[0])[200:].tolist() == lengths
    assert (np.diff(ur[1][:64]) < 0).any()                       # training order, not id order
    return u, i, r, n_users, n_items, ur, ir, E.global_mean(r)


@pytest.mark.parametrize("n_epochs", [0, 1, 10])
def test_baselines_bit_for_bit(length_case, n_epochs):
    u, i, r, n_users, n_items, ur, ir, mean = length_case
    for reg_u, reg_i in ((15, 10), (2.5, 0.75)):
        wu, wi = P.baselines_als(P.rows_of(u, i, r, n_users), P.rows_of(i, u, r, n_items), mean, n_epochs, reg_u, reg_i)
        bu, bi = c_baselines(ur, ir, n_users, n_items, mean, n_epochs, reg_u, reg_i)
        assert bu.tobytes() == wu.tobytes() and bi.tobytes() == wi.tobytes(), (n_epochs, reg_u)
        assert (bu != 0.0).any() == (n_epochs > 0)


def test_baselines_ignore_an_out_of_range_id(length_case):
    u, i, r, n_users, n_items, ur, ir, mean = length_case
    ids = ir[1].copy()
    a, b = int(ir[0][204]) + 70, int(ir[0][201]) + 3             # inside the lists of items 204 and 201
    ids[a], ids[b] = n_users, -1
    rows = P.rows_of(i, u, r, n_items)
    del rows[204][70], rows[201][3]
    wu, wi = P.baselines_als(P.rows_of(u, i, r, n_users), rows, mean, 3)
    bu, bi = c_baselines(ur, (ir[0], ids, ir[2]), n_users, n_items, mean, 3, 15, 10)
    assert bu.tobytes() == wu.tobytes() and bi.tobytes() == wi.tobytes()
    clean = c_baselines(ur, ir, n_users, n_items, mean, 3, 15, 10)
    assert clean[1][204] != bi[204] and clean[1][201] != bi[201]


# ---- 5: argument errors ------------------------------------------------------------------------------------------------

def test_argument_errors_launch_nothing():
    import torch
    L = _L(); lib = L.load()
    n_x, n_y = 4, 10
    dense = torch.ones((n_y, n_x), dtype=torch.float64, device="cuda")
    mask = torch.ones((n_y, n_x), dtype=torch.uint8, device="cuda")
    dp, dy = _dev([0, 2, 4, 6, 8], np.int64), _dev(np.arange(8), np.int32)
    dr, dw = _dev(np.ones(8), np.float64), _dev(np.ones(n_y), np.float64)
    bx, by = _dev(np.zeros(n_x), np.float64), _dev(np.zeros(n_y), np.float64)
    out = _outputs(n_x, "pearson")
    st = L.stream_ptr(dp.device)
    po = _out_ptrs(out, "pearson")

    def dense_call(nx, ny, kind, sim, pbx):
        return lib.n2v_eccknn_pearson(L.ptr(dense), L.ptr(mask), nx, ny, L.ptr(dw), kind, 1, 0.0, pbx, L.ptr(by), 100.0,
                                      sim, *po[1:], st)

    def sparse_call(nx, ny, n, kind, sim, pbx):
        return lib.n2v_eccknn_pearson_sparse(L.ptr(dp), L.ptr(dy), L.ptr(dr), nx, ny, n, L.ptr(dw), kind, 1, 0.0, pbx,
                                             L.ptr(by), 100.0, sim, *po[1:], st)

    sim, pbx = po[0], L.ptr(bx)
    for args, word in (((0, n_y, 0, sim, pbx), "n_x=0"), ((n_x, 0, 0, sim, pbx), "n_y=0"), ((n_x, n_y, 2, sim, pbx), "kind 2"),
                       ((n_x, n_y, -1, sim, pbx), "kind -1"), ((n_x, n_y, 0, None, pbx), "null"),
                       ((n_x, n_y, 1, sim, None), "bx"), ((1 << 20, 1 << 20, 0, sim, pbx), "dense limit"),
                       ((65535 * 64 + 1, 1, 0, sim, pbx), "tiles")):
        assert dense_call(*args) != 0
        assert word in lib.n2v_last_error().decode() and "eccknn_pearson:" in lib.n2v_last_error().decode()
    for args, word in (((0, n_y, 8, 0, sim, pbx), "n_x=0"), ((n_x, 0, 8, 0, sim, pbx), "n_y=0"), ((n_x, 1 << 31, 8, 0, sim, pbx), "n_y="),
                       ((n_x, n_y, -1, 0, sim, pbx), "n=-1"), ((n_x, n_y, 8, 2, sim, pbx), "kind 2"),
                       ((n_x, n_y, 8, 0, None, pbx), "null"), ((n_x, n_y, 8, 1, sim, None), "bx"),
                       ((65535 * 64 + 1, n_y, 8, 0, sim, pbx), "tiles")):
        assert sparse_call(*args) != 0
        assert word in lib.n2v_last_error().decode() and "eccknn_pearson_sparse:" in lib.n2v_last_error().decode()
    bu = torch.full((n_x,), SENT, dtype=torch.float64, device="cuda")
    bi = torch.full((n_x,), SENT, dtype=torch.float64, device="cuda")

    def bsl_call(n_users, n_epochs, reg_u, reg_i, pbu):
        return lib.n2v_eccknn_baselines(L.ptr(dp), L.ptr(dy), L.ptr(dr), n_users, L.ptr(dp), L.ptr(dy), L.ptr(dr), n_x, 1.0,
                                        n_epochs, reg_u, reg_i, pbu, L.ptr(bi), st)

    for args, word in (((0, 1, 15.0, 10.0, L.ptr(bu)), "n_users=0"), ((n_x, -1, 15.0, 10.0, L.ptr(bu)), "n_epochs"),
                       ((n_x, 1, -1.0, 10.0, L.ptr(bu)), "reg_u"), ((n_x, 1, 15.0, -0.5, L.ptr(bu)), "reg_i"),
                       ((n_x, 1, float("nan"), 10.0, L.ptr(bu)), "reg_u"), ((n_x, 1, 15.0, 10.0, None), "null")):
        assert bsl_call(*args) != 0
        assert word in lib.n2v_last_error().decode(), lib.n2v_last_error().decode()
    torch.cuda.synchronize()
    assert all((v == (ISENT if k == "freq" else SENT)).all() for k, v in out.items())
    assert (bu == SENT).all() and (bi == SENT).all()
    # the same buffers are fine once the arguments are: 4 rows of two 1.0 ratings, disjoint y
    assert sparse_call(n_x, n_y, 8, 0, sim, pbx) == 0 and bsl_call(n_x, 1, 15.0, 10.0, L.ptr(bu)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out["freq"].cpu().numpy(), np.diag([2, 2, 2, 2]).astype(np.int32))
    assert np.array_equal(out["sim"].cpu().numpy(), np.eye(4)) and (bu != SENT).all()


# ---- 6: the Python surface ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def raw_case():
    rs = np.random.RandomState(21)
    cells = rs.permutation(90 * 70)[:1500]
    users = ["u%d" % (c // 70) for c in cells]
    items = [1000 + int(c % 70) for c in cells]
    r = rs.randint(1, 11, size=1500) * 0.5
    test = [("u%d" % rs.randint(0, 95), 1000 + int(rs.randint(0, 75)), float(rs.randint(1, 11) * 0.5)) for _ in range(400)]
    return users, items, r, test


def restate_knn(name, xs, ys, r, n_x, n_y, ts, user_based, ms, w, shrinkage, bsl):
    """The restatement's arrays for one of the four names, baselines included."""
    yr = E.build_yr(xs, ys, r)
    if name in E.NUMPY:
        return E.NUMPY[name](n_x, yr, ms, np.ones(n_y) if w is None else w)
    if name == "pearson":
        return P.pearson_numpy(n_x, yr, ms, w)
    bu, bi = P.baselines_als(P.rows_of(ts.u, ts.i, r, ts.n_users), P.rows_of(ts.i, ts.u, r, ts.n_items), E.global_mean(r), **bsl)
    bx, by = (bu, bi) if user_based else (bi, bu)
    return P.pearson_baseline_numpy(n_x, yr, ms, E.global_mean(r), bx, by, shrinkage, w)


@pytest.mark.parametrize("name", ["cosine", "msd", "pearson", "pearson_baseline"])
@pytest.mark.parametrize("user_based", [True, False])
def test_knnbasic_agrees_with_the_c_abi_path_and_the_restatement(raw_case, name, user_based):
    from n2v_hip import eccknn
    users, items, r, test = raw_case
    ts = eccknn.Trainset.from_ratings(users, items, r, rating_scale=(2.5, 3.0))
    bsl = {"n_epochs": 4, "reg_u": 12, "reg_i": 8}
    opts = {"name": name, "user_based": user_based, "min_support": 3, "shrinkage": 40}
    algo = eccknn.KNNBasic(k=20, min_k=3, sim_options=opts, bsl_options=bsl)
    assert algo.fit(ts) is algo
    xs, ys = (ts.u, ts.i) if user_based else (ts.i, ts.u)
    n_x, n_y = (ts.n_users, ts.n_items) if user_based else (ts.n_items, ts.n_users)
    want = restate_knn(name, xs, ys, r, n_x, n_y, ts, user_based, 3, None, 40, bsl)
    sim = algo.sim.cpu().numpy()
    assert tuple(sim.shape) == (n_x, n_x) and E.canon(sim) == E.canon(want["sim"])
    if name in KIND:                                             # the C-ABI path, baselines from the C-ABI too
        bl = None
        if name == "pearson_baseline":
            ur, ir = host_csr(ts.u, ts.i, r, ts.n_users, False), host_csr(ts.i, ts.u, r, ts.n_items, False)
            bu, bi = c_baselines(ur, ir, ts.n_users, ts.n_items, ts.global_mean, 4, 12, 8)
            bl = (ts.global_mean,) + ((bu, bi) if user_based else (bi, bu))
            assert algo.bx.cpu().numpy().tobytes() == bl[1].tobytes() and algo.by.cpu().numpy().tobytes() == bl[2].tobytes()
            gbu, gbi = eccknn.baselines(ts, bsl)
            assert gbu.cpu().numpy().tobytes() == bu.tobytes() and gbi.cpu().numpy().tobytes() == bi.tobytes()
        for form in ("dense", "sparse"):
            assert c_pearson(form, xs, ys, r, None, n_x, n_y, name, 3, bl, 40.0)["sim"].tobytes() == sim.tobytes()
            other = eccknn.KNNBasic(k=20, min_k=3, sim_options=dict(opts, form=form), bsl_options=bsl).fit(ts)
            assert other.sim.cpu().numpy().tobytes() == sim.tobytes()
    else:                                                        # plain cosine / msd: EccenKNN with all-ones weights
        ecc = eccknn.EccenKNN(k=20, min_k=3, sim_options=opts).fit(ts, np.ones(n_y))
        assert ecc.sim.cpu().numpy().tobytes() == sim.tobytes()
        for a, b in zip(ecc.test(test), algo.test(test)):
            assert a.tobytes() == b.tobytes()
        assert ecc.rmse(test) == algo.rmse(test)
    # estimates and RMSE: the existing restatement fed the new sim
    yr = E.build_yr(xs, ys, r)
    qu, qi = ts.inner_uids([t[0] for t in test]), ts.inner_iids([t[1] for t in test])
    qx, qy = (qu, qi) if user_based else (qi, qu)
    west, wak, wimp = E.estimate_all(want["sim"], yr, qx, qy, 20, 3)
    wpred = E.predict_all(west, wimp, E.global_mean(r), 2.5, 3.0)
    pred, ak, imp = algo.test(test)
    assert pred.tobytes() == wpred.tobytes() and np.array_equal(ak, wak) and np.array_equal(imp, wimp.astype(bool))
    assert 0 < imp.sum() < len(test)
    assert algo.rmse(test) == E.rmse([t[2] for t in test], wpred)
    q = int(np.nonzero((qu >= 0) & (qi >= 0) & (wimp == 0))[0][0])
    assert algo.estimate(int(qu[q]), int(qi[q])) == (west[q], {"actual_k": int(wak[q])})


@pytest.mark.parametrize("name", ["pearson", "pearson_baseline"])
def test_knnbasic_weights_and_wrappers(raw_case, name):
    """fit(trainset, weights) weights the products; the wrappers return every accumulator of the restatement."""
    import torch
    from n2v_hip import eccknn
    users, items, r, test = raw_case
    ts = eccknn.Trainset.from_ratings(users, items, r)
    wd = {raw: float(np.sin(i) + 0.3) for i, raw in enumerate(dict.fromkeys(items))}
    w = np.array([wd[raw] for raw in dict.fromkeys(items)])
    algo = eccknn.KNNBasic(sim_options={"name": name, "min_support": 2}).fit(ts, wd)
    want = restate_knn(name, ts.u, ts.i, r, ts.n_users, ts.n_items, ts, True, 2, w, 100, {})
    assert E.canon(algo.sim.cpu().numpy()) == E.canon(want["sim"])
    plain = eccknn.KNNBasic(sim_options={"name": name, "min_support": 2}).fit(ts)
    assert plain.sim.cpu().numpy().tobytes() != algo.sim.cpu().numpy().tobytes()
    to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dt)
    dx, dy, dr, dw = to(ts.u, torch.int32), to(ts.i, torch.int32), to(ts.r, torch.float64), to(w, torch.float64)
    kw = {"w": dw, "min_support": 2}
    if name == "pearson_baseline":
        kw.update(global_mean=ts.global_mean, bx=algo.bx, by=algo.by)
    dense, mask = eccknn.densify(dx, dy, dr, ts.n_users, ts.n_items)
    xr = eccknn.csr_by_x(dx, dy, dr, ts.n_users, ts.n_items)
    for sim, acc in (eccknn.similarity_pearson(dense, mask, name, accumulators=True, **kw),
                     eccknn.similarity_pearson_sparse(xr, ts.n_items, name, accumulators=True, **kw)):
        assert_same(dict({k: v.cpu().numpy() for k, v in acc.items()}, sim=sim.cpu().numpy()), want, (name, "python"))
    bad = (xr[0], torch.flip(xr[1], [0]).contiguous(), xr[2])    # rows descending: refused before the kernel
    with pytest.raises(ValueError, match="ascending"):
        eccknn.similarity_pearson_sparse(bad, ts.n_items, name, **kw)
    with pytest.raises(ValueError, match="weights"):
        eccknn.similarity_pearson(dense, mask, name, **dict(kw, w=dw[:5].contiguous()))
    if name == "pearson_baseline":
        with pytest.raises(ValueError, match="bx"):
            eccknn.similarity_pearson(dense, mask, name, w=dw)


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_main_rec_algo_knn_prints_the_restatements_rmse(tmp_path, capsys, form):
    import main_rec
    rs = np.random.RandomState(31)
    cells = rs.permutation(40 * 30)[:500]
    lines = ["userId,movieId,rating,timestamp"] + ["%d,%d,%.1f,%d" % (c // 30 + 1, c % 30 + 100, rs.randint(1, 11) * 0.5, n)
                                                    for n, c in enumerate(cells)]
    p = tmp_path / "ratings.csv"
    p.write_text("\n".join(lines) + "\n")
    err = main_rec.main(["-input", str(p), "-algo", "knn", "-sim", "pearson_baseline", "-shrinkage", "50", "-k", "20",
                         "-test-ratio", "0.25", "-seed", "4", "-form", form])
    assert capsys.readouterr().out.strip() == "RMSE: %r" % err
    users, items, ratings = main_rec.read_ratings(str(p))
    train, test = main_rec.split(500, 0.25, 4)
    x, xraw = E.inner_ids([users[i] for i in train]); y, yraw = E.inner_ids([items[i] for i in train])
    r = ratings[train]
    mean = E.global_mean(r)
    bu, bi = P.baselines_als(P.rows_of(x, y, r, len(xraw)), P.rows_of(y, x, r, len(yraw)), mean)
    yr = E.build_yr(x, y, r)
    sim = P.pearson_baseline_numpy(len(xraw), yr, 1, mean, bu, bi, 50)["sim"]
    qx = [xraw.index(users[i]) if users[i] in xraw else -1 for i in test]
    qy = [yraw.index(items[i]) if items[i] in yraw else -1 for i in test]
    est, _, imp = E.estimate_all(sim, yr, qx, qy, 20, 1)
    pred = E.predict_all(est, imp, mean, float(ratings.min()), float(ratings.max()))
    assert err == E.rmse(ratings[test], pred)
