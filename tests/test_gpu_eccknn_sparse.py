"""GPU tests: the sparse (rating-list) form of the EccenKNN similarity (n2v_eccknn_sim_sparse, n2v_eccknn_csr_check;
csrc/n2v_eccknn.hip, C-ABI include/n2v_sim.h) against the restatement tests/eccknn_reference.py and against the dense
kernel, through the C-ABI unless a test says otherwise.

Exact comparisons only, as in tests/test_gpu_eccknn.py: fp64 arrays by their bytes (E.canon), integers with array_equal.
Every output buffer starts as a sentinel.  The similarity kernel is never launched on a malformed CSR: what is malformed
goes to n2v_eccknn_csr_check alone, with valid buffers of the stated sizes."""
import numpy as np
import pytest

import eccknn_reference as E

pytestmark = pytest.mark.gpu

SENT = -12345.5
ISENT = -7
METHOD = {"cosine": 0, "msd": 1}


def _L():
    from n2v_hip import _lib as L
    return L


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host_csr(x, y, r, n_x):
    """x-major CSR with every row ascending in y."""
    x, y, r = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(r, np.float64)
    order = np.lexsort((y, x))
    ptr = np.zeros(n_x + 1, np.int64)
    np.cumsum(np.bincount(x, minlength=n_x), out=ptr[1:])
    return ptr, y[order].astype(np.int32), r[order]


def c_check(ptr, ys, n_x, n_y, n=None):
    """n2v_eccknn_csr_check -> the status word."""
    import torch
    L = _L(); lib = L.load()
    n = len(ys) if n is None else n
    dp, dy = _dev(ptr, np.int64), _dev(ys if len(ys) else [0], np.int32)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(lib.n2v_eccknn_csr_check(L.ptr(dp), L.ptr(dy), n_x, n_y, n, L.ptr(status), L.stream_ptr(status.device)))
    return int(status.item())


def c_dense(x, y, r, w, n_x, n_y, name, min_support):
    """n2v_eccknn_densify + n2v_eccknn_sim, sentinel-filled outputs (the dense tests' c_sim, restated)."""
    import torch
    L = _L(); lib = L.load()
    dx, dy, dr, dw = _dev(x, np.int32), _dev(y, np.int32), _dev(r, np.float64), _dev(w, np.float64)
    dense = torch.full((n_y, n_x), SENT, dtype=torch.float64, device="cuda")
    mask = torch.full((n_y, n_x), 9, dtype=torch.uint8, device="cuda")
    st = L.stream_ptr(dense.device)
    L.check(lib.n2v_eccknn_densify(L.ptr(dx), L.ptr(dy), L.ptr(dr), len(r), n_x, n_y, L.ptr(dense), L.ptr(mask), st))
    out = _outputs(n_x, name)
    g = lambda nm: L.ptr(out[nm]) if nm in out else None
    L.check(lib.n2v_eccknn_sim(L.ptr(dense), L.ptr(mask), n_x, n_y, L.ptr(dw), METHOD[name], min_support,
                               g("sim"), g("freq"), g("prods"), g("sqi"), g("sqj"), g("sq_diff"), st))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _outputs(n_x, name):
    import torch
    f64 = lambda: torch.full((n_x, n_x), SENT, dtype=torch.float64, device="cuda")
    out = {"sim": f64(), "freq": torch.full((n_x, n_x), ISENT, dtype=torch.int32, device="cuda")}
    for nm in (("prods", "sqi", "sqj") if name == "cosine" else ("sq_diff",)):
        out[nm] = f64()
    return out


def c_sparse(x, y, r, w, n_x, n_y, name, min_support, dw=None):
    """host CSR -> n2v_eccknn_csr_check (must be clean) -> n2v_eccknn_sim_sparse; numpy arrays out."""
    import torch
    L = _L(); lib = L.load()
    ptr, ys, rs = host_csr(x, y, r, n_x)
    assert c_check(ptr, ys, n_x, n_y) == 0
    dp, dy, dr = _dev(ptr, np.int64), _dev(ys, np.int32), _dev(rs, np.float64)
    dw = _dev(w, np.float64) if dw is None else dw
    out = _outputs(n_x, name)
    g = lambda nm: L.ptr(out[nm]) if nm in out else None
    L.check(lib.n2v_eccknn_sim_sparse(L.ptr(dp), L.ptr(dy), L.ptr(dr), n_x, n_y, len(rs), L.ptr(dw), METHOD[name], min_support,
                                      g("sim"), g("freq"), g("prods"), g("sqi"), g("sqj"), g("sq_diff"),
                                      L.stream_ptr(dp.device)))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same(got, want, what):
    for key in want:
        if key == "freq":
            assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (key,) + what
        else:
            assert E.canon(got[key]) == E.canon(want[key]), (key,) + what


def check_sparse(x, y, r, w, n_x, n_y, name, min_support, dense=True):
    want = E.NUMPY[name](n_x, E.build_yr(x, y, r), min_support, w)
    got = c_sparse(x, y, r, w, n_x, n_y, name, min_support)
    assert_same(got, want, (name, min_support, n_x, n_y, "restatement"))
    if dense:
        assert_same(got, c_dense(x, y, r, w, n_x, n_y, name, min_support), (name, min_support, n_x, n_y, "dense kernel"))
    s = got["sim"]
    assert E.canon(s) == E.canon(s.T) and np.array_equal(np.diag(s), np.ones(n_x))
    return want, got


# ---- 1: the dense grid again -------------------------------------------------------------------------------------------

KINDS = ["int", "half", "fp64"]


@pytest.mark.parametrize("n_y", [1, 31, 32, 33, 100])
@pytest.mark.parametrize("n_x", [1, 2, 63, 64, 65, 130])
def test_sparse_equals_restatement_and_dense_kernel(n_x, n_y):
    """The cases of test_sim_and_accumulators_bit_for_bit: both similarities, min_support 1 and 3, both roles."""
    kind = KINDS[(n_x + n_y) % 3]
    n = max(1, int((0.3 if n_y <= 33 else 0.2) * n_x * n_y))
    x, y, r, w = E.make_case(1000 * n_x + n_y, n_x, n_y, n, kind, zeros=3 if n >= 6 else 0)
    w_swapped = np.random.RandomState(n_x * 7 + n_y).normal(size=n_x)
    if n >= 6:
        assert (r == 0.0).sum() == 3                         # there is no mask here: a 0.0 rating must still count
    for name in ("cosine", "msd"):
        for ms in (1, 3):
            want, got = check_sparse(x, y, r, w, n_x, n_y, name, ms)
            assert got["freq"].trace() == len(r)             # ... and it does: every rating is on its row's diagonal
            check_sparse(y, x, r, w_swapped, n_y, n_x, name, ms)


# ---- 2: row lengths around the staging constant ------------------------------------------------------------------------

def bound_setters(rows, C):
    """Which row sets the bound in every staging round of a tile that holds exactly `rows` (ascending y lists)."""
    pos, who = [0] * len(rows), []
    while any(p < len(v) for p, v in zip(pos, rows)):
        cand = [(v[p + C - 1], k) for k, (p, v) in enumerate(zip(pos, rows)) if len(v) - p > C]
        if not cand:
            break
        bd, k = min(cand)
        who.append(k)
        pos = [p + sum(1 for yy in v[p:p + C] if yy <= bd) for p, v in zip(pos, rows)]
    return who


@pytest.fixture(scope="module")
def chunk_case():
    C = int(_L().load().n2v_eccknn_sparse_chunk())
    assert C >= 2
    n_x, n_y = 70, 40 * C
    lengths = [0, 1, C - 1, C, C + 1, 2 * C, 3 * C + 5]
    rs = np.random.RandomState(1234)
    rows = [sorted(rs.permutation(n_y)[:lengths[i % 7]].tolist()) for i in range(n_x)]
    sup, sub, lo, hi, ev, od = 5, 2, 3, 4, 6, 13             # all inside the first tile
    rows[sub] = sorted(rs.permutation(rows[sup])[:C - 1].tolist())
    rows[lo] = sorted(rs.permutation(6 * C)[:C].tolist())
    rows[hi] = sorted((20 * C + rs.permutation(6 * C)[:C + 1]).tolist())
    rows[ev] = list(range(0, 2 * (3 * C + 5), 2))
    rows[od] = list(range(1, 2 * (3 * C + 5), 2))
    # the structures this test is about are present
    assert [len(v) for v in rows] == [lengths[i % 7] for i in range(n_x)]
    assert set(len(v) for v in rows[64:]) == set(lengths[1:]) and len(rows[63]) == 0
    assert set(rows[sub]) < set(rows[sup])
    assert rows[lo][-1] < rows[hi][0]
    who = bound_setters([rows[ev], rows[od]], C)
    assert len(who) >= 3 and all(a != b for a, b in zip(who, who[1:])), who
    x = np.array([i for i, v in enumerate(rows) for _ in v])
    y = np.array([yy for v in rows for yy in v])
    order = rs.permutation(len(x))                           # training order is not CSR order
    x, y = x[order], y[order]
    r = rs.normal(size=len(x)) * 3.0 + rs.random_sample(len(x))
    w = rs.normal(size=n_y)
    assert (w < 0).any() and (w > 0).any()
    return C, n_x, n_y, rows, x, y, r, w, (ev, od)


@pytest.mark.parametrize("name", ["cosine", "msd"])
def test_row_lengths_around_the_staging_chunk(chunk_case, name):
    C, n_x, n_y, rows, x, y, r, w, (ev, od) = chunk_case
    for ms in (1, 3):
        want, got = check_sparse(x, y, r, w, n_x, n_y, name, ms)
    f = want["freq"]
    assert f[5, 2] == C - 1 and f[3, 4] == 0 and f[ev, od] == 0 and f[0].sum() == 0 and f[69, 69] == 3 * C + 5
    # the two interleaved rows alone in a tile, then each against itself shifted by one
    keep = (x == ev) | (x == od)
    x2 = np.where(x[keep] == ev, 0, 1)
    check_sparse(x2, y[keep], r[keep], w, 2, n_y, name, 1)
    check_sparse(x2, y[keep] - x2, r[keep], w, 2, n_y, name, 1)   # now identical y lists: every entry is a hit


# ---- 3: very sparse, wide y --------------------------------------------------------------------------------------------

def test_very_sparse_wide_y():
    n_x, n_y = 130, 100000
    rs = np.random.RandomState(99)
    cells = rs.randint(0, n_x * n_y, size=2400)
    hot = rs.permutation(n_y)[:40]                           # co-ratings need shared y: fold a third onto 40 of them
    x, y = cells // n_y, cells % n_y
    y[::3] = hot[rs.randint(0, 40, size=len(y[::3]))]
    keys = rs.permutation(np.unique(x * n_y + y))[:2000]
    x, y = keys // n_y, keys % n_y
    r = rs.randint(1, 11, size=len(x)) * 0.5
    w = rs.normal(size=n_y)
    assert len(x) == 2000 and y.max() > 99000
    for name in ("cosine", "msd"):
        want, got = check_sparse(x, y, r, w, n_x, n_y, name, 1)
        f = want["freq"]
        assert (f[np.triu_indices(n_x, 1)] > 0).sum() > 100


# ---- 4: past the dense limit -------------------------------------------------------------------------------------------

def test_past_the_dense_limit():
    import torch
    L = _L(); lib = L.load()
    n_x, n_small, N = 70, 300, (1 << 25) + 3
    x, y, r, w = E.make_case(4321, n_x, n_small, 4000, "half")
    assert n_x * N > lib.n2v_eccknn_max_dense() and set(y.tolist()) == set(range(n_small))
    rs = np.random.RandomState(8)
    inner = np.sort(rs.permutation(np.unique(rs.randint(1, N - 1, size=2 * n_small)))[:n_small - 2])
    ymap = np.concatenate([[0], inner, [N - 1]]).astype(np.int64)
    assert len(ymap) == n_small and (np.diff(ymap) > 0).all() and ymap[y.min()] == 0 and ymap[y.max()] == N - 1
    w_big = np.full(N, np.nan)
    w_big[ymap] = w
    one = torch.zeros(8, dtype=torch.float64, device="cuda")
    rc = lib.n2v_eccknn_sim(L.ptr(one), L.ptr(one), n_x, N, L.ptr(one), 0, 1, L.ptr(one), None, None, None, None, None,
                            L.stream_ptr(one.device))
    assert rc != 0 and "dense limit" in lib.n2v_last_error().decode()
    dw = _dev(w_big, np.float64)
    yr = E.build_yr(x, y, r)                                 # a monotone relabelling of y changes no pair's order
    for name in ("cosine", "msd"):
        want = E.NUMPY[name](n_x, yr, 1, w)
        got = c_sparse(x, ymap[y], r, None, n_x, N, name, 1, dw=dw)
        assert not np.isnan(got["sim"]).any()
        assert_same(got, want, (name, "mapped"))


# ---- 5: csr_check and argument errors ----------------------------------------------------------------------------------

def test_csr_check_names_what_is_wrong():
    """Valid buffers of the stated sizes, logically malformed; only the integer check runs on them."""
    n_x, n_y = 4, 10
    ptr = [0, 2, 4, 6, 8]
    ys = [0, 1, 2, 3, 4, 5, 6, 7]
    assert c_check(ptr, ys, n_x, n_y) == 0
    assert c_check(ptr, [0, 5, 1, 6, 2, 7, 3, 8], n_x, n_y) == 0       # a descent across a row boundary is legal
    assert c_check([0, 0, 2, 2, 8], [4, 5, 0, 1, 2, 3, 8, 9], n_x, n_y) == 0   # empty rows
    assert c_check([0, 0, 0, 0, 0], [], n_x, n_y, n=0) == 0
    assert c_check([0, 4, 2, 6, 8], ys, n_x, n_y) == 1                  # not monotone
    assert c_check([0, 2, 4, 6, 9], ys, n_x, n_y) == 1                  # past n
    assert c_check([-1, 2, 4, 6, 8], ys, n_x, n_y) == 1
    assert c_check(ptr, [-1, 1, 2, 3, 4, 5, 6, 7], n_x, n_y) == 2
    assert c_check(ptr, [0, 1, 2, 3, 4, 5, 6, 10], n_x, n_y) == 2       # y = n_y
    assert c_check(ptr, [1, 0, 2, 3, 4, 5, 6, 7], n_x, n_y) == 4        # a descending row
    assert c_check(ptr, [0, 1, 2, 2, 4, 5, 6, 7], n_x, n_y) == 4        # a repeated y
    assert c_check(ptr, [0, 1, 3, 2, 4, 5, 6, 12], n_x, n_y) == 6


def test_argument_errors_launch_nothing():
    import torch
    L = _L(); lib = L.load()
    assert lib.n2v_eccknn_sparse_chunk() >= 2
    n_x, n_y = 4, 10
    dp, dy = _dev([0, 2, 4, 6, 8], np.int64), _dev(np.arange(8), np.int32)
    dr, dw = _dev(np.ones(8), np.float64), _dev(np.ones(n_y), np.float64)
    out = _outputs(n_x, "cosine")
    st = L.stream_ptr(dp.device)
    call = lambda nx, ny, n, method, sim: lib.n2v_eccknn_sim_sparse(
        L.ptr(dp), L.ptr(dy), L.ptr(dr), nx, ny, n, L.ptr(dw), method, 1, sim, L.ptr(out["freq"]), L.ptr(out["prods"]),
        L.ptr(out["sqi"]), L.ptr(out["sqj"]), None, st)
    for args, word in (((0, n_y, 8, 0, L.ptr(out["sim"])), "n_x=0"), ((n_x, 0, 8, 0, L.ptr(out["sim"])), "n_y=0"),
                       ((n_x, 1 << 31, 8, 0, L.ptr(out["sim"])), "n_y="), ((n_x, n_y, -1, 0, L.ptr(out["sim"])), "n=-1"),
                       ((n_x, n_y, 8, 2, L.ptr(out["sim"])), "method 2"), ((n_x, n_y, 8, 0, None), "null"),
                       ((65535 * 64 + 1, n_y, 8, 0, L.ptr(out["sim"])), "tiles")):
        assert call(*args) != 0
        assert word in lib.n2v_last_error().decode(), lib.n2v_last_error().decode()
    status = torch.full((1,), ISENT, dtype=torch.int32, device="cuda")
    assert lib.n2v_eccknn_csr_check(L.ptr(dp), L.ptr(dy), 0, n_y, 8, L.ptr(status), st) != 0
    assert lib.n2v_eccknn_csr_check(L.ptr(dp), L.ptr(dy), n_x, n_y, 8, None, st) != 0
    torch.cuda.synchronize()
    assert int(status.item()) == ISENT
    assert (out["sim"] == SENT).all() and (out["freq"] == ISENT).all() and (out["prods"] == SENT).all()
    assert call(n_x, n_y, 8, 0, L.ptr(out["sim"])) == 0      # the same buffers are fine once the arguments are
    torch.cuda.synchronize()
    assert np.array_equal(out["freq"].cpu().numpy(), np.diag([2, 2, 2, 2]).astype(np.int32))


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


@pytest.mark.parametrize("name", ["cosine", "msd"])
@pytest.mark.parametrize("user_based", [True, False])
def test_form_sparse_equals_form_dense(raw_case, name, user_based):
    from n2v_hip import eccknn
    users, items, r, test = raw_case
    ts = eccknn.Trainset.from_ratings(users, items, r, rating_scale=(2.5, 3.0))
    wd = {raw: float(np.sin(i) + 0.3) for i, raw in enumerate(dict.fromkeys(items if user_based else users))}
    algos = {}
    for form in ("dense", "sparse"):
        opts = {"name": name, "user_based": user_based, "min_support": 3, "form": form}
        algos[form] = eccknn.EccenKNN(k=20, min_k=8, sim_options=opts).fit(ts, wd)
    d, s = algos["dense"], algos["sparse"]
    assert s.form == "sparse" and tuple(s.sim.shape) == tuple(d.sim.shape)
    assert s.sim.cpu().numpy().tobytes() == d.sim.cpu().numpy().tobytes()
    for a, b in zip(s.test(test), d.test(test)):
        assert a.tobytes() == b.tobytes()
    assert s.rmse(test) == d.rmse(test)
    auto = eccknn.EccenKNN(k=20, min_k=8, sim_options={"name": name, "user_based": user_based, "min_support": 3})
    assert auto.form == "auto" and eccknn.choose_form(ts.n_users, ts.n_items, auto.form) == "dense"


def test_python_wrappers_and_errors(raw_case):
    import torch
    from n2v_hip import eccknn
    with pytest.raises(ValueError, match="bogus"):
        eccknn.EccenKNN(sim_options={"name": "msd", "form": "bogus"})
    x, y, r, w = E.make_case(5, 66, 40, 500, "fp64")
    to = lambda a, dt: torch.as_tensor(a).to(device="cuda", dtype=dt)
    xr = eccknn.csr_by_x(to(x, torch.int32), to(y, torch.int32), to(r, torch.float64), 66, 40)
    ptr, ys, rs = host_csr(x, y, r, 66)
    assert np.array_equal(xr[0].cpu().numpy(), ptr) and np.array_equal(xr[1].cpu().numpy(), ys)
    assert xr[2].cpu().numpy().tobytes() == rs.tobytes() and xr[1].dtype == torch.int32 and xr[0].dtype == torch.int64
    assert all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in
               zip(xr, eccknn.csr_by_x(to(x, torch.int64), to(y, torch.int64), to(r, torch.float64), 66)))
    dw = to(w, torch.float64)
    for name in ("cosine", "msd"):
        want = E.NUMPY[name](66, E.build_yr(x, y, r), 2, w)
        sim, acc = eccknn.similarity_sparse(xr, dw, 40, name, min_support=2, accumulators=True)
        got = dict({k: v.cpu().numpy() for k, v in acc.items()}, sim=sim.cpu().numpy())
        assert set(got) == set(want)
        assert_same(got, want, (name, "python"))
        assert eccknn.similarity_sparse(xr, dw, 40, name, min_support=2).cpu().numpy().tobytes() == got["sim"].tobytes()
    bad = (xr[0], torch.flip(xr[1], [0]).contiguous(), xr[2])            # rows descending: refused before the kernel
    with pytest.raises(ValueError, match="ascending"):
        eccknn.similarity_sparse(bad, dw, 40, "msd")
    with pytest.raises(ValueError, match="outside"):
        eccknn.similarity_sparse(xr, dw[:30].contiguous(), 30, "msd")


def test_main_rec_form_sparse_prints_the_same_rmse(tmp_path, capsys):
    import main_rec
    rs = np.random.RandomState(31)
    cells = rs.permutation(40 * 30)[:500]
    lines = ["userId,movieId,rating,timestamp"] + ["%d,%d,%.1f,%d" % (c // 30 + 1, c % 30 + 100, rs.randint(1, 11) * 0.5, n)
                                                    for n, c in enumerate(cells)]
    p = tmp_path / "ratings.csv"
    p.write_text("\n".join(lines) + "\n")
    q = tmp_path / "w.csv"
    q.write_text("\n".join("%d,%r" % (i + 100, float(rs.normal())) for i in range(30)) + "\n")
    out = {}
    for form in ("dense", "sparse", "auto"):
        for extra in ([], ["-item-based", "-sim", "cosine"]):
            args = ["-input", str(p), "-k", "20", "-sim", "msd", "-test-ratio", "0.25", "-seed", "4", "-form", form]
            args += extra if extra else ["-weights", str(q)]
            err = main_rec.main(args)
            text = capsys.readouterr().out.strip()
            assert text == "RMSE: %r" % err
            out[form, bool(extra)] = text
    for item_based in (False, True):
        assert out["sparse", item_based] == out["dense", item_based] == out["auto", item_based]
