"""The BiNE preparation kernels of csrc/n2v_bine.hip (spmv, HITS normalise, walk counts, walk lengths, walks, negative
pools, init) against their restatements, bit for bit and element for element: through the C-ABI on the launches of
tests/bine_prep_cases.py, and through BineEngine on the same graphs.

Every array that reaches a kernel here is built by tests/bine_prep_cases.py and was replayed with bounds-checked
indexing by tests/test_bine_prep_host.py; nothing else is launched.  The refusal tests pass only arguments that the
C-ABI turns down before it launches anything, and check that the outputs stay as they were.

No comparison in this file has a tolerance.  The whole file (96 tests) took 3.6 s on MI355X when it was added; its
expected values are pure Python and dominate that time."""
import numpy as np
import pytest

import bine_prep_cases as K
import bine_prep_reference as P

pytestmark = pytest.mark.gpu

ERR_INVALID = -1


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


@pytest.fixture(scope="module")
def lib():
    from n2v_hip import _lib
    return _lib.load()


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(t):
    return t.cpu().numpy()


def stream():
    from n2v_hip import _lib
    return _lib.stream_ptr("cuda:0")


def ptr(t):
    from n2v_hip import _lib
    return _lib.ptr(t)


def ok(rc):
    from n2v_hip import _lib
    _lib.check(rc)


# ------------------------------------------------------------------------------------------ HITS
@pytest.mark.parametrize("name", K.HITS_CASES)
def test_spmv_bits(lib, name):
    L = K.spmv_launch(name)
    d = {k: dev(L[k]) for k in ("row_ptr", "col", "w", "x", "y")}
    ok(lib.n2v_bine_spmv(L["n_rows"], ptr(d["row_ptr"]), ptr(d["col"]), ptr(d["w"]), ptr(d["x"]), ptr(d["y"]), stream()))
    assert same_bits(host(d["y"]), P.spmv(L["row_ptr"], L["col"], L["w"], L["x"]))


@pytest.mark.parametrize("key", K.HITS_CASES + K.NORMALISE_SIZES, ids=str)
def test_hits_normalise_bits(lib, key):
    L = K.normalise_launch(key)
    d = {k: dev(L[k]) for k in ("h", "a", "h_last", "state")}
    ok(lib.n2v_bine_hits_normalise(L["n"], ptr(d["h"]), ptr(d["a"]), ptr(d["h_last"]), ptr(d["state"]), stream()))
    h, a, err = P.hits_normalise(L["h"], L["a"], L["h_last"])
    assert same_bits(host(d["h"]), h) and same_bits(host(d["a"]), a) and same_bits(host(d["state"]), [err])
    assert same_bits(host(d["h_last"]), L["h_last"])


@pytest.mark.parametrize("c", K.COUNTS_CASES, ids=K.counts_id)
def test_walk_counts_bits(lib, c):
    L = K.counts_launch(c)
    a, counts, auth = dev(L["a"]), dev(L["counts"]), dev(L["auth_out"])
    ok(lib.n2v_bine_walk_counts(ptr(a), L["lo"], L["hi"], L["maxT"], L["minT"], ptr(counts), ptr(auth), stream()))
    want_c, want_s = P.walk_counts(L["a"], L["lo"], L["hi"], L["maxT"], L["minT"])
    full = L["counts"].copy()
    full[L["lo"]:L["hi"]] = want_c
    assert np.array_equal(host(counts), full)                     # and nothing outside [lo, hi) was written
    if auth is not None:
        full = L["auth_out"].copy()
        full[L["lo"]:L["hi"]] = want_s
        assert same_bits(host(auth), full)


# ------------------------------------------------------------------------------------------ walks
@pytest.mark.parametrize("c", K.WALK_CASES, ids=K.walk_id)
def test_walk_lengths_and_walks_equal_the_oracle(lib, c):
    node, lens, off, want, _ = K.walk_expected(c)
    launches, tokens = K.walk_launches(c)
    tok = dev(tokens)
    g = {k: dev(launches[0][k]) for k in ("row_ptr", "col", "cum2")}
    for L in launches:
        wn, wo, ln = dev(L["walk_node"]), dev(L["walk_off"]), dev(L["lens"])
        ok(lib.n2v_bine_walk_lengths(ptr(g["row_ptr"]), ptr(g["cum2"]), ptr(wn), L["n_walks"], L["gw_base"],
                                     float(L["percentage"]), L["max_len"], L["seed"], ptr(ln), stream()))
        # the walk kernel trusts its offsets: it gets the oracle's (replayed on the host), after the device agreed
        assert np.array_equal(host(ln), lens[L["first"]:L["first"] + L["n_walks"]])
        ok(lib.n2v_bine_walk(ptr(g["row_ptr"]), ptr(g["col"]), ptr(g["cum2"]), ptr(wn), ptr(wo), L["n_walks"],
                             L["gw_base"], L["seed"], ptr(tok), stream()))
    assert np.array_equal(host(tok), want)


# ------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize("c", K.POOL_CASES, ids=K.pool_id)
def test_negative_pools_equal_the_oracle(lib, c):
    L = K.pool_launch(c)
    rp, col, pool = dev(L["row_ptr"]), dev(L["col"]), dev(L["pool"])
    ok(lib.n2v_bine_neg_pools(ptr(rp), ptr(col), L["side_lo"], L["side_hi"], L["v_begin"], L["v_end"], L["pool_size"],
                              float(L["max_jaccard"]), L["seed"], ptr(pool), stream()))
    want, _ = K.pool_expected(c)
    assert np.array_equal(host(pool).reshape(want.shape), want)


# ------------------------------------------------------------------------------------------ init
@pytest.mark.parametrize("c", K.INIT_CASES, ids=str)
def test_init_bits(lib, c):
    L = K.init_launch(c)
    emb, ctx = dev(L["emb"]), dev(L["ctx"])
    ok(lib.n2v_bine_init(ptr(emb), ptr(ctx), L["n"], L["dim"], L["row_stride"], L["seed"], stream()))
    want_e, want_c = K.init_expected(c)
    assert same_bits(host(emb), want_e.ravel()) and same_bits(host(ctx), want_c.ravel())     # padding zeros included


# ------------------------------------------------------------------------------------------ engine path
@pytest.mark.parametrize("c", K.ENGINE_CASES, ids=lambda c: c["graph"])
def test_engine_path_equals_the_restatements(c):
    from n2v_hip import bine
    g = K.graph(c["graph"])
    want = K.engine_expected(c)
    e = bine.BineEngine(g, device="cuda:0", seed=c["seed"])
    e.calculate_centrality()
    assert e.hits_iterations == want["iterations"] and same_bits(host(e.authority), want["authority"])
    if not c["walks"]:
        return
    assert np.array_equal(host(e.cum2), K.cum2(c["graph"]))
    e.generate_walks(percentage=0.15, maxT=c["maxT"], minT=1)
    assert np.array_equal(host(e.counts), want["counts"]) and same_bits(host(e.auth_scaled), want["auth"])
    assert e.n_walks == want["n_walks"] and np.array_equal(host(e.walk_node), want["node"])
    assert np.array_equal(host(e.walk_off), want["off"]) and np.array_equal(host(e.tokens), want["tokens"])
    e.build_negative_pools(pool_size=c["pool_size"], max_jaccard=c["max_jaccard"])
    assert np.array_equal(host(e.pool), want["pool"])
    e.init_embeddings(d=c["dim"])
    assert same_bits(host(e.emb), want["emb"]) and same_bits(host(e.ctx), want["ctx"])


def test_engine_hits_with_user_edges():
    from n2v_hip import bine
    e = bine.BineEngine(K.graph("skew"), device="cuda:0", seed=3)
    src, dst, weight = K.USER_EDGES
    rp, col, w = K.hits_csr("skew+users")
    assert e.add_user_edges(src, dst, weight) == bine.user_edges_csr(e.g, src, dst, weight)[3]
    assert all(np.array_equal(host(t), x) for t, x in zip(e.hits_csr, (rp, col, w)))
    e.calculate_centrality()
    a, iters = K.hits_expected("skew+users")
    assert e.hits_iterations == iters and same_bits(host(e.authority), a)
    assert not same_bits(a, K.hits_expected("skew")[0])


def test_engine_pools_of_a_side_of_one_vertex_and_empty_graph():
    from n2v_hip import bine
    e = bine.BineEngine(K.graph("single_user"), device="cuda:0", seed=1)
    e.build_negative_pools(pool_size=5, max_jaccard=0.1)
    pool = host(e.pool)
    assert (pool[0] == -1).all() and (pool[1:] >= 1).all() and (pool[1:] != np.arange(1, 4)[:, None]).all()
    with pytest.raises(ValueError, match="no ratings"):
        bine.BineEngine(bine.BipartiteGraph([], [], []), device="cuda:0").calculate_centrality()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_return_before_the_launch_and_leave_outputs_alone(lib):
    """Each call differs from a valid one (the table's) in the one argument named, which the C-ABI refuses before
    launching; the arrays themselves are always the valid ones."""
    import torch
    S = K.spmv_launch("rows")
    N = K.normalise_launch(5)
    C = K.counts_launch(K.COUNTS_CASES[0])
    W = K.walk_launches(K.WALK_CASES[3])
    Wl, Wtok = W[0][0], W[1]
    Q = K.pool_launch(K.POOL_CASES[1])
    I = K.init_launch((3, 100))
    d = {k: dev(v) for k, v in dict(rp=S["row_ptr"], col=S["col"], w=S["w"], x=S["x"], y=S["y"], h=N["h"], a=N["a"],
                                    hl=N["h_last"], st=N["state"], ca=C["a"], cc=C["counts"], cs=C["auth_out"],
                                    wrp=Wl["row_ptr"], wcol=Wl["col"], wc2=Wl["cum2"], wn=Wl["walk_node"],
                                    wo=Wl["walk_off"], ln=Wl["lens"], tok=Wtok, qrp=Q["row_ptr"], qcol=Q["col"],
                                    pool=Q["pool"], emb=I["emb"], ctx=I["ctx"]).items()}
    before = {k: t.clone() for k, t in d.items()}
    p = {k: ptr(t) for k, t in d.items()}
    s = stream()
    n, nw = S["n_rows"], Wl["n_walks"]
    lo, hi, vb, ve, ps = Q["side_lo"], Q["side_hi"], Q["v_begin"], Q["v_end"], Q["pool_size"]
    nan = float("nan")
    refused = [
        lib.n2v_bine_spmv(-1, p["rp"], p["col"], p["w"], p["x"], p["y"], s),
        lib.n2v_bine_spmv(n, None, p["col"], p["w"], p["x"], p["y"], s),
        lib.n2v_bine_spmv(n, p["rp"], p["col"], p["w"], None, p["y"], s),
        lib.n2v_bine_spmv(n, p["rp"], p["col"], p["w"], p["x"], None, s),
        lib.n2v_bine_spmv(n, p["rp"], None, p["w"], p["x"], p["y"], s),
        lib.n2v_bine_spmv(n, p["rp"], p["col"], None, p["x"], p["y"], s),
        lib.n2v_bine_hits_normalise(0, p["h"], p["a"], p["hl"], p["st"], s),
        lib.n2v_bine_hits_normalise(-3, p["h"], p["a"], p["hl"], p["st"], s),
        lib.n2v_bine_hits_normalise(5, None, p["a"], p["hl"], p["st"], s),
        lib.n2v_bine_hits_normalise(5, p["h"], None, p["hl"], p["st"], s),
        lib.n2v_bine_hits_normalise(5, p["h"], p["a"], None, p["st"], s),
        lib.n2v_bine_hits_normalise(5, p["h"], p["a"], p["hl"], None, s),
        lib.n2v_bine_walk_counts(None, 0, 9, 8, 1, p["cc"], p["cs"], s),
        lib.n2v_bine_walk_counts(p["ca"], 0, 9, 8, 1, None, p["cs"], s),
        lib.n2v_bine_walk_counts(p["ca"], -1, 9, 8, 1, p["cc"], p["cs"], s),
        lib.n2v_bine_walk_counts(p["ca"], 5, 4, 8, 1, p["cc"], p["cs"], s),
        lib.n2v_bine_walk_counts(p["ca"], 0, 9, -1, 1, p["cc"], p["cs"], s),
        lib.n2v_bine_walk_counts(p["ca"], 0, 9, 8, -1, p["cc"], p["cs"], s),
        lib.n2v_bine_walk_lengths(p["wrp"], p["wc2"], p["wn"], -1, 0, 0.15, 256, 1, p["ln"], s),
        lib.n2v_bine_walk_lengths(p["wrp"], p["wc2"], p["wn"], nw, -1, 0.15, 256, 1, p["ln"], s),
        lib.n2v_bine_walk_lengths(p["wrp"], p["wc2"], p["wn"], nw, 0, 0.15, 0, 1, p["ln"], s),
        lib.n2v_bine_walk_lengths(p["wrp"], p["wc2"], p["wn"], nw, 0, -0.5, 256, 1, p["ln"], s),
        lib.n2v_bine_walk_lengths(p["wrp"], p["wc2"], p["wn"], nw, 0, nan, 256, 1, p["ln"], s),
        lib.n2v_bine_walk_lengths(None, p["wc2"], p["wn"], nw, 0, 0.15, 256, 1, p["ln"], s),
        lib.n2v_bine_walk_lengths(p["wrp"], None, p["wn"], nw, 0, 0.15, 256, 1, p["ln"], s),
        lib.n2v_bine_walk_lengths(p["wrp"], p["wc2"], None, nw, 0, 0.15, 256, 1, p["ln"], s),
        lib.n2v_bine_walk_lengths(p["wrp"], p["wc2"], p["wn"], nw, 0, 0.15, 256, 1, None, s),
        lib.n2v_bine_walk(p["wrp"], p["wcol"], p["wc2"], p["wn"], p["wo"], -1, 0, 1, p["tok"], s),
        lib.n2v_bine_walk(p["wrp"], p["wcol"], p["wc2"], p["wn"], p["wo"], nw, -1, 1, p["tok"], s),
        lib.n2v_bine_walk(None, p["wcol"], p["wc2"], p["wn"], p["wo"], nw, 0, 1, p["tok"], s),
        lib.n2v_bine_walk(p["wrp"], None, p["wc2"], p["wn"], p["wo"], nw, 0, 1, p["tok"], s),
        lib.n2v_bine_walk(p["wrp"], p["wcol"], None, p["wn"], p["wo"], nw, 0, 1, p["tok"], s),
        lib.n2v_bine_walk(p["wrp"], p["wcol"], p["wc2"], None, p["wo"], nw, 0, 1, p["tok"], s),
        lib.n2v_bine_walk(p["wrp"], p["wcol"], p["wc2"], p["wn"], None, nw, 0, 1, p["tok"], s),
        lib.n2v_bine_walk(p["wrp"], p["wcol"], p["wc2"], p["wn"], p["wo"], nw, 0, 1, None, s),
        lib.n2v_bine_neg_pools(p["qrp"], p["qcol"], -1, hi, vb, ve, ps, 0.1, 1, p["pool"], s),
        lib.n2v_bine_neg_pools(p["qrp"], p["qcol"], hi, hi, hi, hi, ps, 0.1, 1, p["pool"], s),
        lib.n2v_bine_neg_pools(p["qrp"], p["qcol"], lo + 1, hi, lo, ve, ps, 0.1, 1, p["pool"], s),
        lib.n2v_bine_neg_pools(p["qrp"], p["qcol"], lo, hi, vb, hi + 1, ps, 0.1, 1, p["pool"], s),
        lib.n2v_bine_neg_pools(p["qrp"], p["qcol"], lo, hi, vb + 2, vb + 1, ps, 0.1, 1, p["pool"], s),
        lib.n2v_bine_neg_pools(p["qrp"], p["qcol"], lo, hi, vb, ve, 0, 0.1, 1, p["pool"], s),
        lib.n2v_bine_neg_pools(p["qrp"], p["qcol"], lo, 2**31, vb, ve, ps, 0.1, 1, p["pool"], s),
        lib.n2v_bine_neg_pools(None, p["qcol"], lo, hi, vb, ve, ps, 0.1, 1, p["pool"], s),
        lib.n2v_bine_neg_pools(p["qrp"], None, lo, hi, vb, ve, ps, 0.1, 1, p["pool"], s),
        lib.n2v_bine_neg_pools(p["qrp"], p["qcol"], lo, hi, vb, ve, ps, 0.1, 1, None, s),
        lib.n2v_bine_init(None, p["ctx"], 3, 100, 128, 1, s),
        lib.n2v_bine_init(p["emb"], None, 3, 100, 128, 1, s),
        lib.n2v_bine_init(p["emb"], p["ctx"], -1, 100, 128, 1, s),
        lib.n2v_bine_init(p["emb"], p["ctx"], 3, 0, 128, 1, s),
        lib.n2v_bine_init(p["emb"], p["ctx"], 3, 100, 64, 1, s),
        lib.n2v_bine_init(p["emb"], p["ctx"], 3, 100, 100, 1, s),
    ]
    assert refused == [ERR_INVALID] * len(refused) and lib.n2v_last_error()
    # an empty range is accepted, and launches nothing either
    accepted = [
        lib.n2v_bine_spmv(0, p["rp"], p["col"], p["w"], p["x"], p["y"], s),
        lib.n2v_bine_walk_counts(p["ca"], 4, 4, 8, 1, p["cc"], p["cs"], s),
        lib.n2v_bine_walk_lengths(p["wrp"], p["wc2"], p["wn"], 0, 0, 0.15, 256, 1, p["ln"], s),
        lib.n2v_bine_walk(p["wrp"], p["wcol"], p["wc2"], p["wn"], p["wo"], 0, 0, 1, p["tok"], s),
        lib.n2v_bine_neg_pools(p["qrp"], p["qcol"], lo, hi, vb, vb, ps, 0.1, 1, p["pool"], s),
        lib.n2v_bine_init(p["emb"], p["ctx"], 0, 100, 128, 1, s),
    ]
    assert accepted == [0] * len(accepted)
    torch.cuda.synchronize()
    assert all(torch.equal(d[k].view(torch.uint8), before[k].view(torch.uint8)) for k in d)
