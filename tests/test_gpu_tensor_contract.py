"""GPU tests: the module-level functions of n2v_hip.eccknn, svd, nmf, slopeone and coclustering hold their callers to the
types their docstrings state (the table of tests/tensor_contract_cases.py).

The malformed half runs with the loaded library replaced by NoLaunch: every ill-formed argument (another dtype, a CPU
tensor, a strided view, one element more or less, another rank, None, another GPU) must be a ValueError that names the
argument, raised before any entry point that takes a pointer is called, with every in-place argument left as it was.
Nothing is launched on ill-formed input, by construction.

The well-formed half runs the kernels: a tensor carved out of a larger buffer at an odd element offset gives the bytes
of the plain call and nothing outside it is written; the classes return what the module-level path returns; and
consistency.feature_rows, which picks its 16-byte path from the alignment of its operands, equals the numpy gather on
both paths."""
import re

import numpy as np
import pytest
import torch

import tensor_contract_cases as TC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
SENTINEL = {torch.float64: -1.2345e300, torch.float32: -1.2345e30, torch.int32: -1234567, torch.int64: -1234567890123,
            torch.uint8: 0xA5}


@pytest.fixture(scope="module")
def world():
    return TC.make_world(DEV)


@pytest.fixture
def armed(world, monkeypatch):
    """The library behind NoLaunch for one test; the world was built before it."""
    from n2v_hip import _lib
    proxy = TC.NoLaunch(_lib.load(), _lib.SIGNATURES)
    monkeypatch.setattr(_lib, "_lib", proxy)
    assert _lib.load() is proxy
    return proxy


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def spec(name, path):
    return next(a for a in TC.TABLE[name]["args"] if a.path == path)


# ---- malformed: refused by name, before the library ---------------------------------------------------------------------

def test_the_proxy_is_armed_and_the_pointer_free_entry_points_still_answer(world, armed):
    from n2v_hip import _lib, eccknn
    lib = _lib.load()
    assert lib.n2v_abi_version() >= 1 and lib.n2v_eccknn_max_k() == eccknn.MAX_K and lib.n2v_topn_segments(70, 150) >= 1
    fn, kwargs = TC.baseline(world, "eccknn.predict")
    with pytest.raises(AssertionError, match="library called: n2v_eccknn_predict"):      # a well-formed call gets this far
        fn(**kwargs)
    assert armed.calls == ["n2v_eccknn_predict"]


@pytest.mark.parametrize("name,path,mutation", TC.malformed_rows(), ids=lambda v: str(v))
def test_a_malformed_argument_is_a_value_error_that_names_it(world, armed, name, path, mutation):
    fn, kwargs = TC.baseline(world, name)
    arg = spec(name, path)
    good = TC.get(kwargs, path)
    assert str(good.dtype) == "torch." + arg.dtype and good.dim() == arg.rank and good.is_contiguous() and good.numel() > 1
    bad = TC.mutate(good, arg, mutation)
    if mutation == "other_device" and bad is None:
        pytest.skip("one visible GPU")
    if bad is not None:
        assert bad.device != good.device or not bad.is_contiguous() or not same_bytes(bad, good)     # the mutation took
    written = {a.path: TC.get(kwargs, a.path) for a in TC.TABLE[name]["args"] if "w" in a.flags}
    before = {p: t.clone() for p, t in written.items()}
    with pytest.raises(ValueError) as e:
        fn(**TC.put(kwargs, path, bad))
    assert re.search(r"\b(%s)\b" % "|".join(re.escape(n) for n in TC.names(arg)), str(e.value)), str(e.value)
    assert armed.calls == [], (armed.calls, str(e.value))
    for p, t in written.items():
        assert same_bytes(t, before[p]), p


def test_torchs_default_integers_are_refused_not_reinterpreted(world, armed):
    """torch.tensor([3, 1, 2]) is int64; read as int32 words it would be the queries 3, 0, 1."""
    from n2v_hip import eccknn
    knn = world["knn"]
    q = torch.tensor([3, 1, 2], device=DEV)
    assert q.dtype == torch.int64
    with pytest.raises(ValueError, match=r"eccknn\.estimate_batch: qx must be a contiguous int32"):
        eccknn.estimate_batch(knn.sim, knn.yr, q, q, 40, 1)
    est = world["est"]
    with pytest.raises(ValueError, match="impossible"):                               # predict takes uint8, as it says: no bool
        eccknn.predict(est, world["imp"].to(torch.bool), 3.0, (1.0, 5.0))
    with pytest.raises(TypeError, match="qx"):
        eccknn.estimate_batch(knn.sim, knn.yr, [3, 1, 2], q.to(torch.int32), 40, 1)
    assert armed.calls == []


# ---- well-formed (a): carved views ------------------------------------------------------------------------------------------

def carve(t, offset):
    """(buffer, view): the values of t at element `offset` past GUARD sentinels, GUARD more after them."""
    n = t.numel()
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL[t.dtype], dtype=t.dtype, device=t.device)
    view = buf[GUARD + offset:GUARD + offset + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + (GUARD + offset) * t.element_size()
    return buf, view


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("name", TC.PUBLIC)
def test_a_carved_view_gives_the_plain_calls_bytes_and_nothing_outside_is_written(world, name, offset):
    fn, kwargs = TC.baseline(world, name)
    args = [a for a in TC.TABLE[name]["args"] if "c" not in a.flags and TC.get(kwargs, a.path) is not None]
    inputs = {a.path: TC.get(kwargs, a.path).clone() for a in args if "w" not in a.flags}
    plain = TC.flatten(fn(**kwargs))
    plain_written = {a.path: TC.get(kwargs, a.path) for a in args if "w" in a.flags}
    for p, t in inputs.items():
        assert same_bytes(TC.get(kwargs, p), t), p                   # the plain call left its inputs alone

    _, carved_kwargs = TC.baseline(world, name)
    bufs = {}
    for a in args:
        buf, view = carve(TC.get(carved_kwargs, a.path), offset)
        bufs[a.path] = (buf, buf.clone(), view)
        carved_kwargs = TC.put(carved_kwargs, a.path, view)
    got = TC.flatten(fn(**carved_kwargs))
    torch.cuda.synchronize()
    assert len(got) == len(plain) and all(g == w for g, w in zip(got, plain)), name
    for a in args:
        buf, snapshot, view = bufs[a.path]
        if "w" in a.flags:
            lo = GUARD + offset
            assert same_bytes(buf[:lo], snapshot[:lo]) and same_bytes(buf[lo + view.numel():], snapshot[lo + view.numel():]), a.path
            assert same_bytes(view, plain_written[a.path]), a.path
        else:
            assert same_bytes(buf, snapshot), a.path


def test_the_in_place_calls_did_write(world):
    """What the carved test compares is not an untouched copy: each in-place call changes its argument."""
    for name in ("svd.epoch", "nmf.epoch", "coclustering.assign"):
        fn, kwargs = TC.baseline(world, name)
        written = [a.path for a in TC.TABLE[name]["args"] if "w" in a.flags]
        before = {p: TC.get(kwargs, p).clone() for p in written}
        fn(**kwargs)
        changed = [p for p in written if not same_bytes(TC.get(kwargs, p), before[p])]
        assert changed if name == "coclustering.assign" else changed == written, (name, changed)


# ---- well-formed (b): the classes return what the module-level path returns -----------------------------------------------------

def module_level(W, key):
    """(estimates of the world's queries, top-10 lists) through the module-level functions, from the fitted tensors of W[key]."""
    from n2v_hip import coclustering, eccknn, slopeone, svd
    a, ts = W[key], W["ts"]
    mean, scale, seen, qu, qi = ts.global_mean, ts.rating_scale, W["seen"], W["qu"], W["qi"]
    if key in ("knn", "eccen"):
        return (eccknn.estimate_batch(a.sim, a.yr, qu, qi, a.k, a.min_k),
                eccknn.top_n(a.sim, a.yr, seen, True, a.k, a.min_k, mean, scale, 10))
    if key in ("means", "zscore", "baseline"):
        return (eccknn.estimate_batch_centered(a.sim, a.yr, qu, qi, a.k, a.min_k, a.centering),
                eccknn.top_n_centered(a.sim, a.yr, seen, a.k, a.min_k, scale, 10, a.centering))
    if key in ("svd", "nmf"):
        return (svd.estimate_batch(a.mu, a.biased, a.bu, a.bi, a.pu, a.qi, qu, qi),
                svd.top_n(a.mu, a.biased, a.bu, a.bi, a.pu, a.qi, seen, mean, scale, 10))
    if key == "slopeone":
        return (slopeone.estimate_batch(a.dev, a.freq, a.ur, a.user_mean, qu, qi),
                slopeone.top_n(a.dev, a.freq, a.ur, a.user_mean, seen, mean, scale, 10))
    assert key == "cocl"
    return (coclustering.estimate_batch(a.cltr_u, a.cltr_i, a._avgs(), a.user_mean, a.item_mean, mean, qu, qi),
            coclustering.top_n(a.cltr_u, a.cltr_i, a._avgs(), a.user_mean, a.item_mean, seen, mean, scale, 10))


@pytest.mark.parametrize("key", ["eccen", "knn", "means", "zscore", "baseline", "svd", "nmf", "slopeone", "cocl"])
def test_the_classes_return_what_the_module_level_path_returns(world, key):
    from n2v_hip import eccknn
    algo, ts = world[key], world["ts"]
    (est, *extras, imp), (items, score) = module_level(world, key)
    pred, rmse = eccknn.predict(est, imp, ts.global_mean, ts.rating_scale, world["r_true"])
    got = algo.test(world["testset"])
    assert len(got) == 2 + len(extras)
    assert got[0].tobytes() == pred.cpu().numpy().tobytes() and np.array_equal(got[-1], imp.cpu().numpy().astype(bool))
    for g, w in zip(got[1:-1], extras):
        assert np.array_equal(g, w.cpu().numpy())
    assert algo.rmse(world["testset"]) == rmse
    assert float(eccknn.errors(pred, world["r_true"])[1][0]) == algo.mae(world["testset"])
    c_items, c_score = algo.top_n_lists(10)
    assert torch.equal(c_items, items) and same_bytes(c_score, score)


def test_the_fits_are_the_module_level_calls(world):
    from n2v_hip import coclustering, eccknn, slopeone
    ts, u, i, r = world["ts"], world["u"], world["i"], world["r"]
    ones = torch.ones(ts.n_items, dtype=torch.float64, device=DEV)
    assert same_bytes(eccknn.similarity(*world["dense"], ones, "cosine"), world["knn"].sim)
    assert same_bytes(eccknn.similarity(*world["dense"], world["w"], "cosine"), world["eccen"].sim)
    assert same_bytes(eccknn.similarity_sparse(world["seen"], ones, ts.n_items, "cosine"), world["knn"].sim)
    so = world["slopeone"]
    dev, freq = slopeone.deviations(*eccknn.densify(i, u, r, ts.n_items, ts.n_users))
    assert same_bytes(dev, so.dev) and torch.equal(freq, so.freq)
    dev, freq = slopeone.deviations_sparse(world["xr_items"], ts.n_users)
    assert same_bytes(dev, so.dev) and torch.equal(freq, so.freq)
    cc = world["cocl"]
    avgs = coclustering.averages(cc.ur, ts.n_items, cc.cltr_u, cc.cltr_i, TC.N_CLTR[0], TC.N_CLTR[1], ts.global_mean)
    assert all(same_bytes(a, b) for a, b in zip(avgs, (cc.avg_cltr_u, cc.avg_cltr_i, cc.avg_cocltr, cc.count_cocltr)))
    assert same_bytes(eccknn.row_moments(cc.ur[0], cc.ur[2])[0], cc.user_mean)


# ---- well-formed (c): consistency.feature_rows on both of its paths ---------------------------------------------------------------

@pytest.mark.parametrize("n_bins,d", [(6, 2), (100, 100)])
@pytest.mark.parametrize("prof_offset,vec_offset", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_feature_rows_equal_the_gather_whatever_the_alignment(n_bins, d, prof_offset, vec_offset):
    """Both extents even: the 16-byte path is taken iff profile, vec and X are 16-byte aligned.  One fp64 (8 bytes) or one
    fp32 (4 bytes) of offset takes the scalar path; all four combinations are the same gather."""
    import consistency_reference as R
    import test_gpu_consistency as G
    from n2v_hip import consistency
    user, item, fb, prof, slot, vec = G._feature_case(n_bins, d, "some")
    (pbuf, dprof), (vbuf, dvec) = carve(G._dev(prof, np.float64), prof_offset), carve(G._dev(vec, np.float32), vec_offset)
    assert (dprof.data_ptr() % 16 == 0) == (prof_offset == 0) and (dvec.data_ptr() % 16 == 0) == (vec_offset == 0)
    snapshots = pbuf.clone(), vbuf.clone()
    X, y, rows = consistency.feature_rows(G._dev(user, np.int64), G._dev(item, np.int64), G._dev(fb, np.float64), dprof,
                                          G._dev(slot, np.int32), dvec)
    wX, wy, wrows = G._features_numpy(user, item, fb, prof, slot, vec)
    assert 0 < len(wrows) < len(user)
    assert np.array_equal(rows.cpu().numpy(), wrows) and y.cpu().numpy().tobytes() == wy.tobytes()
    assert tuple(X.shape) == (len(wrows), n_bins + d) and R.canon(X.cpu().numpy()) == R.canon(wX)
    assert same_bytes(pbuf, snapshots[0]) and same_bytes(vbuf, snapshots[1])
