"""TEST INFRASTRUCTURE — the device-tensor contract of the rating modules' module-level functions, as a table, with one
well-formed call per function and the proxy that keeps a malformed call from ever reaching the library.  Shared by
tests/test_tensor_contract_host.py and tests/test_gpu_tensor_contract.py.  The product never imports this file, and this
file imports neither torch nor the package before a builder runs.

The table: for every function (or __init__) of MODULES whose source hands a tensor to the library, the tensor arguments
by path (`w`, `yr[0]`, `centering.tx`), each with its dtype, its rank and, where the contract ties its length to another
argument, the rule in words.  An argument without a rule *defines* a size (sim defines n_x, qx together with qy n_q), so
one element more or less is another well-formed call, or a mismatch the function reports under the other argument's name.

Flags: "o" optional (None is allowed), "w" written in place, "c" converted by the function itself (any integer sequence or
tensor is accepted, so there is nothing to refuse), "f" either rank 1 or rank 2 is accepted.
"""
import collections
import ctypes
import inspect
import re

MODULES = ("eccknn", "svd", "nmf", "slopeone", "coclustering")
HANDS_OVER = ("_lib.ptr(", "_lib.tensor(")            # what the completeness test looks for in a function's source

Arg = collections.namedtuple("Arg", "path dtype rank tie flags alias")


def A(path, dtype, rank=1, tie=None, flags="", alias=()):
    return Arg(path, dtype, rank, tie, flags, tuple(alias))


def _csr(name, ids, ptr_tie=None, r=True, ids_tie="as many ids as ratings"):
    rows = [A(name + "[0]", "int64", 1, ptr_tie), A(name + "[1]", "int32", 1, ids_tie if r else None)]
    return rows + ([A(name + "[2]", "float64", 1, "as many ratings as ids")] if r else [])


_SIM = [A("sim", "float64", 2, "square: [n_x][n_x]")]
_YR = _csr("yr", "x")
_Q = [A("qx", "int32", 1, "as many as qy"), A("qy", "int32", 1, "as many as qx")]
_QU = [A("qu", "int32", 1, "as many as qi"), A("qi", "int32", 1, "as many as qu")]
_SEEN = _csr("seen", "item", "n_users + 1 entries", r=False) + [A("owners", "int32", 1, None, "oc")]
_DENSE = [A("dense", "float64", 2), A("mask", "uint8", 2, "the shape of dense")]
_XR = _csr("xr", "y")
_FACTORS_FREE = [A("bu", "float64", 1, "n_users = pu's rows"), A("bi", "float64", 1, "n_items = qi's rows"),
                 A("pu", "float64", 2), A("qi", "float64", 2)]
_COCL_MODEL = [A("cltr_u", "int32", 1, "n_users = user_mean's length"), A("cltr_i", "int32", 1, "n_items = item_mean's length"),
               A("avgs[0]", "float64", 1, None, alias=("avg_cltr_u",)), A("avgs[1]", "float64", 1, None, alias=("avg_cltr_i",)),
               A("avgs[2]", "float64", 2, "[n_cltr_u][n_cltr_i]", alias=("avg_cocltr",)),
               A("user_mean", "float64", 1), A("item_mean", "float64", 1)]
_SLOPE_MODEL = [A("dev", "float64", 2, "square: [n_items][n_items]"), A("freq", "int32", 2, "the shape of dev")] \
    + _csr("ur", "item") + [A("user_mean", "float64", 1, "n_users = ur's rows")]

_NMF_LISTS = [A("ur[0]", "int64", 1, "n_users + 1 entries", alias=("user ptr",))] + _csr("ur", "item")[1:] \
    + [A("ir[0]", "int64", 1, "n_items + 1 entries", alias=("item ptr",))] + _csr("ir", "user")[1:] \
    + [A("order[0]", "int32", 1, "n_users", "o"), A("order[1]", "int32", 1, "n_items", "o")]

# name -> dict(args=[Arg], via=[public rows that exercise an internal helper])
TABLE = {
    # ---- eccknn ------------------------------------------------------------------------------------------------------
    "eccknn.densify": dict(args=[A("x", "int32", 1, "as many as r"), A("y", "int32", 1, "as many as r"), A("r", "float64", 1)]),
    "eccknn.similarity": dict(args=_DENSE + [A("w", "float64", 1, "n_y = dense's rows")]),
    "eccknn.csr_check": dict(args=_csr("xr", "y", r=False)),
    "eccknn.similarity_sparse": dict(args=_XR + [A("w", "float64", 1, "n_y")]),
    "eccknn.similarity_pearson": dict(args=_DENSE + [A("w", "float64", 1, "n_y = dense's rows", "o"),
                                                     A("bx", "float64", 1, "n_x = dense's columns"),
                                                     A("by", "float64", 1, "n_y = dense's rows")],
                                      note="bx and by are optional under pearson; the baseline call is pearson_baseline"),
    "eccknn.similarity_pearson_sparse": dict(args=_XR + [A("w", "float64", 1, "n_y", "o"), A("bx", "float64", 1, "n_x = xr's rows"),
                                                         A("by", "float64", 1, "n_y")]),
    "eccknn.row_moments": dict(args=[A("ptr", "int64", 1), A("r", "float64", 1)]),
    "eccknn.yr_check": dict(args=_YR),
    "eccknn.estimate_batch": dict(args=_SIM + _YR + _Q),
    "eccknn.estimate_batch_centered": dict(args=_SIM + _YR + _Q + [A("centering.tx", "float64", 1, "n_x"),
                                                                   A("centering.sd", "float64", 1, "n_x")]),
    "eccknn.predict": dict(args=[A("est", "float64", 1), A("impossible", "uint8", 1, "as many as est"),
                                 A("r_true", "float64", 1, "as many as est", "o")]),
    "eccknn.estimate_sweep": dict(args=_SIM + _YR + _Q + [A("centering.tx", "float64", 1, "n_x"),
                                                          A("centering.by", "float64", 1, "n_y = yr's rows")]),
    "eccknn.errors": dict(args=[A("pred", "float64", 2, None, "f"), A("r_true", "float64", 1, "n_q = pred's columns")]),
    "eccknn.top_n": dict(args=_SIM + _YR + _SEEN),
    "eccknn.top_n_centered": dict(args=_SIM + _YR + _SEEN + [A("centering.tx", "float64", 1, "n_x")]),
    "eccknn.baselines": dict(args=[], note="takes a Trainset and uploads it itself"),
    "eccknn._queries_ptrs": dict(args=_Q, via=["eccknn.estimate_batch", "svd.estimate_batch"]),
    "eccknn._csr_ptrs": dict(args=_csr("triple", "ids"), via=["eccknn.yr_check", "eccknn.csr_check", "nmf.lists"]),
    "eccknn._dense_ptrs": dict(args=_DENSE, via=["eccknn.similarity", "slopeone.deviations"]),
    "eccknn._pearson_inputs": dict(args=[A("w", "float64", 1, "n_y", "o"), A("bx", "float64", 1, "n_x", "o"),
                                         A("by", "float64", 1, "n_y", "o")],
                                   via=["eccknn.similarity_pearson", "eccknn.similarity_pearson_sparse"]),
    "eccknn._pearson_outputs": dict(args=[], note="allocates what it hands over"),
    "eccknn._centering_args": dict(args=[A("c.tx", "float64", 1, "n_x"), A("c.sd", "float64", 1, "n_x", "o"),
                                         A("c.by", "float64", 1, "n_y", "o")],
                                   via=["eccknn.estimate_batch_centered", "eccknn.estimate_sweep", "eccknn.top_n_centered"]),
    "eccknn._knn_model": dict(args=_SIM + _YR, via=["eccknn.estimate_batch", "eccknn.estimate_sweep", "eccknn.top_n"]),
    "eccknn._estimate_batch": dict(args=_SIM + _YR + _Q, via=["eccknn.estimate_batch", "eccknn.estimate_batch_centered"]),
    "eccknn._topn_call": dict(args=_SEEN, via=["eccknn.top_n", "svd.top_n", "slopeone.top_n", "coclustering.top_n"]),
    # ---- svd ---------------------------------------------------------------------------------------------------------
    "svd.Blocks.__init__": dict(args=[A("lists[0]", "int64", 1, "n_strata^2 + 1 entries", alias=("blk_ptr",)),
                                      A("lists[1]", "int32", 1, "as many as blk_i and blk_r", alias=("blk_u", "u")),
                                      A("lists[2]", "int32", 1, "as many as blk_u", alias=("blk_i", "i")),
                                      A("lists[3]", "float64", 1, "as many as blk_u", alias=("blk_r", "r"))]),
    "svd.epoch": dict(args=[A("bu", "float64", 1, "n_users of the blocks", "w"), A("bi", "float64", 1, "n_items of the blocks", "w"),
                            A("pu", "float64", 2, "n_users rows", "w"), A("qi", "float64", 2, "n_items rows", "w")],
                      note="blocks is a checked svd.Blocks, whose fields were held to the contract when it was built"),
    "svd.estimate_batch": dict(args=_FACTORS_FREE + [A("qu", "int32", 1, "as many as qi_ids"), A("qi_ids", "int32", 1, "as many as qu")]),
    "svd.top_n": dict(args=_FACTORS_FREE + _SEEN),
    "svd._model_ptrs": dict(args=_FACTORS_FREE, via=["svd.estimate_batch", "svd.top_n", "svd.epoch"]),
    # ---- nmf ---------------------------------------------------------------------------------------------------------
    "nmf.lists": dict(args=_NMF_LISTS),
    "nmf.Lists.__init__": dict(args=_NMF_LISTS, via=["nmf.lists"]),
    "nmf.epoch": dict(args=[A("pu", "float64", 2, "n_users rows"), A("qi", "float64", 2, "n_items rows"),
                            A("pu_out", "float64", 2, "the shape of pu", "w"), A("qi_out", "float64", 2, "the shape of qi", "w")],
                      note="lists_ is a checked nmf.Lists"),
    # ---- slopeone ----------------------------------------------------------------------------------------------------
    "slopeone.deviations": dict(args=_DENSE),
    "slopeone.deviations_sparse": dict(args=_XR),
    "slopeone.estimate_batch": dict(args=_SLOPE_MODEL + _QU),
    "slopeone.top_n": dict(args=_SLOPE_MODEL + _SEEN),
    "slopeone._model_args": dict(args=_SLOPE_MODEL, via=["slopeone.estimate_batch", "slopeone.top_n"]),
    # ---- coclustering ------------------------------------------------------------------------------------------------
    "coclustering.averages": dict(args=_csr("ur", "item") + [A("cltr_u", "int32", 1, "n_users = ur's rows"),
                                                             A("cltr_i", "int32", 1, "n_items")]),
    "coclustering.assign": dict(args=_csr("lst", "item", "one row per entry of cltr_u")
                                + [A("cltr_u", "int32", 1, None, "w"), A("cltr_i", "int32", 1, None, "w")] + _COCL_MODEL[2:5]
                                + [A("user_mean", "float64", 1, "as many as cltr_u"), A("item_mean", "float64", 1, "as many as cltr_i"),
                                   A("order", "int32", 1, "one entry per row of lst", "o")]),
    "coclustering.estimate_batch": dict(args=_COCL_MODEL + _QU),
    "coclustering.top_n": dict(args=_COCL_MODEL + _SEEN),
    "coclustering._tables": dict(args=_COCL_MODEL[2:], via=["coclustering.assign", "coclustering.estimate_batch"]),
    "coclustering._model_args": dict(args=_COCL_MODEL, via=["coclustering.estimate_batch", "coclustering.top_n"]),
}

PUBLIC = [name for name, row in TABLE.items() if "via" not in row and row["args"]]


# ---- paths ------------------------------------------------------------------------------------------------------------

def root(path):
    return re.match(r"\w+", path).group(0)


def _step(path):
    m = re.fullmatch(r"(\w+)(?:\[(\d+)\]|\.(\w+))?", path)
    return m.group(1), (None if m.group(2) is None else int(m.group(2))), m.group(3)


def get(kwargs, path):
    name, idx, attr = _step(path)
    v = kwargs[name]
    return v[idx] if idx is not None else getattr(v, attr) if attr else v


def put(kwargs, path, value):
    """A copy of kwargs with the tensor at `path` replaced; tuples and namedtuples are rebuilt, never edited."""
    name, idx, attr = _step(path)
    out = dict(kwargs)
    if idx is not None:
        seq = list(kwargs[name])
        seq[idx] = value
        out[name] = tuple(seq)
    elif attr:
        out[name] = kwargs[name]._replace(**{attr: value})
    else:
        out[name] = value
    return out


def names(arg):
    """What a refusal may call the argument: its parameter, or the name the docstrings give a tuple's entry."""
    return (root(arg.path),) + arg.alias


def functions_that_hand_over(module):
    """{name: function} of the module-level functions of `module`, and the methods its own classes define, whose source
    hands a tensor to the library."""
    found = {}
    short = module.__name__.rsplit(".", 1)[-1]
    for name, obj in vars(module).items():
        if getattr(obj, "__module__", None) != module.__name__:
            continue
        members = [(name, obj)] if inspect.isfunction(obj) else \
            [(name + "." + m, f) for m, f in vars(obj).items() if inspect.isfunction(f)] if inspect.isclass(obj) else []
        for label, fn in members:
            if any(mark in inspect.getsource(fn) for mark in HANDS_OVER):
                found[short + "." + label] = fn
    return found


# ---- the malformed calls ----------------------------------------------------------------------------------------------------

MUTATIONS = ("dtype", "cpu", "strided", "longer", "shorter", "rank", "none", "other_device")
_OTHER_DTYPE = {"int32": "int64", "int64": "int32", "float64": "float32", "uint8": "int32"}


def applies(arg, mutation):
    if "c" in arg.flags:
        return False
    if mutation in ("longer", "shorter"):
        return arg.tie is not None
    if mutation == "rank":
        return "f" not in arg.flags
    if mutation == "none":
        return "o" not in arg.flags
    return True


def malformed_rows():
    """(function, path, mutation) of every malformed call the table implies, public functions only."""
    return [(name, arg.path, m) for name in PUBLIC for arg in TABLE[name]["args"] for m in MUTATIONS if applies(arg, m)]


def mutate(t, arg, mutation):
    """The tensor `t` of a well-formed call, made ill-formed in one respect.  None: the mutation cannot be made here."""
    import torch
    if mutation == "dtype":
        return t.to(getattr(torch, _OTHER_DTYPE[arg.dtype]))
    if mutation == "cpu":
        return t.cpu()
    if mutation == "strided":
        if t.dim() == 2:
            return t.t().contiguous().t()                       # the same values and shape over a transposed layout
        big = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
        big[::2] = t
        return big[::2]
    if mutation == "longer":
        return torch.cat([t, t[-1:]], 0).contiguous()
    if mutation == "shorter":
        return t[:-1].contiguous()
    if mutation == "rank":
        return t.reshape(-1) if t.dim() == 2 else t.reshape(-1, 1)
    if mutation == "none":
        return None
    if mutation == "other_device":
        return t.to("cuda:1") if torch.cuda.device_count() >= 2 else None
    raise KeyError(mutation)


# ---- NoLaunch ---------------------------------------------------------------------------------------------------------------

def pass_through(signatures):
    """The entry points that take no pointer: they read constants and launch nothing."""
    return sorted(name for name, (_, args) in signatures.items() if ctypes.c_void_p not in args)


class NoLaunch:
    """Stands in for the loaded library: an entry point that takes no pointer passes through, any other call is recorded
    and raises.  While it is installed no kernel can receive an argument, well-formed or not."""

    def __init__(self, lib, signatures):
        self._lib, self._signatures, self._passes = lib, signatures, set(pass_through(signatures))
        self.calls = []

    def __getattr__(self, name):
        if name not in self._signatures:
            raise AttributeError(name)
        if name in self._passes:
            return getattr(self._lib, name)

        def refuse(*args):
            self.calls.append(name)
            raise AssertionError("library called: " + name)
        return refuse


# ---- the well-formed calls --------------------------------------------------------------------------------------------------

K, N_FACTORS, N_CLTR = 40, 8, (3, 4)


def make_world(device="cuda:0"):
    """One tiny fitted world: topn_reference.make_case("int") and every class fitted on it once.  Needs a GPU."""
    import numpy as np
    import torch
    import topn_reference as T
    from n2v_hip import coclustering, eccknn, nmf, slopeone, svd
    case = T.make_case("int")
    ts = eccknn.Trainset.from_ratings(case["raw_u"], case["raw_i"], case["r"], rating_scale=case["scale"])
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dt)
    W = dict(case=case, ts=ts, device=device)
    W["u"], W["i"], W["r"] = d(ts.u, torch.int32), d(ts.i, torch.int32), d(ts.r, torch.float64)
    W["seen"] = eccknn.csr_by_x(W["u"], W["i"], W["r"], ts.n_users, ts.n_items)
    W["xr_items"] = eccknn.csr_by_x(W["i"], W["u"], W["r"], ts.n_items, ts.n_users)
    W["w"] = d(case["w_items"], torch.float64)
    opts = {"name": "cosine", "user_based": True}
    W["knn"] = eccknn.KNNBasic(k=K, sim_options=opts, device=device).fit(ts)
    W["means"] = eccknn.KNNWithMeans(k=K, sim_options=opts, device=device).fit(ts)
    W["zscore"] = eccknn.KNNWithZScore(k=K, sim_options=opts, device=device).fit(ts)
    W["baseline"] = eccknn.KNNBaseline(k=K, sim_options=opts, device=device).fit(ts)
    W["svd"] = svd.SVD(n_factors=N_FACTORS, n_epochs=2, n_strata=2, device=device).fit(ts)
    W["nmf"] = nmf.NMF(n_factors=N_FACTORS, n_epochs=2, device=device).fit(ts)
    W["slopeone"] = slopeone.SlopeOne(device=device).fit(ts)
    W["cocl"] = coclustering.CoClustering(N_CLTR[0], N_CLTR[1], n_epochs=2, device=device).fit(ts)
    rs = np.random.RandomState(5)
    qu = np.concatenate([rs.randint(0, ts.n_users, 29), [-1, 3]])
    qi = np.concatenate([rs.randint(0, ts.n_items, 29), [7, -1]])
    W["qu"], W["qi"] = d(qu, torch.int32), d(qi, torch.int32)
    W["r_true"] = d(rs.randint(1, 6, len(qu)), torch.float64)
    W["testset"] = [(case["users"][a] if a >= 0 else "nobody", case["items"][b] if b >= 0 else "nothing", float(c))
                    for a, b, c in zip(qu, qi, W["r_true"].cpu().numpy())]
    W["est"], _, W["imp"] = eccknn.estimate_batch(W["knn"].sim, W["knn"].yr, W["qu"], W["qi"], K, 1)
    W["pred2"] = torch.stack([W["est"], W["est"] * 0.5 + 1.0]).contiguous()
    W["dense"] = eccknn.densify(W["u"], W["i"], W["r"], ts.n_users, ts.n_items)
    W["eccen"] = eccknn.EccenKNN(k=K, sim_options=opts, device=device).fit(ts, case["w_items"])
    return W


def baseline(W, name):
    """(callable, keyword arguments) of one well-formed call of the public function `name`.  The arguments a call writes
    in place are fresh copies; everything else is shared and must be left as it is."""
    import torch
    from n2v_hip import coclustering, eccknn, nmf, slopeone, svd
    ts, case = W["ts"], W["case"]
    knn, s, m, so, cc = W["knn"], W["svd"], W["nmf"], W["slopeone"], W["cocl"]
    mean, scale = ts.global_mean, ts.rating_scale
    model = dict(sim=knn.sim, yr=knn.yr)
    q = dict(qx=W["qu"], qy=W["qi"])
    quqi = dict(qu=W["qu"], qi=W["qi"])
    tables = dict(bu=s.bu, bi=s.bi, pu=s.pu, qi=s.qi)
    so_model = dict(dev=so.dev, freq=so.freq, ur=so.ur, user_mean=so.user_mean)
    cc_model = dict(cltr_u=cc.cltr_u, cltr_i=cc.cltr_i, avgs=cc._avgs(), user_mean=cc.user_mean, item_mean=cc.item_mean)
    topn = dict(seen=W["seen"], global_mean=mean, rating_scale=scale, n=10, owners=None)
    mod, fn = name.split(".", 1)
    if name == "eccknn.densify":
        return eccknn.densify, dict(x=W["u"], y=W["i"], r=W["r"], n_x=ts.n_users, n_y=ts.n_items)
    if name in ("eccknn.similarity", "eccknn.similarity_pearson", "slopeone.deviations"):
        dense, mask = W["dense"]
        if name == "eccknn.similarity":
            return eccknn.similarity, dict(dense=dense, mask=mask, w=W["w"], name="cosine", accumulators=True)
        if name == "slopeone.deviations":                       # any y-major pair will do: here the users play the items
            return slopeone.deviations, dict(dense=dense, mask=mask, accumulators=True)
        b = W["baseline"]
        return eccknn.similarity_pearson, dict(dense=dense, mask=mask, name="pearson_baseline", w=W["w"], global_mean=mean,
                                               bx=b.bx, by=b.by, accumulators=True)
    if name == "eccknn.csr_check":
        return eccknn.csr_check, dict(xr=W["seen"][:2], n_y=ts.n_items)
    if name == "eccknn.similarity_sparse":
        return eccknn.similarity_sparse, dict(xr=W["seen"], w=W["w"], n_y=ts.n_items, name="msd")
    if name == "eccknn.similarity_pearson_sparse":
        b = W["baseline"]
        return eccknn.similarity_pearson_sparse, dict(xr=W["seen"], n_y=ts.n_items, name="pearson_baseline", w=W["w"],
                                                      global_mean=mean, bx=b.bx, by=b.by)
    if name == "eccknn.row_moments":
        return eccknn.row_moments, dict(ptr=so.ur[0], r=so.ur[2], zero_sigma=1.0)
    if name == "eccknn.yr_check":
        return eccknn.yr_check, dict(yr=knn.yr, n_x=ts.n_users)
    if name == "eccknn.estimate_batch":
        return eccknn.estimate_batch, dict(model, k=K, min_k=1, **q)
    if name == "eccknn.estimate_batch_centered":
        return eccknn.estimate_batch_centered, dict(model, k=K, min_k=2, centering=W["zscore"].centering, **q)
    if name == "eccknn.predict":
        return eccknn.predict, dict(est=W["est"], impossible=W["imp"], global_mean=mean, rating_scale=scale, r_true=W["r_true"])
    if name == "eccknn.estimate_sweep":
        return eccknn.estimate_sweep, dict(model, ks=(5, K), min_ks=(1, 3), centering=W["baseline"].centering, **q)
    if name == "eccknn.errors":
        return eccknn.errors, dict(pred=W["pred2"], r_true=W["r_true"])
    if name == "eccknn.top_n":
        return eccknn.top_n, dict(model, user_based=True, k=K, min_k=1, **topn)
    if name == "eccknn.top_n_centered":
        return eccknn.top_n_centered, dict(model, seen=W["seen"], k=K, min_k=1, rating_scale=scale, n=10,
                                           centering=W["means"].centering, owners=None)
    if name == "svd.Blocks.__init__":
        b = s.blocks
        return svd.Blocks, dict(lists=(b.ptr, b.u, b.i, b.r), n_users=ts.n_users, n_items=ts.n_items, n_strata=b.n_strata)
    if name == "svd.epoch":
        return svd.epoch, dict(blocks=s.blocks, mu=s.mu, biased=True, rates=s.rates, bu=s.bu.clone(), bi=s.bi.clone(),
                               pu=s.pu.clone(), qi=s.qi.clone())
    if name == "svd.estimate_batch":
        return svd.estimate_batch, dict(tables, mu=s.mu, biased=True, qu=W["qu"], qi_ids=W["qi"])
    if name == "svd.top_n":
        return svd.top_n, dict(tables, mu=s.mu, biased=True, **topn)
    if name == "nmf.lists":
        ur, ir = m.lists.ur, m.lists.ir
        return nmf.lists, dict(ur=ur, n_users=ts.n_users, n_items=ts.n_items, ir=ir, order=m.lists.order)
    if name == "nmf.epoch":
        return nmf.epoch, dict(lists_=m.lists, reg_pu=0.06, reg_qi=0.06, pu=m.pu, qi=m.qi, pu_out=torch.zeros_like(m.pu),
                               qi_out=torch.zeros_like(m.qi))
    if name == "slopeone.deviations_sparse":
        return slopeone.deviations_sparse, dict(xr=W["xr_items"], n_users=ts.n_users, accumulators=True)
    if name == "slopeone.estimate_batch":
        return slopeone.estimate_batch, dict(so_model, **quqi)
    if name == "slopeone.top_n":
        return slopeone.top_n, dict(so_model, **topn)
    if name == "coclustering.averages":
        return coclustering.averages, dict(ur=cc.ur, n_items=ts.n_items, cltr_u=cc.cltr_u, cltr_i=cc.cltr_i,
                                           n_cltr_u=N_CLTR[0], n_cltr_i=N_CLTR[1], global_mean=mean)
    if name == "coclustering.assign":
        from n2v_hip.nmf import row_order
        return coclustering.assign, dict(lst=cc.ur, user_side=True, cltr_u=cc.cltr_u.clone(), cltr_i=cc.cltr_i.clone(),
                                         avgs=cc._avgs(), user_mean=cc.user_mean, item_mean=cc.item_mean, order=row_order(cc.ur[0]))
    if name == "coclustering.estimate_batch":
        return coclustering.estimate_batch, dict(cc_model, global_mean=mean, **quqi)
    if name == "coclustering.top_n":
        return coclustering.top_n, dict(cc_model, **topn)
    raise KeyError(name)


def flatten(out):
    """A call's result as a list of byte strings: tensors, arrays, floats and the fields of the checked list objects."""
    import numpy as np
    import torch
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out.detach().cpu().contiguous().numpy().tobytes()]
    if isinstance(out, np.ndarray):
        return [out.tobytes()]
    if isinstance(out, (float, int)):
        return [np.float64(out).tobytes()]
    if isinstance(out, dict):
        return [b for key in sorted(out) for b in flatten(out[key])]
    if isinstance(out, (tuple, list)):
        return [b for v in out for b in flatten(v)]
    fields = [getattr(out, f) for f in ("ptr", "u", "i", "r", "ur", "ir", "order") if hasattr(out, f)]
    assert fields, type(out)
    return flatten(fields)
