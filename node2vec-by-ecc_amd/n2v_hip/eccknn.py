"""EccenKNN: eccentricity-weighted k-NN rating prediction on the device (csrc/n2v_eccknn.hip, C-ABI include/n2v_sim.h).

Reference: src/main_rec.py:63-329, a user-based or item-based k-NN collaborative filter whose similarity (cosine or
mean squared difference over co-rated entries) weights every co-rating by a per-item statistic.  Parity is unpinned:
the reference needs `surprise`, which is not a dependency here, and its main() raises unconditionally; the semantics are
restated from the text (tests/eccknn_reference.py) and the kernels are held to that restatement bit for bit.

x is the side similarities are formed over, y the other one: users and items when `user_based`, swapped otherwise.
The weights are an input (an array over y, or a dict raw id -> weight); the pandas statistics that produce them in the
reference (src/utils.py:95-153) are not part of this module.

Reference quirk, not reproduced: in item-based mode the reference indexes its per-item dictionary with inner *user*
ids (src/main_rec.py:174 and :99).  Here the weight array is indexed by y, whichever side y is.

`Trainset` and `predict` restate the documented behaviour of surprise's Trainset / AlgoBase.predict: inner ids by first
appearance, an unknown user or item or an impossible estimate falls back to the training mean, and every estimate is
clipped to the rating scale.  The training mean is sum(r) / n in training order.

The similarity has two forms with the same bytes: the dense one (a y-major fp64 matrix plus a mask, n_x * n_y at most
n2v_eccknn_max_dense() elements) and the sparse one (the x-major CSR of the ratings, no such bound).
sim_options["form"] = "auto" (the default: dense inside the limit, sparse past it), "dense" or "sparse".

KNNBasic is the plain k-NN the reference compares EccenKNN against (src/main_rec.py:19-29, 341-348: `-algo knn`,
surprise's KNNBasic) under the four similarities of its `-sim` flag.  cosine and msd are the kernels above with all-ones
weights; pearson and pearson_baseline are surprise's own functions, restated (tests/eccknn_pearson_reference.py) together
with the ALS baselines the second one needs (src/main_rec.py:181-189).  Parity with surprise itself is unpinned for the
same reason as above: the restatement is the definition and the kernels equal it bit for bit.  Optional weights multiply
each co-rating's product, which is what the reference meant by passing its per-item dictionary to every similarity (:197).

KNNWithMeans, KNNWithZScore and KNNBaseline are surprise's other three k-NN predictors on top of KNNBasic: the same
neighbours, each neighbour's rating centred on its row mean, on its row mean in units of its row sigma, or on the ALS
baseline of the pair, and too few neighbours leave the base estimate instead of an impossible prediction
(`row_moments`, `estimate_batch_centered`, `top_n_centered`; three more instantiations of the one estimate function).
fit(trainset, weights) weights the co-ratings as for KNNBasic, which gives the eccentricity-weighted centred k-NN.  The
rules are restated from memory of scikit-surprise 1.0.6 (tests/knn_centered_reference.py); parity with surprise itself is
unpinned, the restatement is the definition and the kernels equal it bit for bit.  Deviation: the row means and sigmas
are sequential sums in training order, where numpy's mean / std add pairwise above 8 elements.

Top-N lists (`top_n`, and `TopN.top_n_lists` / `recommend` / `ranking_metrics` on every fitted class, n2v_hip.svd.SVD
included): what the reference's unfinished src/recsys.py sketches and surprise documents as
algo.test(trainset.build_anti_testset()) plus a per-user stable sort.  One fused kernel forms a user's predictions for all
unrated items, by the same device functions as estimate_batch + predict and so by the same bits, and keeps the best n;
the n_users x n_items predictions are never stored.  Equal predictions rank by inner item id.  The definition is
tests/topn_reference.py; parity with surprise is unpinned as above.

The k-NN sweep (`estimate_sweep`, `test_sweep` / `accuracy_sweep` on every k-NN class, main_rec.py -sweep-k) is the step
the reference's experiment is made of: every (k, min_k) of a grid over one fit.  The selection list is in a total order, so
the neighbours for k are the head of the neighbours for any larger k and the rank-order sums for k a prefix of the sums for
the largest; one selection and one walk down it give every cell with the bits of the single-cell call
(tests/knn_sweep_reference.py is the definition: the single-cell restatement, cell by cell).  `errors` / `Predictor.mae`
add the second measure of surprise's cross_validate, the mean absolute error, to every predictor.

There is no CPU fallback.
"""
import collections
import collections.abc

import numpy as np
import torch

from . import _lib

MAX_K = 256                      # N2V_ECCKNN_MAX_K
MAX_SWEEP = 16                   # N2V_ECCKNN_MAX_SWEEP: values a side of a (k, min_k) grid
MAX_TOP_N = 256                  # N2V_TOPN_MAX_N
MAX_SEGMENTS = 64                # segments of the candidate range per owner in the top-N kernels
SIM_NAMES = ("cosine", "msd", "pearson", "pearson_baseline")   # the reference's construction_func keys
_METHOD = {"cosine": 0, "msd": 1}
_PEARSON_KIND = {"pearson": 0, "pearson_baseline": 1}          # N2V_ECCKNN_PEARSON, N2V_ECCKNN_PEARSON_BASELINE
_PEARSON_ACC = {"pearson": ("sqi", "sqj", "si", "sj"), "pearson_baseline": ("sq_diff_i", "sq_diff_j")}   # a1 .. a4
BSL_DEFAULTS = {"method": "als", "n_epochs": 10, "reg_u": 15, "reg_i": 10}   # surprise's baseline_als
FORMS = ("auto", "dense", "sparse")
CENTERINGS = {"means": 1, "zscore": 2, "baseline": 3}          # N2V_ECCKNN_CENTER_MEANS, _ZSCORE, _BASELINE
MAX_DENSE = 1 << 31              # n2v_eccknn_max_dense()
CSR_BAD = ((1, "xr_ptr is not monotone or leaves [0, n]"), (2, "a y outside [0, n_y)"),
           (4, "a row is not strictly ascending in y (a duplicate (x, y) pair?)"))


class PredictionImpossible(Exception):
    pass


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("n2v_hip.eccknn: no GPU visible (torch.cuda.is_available() is False); no CPU fallback")


_PLAIN = object()                # in place of a Centering: the call that centres nothing


def _first_appearance(raw):
    """(inner id of every entry, {raw id: inner id}) in order of first appearance, for raw ids of any hashable kind, as
    surprise takes them.  eccstats.first_appearance numbers the columns of a ratings file the same way through np.unique,
    which is the faster of the two and holds for ids of one sortable type only; so there are two."""
    table, inner = {}, np.empty(len(raw), dtype=np.int64)
    for n, v in enumerate(raw):
        i = table.get(v)
        if i is None:
            i = table[v] = len(table)
        inner[n] = i
    return inner, table


def _to_device(a, dtype, dev):
    """A host array (or list) as a contiguous tensor of `dtype` on `dev`."""
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _csr_to_device(triple, dev):
    """A host CSR triple (ptr, ids, r) as (int64, int32, fp64) tensors on `dev`."""
    return tuple(_to_device(a, dt, dev) for a, dt in zip(triple, (torch.int64, torch.int32, torch.float64)))


def _knn_options(k, min_k):
    """(k, min_k) as every k-NN call takes them; host only."""
    k, min_k = int(k), int(min_k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k %d outside [1, %d]" % (k, MAX_K))
    if min_k < 1:
        raise ValueError("min_k %d < 1" % min_k)
    return k, min_k


def _query_count(qx, qy, sides=("x", "y"), names=("qx", "qy")):
    """The number of queries of an estimate call: at least one, and as many on one side as on the other."""
    n_q = qx.numel()
    if n_q == 0 or qy.numel() != n_q:
        raise ValueError("estimate: %d %s (%s) and %d %s (%s) queries: nothing to estimate"
                         % (n_q, sides[0], names[0], qy.numel(), sides[1], names[1]))
    return n_q


def _queries_ptrs(fn, qx, qy, dev, names=("qx", "qy")):
    """(qx pointer, qy pointer) of the int32 query pair of an estimate call, each a 1-D tensor on `dev`."""
    return (_lib.tensor(fn, names[0], qx, torch.int32, dev, (None,)), _lib.tensor(fn, names[1], qy, torch.int32, dev, (None,)))


def _csr_ptrs(fn, name, triple, dev=None, roles=("ptr", "ids", "r"), n_rows=None):
    """([ptr, ids(, r)] pointers, n, dev) of a caller's CSR (int64 ptr[n_rows + 1], int32 ids[n], fp64 r[n]) on `dev`, or,
    when dev is None, on the GPU of its last entry, which then is the device of the call.  With two roles the list has no
    ratings, and a third entry of the tuple is not read.  n_rows None leaves ptr's length to the caller, which has its
    own message for it.  The pointers of an empty list are NULL."""
    kinds = list(zip(roles, (torch.int64, torch.int32, torch.float64)))
    if not isinstance(triple, (tuple, list)) or len(triple) < len(kinds):
        raise ValueError("%s: %s must be (%s)" % (fn, name, ", ".join("%s %s" % (str(dt).replace("torch.", ""), role)
                                                                        for role, dt in kinds)))
    label = ["%s[%d] (%s %s)" % (name, j, str(dt).replace("torch.", ""), role) for j, (role, dt) in enumerate(kinds)]
    if dev is None:
        dev = _lib.call_device(fn, label[-1], triple[len(kinds) - 1])
    out = [_lib.tensor(fn, label[0], triple[0], torch.int64, dev, (None,) if n_rows is None else int(n_rows) + 1),
           _lib.tensor(fn, label[1], triple[1], torch.int32, dev, (None,))]
    n = triple[1].numel()
    if len(kinds) == 3:
        out.append(_lib.tensor(fn, label[2], triple[2], torch.float64, dev, n))
    if triple[0].numel() < 2:
        raise ValueError("%s: %s: %d ptr entries: at least one row" % (fn, label[0], triple[0].numel()))
    return [out[0]] + [q if n else None for q in out[1:]], n, dev


def _csr(major, minor, r, n_major):
    """Lists of (minor, r) per major id, each in training order (a stable sort by major id)."""
    order = np.argsort(major, kind="stable")
    ptr = np.zeros(n_major + 1, dtype=np.int64)
    np.cumsum(np.bincount(major, minlength=n_major), out=ptr[1:])
    return ptr, minor[order].astype(np.int32), r[order].astype(np.float64)


class Trainset:
    """Ratings with inner ids, the way surprise's Trainset holds them.  ur / ir are CSR triples (ptr, other id, rating):
    the ratings of inner user u are ur[1][ur[0][u]:ur[0][u + 1]] (inner item ids) with ur[2] alongside."""

    @classmethod
    def from_ratings(cls, users, items, ratings, rating_scale=None):
        users, items = list(users), list(items)
        r = np.asarray(ratings, dtype=np.float64)
        if not (len(users) == len(items) == len(r)) or len(r) == 0:
            raise ValueError("from_ratings: %d users, %d items, %d ratings" % (len(users), len(items), len(r)))
        t = cls()
        t.u, t._raw2inner_u = _first_appearance(users)
        t.i, t._raw2inner_i = _first_appearance(items)
        t.r = r
        t.n_users, t.n_items, t.n_ratings = len(t._raw2inner_u), len(t._raw2inner_i), len(r)
        key = t.u * t.n_items + t.i
        if len(np.unique(key)) != len(key):
            raise ValueError("from_ratings: duplicate (user, item) pair")
        t.ur = _csr(t.u, t.i, r, t.n_users)
        t.ir = _csr(t.i, t.u, r, t.n_items)
        t.global_mean = float(np.cumsum(r)[-1] / len(r))       # cumsum adds one after the other, in training order
        t.rating_scale = (float(r.min()), float(r.max())) if rating_scale is None else tuple(map(float, rating_scale))
        return t

    def knows_user(self, uid):
        return isinstance(uid, (int, np.integer)) and 0 <= uid < self.n_users

    def knows_item(self, iid):
        return isinstance(iid, (int, np.integer)) and 0 <= iid < self.n_items

    def to_inner_uid(self, ruid):
        try:
            return self._raw2inner_u[ruid]
        except KeyError:
            raise ValueError("User %s is not part of the trainset." % str(ruid))

    def to_inner_iid(self, riid):
        try:
            return self._raw2inner_i[riid]
        except KeyError:
            raise ValueError("Item %s is not part of the trainset." % str(riid))

    def inner_uids(self, raw):
        """Inner ids of raw ids, -1 for unknown ones."""
        return np.array([self._raw2inner_u.get(v, -1) for v in raw], dtype=np.int32)

    def inner_iids(self, raw):
        return np.array([self._raw2inner_i.get(v, -1) for v in raw], dtype=np.int32)


# ---- C-ABI wrappers (device tensors in, device tensors out) -----------------------------------------------------------
# The types the docstrings state are enforced, not converted: every tensor a caller supplies goes through _lib.tensor
# before the first library call that takes a pointer (contiguous, the stated dtype, rank and length, on the GPU of the
# call's first tensor argument); anything else is a ValueError naming the function and the argument.  Host work only.

def densify(x, y, r, n_x, n_y):
    """(dense fp64 [n_y][n_x], mask uint8 [n_y][n_x]) of int32 / fp64 device triples."""
    _require_gpu()
    lib = _lib.load()
    if n_x * n_y > int(lib.n2v_eccknn_max_dense()):
        raise ValueError("eccknn: n_x * n_y = %d x %d exceeds the dense limit of %d elements"
                         % (n_x, n_y, lib.n2v_eccknn_max_dense()))
    dev = _lib.call_device("eccknn.densify", "r", r)
    p_r = _lib.tensor("eccknn.densify", "r", r, torch.float64, dev, (None,))
    p_x = _lib.tensor("eccknn.densify", "x", x, torch.int32, dev, r.numel())
    p_y = _lib.tensor("eccknn.densify", "y", y, torch.int32, dev, r.numel())
    with torch.cuda.device(dev):
        dense = torch.empty((n_y, n_x), dtype=torch.float64, device=dev)
        mask = torch.empty((n_y, n_x), dtype=torch.uint8, device=dev)
        _lib.check(lib.n2v_eccknn_densify(p_x, p_y, p_r, r.numel(), n_x, n_y, _lib.ptr(dense),
                                          _lib.ptr(mask), _lib.stream_ptr(dev)))
    return dense, mask


def _dense_ptrs(fn, dense, mask):
    """(dense pointer, mask pointer, n_x, n_y, device) of densify's pair: fp64 and uint8 [n_y][n_x] on one GPU."""
    dev = _lib.call_device(fn, "dense", dense)
    p_dense = _lib.tensor(fn, "dense", dense, torch.float64, dev, (None, None))
    n_y, n_x = dense.shape
    return p_dense, _lib.tensor(fn, "mask", mask, torch.uint8, dev, (n_y, n_x)), n_x, n_y, dev


def similarity(dense, mask, w, name, min_support=1, accumulators=False):
    """sim fp64 [n_x][n_x] from densify's pair (dense fp64, mask uint8, both [n_y][n_x]) and the weights w fp64[n_y]; with
    accumulators also a dict of the reference's arrays (freq, and prods / sqi / sqj or sq_diff)."""
    _require_gpu()
    p_dense, p_mask, n_x, n_y, dev = _dense_ptrs("eccknn.similarity", dense, mask)
    p_w = _lib.tensor("eccknn.similarity", "w", w, torch.float64, dev, n_y)
    lib = _lib.load()
    with torch.cuda.device(dev):
        sim = torch.empty((n_x, n_x), dtype=torch.float64, device=dev)
        acc = {}
        if accumulators:
            acc["freq"] = torch.empty((n_x, n_x), dtype=torch.int32, device=dev)
            for nm in (("prods", "sqi", "sqj") if name == "cosine" else ("sq_diff",)):
                acc[nm] = torch.empty((n_x, n_x), dtype=torch.float64, device=dev)
        _lib.check(lib.n2v_eccknn_sim(p_dense, p_mask, n_x, n_y, p_w, _METHOD[name], int(min_support),
                                      _lib.ptr(sim), _lib.ptr(acc.get("freq")), _lib.ptr(acc.get("prods")),
                                      _lib.ptr(acc.get("sqi")), _lib.ptr(acc.get("sqj")), _lib.ptr(acc.get("sq_diff")),
                                      _lib.stream_ptr(dev)))
    return (sim, acc) if accumulators else sim


def choose_form(n_x, n_y, form, limit=MAX_DENSE):
    """"dense" or "sparse" for an n_x x n_y problem.  Host arithmetic only.  "auto" is dense iff n_x * n_y <= limit; an
    explicit "dense" past the limit is the dense path's own error."""
    if form not in FORMS:
        raise ValueError("eccknn: form %r, allowed values are %s" % (form, ", ".join(FORMS)))
    over = int(n_x) * int(n_y) > int(limit)
    if form == "dense" and over:
        raise ValueError("eccknn: n_x * n_y = %d x %d exceeds the dense limit of %d elements" % (n_x, n_y, limit))
    if form == "auto":
        return "sparse" if over else "dense"
    return form


def csr_by_x(x, y, r, n_x, n_y=None):
    """Device triples (x, y int32 / int64, r fp64), no duplicate (x, y) -> the x-major CSR (xr_ptr int64[n_x + 1],
    xr_y int32, xr_r fp64), every row ascending in y: a stable sort on the key x * n_y + y.  n_y None: the largest y + 1."""
    _require_gpu()
    x64, y64 = x.to(torch.int64), y.to(torch.int64)
    if n_y is None:
        n_y = int(y64.max().item()) + 1 if y64.numel() else 1
    _, order = torch.sort(x64 * int(n_y) + y64, stable=True)
    ptr = torch.zeros(int(n_x) + 1, dtype=torch.int64, device=x.device)
    ptr[1:] = torch.cumsum(torch.bincount(x64, minlength=int(n_x)), 0)
    return ptr, y64[order].to(torch.int32).contiguous(), r[order].to(torch.float64).contiguous()


def csr_check(xr, n_y):
    """Raises ValueError when the x-major CSR is malformed (n2v_eccknn_csr_check); one read-back of an int32."""
    _require_gpu()
    (p_ptr, p_ys), _, dev = _csr_ptrs("eccknn.csr_check", "xr", xr, None, ("ptr", "y"))
    ptr_, ys = xr[0], xr[1]
    lib = _lib.load()
    with torch.cuda.device(dev):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.n2v_eccknn_csr_check(p_ptr, p_ys, ptr_.numel() - 1, int(n_y), ys.numel(),
                                            _lib.ptr(status), _lib.stream_ptr(dev)))
        bits = int(status.item())
    if bits:
        raise ValueError("eccknn: malformed CSR: " + "; ".join(msg for b, msg in CSR_BAD if bits & b))


def similarity_sparse(xr, w, n_y, name, min_support=1, accumulators=False):
    """similarity() from the x-major CSR xr = (xr_ptr, xr_y, xr_r) of csr_by_x: the same return value, the same bytes, and
    no n_x * n_y limit.  The CSR is checked first; a malformed one is a ValueError."""
    _require_gpu()
    fn = "eccknn.similarity_sparse"
    p_xr, n, dev = _csr_ptrs(fn, "xr", xr, None, ("ptr", "y", "r"))
    n_x = xr[0].numel() - 1
    p_w = _lib.tensor(fn, "w", w, torch.float64, dev, int(n_y))
    csr_check(xr, n_y)
    lib = _lib.load()
    with torch.cuda.device(dev):
        sim = torch.empty((n_x, n_x), dtype=torch.float64, device=dev)
        acc = {}
        if accumulators:
            acc["freq"] = torch.empty((n_x, n_x), dtype=torch.int32, device=dev)
            for nm in (("prods", "sqi", "sqj") if name == "cosine" else ("sq_diff",)):
                acc[nm] = torch.empty((n_x, n_x), dtype=torch.float64, device=dev)
        _lib.check(lib.n2v_eccknn_sim_sparse(*p_xr, n_x, int(n_y), n, p_w, _METHOD[name], int(min_support), _lib.ptr(sim),
                                             _lib.ptr(acc.get("freq")), _lib.ptr(acc.get("prods")), _lib.ptr(acc.get("sqi")),
                                             _lib.ptr(acc.get("sqj")), _lib.ptr(acc.get("sq_diff")), _lib.stream_ptr(dev)))
    return (sim, acc) if accumulators else sim


def bsl_check(bsl_options):
    """bsl_options with surprise's defaults filled in; host only.  sgd is refused: its updates are sequential."""
    opts = dict(BSL_DEFAULTS, **(bsl_options or {}))
    unknown = sorted(set(opts) - set(BSL_DEFAULTS))
    if unknown:
        raise ValueError("bsl_options: unknown key %s, allowed keys are %s" % (", ".join(unknown), ", ".join(BSL_DEFAULTS)))
    if opts["method"] == "sgd":
        raise ValueError("bsl_options: method sgd is not built (its updates are sequential across rows); use als")
    if opts["method"] != "als":
        raise ValueError("Invalid method " + str(opts["method"]) + " for baseline computation. Available methods are als and sgd.")
    if int(opts["n_epochs"]) < 0 or not float(opts["reg_u"]) >= 0 or not float(opts["reg_i"]) >= 0:
        raise ValueError("bsl_options: n_epochs %r, reg_u %r, reg_i %r: none may be negative"
                         % (opts["n_epochs"], opts["reg_u"], opts["reg_i"]))
    return opts


def baselines(trainset, bsl_options=None, device="cuda:0"):
    """(bu, bi) device fp64 tensors: surprise's baseline_als on the trainset's ur / ir lists (n2v_eccknn_baselines)."""
    opts = bsl_check(bsl_options)
    _require_gpu()
    dev = torch.device(device)
    lib = _lib.load()
    ts = trainset
    with torch.cuda.device(dev):
        ur, ir = _csr_to_device(ts.ur, dev), _csr_to_device(ts.ir, dev)
        bu = torch.empty(ts.n_users, dtype=torch.float64, device=dev)
        bi = torch.empty(ts.n_items, dtype=torch.float64, device=dev)
        _lib.check(lib.n2v_eccknn_baselines(_lib.ptr(ur[0]), _lib.ptr(ur[1]), _lib.ptr(ur[2]), ts.n_users, _lib.ptr(ir[0]),
                                            _lib.ptr(ir[1]), _lib.ptr(ir[2]), ts.n_items, float(ts.global_mean),
                                            int(opts["n_epochs"]), float(opts["reg_u"]), float(opts["reg_i"]), _lib.ptr(bu),
                                            _lib.ptr(bi), _lib.stream_ptr(dev)))
    return bu, bi


def _pearson_outputs(name, n_x, dev, accumulators):
    sim = torch.empty((n_x, n_x), dtype=torch.float64, device=dev)
    acc = {}
    if accumulators:
        acc["freq"] = torch.empty((n_x, n_x), dtype=torch.int32, device=dev)
        for nm in ("prods",) + _PEARSON_ACC[name]:
            acc[nm] = torch.empty((n_x, n_x), dtype=torch.float64, device=dev)
    a = [_lib.ptr(acc.get(nm)) for nm in _PEARSON_ACC[name]] + [None, None]
    return sim, acc, [_lib.ptr(sim), _lib.ptr(acc.get("freq")), _lib.ptr(acc.get("prods"))] + a[:4]


def _pearson_inputs(fn, name, n_x, n_y, w, bx, by, dev):
    """(w, bx, by) pointers: fp64 w[n_y] or None, and fp64 bx[n_x], by[n_y], which pearson_baseline needs and pearson
    does not read."""
    if name not in _PEARSON_KIND:
        raise NameError("Wrong sim name " + str(name) + ". Allowed values are " + ", ".join(_PEARSON_KIND) + ".")
    ptrs = [_lib.tensor(fn, "w (the weights)", w, torch.float64, dev, int(n_y), optional=True)]
    if name == "pearson_baseline" and (bx is None or by is None):
        raise ValueError("similarity_pearson: pearson_baseline needs bx[%d] and by[%d]" % (n_x, n_y))
    return ptrs + [_lib.tensor(fn, "bx", bx, torch.float64, dev, int(n_x), optional=True),
                   _lib.tensor(fn, "by", by, torch.float64, dev, int(n_y), optional=True)]


def similarity_pearson(dense, mask, name, w=None, min_support=1, global_mean=0.0, bx=None, by=None, shrinkage=100,
                       accumulators=False):
    """similarity() for "pearson" and "pearson_baseline" (n2v_eccknn_pearson).  w None: no weights.  The accumulators are
    freq, prods and sqi / sqj / si / sj, or sq_diff_i / sq_diff_j.  pearson_baseline needs global_mean, bx[n_x], by[n_y]."""
    _require_gpu()
    p_dense, p_mask, n_x, n_y, dev = _dense_ptrs("eccknn.similarity_pearson", dense, mask)
    p_w, p_bx, p_by = _pearson_inputs("eccknn.similarity_pearson", name, n_x, n_y, w, bx, by, dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        sim, acc, outs = _pearson_outputs(name, n_x, dev, accumulators)
        _lib.check(lib.n2v_eccknn_pearson(p_dense, p_mask, n_x, n_y, p_w, _PEARSON_KIND[name],
                                          int(min_support), float(global_mean), p_bx, p_by, float(shrinkage),
                                          *outs, _lib.stream_ptr(dev)))
    return (sim, acc) if accumulators else sim


def similarity_pearson_sparse(xr, n_y, name, w=None, min_support=1, global_mean=0.0, bx=None, by=None, shrinkage=100,
                              accumulators=False):
    """similarity_pearson() from the x-major CSR of csr_by_x: the same bytes, no n_x * n_y limit.  The CSR is checked
    first; a malformed one is a ValueError."""
    _require_gpu()
    fn = "eccknn.similarity_pearson_sparse"
    p_xr, n, dev = _csr_ptrs(fn, "xr", xr, None, ("ptr", "y", "r"))
    n_x = xr[0].numel() - 1
    p_w, p_bx, p_by = _pearson_inputs(fn, name, n_x, n_y, w, bx, by, dev)
    csr_check(xr, n_y)
    lib = _lib.load()
    with torch.cuda.device(dev):
        sim, acc, outs = _pearson_outputs(name, n_x, dev, accumulators)
        _lib.check(lib.n2v_eccknn_pearson_sparse(*p_xr, n_x, int(n_y), n, p_w, _PEARSON_KIND[name], int(min_support),
                                                 float(global_mean), p_bx, p_by, float(shrinkage), *outs,
                                                 _lib.stream_ptr(dev)))
    return (sim, acc) if accumulators else sim


def estimate_batch(sim, yr, qx, qy, k, min_k):
    """(est fp64, actual_k int32, impossible uint8) device tensors.  yr: device CSR triple (ptr int64, x int32, r fp64);
    qx / qy: int32 device tensors, -1 = unknown."""
    return _estimate_batch(sim, yr, qx, qy, k, min_k, _PLAIN, False)


# ---- centred k-NN: KNNWithMeans, KNNWithZScore, KNNBaseline -------------------------------------------------------------

def row_moments(ptr, r, zero_sigma=None):
    """(mu, sd) device fp64 tensors over the rows of the CSR (ptr int64[n_rows + 1], r fp64): each row's mean and
    population sigma, both sums sequential in list order (n2v_eccknn_row_moments).  An empty row is NaN.  zero_sigma: what
    replaces a sigma equal to 0.0; None leaves it.  surprise's overall sigma is row_moments(tensor([0, n]), r)[1]."""
    _require_gpu()
    dev = _lib.call_device("eccknn.row_moments", "r", r)
    p_r = _lib.tensor("eccknn.row_moments", "r", r, torch.float64, dev, (None,))
    p_ptr = _lib.tensor("eccknn.row_moments", "ptr", ptr, torch.int64, dev, (None,))
    if ptr.numel() < 2:
        raise ValueError("row_moments: ptr must be int64[n_rows + 1] with n_rows >= 1, r fp64[n]")
    lib = _lib.load()
    n_rows, n = ptr.numel() - 1, r.numel()
    with torch.cuda.device(dev):
        mu = torch.empty(n_rows, dtype=torch.float64, device=dev)
        sd = torch.empty(n_rows, dtype=torch.float64, device=dev)
        _lib.check(lib.n2v_eccknn_row_moments(p_ptr, p_r if n else None, n_rows, n,
                                              float("nan") if zero_sigma is None else float(zero_sigma), _lib.ptr(mu),
                                              _lib.ptr(sd), _lib.stream_ptr(dev)))
    return mu, sd


class Centering(collections.namedtuple("Centering", "mode user_based global_mean tx sd by")):
    """What the centred estimates read beside sim and yr.  mode: "means", "zscore" or "baseline"; tx: mu[n_x] (means,
    zscore) or bx[n_x] (baseline); sd: sigma[n_x] (zscore, else None); by[n_y] (baseline, else None); (bx, by) = (bu, bi)
    when user_based, (bi, bu) otherwise.  Device fp64 tensors."""
    __slots__ = ()


def _centering_args(c, n_x, n_y, fn="centering", dev=None):
    """(code, tx, sd, by pointers) after the host checks; a table the mode reads must be there, fp64, on `dev` and of the
    right length.  A table the mode does not read is not passed on."""
    if not isinstance(c, Centering) or c.mode not in CENTERINGS:
        raise ValueError("centering: a Centering whose mode is one of %s" % ", ".join(CENTERINGS))
    need = {"means": (("tx", n_x),), "zscore": (("tx", n_x), ("sd", n_x)), "baseline": (("tx", n_x), ("by", n_y))}[c.mode]
    used = {name: _lib.tensor(fn, "centering.%s (mode %s)" % (name, c.mode), getattr(c, name), torch.float64, dev, int(length))
            for name, length in need}
    return CENTERINGS[c.mode], used["tx"], used.get("sd"), used.get("by")


def yr_check(yr, n_x):
    """Raises ValueError when the rating lists yr = (ptr int64[n_y + 1], x int32, r fp64) are malformed: the centred
    estimates index their tables with yr's x ids.  The lists are in training order, not ascending, so csr_check does not
    apply; a minimum and a maximum on the device are enough."""
    _require_gpu()
    _, n, _ = _csr_ptrs("eccknn.yr_check", "yr", yr, None, ("ptr", "x", "r"))
    ptr_, xs, rs = yr
    if int(ptr_[0].item()) != 0 or int(ptr_[-1].item()) != n or bool((ptr_[1:] < ptr_[:-1]).any().item()):
        raise ValueError("yr: malformed lists: ptr is not monotone from 0 to %d" % n)
    if n and (int(xs.min().item()) < 0 or int(xs.max().item()) >= int(n_x)):
        raise ValueError("yr: malformed lists: an x outside [0, %d)" % n_x)


def _knn_model(fn, sim, yr):
    """([sim, n_x, yr_ptr, yr_x, yr_r, n_y] as the k-NN entry points take them, n_x, n_y, device): sim fp64 [n_x][n_x] on a
    GPU, which is the device of the call, and the rating lists yr on it."""
    dev = _lib.call_device(fn, "sim", sim)
    n_x = sim.shape[0] if sim.dim() else 0
    p_sim = _lib.tensor(fn, "sim", sim, torch.float64, dev, (n_x, n_x))
    p_yr, _, _ = _csr_ptrs(fn, "yr", yr, dev, ("ptr", "x", "r"))
    n_y = yr[0].numel() - 1
    return [p_sim, n_x] + p_yr + [n_y], n_x, n_y, dev


def _estimate_batch(sim, yr, qx, qy, k, min_k, centering, check):
    """The one body of estimate_batch (centering _PLAIN: n2v_eccknn_estimate) and estimate_batch_centered."""
    _require_gpu()
    k, min_k = _knn_options(k, min_k)
    fn = "eccknn.estimate_batch" if centering is _PLAIN else "eccknn.estimate_batch_centered"
    model, n_x, n_y, dev = _knn_model(fn, sim, yr)
    p_qx, p_qy = _queries_ptrs(fn, qx, qy, dev)
    n_q = _query_count(qx, qy)
    model += [p_qx, p_qy, n_q, k, min_k]
    if centering is not _PLAIN:
        code, tx, sd, by = _centering_args(centering, n_x, n_y, fn, dev)
        if check:
            yr_check(yr, n_x)
        model += [code, 1 if centering.user_based else 0, float(centering.global_mean), tx, sd, by]
    lib = _lib.load()
    with torch.cuda.device(dev):
        est = torch.empty(n_q, dtype=torch.float64, device=dev)
        actual_k = torch.empty(n_q, dtype=torch.int32, device=dev)
        imp = torch.empty(n_q, dtype=torch.uint8, device=dev)
        entry = lib.n2v_eccknn_estimate if centering is _PLAIN else lib.n2v_eccknn_estimate_centered
        _lib.check(entry(*model, _lib.ptr(est), _lib.ptr(actual_k), _lib.ptr(imp), _lib.stream_ptr(dev)))
    return est, actual_k, imp


def estimate_batch_centered(sim, yr, qx, qy, k, min_k, centering, check=True):
    """estimate_batch under a Centering (n2v_eccknn_estimate_centered): the same neighbours, centred sums.  Too few
    neighbours is not impossible here (the estimate is the base alone); under "baseline" nothing is.  yr is checked first
    (yr_check): a malformed list is a ValueError, not a launch.  check False: the caller has run yr_check on these lists."""
    return _estimate_batch(sim, yr, qx, qy, k, min_k, centering, check)


def predict(est, impossible, global_mean, rating_scale, r_true=None):
    """pred (device fp64), and the rmse (a Python float) when r_true is given.  est: device fp64 [n]; impossible: device
    uint8 [n], the type the estimate calls return (a bool tensor is refused although it has the same bytes: pass
    impossible.view(torch.uint8)); r_true: device fp64 [n] or None."""
    _require_gpu()
    dev = _lib.call_device("eccknn.predict", "est", est)
    p_est = _lib.tensor("eccknn.predict", "est", est, torch.float64, dev, (None,))
    p_imp = _lib.tensor("eccknn.predict", "impossible", impossible, torch.uint8, dev, est.numel())
    p_true = _lib.tensor("eccknn.predict", "r_true", r_true, torch.float64, dev, est.numel(), optional=True)
    lib = _lib.load()
    with torch.cuda.device(dev):
        pred = torch.empty_like(est)
        out = torch.zeros(1, dtype=torch.float64, device=dev) if r_true is not None else None
        _lib.check(lib.n2v_eccknn_predict(p_est, p_imp, p_true, est.numel(), float(global_mean),
                                          float(rating_scale[0]), float(rating_scale[1]), _lib.ptr(pred), _lib.ptr(out),
                                          _lib.stream_ptr(dev)))
    return (pred, float(out.item())) if r_true is not None else pred


# ---- k-NN sweep: every (k, min_k) of a grid from one neighbour selection ------------------------------------------------

def sweep_options(ks, min_ks):
    """(ks, min_ks) as lists of ints, the grid every sweep call takes; host only.  Each side has 1 to MAX_SWEEP values,
    strictly ascending; every k in [1, MAX_K], every min_k >= 1."""
    out = []
    for name, values in (("ks", ks), ("min_ks", min_ks)):
        if isinstance(values, (str, bytes)) or not isinstance(values, (collections.abc.Sequence, np.ndarray)):
            raise ValueError("%s %r: a list of 1 to %d integers" % (name, values, MAX_SWEEP))
        values = list(values)
        if not 1 <= len(values) <= MAX_SWEEP:
            raise ValueError("%s: %d values, outside [1, %d]" % (name, len(values), MAX_SWEEP))
        for v in values:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s: %r is not an integer" % (name, v))
        values = [int(v) for v in values]
        for v in values:                                         # the rules and the messages of a single k or min_k
            _knn_options(*((v, 1) if name == "ks" else (1, v)))
        if any(b <= a for a, b in zip(values, values[1:])):
            raise ValueError("%s %r: not strictly ascending" % (name, values))
        out.append(values)
    return out[0], out[1]


def estimate_sweep(sim, yr, qx, qy, ks, min_ks, centering=None, check=True):
    """(est fp64 [n_k][n_m][n_q], actual_k int32 [n_k][n_q], impossible uint8 [n_k][n_m][n_q]) device tensors: cell (j, m)
    is estimate_batch(sim, yr, qx, qy, ks[j], min_ks[m]) bit for bit, all of them from one selection at the largest k and one
    walk down it (n2v_eccknn_estimate_sweep).  The selection list is in a total order, so the list for k is the head of
    the list for any larger k, the rank-order sums for k are a prefix of the sums for the largest k, and min_k enters in
    the finish alone.  With a Centering the cells are estimate_batch_centered's (n2v_eccknn_estimate_sweep_centered), and yr
    is checked first as there; check False: the caller has run yr_check on these lists."""
    ks, min_ks = sweep_options(ks, min_ks)
    _require_gpu()
    model, n_x, n_y, dev = _knn_model("eccknn.estimate_sweep", sim, yr)
    p_qx, p_qy = _queries_ptrs("eccknn.estimate_sweep", qx, qy, dev)
    n_q = _query_count(qx, qy)
    n_k, n_m = len(ks), len(min_ks)
    tail = []
    if centering is not None:
        code, tx, sd, by = _centering_args(centering, n_x, n_y, "eccknn.estimate_sweep", dev)
        if check:
            yr_check(yr, n_x)
        tail = [code, 1 if centering.user_based else 0, float(centering.global_mean), tx, sd, by]
    lib = _lib.load()
    with torch.cuda.device(dev):
        est = torch.empty((n_k, n_m, n_q), dtype=torch.float64, device=dev)
        actual_k = torch.empty((n_k, n_q), dtype=torch.int32, device=dev)
        imp = torch.empty((n_k, n_m, n_q), dtype=torch.uint8, device=dev)
        fn = lib.n2v_eccknn_estimate_sweep if centering is None else lib.n2v_eccknn_estimate_sweep_centered
        _lib.check(fn(*model, p_qx, p_qy, n_q,
                      (_lib.C.c_int32 * n_k)(*ks), n_k, (_lib.C.c_int32 * n_m)(*min_ks), n_m, *tail, _lib.ptr(est),
                      _lib.ptr(actual_k), _lib.ptr(imp), _lib.stream_ptr(dev)))
    return est, actual_k, imp


def errors(pred, r_true):
    """(rmse, mae) host fp64 arrays over the columns of pred, a device fp64 tensor [n_cols][n_q] (or [n_q]: one column),
    against r_true, device fp64 [n_q] (n2v_eccknn_errors): both sums in query order, the rmse of a column the bits
    predict() gives for it."""
    _require_gpu()
    dev = _lib.call_device("eccknn.errors", "pred", pred)
    if pred.dim() == 1 and pred.is_contiguous():
        pred = pred.view(1, -1)
    p_pred = _lib.tensor("eccknn.errors", "pred", pred, torch.float64, dev, (None, None))
    p_true = _lib.tensor("eccknn.errors", "r_true", r_true, torch.float64, dev, pred.shape[1])
    if pred.numel() == 0:
        raise ValueError("errors: pred must be fp64 [n_cols][n_q] or [n_q] and r_true fp64 [n_q], n_q >= 1")
    lib = _lib.load()
    n_cols, n_q = pred.shape
    with torch.cuda.device(dev):
        out = torch.empty((2, n_cols), dtype=torch.float64, device=dev)
        _lib.check(lib.n2v_eccknn_errors(p_pred, p_true, n_q, n_cols, _lib.ptr(out[0]), _lib.ptr(out[1]),
                                         _lib.stream_ptr(dev)))
        out = out.cpu().numpy()
    return out[0].copy(), out[1].copy()


# ---- top-N lists ------------------------------------------------------------------------------------------------------

def topn_options(n, segments):
    """(n, segments) as the top-N calls take them; host only.  n in [1, MAX_TOP_N]; segments None (the library's choice,
    passed on as 0) or in [1, MAX_SEGMENTS]."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise ValueError("n %r: an integer in [1, %d]" % (n, MAX_TOP_N))
    if not 1 <= n <= MAX_TOP_N:
        raise ValueError("n %d outside [1, %d]" % (n, MAX_TOP_N))
    if segments is None:
        return int(n), 0
    if isinstance(segments, bool) or not isinstance(segments, (int, np.integer)):
        raise ValueError("segments %r: None or an integer in [1, %d]" % (segments, MAX_SEGMENTS))
    if not 1 <= segments <= MAX_SEGMENTS:
        raise ValueError("segments %d outside [1, %d]" % (segments, MAX_SEGMENTS))
    return int(n), int(segments)


def threshold_option(threshold):
    """ranking_metrics' threshold: None (every test item is ground truth) or a number that is not NaN; host only."""
    if threshold is None:
        return None
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or threshold != threshold:
        raise ValueError("threshold %r: None or a number" % (threshold,))
    return float(threshold)


def _topn_inputs(seen, n_users, n_items, owners, dev):
    """(the pointers of the checked seen CSR, its length, the int32 owners on `dev` (every user when owners is None))."""
    if not isinstance(seen, (tuple, list)) or len(seen) < 2 or getattr(seen[0], "dtype", None) != torch.int64 \
            or getattr(seen[1], "dtype", None) != torch.int32:
        raise ValueError("top_n: seen must be (int64 ptr, int32 item[, r]), the CSR of csr_by_x(u, i, r, n_users, n_items)")
    p_seen, n_seen, _ = _csr_ptrs("top_n", "seen", seen, dev, ("ptr", "item"))
    if seen[0].numel() != int(n_users) + 1:
        raise ValueError("top_n: seen has %d rows for %d users" % (seen[0].numel() - 1, n_users))
    csr_check(seen, n_items)
    if owners is None:
        owners = torch.arange(int(n_users), dtype=torch.int32, device=dev)
    owners = torch.as_tensor(owners).to(device=dev, dtype=torch.int32).contiguous()
    if owners.dim() != 1 or owners.numel() == 0:
        raise ValueError("top_n: owners must be a non-empty list of inner user ids")
    return p_seen, n_seen, owners


def _topn_call(fn, head, mid, tail, seen, n_users, n_items, owners, global_mean, rating_scale, n, segments, dev):
    """What the top_n of every predictor does after its own checks: the checked seen CSR and owners, the segment count,
    the buffers, and the one C call fn(*head, seen, owners, *mid, fallback, scale, n, S, *tail, buffers, stream),
    where fn is the library's function and head, mid and tail are the model's own arguments.  n and segments are topn_options'."""
    p_seen, n_seen, owners = _topn_inputs(seen, n_users, n_items, owners, dev)
    lib = _lib.load()
    n_owners = owners.numel()
    S = segments or int(lib.n2v_topn_segments(n_owners, n_items))
    with torch.cuda.device(dev):
        part_score = torch.empty((n_owners, S, n), dtype=torch.float64, device=dev)
        part_pos = torch.empty((n_owners, S, n), dtype=torch.int32, device=dev)
        items = torch.empty((n_owners, n), dtype=torch.int32, device=dev)
        score = torch.empty((n_owners, n), dtype=torch.float64, device=dev)
        _lib.check(fn(*head, *p_seen, n_seen, _lib.ptr(owners), n_owners,
                      *mid, float(global_mean), float(rating_scale[0]), float(rating_scale[1]), n, S, *tail,
                      _lib.ptr(part_score), _lib.ptr(part_pos), _lib.ptr(items), _lib.ptr(score), _lib.stream_ptr(dev)))
    return items, score


def _top_n(sim, yr, seen, user_based, k, min_k, global_mean, rating_scale, n, owners, segments, centering, check):
    """The one body of top_n (centering _PLAIN: n2v_eccknn_topn) and top_n_centered."""
    n, segments = topn_options(n, segments)
    _require_gpu()
    k, min_k = _knn_options(k, min_k)
    name = "eccknn.top_n" if centering is _PLAIN else "eccknn.top_n_centered"
    model, n_x, n_y, dev = _knn_model(name, sim, yr)
    tail = []
    if centering is not _PLAIN:
        tail = list(_centering_args(centering, n_x, n_y, name, dev))
        user_based, global_mean = bool(centering.user_based), centering.global_mean
        if check:
            yr_check(yr, n_x)
    n_users, n_items = (n_x, n_y) if user_based else (n_y, n_x)
    head = model + [1 if user_based else 0]
    fn = _lib.load().n2v_eccknn_topn if centering is _PLAIN else _lib.load().n2v_eccknn_topn_centered
    return _topn_call(fn, head, [k, min_k], tail, seen, n_users, n_items, owners, global_mean, rating_scale, n, segments,
                      dev)


def top_n(sim, yr, seen, user_based, k, min_k, global_mean, rating_scale, n, owners=None, segments=None):
    """(items int32 [n_owners][n], score fp64 [n_owners][n]) device tensors: per owner (inner user id, -1 = unknown) the n
    unseen inner items with the best predictions, each prediction the bits of estimate_batch + predict for that pair, ranked
    by descending score and ascending item id; (-1, NaN) where an owner has fewer than n candidates (n2v_eccknn_topn).
    seen: the owner-major CSR csr_by_x(u, i, r, n_users, n_items) of the training ratings; it is checked first and a
    malformed one is a ValueError.  owners None: every user.  segments None: the library's choice; the result does not
    depend on it."""
    return _top_n(sim, yr, seen, user_based, k, min_k, global_mean, rating_scale, n, owners, segments, _PLAIN, False)


def top_n_centered(sim, yr, seen, k, min_k, rating_scale, n, centering, owners=None, segments=None, check=True):
    """top_n under a Centering (n2v_eccknn_topn_centered): every prediction the bits of estimate_batch_centered + predict.
    user_based and global_mean are the centering's.  Under "baseline" an unknown owner's items score global_mean + bi[i],
    clipped, and so are ranked by it.  yr is checked first as estimate_batch_centered checks it."""
    return _top_n(sim, yr, seen, None, k, min_k, None, rating_scale, n, owners, segments, centering, check)


class TopN:
    """What the fitted rating predictors share above their top-N kernel: raw ids in, lists or metrics out.  A subclass
    has self.trainset after fit and implements _top_n(owners, n, segments) and _device() (Predictor's, below)."""

    def _seen(self):
        """The owner-major CSR of the training ratings on the device, built once per fit."""
        ts = self.trainset
        if getattr(self, "_seen_of", None) is not ts:
            dev = self._device()
            self._seen_csr = csr_by_x(_to_device(ts.u, torch.int32, dev), _to_device(ts.i, torch.int32, dev),
                                      _to_device(ts.r, torch.float64, dev), ts.n_users, ts.n_items)
            self._seen_of = ts
        return self._seen_csr

    def top_n_lists(self, n=10, users=None, segments=None):
        """(items int32 [len(users)][n], score fp64) device tensors for raw user ids (None: every training user in
        inner-id order); a user the trainset does not know is owner -1: items 0 .. n - 1 at the clipped training mean."""
        topn_options(n, segments)
        owners = None if users is None else self.trainset.inner_uids(list(users))
        return self._top_n(owners, n, segments)

    def recommend(self, n=10, users=None):
        """{raw user: [(raw item, score), ...]} best first, at most n entries each."""
        ts = self.trainset
        users = list(ts._raw2inner_u) if users is None else list(users)
        items, score = self.top_n_lists(n, users)
        items, score = items.cpu().numpy(), score.cpu().numpy()
        raw_items = list(ts._raw2inner_i)
        return {ru: [(raw_items[i], float(s)) for i, s in zip(items[row], score[row]) if i >= 0]
                for row, ru in enumerate(users)}

    def ranking_metrics(self, testset, n=10, threshold=None):
        """(f1, map, mrr, ndcg, per_user) of the top-n lists against the testset's (raw user, raw item, rating) triples,
        through recommend.user_metrics / averages (BiNE's top_N metrics).  A user's ground truth is their test items, those
        rated >= threshold when it is given; users without any are left out; the others keep their order of first
        appearance.  Test items the trainset does not know count in the ground truth's length only."""
        from . import recommend as rec
        topn_options(n, None)
        threshold = threshold_option(threshold)
        truth = {}
        for ru, ri, r in testset:
            rated = truth.setdefault(ru, {})
            if threshold is None or r >= threshold:
                rated[ri] = r
        users = [ru for ru, rated in truth.items() if rated]
        if not users:
            raise ValueError("ranking_metrics: no user of the testset has a ground-truth item")
        ptr, pos, lens = rec.truth_csr(users, list(self.trainset._raw2inner_i), truth)
        items, _ = self.top_n_lists(n, users)
        per_user = rec.user_metrics(items, ptr, pos, lens).cpu().numpy()
        return rec.averages(per_user) + (per_user,)


class Predictor(TopN):
    """What the fitted rating predictors share around their estimate kernel: raw test triples in, predictions out.  A
    subclass implements _estimate_batch(qx, qy) -> (est, *extras, impossible) device tensors and names in _MODEL a tensor
    of the fitted model (the predictor lives on its device); an item-based k-NN says _swapped(): its x are the items."""
    _MODEL = None

    def _swapped(self):
        return False

    def _device(self):
        return getattr(self, self._MODEL).device

    def _queries(self, u, i):
        """Inner user and item ids (-1 = unknown) as the int32 device pair _estimate_batch takes."""
        u, i = _to_device(u, torch.int32, self._device()), _to_device(i, torch.int32, self._device())
        return (i, u) if self._swapped() else (u, i)

    def _test_inputs(self, testset):
        """testset: (raw user, raw item, true rating) triples -> the query pair of _queries and the true ratings on the device."""
        testset = list(testset)
        if not testset:
            raise ValueError("test: empty testset")
        ts = self.trainset
        qx, qy = self._queries(ts.inner_uids([t[0] for t in testset]), ts.inner_iids([t[1] for t in testset]))
        return qx, qy, _to_device(np.array([t[2] for t in testset], dtype=np.float64), torch.float64, self._device())

    def _test(self, testset):
        """testset: (raw user, raw item, true rating) triples -> (pred, *extras, impossible, rmse)."""
        qx, qy, r_true = self._test_inputs(testset)
        est, *extras, imp = self._estimate_batch(qx, qy)
        pred, err = predict(est, imp, self.trainset.global_mean, self.trainset.rating_scale, r_true)
        return (pred, *extras, imp, err)

    def test(self, testset):
        """Arrays (est, *extras, was_impossible): est after the global-mean fallback and clipping; the extras are
        actual_k for a k-NN, n_deviations for SlopeOne, none for the factor models."""
        pred, *extras, imp, _ = self._test(testset)
        return (pred.cpu().numpy(), *[e.cpu().numpy() for e in extras], imp.cpu().numpy().astype(bool))

    def rmse(self, testset):
        return self._test(testset)[-1]

    def mae(self, testset):
        """The mean absolute error of test()'s predictions, the second measure of surprise's cross_validate: the sum in
        test order (errors)."""
        qx, qy, r_true = self._test_inputs(testset)
        est, *_, imp = self._estimate_batch(qx, qy)
        pred = predict(est, imp, self.trainset.global_mean, self.trainset.rating_scale)
        return float(errors(pred, r_true)[1][0])


# ---- the algorithm ----------------------------------------------------------------------------------------------------

class _SymmetricKNN(Predictor):
    """What EccenKNN and KNNBasic share: the options, the weights, the device fit and estimate / test / rmse.  A subclass
    names its similarities (_check_name) and may add to them (_similarity)."""
    _MODEL = "sim"

    def __init__(self, k=40, min_k=1, sim_options=None, device="cuda:0"):
        self.k, self.min_k = int(k), int(min_k)
        self.sim_options = dict(sim_options or {})
        self.sim_options.setdefault("user_based", True)
        self.device = device
        name = self.sim_options.get("name", "msd").lower()
        self._check_name(name)
        _knn_options(self.k, self.min_k)
        self.name = name
        self.form = self.sim_options.get("form", "auto")
        if self.form not in FORMS:
            raise ValueError("eccknn: form %r, allowed values are %s" % (self.form, ", ".join(FORMS)))

    def _weights(self, trainset, weights):
        user_based = self.sim_options["user_based"]
        n_y = trainset.n_items if user_based else trainset.n_users
        if isinstance(weights, dict):
            table = trainset._raw2inner_i if user_based else trainset._raw2inner_u
            w = np.empty(n_y, dtype=np.float64)
            for raw, inner in table.items():
                w[inner] = weights[raw]                     # KeyError for a missing id, as i_dict[y] raises
            return w
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != (n_y,):
            raise ValueError("weights: shape %s, expected (%d,)" % (w.shape, n_y))
        return w

    def _similarity(self, dense_mask, xr, dw):
        """cosine / msd from whichever form _fit prepared."""
        ms = self.sim_options.get("min_support", 1)
        if dense_mask is not None:
            return similarity(dense_mask[0], dense_mask[1], dw, self.name, ms)
        return similarity_sparse(xr, dw, self.n_y, self.name, ms)

    def _fit(self, trainset, w):
        """w: host fp64[n_y], or None where the similarity takes no weights."""
        _require_gpu()
        dev = torch.device(self.device)
        ts = trainset
        user_based = self.sim_options["user_based"]
        x, y, yr = (ts.u, ts.i, ts.ir) if user_based else (ts.i, ts.u, ts.ur)
        self.n_x, self.n_y = (ts.n_users, ts.n_items) if user_based else (ts.n_items, ts.n_users)
        self.trainset = ts
        form = choose_form(self.n_x, self.n_y, self.form, int(_lib.load().n2v_eccknn_max_dense()))
        dx, dy, dr = _to_device(x, torch.int32, dev), _to_device(y, torch.int32, dev), _to_device(ts.r, torch.float64, dev)
        dw = None if w is None else _to_device(w, torch.float64, dev)
        if form == "dense":
            self.sim = self._similarity(densify(dx, dy, dr, self.n_x, self.n_y), None, dw)
        else:
            self.sim = self._similarity(None, csr_by_x(dx, dy, dr, self.n_x, self.n_y), dw)
        self.yr = _csr_to_device(yr, dev)
        return self

    def _swapped(self):
        return not self.sim_options["user_based"]

    def _estimate_batch(self, qx, qy):
        return estimate_batch(self.sim, self.yr, qx, qy, self.k, self.min_k)

    def estimate(self, u, i):
        """(est, {'actual_k': n}) for inner ids u, i; PredictionImpossible as the reference raises it."""
        if not (self.trainset.knows_user(u) and self.trainset.knows_item(i)):
            raise PredictionImpossible("User and/or item is unkown.")
        est, ak, imp = self._estimate_batch(*self._queries([u], [i]))
        if int(imp.item()):
            raise PredictionImpossible("Not enough neighbors.")
        return float(est.item()), {"actual_k": int(ak.item())}

    def _top_n(self, owners, n, segments):
        ts = self.trainset
        return top_n(self.sim, self.yr, self._seen(), self.sim_options["user_based"], self.k, self.min_k, ts.global_mean,
                     ts.rating_scale, n, owners, segments)

    def _sweep_centering(self):
        """What estimate_sweep takes as its centering: None here, the fit's Centering in the centred classes."""
        return None

    def _sweep(self, testset, ks, min_ks):
        """(ks, min_ks, pred [n_k][n_m][n_q], actual_k, impossible, r_true): the grid's estimates of the test pairs from
        one estimate_sweep, then the fallback and the clip of every cell in one predict call (it is elementwise)."""
        ks, min_ks = sweep_options(ks, min_ks)
        qx, qy, r_true = self._test_inputs(testset)
        est, actual_k, imp = estimate_sweep(self.sim, self.yr, qx, qy, ks, min_ks, self._sweep_centering(), check=False)
        pred = predict(est.view(-1), imp.view(-1), self.trainset.global_mean, self.trainset.rating_scale).view(est.shape)
        return ks, min_ks, pred, actual_k, imp, r_true

    def test_sweep(self, testset, ks, min_ks):
        """{(k, min_k): (pred, actual_k, was_impossible)} over the grid ks x min_ks: every value what test() returns from a
        model with that k and min_k, all from one neighbour selection at the largest k.  self.k and self.min_k play no part
        and are not touched."""
        ks, min_ks, pred, actual_k, imp, _ = self._sweep(testset, ks, min_ks)
        pred, actual_k, imp = pred.cpu().numpy(), actual_k.cpu().numpy(), imp.cpu().numpy().astype(bool)
        return {(k, m): (pred[j, n], actual_k[j], imp[j, n]) for j, k in enumerate(ks) for n, m in enumerate(min_ks)}

    def accuracy_sweep(self, testset, ks, min_ks):
        """{(k, min_k): {"rmse": ..., "mae": ...}} over the grid, in grid order: the rmse() and mae() of a model with that k
        and min_k, from one estimate_sweep, one predict and one errors call."""
        ks, min_ks, pred, _, _, r_true = self._sweep(testset, ks, min_ks)
        rmse, mae = errors(pred.view(len(ks) * len(min_ks), -1), r_true)
        cells = [(k, m) for k in ks for m in min_ks]
        return {cell: {"rmse": float(rmse[c]), "mae": float(mae[c])} for c, cell in enumerate(cells)}


class EccenKNN(_SymmetricKNN):
    def _check_name(self, name):
        if name not in SIM_NAMES:
            raise NameError("Wrong sim name " + name + ". Allowed values " + "are " + ", ".join(SIM_NAMES) + ".")
        if name not in _METHOD:
            raise NameError("Wrong sim name " + name + ". " + name + " is surprise's own similarity, not the reference's; "
                            "here the allowed values are " + ", ".join(_METHOD) + ".")

    def fit(self, trainset, weights):
        return self._fit(trainset, self._weights(trainset, weights))


class KNNBasic(_SymmetricKNN):
    """surprise's KNNBasic under cosine, msd, pearson and pearson_baseline.  fit(trainset) is the plain baseline;
    fit(trainset, weights) weights every co-rating's product by w[y] as EccenKNN does.  pearson_baseline computes the ALS
    baselines first (bsl_options) and reads sim_options["shrinkage"] (default 100)."""

    def __init__(self, k=40, min_k=1, sim_options=None, bsl_options=None, device="cuda:0"):
        _SymmetricKNN.__init__(self, k, min_k, sim_options, device)
        self.bsl_options = bsl_check(bsl_options)
        self.shrinkage = float(self.sim_options.get("shrinkage", 100))

    def _check_name(self, name):
        if name not in SIM_NAMES:
            raise NameError("Wrong sim name " + name + ". Allowed values " + "are " + ", ".join(SIM_NAMES) + ".")

    def _similarity(self, dense_mask, xr, dw):
        if self.name in _METHOD:
            return _SymmetricKNN._similarity(self, dense_mask, xr, dw)
        kw = {"w": dw, "min_support": self.sim_options.get("min_support", 1)}
        if self.name == "pearson_baseline":
            self._bsl()
            kw.update(global_mean=self.trainset.global_mean, bx=self.bx, by=self.by, shrinkage=self.shrinkage)
        if dense_mask is not None:
            return similarity_pearson(dense_mask[0], dense_mask[1], self.name, **kw)
        return similarity_pearson_sparse(xr, self.n_y, self.name, **kw)

    def _bsl(self):
        """The ALS baselines of the trainset being fitted as (self.bx, self.by), computed once per fit."""
        if self._bsl_of is not self.trainset:
            bu, bi = baselines(self.trainset, self.bsl_options, self.device)
            self.bx, self.by = (bu, bi) if self.sim_options["user_based"] else (bi, bu)
            self._bsl_of = self.trainset

    def fit(self, trainset, weights=None):
        self._bsl_of = None
        if weights is not None:
            w = self._weights(trainset, weights)
        elif self.name in _METHOD:                              # the old kernels take their weights as given: ones
            w = np.ones(trainset.n_items if self.sim_options["user_based"] else trainset.n_users)
        else:
            w = None
        return self._fit(trainset, w)


class _CenteredKNN(KNNBasic):
    """What KNNWithMeans, KNNWithZScore and KNNBaseline share above KNNBasic: its constructor, similarities, forms, weights,
    bsl_options and shrinkage; after the fit a Centering (_tables), and estimate / test / rmse / top-N through the centred
    kernels (_estimate_batch, _top_n).  The rules are surprise 1.0.6's, restated from memory (tests/knn_centered_reference.py is the definition; parity
    with surprise itself is unpinned): the neighbours of KNNBasic, each rating centred before it is weighted, and too few
    neighbours leave the base estimate instead of making the prediction impossible."""
    MODE = None

    def fit(self, trainset, weights=None):
        KNNBasic.fit(self, trainset, weights)
        yr_check(self.yr, self.n_x)                             # once per fit: the kernels index their tables with yr's ids
        self.centering = self._tables()
        return self

    def _x_rows(self):
        """The rating lists of the x side on the device, (ptr, r), each in training order."""
        ts = self.trainset
        xr = ts.ur if self.sim_options["user_based"] else ts.ir
        dev = torch.device(self.device)
        return _to_device(xr[0], torch.int64, dev), _to_device(xr[2], torch.float64, dev)

    def _estimate_batch(self, qx, qy):
        return estimate_batch_centered(self.sim, self.yr, qx, qy, self.k, self.min_k, self.centering, check=False)

    def estimate(self, u, i):
        """(est, {'actual_k': n}) for inner ids u, i.  PredictionImpossible only for an unknown user or item."""
        if not (self.trainset.knows_user(u) and self.trainset.knows_item(i)):
            raise PredictionImpossible("User and/or item is unkown.")
        est, ak, _ = self._estimate_batch(*self._queries([u], [i]))
        return float(est.item()), {"actual_k": int(ak.item())}

    def _sweep_centering(self):
        return self.centering

    def _top_n(self, owners, n, segments):
        return top_n_centered(self.sim, self.yr, self._seen(), self.k, self.min_k, self.trainset.rating_scale, n,
                              self.centering, owners, segments, check=False)


class KNNWithMeans(_CenteredKNN):
    """surprise's KNNWithMeans: est = mu[x] + sum sim * (r - mu[x2]) / sum sim, mu the mean of a row's ratings summed in
    training order (numpy's pairwise sum above 8 elements is a documented deviation)."""
    MODE = "means"

    def _tables(self):
        ptr_, r = self._x_rows()
        self.means, _ = row_moments(ptr_, r)
        return Centering(self.MODE, self.sim_options["user_based"], self.trainset.global_mean, self.means, None, None)


class KNNWithZScore(_CenteredKNN):
    """surprise's KNNWithZScore: est = mu[x] + sd[x] * sum sim * ((r - mu[x2]) / sd[x2]) / sum sim.  A row whose sigma is 0.0
    takes the sigma of all ratings; where that is 0.0 too (every rating equal) the NaN that follows is kept, and predict
    turns it into the upper end of the scale."""
    MODE = "zscore"

    def _tables(self):
        ptr_, r = self._x_rows()
        dev = r.device
        all_r = _to_device(self.trainset.r, torch.float64, dev)
        one_row = torch.tensor([0, all_r.numel()], dtype=torch.int64, device=dev)
        self.overall_sigma = float(row_moments(one_row, all_r)[1].item())
        self.means, self.sigmas = row_moments(ptr_, r, zero_sigma=self.overall_sigma)
        return Centering(self.MODE, self.sim_options["user_based"], self.trainset.global_mean, self.means, self.sigmas, None)


class KNNBaseline(_CenteredKNN):
    """surprise's KNNBaseline: est = b_ui + sum sim * (r - b_vi) / sum sim with the ALS baselines of bsl_options, computed
    once per fit; -sim pearson_baseline reads the same pair.  Nothing is impossible: an unknown user drops bu, an unknown
    item bi, and estimate never raises.  So an unknown owner's top-N list is not a constant: it is the items ranked by the
    clipped global_mean + bi[i]."""
    MODE = "baseline"

    def _tables(self):
        self._bsl()
        return Centering(self.MODE, self.sim_options["user_based"], self.trainset.global_mean, self.bx, None, self.by)

    def estimate(self, u, i):
        """(est, {'actual_k': n}) for inner ids u, i, anything else being an unknown id.  Never raises."""
        ts = self.trainset
        est, ak, _ = self._estimate_batch(*self._queries([u if ts.knows_user(u) else -1], [i if ts.knows_item(i) else -1]))
        return float(est.item()), {"actual_k": int(ak.item())}
