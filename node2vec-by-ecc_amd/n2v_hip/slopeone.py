"""SlopeOne rating prediction on the device (csrc/n2v_eccknn.hip and csrc/n2v_slopeone.hip, C-ABI include/n2v_sim.h).

surprise 1.0.6's SlopeOne (Lemire and Maclachlan 2005), the parameter-free baseline of its prediction_algorithms package:
dev[i][j] is the mean of r[u][i] - r[u][j] over the users who rated both items, and a prediction is the user's mean plus
the mean of dev[i][j] over the items j the user rated that share a rater with i.  Parity is UNPINNED: `surprise` is not a
dependency here, the rules are restated from memory (tests/slopeone_reference.py, which is the definition) and the kernels
are held to that restatement bit for bit.  Deviation: the user means are sequential sums in training order
(eccknn.row_moments), where numpy's mean adds pairwise above 8 elements.

The model has no hyper-parameter, no random state and no sequential update, so it follows surprise's own order of the
ratings.  The fit is the co-rated pair pass of the similarity kernels with a lighter accumulator, in the same two forms
with the same bytes: sim_options["form"] = "auto" (dense inside n_items * n_users <= 2^31, sparse past it), "dense" or
"sparse".  The table is n_items x n_items (fp64 dev, int32 freq), n_items^2 <= 2^31.  The top-N lists read it densely:
for a user and 64 neighbouring candidates every rated item contributes one contiguous piece of its row.

Everything is fp64.  There is no CPU fallback.
"""
import torch

from . import _lib
from .eccknn import (PredictionImpossible, Predictor, _csr_ptrs, _csr_to_device, _dense_ptrs, _queries_ptrs, _query_count,
                     _require_gpu, _to_device, _topn_call, choose_form, csr_by_x, csr_check, densify, row_moments,
                     topn_options, yr_check, FORMS)

MAX_TABLE = 1 << 31              # elements of dev: n_items * n_items


def check_items(n_items):
    """n_items as the table allows it; host arithmetic only, before anything is allocated."""
    n_items = int(n_items)
    if n_items < 1 or n_items * n_items > MAX_TABLE:
        raise ValueError("slopeone: n_items^2 = %d^2 exceeds the table limit of %d elements (16 GiB of dev, 8 GiB of freq)"
                         % (n_items, MAX_TABLE))
    return n_items


# ---- C-ABI wrappers (device tensors in, device tensors out) -----------------------------------------------------------

def _table(n_items, dev_, accumulators):
    return (torch.empty((n_items, n_items), dtype=torch.float64, device=dev_),
            torch.empty((n_items, n_items), dtype=torch.int32, device=dev_),
            torch.empty((n_items, n_items), dtype=torch.float64, device=dev_) if accumulators else None)


def deviations(dense, mask, accumulators=False):
    """(dev fp64, freq int32) [n_items][n_items] from eccknn.densify(items, users, r, n_items, n_users)
    (n2v_slopeone_dev); with accumulators also acc, the raw sums."""
    if isinstance(dense, torch.Tensor) and dense.dim() == 2:
        check_items(dense.shape[1])                             # host arithmetic, before the GPU is asked for
    _require_gpu()
    p_dense, p_mask, n_items, n_users, d = _dense_ptrs("slopeone.deviations", dense, mask)
    with torch.cuda.device(d):
        dev, freq, acc = _table(n_items, d, accumulators)
        _lib.check(_lib.load().n2v_slopeone_dev(p_dense, p_mask, n_items, n_users, _lib.ptr(dev), _lib.ptr(freq),
                                                _lib.ptr(acc), _lib.stream_ptr(d)))
    return (dev, freq, acc) if accumulators else (dev, freq)


def deviations_sparse(xr, n_users, accumulators=False):
    """deviations() from the item-major CSR xr = eccknn.csr_by_x(items, users, r, n_items, n_users): the same bytes, no
    n_items * n_users limit (n2v_slopeone_dev_sparse).  The CSR is checked first; a malformed one is a ValueError."""
    if isinstance(xr, (tuple, list)) and len(xr) == 3 and isinstance(xr[0], torch.Tensor):
        check_items(xr[0].numel() - 1)                          # host arithmetic, before the GPU is asked for
    _require_gpu()
    p_xr, n, d = _csr_ptrs("slopeone.deviations_sparse", "xr", xr, None, ("ptr", "user", "r"))
    n_items = xr[0].numel() - 1
    csr_check(xr, n_users)
    with torch.cuda.device(d):
        dev, freq, acc = _table(n_items, d, accumulators)
        _lib.check(_lib.load().n2v_slopeone_dev_sparse(*p_xr, n_items, int(n_users), n, _lib.ptr(dev),
                                                       _lib.ptr(freq), _lib.ptr(acc), _lib.stream_ptr(d)))
    return (dev, freq, acc) if accumulators else (dev, freq)


def _model_args(fn, dev, freq, ur, user_mean, check):
    """The model's part of the two calls below after the host checks; ur = (ptr int64[n_users + 1], item int32, r fp64) in
    training order.  check: eccknn.yr_check on ur (integers only): a malformed list is a ValueError, not a launch."""
    d = _lib.call_device(fn, "dev", dev)
    n_items = dev.shape[0] if dev.dim() else 0
    p_dev = _lib.tensor(fn, "dev", dev, torch.float64, d, (n_items, n_items))
    check_items(n_items)
    p_freq = _lib.tensor(fn, "freq", freq, torch.int32, d, (n_items, n_items))
    p_ur, n, _ = _csr_ptrs(fn, "ur", ur, d, ("ptr", "item", "r"))
    n_users = ur[0].numel() - 1
    p_mean = _lib.tensor(fn, "user_mean", user_mean, torch.float64, d, n_users)
    if check:
        yr_check(ur, n_items)
    return [p_dev, p_freq, n_items, p_ur[0], p_ur[1], n_users, n, p_mean]


def estimate_batch(dev, freq, ur, user_mean, qu, qi, check=True):
    """(est fp64, n_deviations int32, impossible uint8) device tensors for int32 device queries, -1 = unknown
    (n2v_slopeone_estimate)."""
    _require_gpu()
    model = _model_args("slopeone.estimate_batch", dev, freq, ur, user_mean, check)
    d = dev.device
    p_qu, p_qi = _queries_ptrs("slopeone.estimate_batch", qu, qi, d, ("qu", "qi"))
    n_q = _query_count(qu, qi, ("user", "item"), ("qu", "qi"))
    with torch.cuda.device(d):
        est = torch.empty(n_q, dtype=torch.float64, device=d)
        n_dev = torch.empty(n_q, dtype=torch.int32, device=d)
        imp = torch.empty(n_q, dtype=torch.uint8, device=d)
        _lib.check(_lib.load().n2v_slopeone_estimate(*model, p_qu, p_qi, n_q, _lib.ptr(est), _lib.ptr(n_dev),
                                                     _lib.ptr(imp), _lib.stream_ptr(d)))
    return est, n_dev, imp


def top_n(dev, freq, ur, user_mean, seen, global_mean, rating_scale, n, owners=None, segments=None, check=True):
    """eccknn.top_n for the deviation table (n2v_slopeone_topn): per owner the n unseen inner items with the best
    predictions, each the bits of estimate_batch + eccknn.predict for that pair."""
    n, segments = topn_options(n, segments)
    _require_gpu()
    model = _model_args("slopeone.top_n", dev, freq, ur, user_mean, check)
    return _topn_call(_lib.load().n2v_slopeone_topn, model, [], [], seen, model[5], model[2], owners, global_mean, rating_scale, n,
                      segments, dev.device)


# ---- the algorithm ----------------------------------------------------------------------------------------------------

class SlopeOne(Predictor):
    """surprise's SlopeOne, plus sim_options["form"] and device.  fit(trainset) takes an eccknn.Trainset; afterwards dev
    (fp64), freq (int32) [n_items][n_items] and user_mean (fp64[n_users]) are device tensors."""
    _MODEL = "dev"

    def __init__(self, sim_options=None, device="cuda:0"):
        self.sim_options = dict(sim_options or {})
        unknown = sorted(set(self.sim_options) - {"form"})
        if unknown:
            raise ValueError("slopeone: sim_options key %s: SlopeOne has no similarity, the one key is form" % ", ".join(unknown))
        self.form = self.sim_options.get("form", "auto")
        if self.form not in FORMS:
            raise ValueError("slopeone: form %r, allowed values are %s" % (self.form, ", ".join(FORMS)))
        self.device = device

    def fit(self, trainset):
        ts = trainset
        check_items(ts.n_items)
        form = choose_form(ts.n_items, ts.n_users, self.form)
        _require_gpu()
        d = torch.device(self.device)
        self.trainset = ts
        di, du, dr = _to_device(ts.i, torch.int32, d), _to_device(ts.u, torch.int32, d), _to_device(ts.r, torch.float64, d)
        if form == "dense":
            self.dev, self.freq = deviations(*densify(di, du, dr, ts.n_items, ts.n_users))
        else:
            self.dev, self.freq = deviations_sparse(csr_by_x(di, du, dr, ts.n_items, ts.n_users), ts.n_users)
        self.ur = _csr_to_device(ts.ur, d)
        yr_check(self.ur, ts.n_items)
        self.user_mean = row_moments(self.ur[0], self.ur[2])[0]
        return self

    def _estimate_batch(self, qu, qi):
        return estimate_batch(self.dev, self.freq, self.ur, self.user_mean, qu, qi, check=False)

    def estimate(self, u, i):
        """(est, {'n_deviations': n}) for inner ids u, i; PredictionImpossible for an unknown one, as surprise raises it."""
        if not (self.trainset.knows_user(u) and self.trainset.knows_item(i)):
            raise PredictionImpossible("User and/or item is unkown.")
        est, n_dev, _ = self._estimate_batch(*self._queries([u], [i]))
        return float(est.item()), {"n_deviations": int(n_dev.item())}

    def _top_n(self, owners, n, segments):
        ts = self.trainset
        return top_n(self.dev, self.freq, self.ur, self.user_mean, self._seen(), ts.global_mean, ts.rating_scale, n, owners,
                     segments, check=False)
