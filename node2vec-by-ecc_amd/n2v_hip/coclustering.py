"""Co-clustering rating prediction trained on the device (csrc/n2v_cocl.hip, C-ABI include/n2v_sim.h).

surprise 1.0.6's CoClustering (George and Merugu 2005): every user and every item belongs to one cluster, and a prediction
is the co-cluster's average plus what the user's mean and the item's mean differ from their clusters' averages.  Parity is
UNPINNED: `surprise` is not a dependency here, the algorithm is restated from memory (tests/coclustering_reference.py,
which is the definition) and the kernels are held to that restatement bit for bit.

Every step of an epoch reads only tables fixed when the step began (the averages and the other side's assignment), so all
users, and then all items, are reassigned in parallel, one wavefront per row with one candidate cluster per lane, in
surprise's own order of the ratings, and two fits give the same bytes.  That bounds the cluster counts to [1, 64] a side.
Deviations: the cluster sums are grouped by user row instead of one chain over all ratings (the same bytes wherever the
sums are exact, as on ratings that are multiples of 1/2), and the user and item means are sequential sums in training
order (eccknn.row_moments), where numpy's mean adds pairwise above 8 elements.  The clusters are drawn on the host
(numpy's RandomState, as surprise draws them) and uploaded.  Everything is fp64.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from .eccknn import (Predictor, _csr_ptrs, _csr_to_device, _queries_ptrs, _query_count, _require_gpu, _to_device, _topn_call,
                     row_moments, topn_options, yr_check)
from .nmf import row_order

MAX_CLUSTERS = 64                # n2v_cocl_max_clusters()


def check_clusters(n_cltr_u, n_cltr_i):
    """(n_cltr_u, n_cltr_i) as the kernels allow them; host arithmetic only."""
    n_cltr_u, n_cltr_i = int(n_cltr_u), int(n_cltr_i)
    if not (1 <= n_cltr_u <= MAX_CLUSTERS and 1 <= n_cltr_i <= MAX_CLUSTERS):
        raise ValueError("coclustering: n_cltr_u %d, n_cltr_i %d outside [1, %d] (one lane holds one cluster)"
                         % (n_cltr_u, n_cltr_i, MAX_CLUSTERS))
    return n_cltr_u, n_cltr_i


# ---- C-ABI wrappers (device tensors in, device tensors out) -----------------------------------------------------------

def _check_assignment(what, cltr, n_rows, n_cltr):
    """Integers only: every entry of an assignment in [0, n_cltr).  Its type and length are the wrappers' own check."""
    if int(cltr.min().item()) < 0 or int(cltr.max().item()) >= int(n_cltr):
        raise ValueError("coclustering: %s holds a cluster id outside [0, %d)" % (what, n_cltr))


def _tables(fn, avgs, user_mean, item_mean, dev=None, n_users=None, n_items=None):
    """([avg_cltr_u, avg_cltr_i, avg_cocltr, user_mean, item_mean] pointers, n_cltr_u, n_cltr_i, n_users, n_items, device)
    of the fp64 tables both the assignment pass and the estimates read.  dev None: the GPU of user_mean; n_users, n_items
    None: the lengths of the two means."""
    if not isinstance(avgs, (tuple, list)) or len(avgs) < 3:
        raise ValueError("%s: avgs must be (avg_cltr_u, avg_cltr_i, avg_cocltr[, ...]) of averages()" % fn)
    if dev is None:
        dev = _lib.call_device(fn, "user_mean", user_mean)
    p_um = _lib.tensor(fn, "user_mean", user_mean, torch.float64, dev, (n_users,))
    p_im = _lib.tensor(fn, "item_mean", item_mean, torch.float64, dev, (n_items,))
    p_u = _lib.tensor(fn, "avgs[0] (avg_cltr_u)", avgs[0], torch.float64, dev, (None,))
    p_i = _lib.tensor(fn, "avgs[1] (avg_cltr_i)", avgs[1], torch.float64, dev, (None,))
    n_cltr_u, n_cltr_i = check_clusters(avgs[0].numel(), avgs[1].numel())
    p_cc = _lib.tensor(fn, "avgs[2] (avg_cocltr)", avgs[2], torch.float64, dev, (n_cltr_u, n_cltr_i))
    return [p_u, p_i, p_cc, p_um, p_im], n_cltr_u, n_cltr_i, user_mean.numel(), item_mean.numel(), dev


def _overlaps(a, b):
    return a.data_ptr() < b.data_ptr() + b.numel() * 4 and b.data_ptr() < a.data_ptr() + a.numel() * 4


def averages(ur, n_items, cltr_u, cltr_i, n_cltr_u, n_cltr_i, global_mean, check=True):
    """(avg_cltr_u fp64[n_cltr_u], avg_cltr_i fp64[n_cltr_i], avg_cocltr fp64[n_cltr_u][n_cltr_i], count_cocltr int64) of the
    assignment (cltr_u int32[n_users], cltr_i int32[n_items]) over the user-major lists ur = (ptr int64[n_users + 1], item
    int32, r fp64) in training order (n2v_cocl_averages).  check: eccknn.yr_check on ur and the cluster ids' ranges
    (integers only); a malformed input is a ValueError, not a launch."""
    _require_gpu()
    n_cltr_u, n_cltr_i = check_clusters(n_cltr_u, n_cltr_i)
    fn = "coclustering.averages"
    p_ur, n, d = _csr_ptrs(fn, "ur", ur, None, ("ptr", "item", "r"))
    n_users, n_items = ur[0].numel() - 1, int(n_items)
    p_cu = _lib.tensor(fn, "cltr_u", cltr_u, torch.int32, d, n_users)
    p_ci = _lib.tensor(fn, "cltr_i", cltr_i, torch.int32, d, n_items)
    if check:
        yr_check(ur, n_items)
        _check_assignment("cltr_u", cltr_u, n_users, n_cltr_u)
        _check_assignment("cltr_i", cltr_i, n_items, n_cltr_i)
    with torch.cuda.device(d):
        part = torch.empty((n_users, n_cltr_i + 1), dtype=torch.float64, device=d)
        avg_u = torch.empty(n_cltr_u, dtype=torch.float64, device=d)
        avg_i = torch.empty(n_cltr_i, dtype=torch.float64, device=d)
        avg_cc = torch.empty((n_cltr_u, n_cltr_i), dtype=torch.float64, device=d)
        count = torch.empty((n_cltr_u, n_cltr_i), dtype=torch.int64, device=d)
        _lib.check(_lib.load().n2v_cocl_averages(*p_ur, n_users, n_items, n, p_cu, p_ci, n_cltr_u, n_cltr_i,
                                                 float(global_mean), _lib.ptr(part), _lib.ptr(avg_u), _lib.ptr(avg_i),
                                                 _lib.ptr(avg_cc), _lib.ptr(count), _lib.stream_ptr(d)))
    return avg_u, avg_i, avg_cc, count


def assign(lst, user_side, cltr_u, cltr_i, avgs, user_mean, item_mean, order=None, check=True):
    """One assignment pass of one side, in place (n2v_cocl_assign).  user_side: lst is the user-major list (ptr, item, r),
    cltr_i is read and cltr_u written; otherwise lst is the item-major list (ptr, user, r), cltr_u is read and cltr_i
    written.  avgs: (avg_cltr_u, avg_cltr_i, avg_cocltr[, ...]) of averages().  order: None or an int32 permutation of the
    rows (nmf.row_order: longest lists first); it changes no bit.  check as averages(), on the side that is read."""
    _require_gpu()
    fn = "coclustering.assign"
    p_lst, n, d = _csr_ptrs(fn, "lst", lst, None, ("ptr", "item" if user_side else "user", "r"))
    p_cu = _lib.tensor(fn, "cltr_u", cltr_u, torch.int32, d, (None,))
    p_ci = _lib.tensor(fn, "cltr_i", cltr_i, torch.int32, d, (None,))
    n_users, n_items = cltr_u.numel(), cltr_i.numel()
    n_rows, n_other = (n_users, n_items) if user_side else (n_items, n_users)
    (p_au, p_ai, p_cc, p_um, p_im), n_cltr_u, n_cltr_i, _, _, _ = _tables(fn, avgs, user_mean, item_mean, d, n_users, n_items)
    _lib.tensor(fn, "lst[0] (int64 ptr)", lst[0], torch.int64, d, n_rows + 1)
    if _overlaps(cltr_u, cltr_i):
        raise ValueError("coclustering.assign: aliased buffers: cltr_u and cltr_i overlap, and one is read while the other is written")
    p_order = _lib.tensor(fn, "order", order, torch.int32, d, n_rows, optional=True)
    if check:
        yr_check(lst, n_other)
        if user_side:
            _check_assignment("cltr_i", cltr_i, n_items, n_cltr_i)
        else:
            _check_assignment("cltr_u", cltr_u, n_users, n_cltr_u)
    with torch.cuda.device(d):
        _lib.check(_lib.load().n2v_cocl_assign(*p_lst, p_order, n_users, n_items, n, 1 if user_side else 0, n_cltr_u, n_cltr_i,
                                               p_um, p_im, p_au, p_ai, p_cc, p_cu, p_ci, _lib.stream_ptr(d)))


def epoch(ur, ir, cltr_u, cltr_i, n_cltr_u, n_cltr_i, global_mean, user_mean, item_mean, order=(None, None), check=True):
    """One epoch in place: the averages of (cltr_u, cltr_i), the user pass, then the item pass over the assignment the user
    pass wrote and the same averages.  Returns the averages the epoch used."""
    avgs = averages(ur, cltr_i.numel(), cltr_u, cltr_i, n_cltr_u, n_cltr_i, global_mean, check=check)
    assign(ur, True, cltr_u, cltr_i, avgs, user_mean, item_mean, order[0], check=False)     # averages() checked ur and both sides
    assign(ir, False, cltr_u, cltr_i, avgs, user_mean, item_mean, order[1], check=check)
    return avgs


def _model_args(fn, cltr_u, cltr_i, avgs, user_mean, item_mean, check):
    """(the model's part of the two calls below after the host checks, the device of the call: user_mean's)."""
    tables, n_cltr_u, n_cltr_i, n_users, n_items, d = _tables(fn, avgs, user_mean, item_mean)
    p_cu = _lib.tensor(fn, "cltr_u", cltr_u, torch.int32, d, n_users)
    p_ci = _lib.tensor(fn, "cltr_i", cltr_i, torch.int32, d, n_items)
    if check:
        _check_assignment("cltr_u", cltr_u, n_users, n_cltr_u)
        _check_assignment("cltr_i", cltr_i, n_items, n_cltr_i)
    return [p_cu, p_ci] + tables + [n_users, n_items, n_cltr_u, n_cltr_i], d


def estimate_batch(cltr_u, cltr_i, avgs, user_mean, item_mean, global_mean, qu, qi, check=True):
    """(est fp64, impossible uint8, all zero) device tensors for int32 device queries, -1 = unknown (n2v_cocl_estimate)."""
    _require_gpu()
    model, d = _model_args("coclustering.estimate_batch", cltr_u, cltr_i, avgs, user_mean, item_mean, check)
    p_qu, p_qi = _queries_ptrs("coclustering.estimate_batch", qu, qi, d, ("qu", "qi"))
    n_q = _query_count(qu, qi, ("user", "item"), ("qu", "qi"))
    with torch.cuda.device(d):
        est = torch.empty(n_q, dtype=torch.float64, device=d)
        imp = torch.empty(n_q, dtype=torch.uint8, device=d)
        _lib.check(_lib.load().n2v_cocl_estimate(*model, float(global_mean), p_qu, p_qi, n_q, _lib.ptr(est),
                                                 _lib.ptr(imp), _lib.stream_ptr(d)))
    return est, imp


def top_n(cltr_u, cltr_i, avgs, user_mean, item_mean, seen, global_mean, rating_scale, n, owners=None, segments=None, check=True):
    """eccknn.top_n for the co-clustering model (n2v_cocl_topn): per owner the n unseen inner items with the best
    predictions, each the bits of estimate_batch + eccknn.predict for that pair.  An unknown owner's items score their
    clipped item_mean."""
    n, segments = topn_options(n, segments)
    _require_gpu()
    model, d = _model_args("coclustering.top_n", cltr_u, cltr_i, avgs, user_mean, item_mean, check)
    return _topn_call(_lib.load().n2v_cocl_topn, model, [], [], seen, model[7], model[8], owners, global_mean, rating_scale, n,
                      segments, d)


# ---- the algorithm ----------------------------------------------------------------------------------------------------

class CoClustering(Predictor):
    """surprise's CoClustering with its options and defaults, plus device.  fit(trainset) takes an eccknn.Trainset;
    afterwards cltr_u, cltr_i (int32), avg_cltr_u, avg_cltr_i, avg_cocltr, user_mean and item_mean (fp64) are device
    tensors."""
    _MODEL = "avg_cocltr"

    def __init__(self, n_cltr_u=3, n_cltr_i=3, n_epochs=20, random_state=0, device="cuda:0"):
        self.n_cltr_u, self.n_cltr_i = check_clusters(n_cltr_u, n_cltr_i)
        self.n_epochs = int(n_epochs)
        if self.n_epochs < 0:
            raise ValueError("n_epochs %d < 0" % self.n_epochs)
        self.random_state = random_state
        self.device = device

    def fit(self, trainset):
        _require_gpu()
        d = torch.device(self.device)
        ts = self.trainset = trainset
        rng = np.random.RandomState(self.random_state)
        cltr_u = rng.randint(self.n_cltr_u, size=ts.n_users)
        cltr_i = rng.randint(self.n_cltr_i, size=ts.n_items)
        with torch.cuda.device(d):
            self.ur, self.ir = _csr_to_device(ts.ur, d), _csr_to_device(ts.ir, d)
            yr_check(self.ur, ts.n_items)
            yr_check(self.ir, ts.n_users)
            self.user_mean = row_moments(self.ur[0], self.ur[2])[0]
            self.item_mean = row_moments(self.ir[0], self.ir[2])[0]
            self.cltr_u, self.cltr_i = _to_device(cltr_u, torch.int32, d), _to_device(cltr_i, torch.int32, d)
            order = (row_order(self.ur[0]), row_order(self.ir[0]))
            args = (self.ur, self.ir, self.cltr_u, self.cltr_i, self.n_cltr_u, self.n_cltr_i, ts.global_mean, self.user_mean,
                    self.item_mean)
            for _ in range(self.n_epochs):                        # the lists were checked above, and the kernels write ids in range
                epoch(*args, order=order, check=False)
            self.avg_cltr_u, self.avg_cltr_i, self.avg_cocltr, self.count_cocltr = averages(
                self.ur, ts.n_items, self.cltr_u, self.cltr_i, self.n_cltr_u, self.n_cltr_i, ts.global_mean, check=False)
        return self

    def _avgs(self):
        return self.avg_cltr_u, self.avg_cltr_i, self.avg_cocltr

    def _estimate_batch(self, qu, qi):
        return estimate_batch(self.cltr_u, self.cltr_i, self._avgs(), self.user_mean, self.item_mean, self.trainset.global_mean,
                              qu, qi, check=False)

    def estimate(self, u, i):
        """The estimate for inner ids u, i, anything else being an unknown id: the user's mean, the item's mean or the
        training mean where one or both are unknown.  Never raises PredictionImpossible, as surprise's never does."""
        ts = self.trainset
        est, _ = self._estimate_batch(*self._queries([u if ts.knows_user(u) else -1], [i if ts.knows_item(i) else -1]))
        return float(est.item())

    def _top_n(self, owners, n, segments):
        ts = self.trainset
        return top_n(self.cltr_u, self.cltr_i, self._avgs(), self.user_mean, self.item_mean, self._seen(), ts.global_mean,
                     ts.rating_scale, n, owners, segments, check=False)
