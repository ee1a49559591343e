"""Non-negative matrix factorisation trained on the device (csrc/n2v_nmf.hip, C-ABI include/n2v_sim.h).

surprise 1.0.6's NMF with biased=False (Luo et al. 2014): factor tables pu and qi that stay non-negative under a
multiplicative update, est = qi[i] . pu[u].  Parity is UNPINNED: `surprise` is not a dependency here, the update is
restated from memory (tests/nmf_reference.py, which is the definition) and the kernels are held to that restatement bit
for bit.

The update freezes both tables for an epoch: every row's new value is a sum over its own ratings, in a fixed order, of
terms that read the old tables only.  So, unlike svd.SVD, this model trains in surprise's own order with every row in
parallel, one wavefront each, and needs no schedule: a user's ratings in training order (Trainset.ur), an item's by
ascending inner user id (all_ratings() order, NOT Trainset.ir, which is in training order).  The item-major list is one
stable sort of the user-major entries by item, on the device.

The prediction is SVD's with biased=False, so estimate, test, rmse and the top-N lists are svd.SVD's own paths and
kernels.  biased=True is refused: surprise's bias updates there are sequential SGD across rows.  The factors are drawn
on the host (numpy's RandomState, as surprise draws them) and uploaded.  Everything is fp64.  There is no CPU fallback.
"""
import math

import numpy as np
import torch

from . import _lib
from .eccknn import PredictionImpossible  # noqa: F401  (what estimate raises)
from .eccknn import _csr_ptrs, _csr_to_device, _require_gpu, _to_device
from .svd import MAX_FACTORS, SVD

LISTS_BAD = ((1, "a ptr does not start at 0, is not monotone or leaves [0, n]"), (2, "a ptr does not end at n"),
             (4, "a user or item id out of range"), (8, "an item row is not strictly ascending in u"),
             (16, "the two lists do not hold the same ratings: an id's count in one differs from its row length in the other"))


# ---- C-ABI wrappers (device tensors in, device tensors out) -----------------------------------------------------------

def _check_triple(what, triple):
    """What the host can see of a list: a tuple of three GPU tensors of the types above, ids and r of one length.
    Returns n."""
    if not isinstance(triple, (tuple, list)) or len(triple) != 3:
        raise ValueError("nmf: the %s list must be (int64 ptr, int32 ids, fp64 r)" % what)
    return _csr_ptrs("nmf", {"user-major": "ur", "item-major": "ir"}[what], triple)[1]


def item_major(ur, n_items):
    """The device user-major triple (ptr int64[n_users + 1], item int32[n], r fp64[n]) -> the item-major triple (ptr
    int64[n_items + 1], user int32[n], r fp64[n]): one stable sort by item, so every item's raters ascend in u.
    Whatever ptr and the ids hold, every index formed here is in range: an entry's user is found by a search of ptr and
    an item id is clamped into [0, n_items); the check of the pair of lists (Lists) then names what was wrong."""
    _require_gpu()
    n = _check_triple("user-major", ur)
    ptr_, ids, r = ur
    n_users, n_items = ptr_.numel() - 1, int(n_items)
    if n_items < 1:
        raise ValueError("nmf: %d items" % n_items)
    pos = torch.arange(n, dtype=torch.int64, device=ids.device)
    u = torch.searchsorted(ptr_[1:].contiguous(), pos, right=True).clamp_(max=n_users - 1).to(torch.int32)
    key = ids.to(torch.int64).clamp_(0, n_items - 1)
    _, order = torch.sort(key, stable=True)
    iptr = torch.zeros(n_items + 1, dtype=torch.int64, device=ids.device)
    iptr[1:] = torch.cumsum(torch.bincount(key, minlength=n_items), 0)
    return iptr, u[order].contiguous(), r[order].contiguous()


def row_order(ptr_):
    """int32 rows by descending list length (equal lengths by ascending row): the longest lists start first."""
    _, order = torch.sort(ptr_[1:] - ptr_[:-1], descending=True, stable=True)
    return order.to(torch.int32).contiguous()


class Lists:
    """A user-major and an item-major list that passed n2v_nmf_lists_check, with their row order tables: the only thing
    epoch() accepts.  A malformed pair is a ValueError that names the cause (one read-back of an int32) and never
    reaches the pass kernel."""

    def __init__(self, ur, ir, n_users, n_items, order):
        n_users, n_items, n = int(n_users), int(n_items), _check_triple("user-major", ur)
        if _check_triple("item-major", ir) != n:
            raise ValueError("nmf: mismatched n: the user-major list holds %d ratings, the item-major list %d" % (n, ir[1].numel()))
        if n < 1 or n_users < 1 or n_items < 1 or ur[0].numel() != n_users + 1 or ir[0].numel() != n_items + 1:
            raise ValueError("nmf: %d ratings, %d user ptr entries for %d users, %d item ptr entries for %d items"
                             % (n, ur[0].numel(), n_users, ir[0].numel(), n_items))
        p_ur, _, dev = _csr_ptrs("nmf.Lists", "ur", ur)
        p_ir, _, _ = _csr_ptrs("nmf.Lists", "ir", ir, dev)
        if not isinstance(order, str):
            if not isinstance(order, (tuple, list)) or len(order) != 2:
                raise ValueError("nmf: order tables must be int32[n_users] and int32[n_items]")
            for j, k in enumerate((n_users, n_items)):
                _lib.tensor("nmf.Lists", "order[%d]" % j, order[j], torch.int32, dev, k, optional=True)
        lib = _lib.load()
        with torch.cuda.device(dev):
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            scratch = torch.empty(n_users + n_items, dtype=torch.int32, device=dev)
            _lib.check(lib.n2v_nmf_lists_check(p_ur[0], p_ur[1], p_ir[0], p_ir[1], n_users,
                                               n_items, n, _lib.ptr(scratch), _lib.ptr(status), _lib.stream_ptr(dev)))
            bits = int(status.item())
            if bits:
                raise ValueError("nmf: malformed lists: " + "; ".join(msg for b, msg in LISTS_BAD if bits & b))
            if order == "descending":
                order = (row_order(ur[0]), row_order(ir[0]))
            elif order == "identity":
                order = (None, None)
        self.ur, self.ir, self.order = tuple(ur), tuple(ir), tuple(order)
        self.n_users, self.n_items, self.n = n_users, n_items, n


def lists(ur, n_users, n_items, ir=None, order="descending"):
    """Checked Lists of the device user-major triple ur; the item-major triple is item_major(ur) unless ir is given.
    order: "descending" (row_order of both sides), "identity", or a pair of int32 device permutations (None: identity)."""
    _require_gpu()
    if ir is None:
        if _check_triple("user-major", ur) < 1 or ur[0].numel() != int(n_users) + 1:
            raise ValueError("nmf: %d ratings, %d user ptr entries for %d users" % (ur[1].numel(), ur[0].numel(), int(n_users)))
        ir = item_major(ur, n_items)
    return Lists(ur, ir, n_users, n_items, order)


def _overlaps(a, b):
    return a.data_ptr() < b.data_ptr() + b.numel() * 8 and b.data_ptr() < a.data_ptr() + a.numel() * 8


def epoch(lists_, reg_pu, reg_qi, pu, qi, pu_out, qi_out):
    """One epoch (n2v_nmf_epoch): reads pu and qi, writes pu_out and qi_out, which must not overlap them or each other.
    The caller swaps the pairs between epochs."""
    _require_gpu()
    if not isinstance(lists_, Lists):
        raise TypeError("nmf.epoch: lists must be a checked nmf.Lists")
    dev = _lib.call_device("nmf.epoch", "pu", pu)
    if lists_.ur[2].device != dev:
        raise ValueError("nmf.epoch: lists are on %s, pu on %s" % (lists_.ur[2].device, dev))
    tables = [_lib.tensor("nmf.epoch", "pu", pu, torch.float64, dev, (lists_.n_users, None))]
    n_factors = pu.shape[1]
    tables += [_lib.tensor("nmf.epoch", name, t, torch.float64, dev, (rows, n_factors))
               for name, t, rows in (("qi", qi, lists_.n_items), ("pu_out", pu_out, lists_.n_users), ("qi_out", qi_out, lists_.n_items))]
    if any(_overlaps(o, t) for o in (pu_out, qi_out) for t in (pu, qi)) or _overlaps(pu_out, qi_out):
        raise ValueError("nmf.epoch: aliased tables: an output table overlaps an input table or the other output")
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.n2v_nmf_epoch(*[_lib.ptr(t) for t in lists_.ur + lists_.ir + lists_.order], lists_.n_users,
                                     lists_.n_items, lists_.n, int(n_factors), float(reg_pu), float(reg_qi), *tables,
                                     _lib.stream_ptr(dev)))


# ---- the algorithm ----------------------------------------------------------------------------------------------------

class NMF(SVD):
    """surprise's NMF with its options and defaults, plus device.  fit(trainset) takes an eccknn.Trainset; afterwards
    pu and qi are device fp64 tensors, and everything after fit is svd.SVD's with biased=False, mu = 0."""

    def __init__(self, n_factors=15, n_epochs=50, biased=False, reg_pu=0.06, reg_qi=0.06, init_low=0, init_high=1,
                 random_state=0, device="cuda:0"):
        if biased:
            raise ValueError("biased=True is not built: surprise's bias updates of NMF are sequential SGD across rows "
                             "(the reason bsl_options method \"sgd\" is refused)")
        self.n_factors, self.n_epochs, self.biased = int(n_factors), int(n_epochs), False
        if not 1 <= self.n_factors <= MAX_FACTORS:
            raise ValueError("n_factors %d outside [1, %d]" % (self.n_factors, MAX_FACTORS))
        if self.n_epochs < 0:
            raise ValueError("n_epochs %d < 0" % self.n_epochs)
        self.reg_pu, self.reg_qi = float(reg_pu), float(reg_qi)
        for name in ("reg_pu", "reg_qi"):
            if not math.isfinite(getattr(self, name)):
                raise ValueError("%s %r is not finite" % (name, getattr(self, name)))
        self.init_low, self.init_high = float(init_low), float(init_high)
        if not (math.isfinite(self.init_low) and math.isfinite(self.init_high)) or self.init_low > self.init_high:
            raise ValueError("init_low %r, init_high %r" % (init_low, init_high))
        self.random_state = random_state
        self.device = device
        self.mu, self.bu, self.bi = 0.0, None, None

    def fit(self, trainset):
        _require_gpu()
        dev = torch.device(self.device)
        ts = self.trainset = trainset
        rng = np.random.RandomState(self.random_state)
        pu = rng.uniform(self.init_low, self.init_high, (ts.n_users, self.n_factors))
        qi = rng.uniform(self.init_low, self.init_high, (ts.n_items, self.n_factors))
        with torch.cuda.device(dev):
            self.lists = lists(_csr_to_device(ts.ur, dev), ts.n_users, ts.n_items)
            self.pu, self.qi = _to_device(pu, torch.float64, dev), _to_device(qi, torch.float64, dev)
            pu_out, qi_out = torch.empty_like(self.pu), torch.empty_like(self.qi)
            for _ in range(self.n_epochs):
                epoch(self.lists, self.reg_pu, self.reg_qi, self.pu, self.qi, pu_out, qi_out)
                self.pu, pu_out = pu_out, self.pu
                self.qi, qi_out = qi_out, self.qi
        return self
