"""Matrix-factorisation rating prediction trained on the device (csrc/n2v_svd.hip, C-ABI include/n2v_sim.h).

Reference: the third algorithm of src/main_rec.py:341-348, `-algo svd`: surprise 1.0.6's SVD, biases plus n_factors
latent factors per user and item, plain SGD.  Parity is UNPINNED: `surprise` is not a dependency here, the model and
the update are restated from memory (tests/svd_reference.py, which is the definition) and the kernels are held to that
restatement bit for bit.

surprise applies the ratings one after the other.  Here an epoch follows a deterministic stratified schedule (DSGD,
Gemulla et al., KDD 2011): with P = n_strata, user u is in block (u * P) // n_users and item i in block
(i * P) // n_items, a rating is in stratum (ib - ub) mod P, and the P blocks of a stratum share no user and no item.
The device runs a stratum's blocks concurrently, one wavefront each, and the strata one launch after the other, which
gives exactly the result of the sequential loop `for s: for ub: block (s, ub)` with surprise's all_ratings() order
inside a block.  n_strata = 1 is surprise's own order; any other P is another fixed permutation of the ratings.

The factors are drawn on the host (numpy's RandomState, as surprise draws them) and uploaded.  Everything is fp64.
There is no CPU fallback.
"""
import math

import numpy as np
import torch

from . import _lib
from .eccknn import (PredictionImpossible, Predictor, _queries_ptrs, _query_count, _require_gpu, _to_device, _topn_call,
                     topn_options)

MAX_FACTORS = 256                # n2v_svd_max_factors()
MAX_STRATA = 32768               # n2v_svd_max_strata()
AUTO_MAX_STRATA = 256            # see auto_strata
AUTO_RATINGS_PER_BLOCK = 8
BLOCKS_BAD = ((1, "blk_ptr does not start at 0, is not monotone or leaves [0, n]"), (2, "blk_ptr does not end at n"),
              (4, "a user or item id out of range"), (8, "a rating outside the block its ids put it in"),
              (16, "a block is not ascending in u"))
_RATES = ("lr_bu", "lr_bi", "lr_pu", "lr_qi", "reg_bu", "reg_bi", "reg_pu", "reg_qi")


def auto_strata(n_users, n_items, n_ratings):
    """The n_strata="auto" rule; host arithmetic only.  The parallel width of a launch is P and an epoch is P launches
    over P * P blocks, so P grows until a block would hold fewer than AUTO_RATINGS_PER_BLOCK ratings on average: the
    largest power of two with P * P * 8 <= n_ratings, at most AUTO_MAX_STRATA, and never more than the shorter side
    (beyond it blocks are empty by construction)."""
    n_users, n_items, n_ratings = int(n_users), int(n_items), int(n_ratings)
    if n_users < 1 or n_items < 1 or n_ratings < 1:
        raise ValueError("auto_strata: %d users, %d items, %d ratings" % (n_users, n_items, n_ratings))
    p = 1
    while 2 * p <= AUTO_MAX_STRATA and (2 * p) * (2 * p) * AUTO_RATINGS_PER_BLOCK <= n_ratings:
        p *= 2
    return max(1, min(p, n_users, n_items))


def check_strata(n_strata):
    """n_strata as given to SVD: "auto" or an integer in [1, MAX_STRATA]."""
    if n_strata == "auto":
        return n_strata
    if isinstance(n_strata, bool) or not isinstance(n_strata, (int, np.integer)):
        raise ValueError("n_strata %r: an integer >= 1 or \"auto\"" % (n_strata,))
    if not 1 <= n_strata <= MAX_STRATA:
        raise ValueError("n_strata %d outside [1, %d]" % (n_strata, MAX_STRATA))
    return int(n_strata)


# ---- C-ABI wrappers (device tensors in, device tensors out) -----------------------------------------------------------

def build_blocks(u, i, r, n_users, n_items, n_strata):
    """Device triples (u, i integer, r fp64) in all_ratings() order -> the device block lists (blk_ptr int64[P * P + 1],
    blk_u int32, blk_i int32, blk_r fp64): a stable sort on the key s * P + ub."""
    _require_gpu()
    P = int(n_strata)
    u64, i64 = u.to(torch.int64), i.to(torch.int64)
    ub, ib = (u64 * P) // int(n_users), (i64 * P) // int(n_items)
    key = torch.remainder(ib - ub, P) * P + ub
    _, order = torch.sort(key, stable=True)
    ptr = torch.zeros(P * P + 1, dtype=torch.int64, device=u.device)
    ptr[1:] = torch.cumsum(torch.bincount(key, minlength=P * P), 0)
    return (ptr, u64[order].to(torch.int32).contiguous(), i64[order].to(torch.int32).contiguous(),
            r[order].to(torch.float64).contiguous())


class Blocks:
    """Block lists that passed n2v_svd_blocks_check: the only thing epoch() accepts.  A malformed list is a ValueError
    that names the cause (one read-back of an int32) and never reaches the training kernel."""

    def __init__(self, lists, n_users, n_items, n_strata):
        _require_gpu()
        if not isinstance(lists, (tuple, list)) or len(lists) != 4:
            raise ValueError("svd: block lists must be (int64 blk_ptr, int32 blk_u, int32 blk_i, fp64 blk_r)")
        ptr_, bu_, bi_, br_ = lists
        dev = _lib.call_device("svd.Blocks", "lists[3] (float64 blk_r)", br_)
        p_ptr, p_u, p_i, _ = [_lib.tensor("svd.Blocks", "lists[%d] (%s blk_%s)" % (j, str(dt).replace("torch.", ""), role), t, dt,
                                          dev, (None,))
                              for j, (role, t, dt) in enumerate((("ptr", ptr_, torch.int64), ("u", bu_, torch.int32),
                                                                 ("i", bi_, torch.int32), ("r", br_, torch.float64)))]
        P, n = int(n_strata), bu_.numel()
        if not 1 <= P <= MAX_STRATA:
            raise ValueError("n_strata %d outside [1, %d]" % (P, MAX_STRATA))
        if n < 1 or bi_.numel() != n or br_.numel() != n or ptr_.numel() != P * P + 1:
            raise ValueError("svd: %d blk_ptr entries for n_strata = %d, %d u, %d i, %d r"
                             % (ptr_.numel(), P, n, bi_.numel(), br_.numel()))
        lib = _lib.load()
        with torch.cuda.device(dev):
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(lib.n2v_svd_blocks_check(p_ptr, p_u, p_i, P, int(n_users), int(n_items), n,
                                                _lib.ptr(status), _lib.stream_ptr(dev)))
            bits = int(status.item())
        if bits:
            raise ValueError("svd: malformed block lists: " + "; ".join(msg for b, msg in BLOCKS_BAD if bits & b))
        self.ptr, self.u, self.i, self.r = ptr_, bu_, bi_, br_
        self.n_users, self.n_items, self.n_strata, self.n = int(n_users), int(n_items), P, n


def _model_ptrs(fn, biased, bu, bi, pu, qi, n_users=None, n_items=None):
    """([bu, bi, pu, qi] pointers, n_users, n_items, n_factors, device) of a factor model: fp64 pu[n_users][n_factors] on
    a GPU, which is the device of the call, qi[n_items][n_factors], bu[n_users] and bi[n_items]; the biases may be None
    when not biased.  n_users, n_items None: the rows of pu and qi."""
    dev = _lib.call_device(fn, "pu", pu)
    p_pu = _lib.tensor(fn, "pu", pu, torch.float64, dev, (n_users, None))
    n_users, n_factors = pu.shape
    p_qi = _lib.tensor(fn, "qi", qi, torch.float64, dev, (n_items, n_factors))
    n_items = qi.shape[0]
    p_bu = _lib.tensor(fn, "bu", bu, torch.float64, dev, n_users, optional=not biased)
    p_bi = _lib.tensor(fn, "bi", bi, torch.float64, dev, n_items, optional=not biased)
    return [p_bu, p_bi, p_pu, p_qi], n_users, n_items, n_factors, dev


def epoch(blocks, mu, biased, rates, bu, bi, pu, qi):
    """One epoch in place (n2v_svd_epoch).  rates: the eight values lr_bu, lr_bi, lr_pu, lr_qi, reg_bu, reg_bi, reg_pu,
    reg_qi.  bu / bi may be None when not biased."""
    _require_gpu()
    if not isinstance(blocks, Blocks):
        raise TypeError("svd.epoch: blocks must be a checked svd.Blocks")
    tables, _, _, n_factors, dev = _model_ptrs("svd.epoch", biased, bu, bi, pu, qi, blocks.n_users, blocks.n_items)
    if blocks.r.device != dev:
        raise ValueError("svd.epoch: blocks are on %s, pu on %s" % (blocks.r.device, dev))
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.n2v_svd_epoch(_lib.ptr(blocks.ptr), _lib.ptr(blocks.u), _lib.ptr(blocks.i), _lib.ptr(blocks.r),
                                     blocks.n_strata, blocks.n_users, blocks.n_items, blocks.n, int(n_factors), float(mu),
                                     1 if biased else 0, *[float(v) for v in rates], *tables, _lib.stream_ptr(dev)))


def estimate_batch(mu, biased, bu, bi, pu, qi, qu, qi_ids):
    """(est fp64, impossible uint8) device tensors for int32 device queries, -1 = unknown (n2v_svd_estimate)."""
    _require_gpu()
    tables, n_users, n_items, n_factors, dev = _model_ptrs("svd.estimate_batch", biased, bu, bi, pu, qi)
    p_qu, p_qi = _queries_ptrs("svd.estimate_batch", qu, qi_ids, dev, ("qu", "qi_ids"))
    n_q = _query_count(qu, qi_ids, ("user", "item"), ("qu", "qi_ids"))
    lib = _lib.load()
    with torch.cuda.device(dev):
        est = torch.empty(n_q, dtype=torch.float64, device=dev)
        imp = torch.empty(n_q, dtype=torch.uint8, device=dev)
        _lib.check(lib.n2v_svd_estimate(*tables, n_users, n_items,
                                        n_factors, float(mu), 1 if biased else 0, p_qu, p_qi, n_q,
                                        _lib.ptr(est), _lib.ptr(imp), _lib.stream_ptr(dev)))
    return est, imp


def top_n(mu, biased, bu, bi, pu, qi, seen, global_mean, rating_scale, n, owners=None, segments=None):
    """eccknn.top_n for the factor tables (n2v_svd_topn): per owner the n unseen inner items with the best predictions,
    each the bits of estimate_batch + eccknn.predict for that pair.  global_mean is predict's fallback (the training mean),
    mu the model's (0.0 when not biased)."""
    n, segments = topn_options(n, segments)
    _require_gpu()
    tables, n_users, n_items, n_factors, dev = _model_ptrs("svd.top_n", biased, bu, bi, pu, qi)
    head = tables + [n_users, n_items, n_factors, float(mu), 1 if biased else 0]
    return _topn_call(_lib.load().n2v_svd_topn, head, [], [], seen, n_users, n_items, owners, global_mean, rating_scale, n, segments,
                      dev)


# ---- the algorithm ----------------------------------------------------------------------------------------------------

class SVD(Predictor):
    """surprise's SVD with its options and defaults, plus n_strata (an integer, or "auto": auto_strata) and device.
    fit(trainset) takes an eccknn.Trainset; afterwards bu, bi, pu, qi are device fp64 tensors."""
    _MODEL = "pu"

    def __init__(self, n_factors=100, n_epochs=20, biased=True, init_mean=0, init_std_dev=0.1, lr_all=0.005, reg_all=0.02,
                 lr_bu=None, lr_bi=None, lr_pu=None, lr_qi=None, reg_bu=None, reg_bi=None, reg_pu=None, reg_qi=None,
                 random_state=0, n_strata="auto", device="cuda:0"):
        self.n_factors, self.n_epochs, self.biased = int(n_factors), int(n_epochs), bool(biased)
        if not 1 <= self.n_factors <= MAX_FACTORS:
            raise ValueError("n_factors %d outside [1, %d]" % (self.n_factors, MAX_FACTORS))
        if self.n_epochs < 0:
            raise ValueError("n_epochs %d < 0" % self.n_epochs)
        given = dict(lr_bu=lr_bu, lr_bi=lr_bi, lr_pu=lr_pu, lr_qi=lr_qi, reg_bu=reg_bu, reg_bi=reg_bi, reg_pu=reg_pu,
                     reg_qi=reg_qi)
        alls = {"lr": lr_all, "reg": reg_all}
        self.rates = []
        for name in _RATES:
            v = float(alls[name[:name.index("_")]] if given[name] is None else given[name])
            if not math.isfinite(v):
                raise ValueError("%s %r is not finite" % (name, v))
            self.rates.append(v)
            setattr(self, name, v)
        self.init_mean, self.init_std_dev = float(init_mean), float(init_std_dev)
        if not (math.isfinite(self.init_mean) and math.isfinite(self.init_std_dev)) or self.init_std_dev < 0:
            raise ValueError("init_mean %r, init_std_dev %r" % (init_mean, init_std_dev))
        self.random_state = random_state
        self.n_strata = check_strata(n_strata)
        self.device = device

    def fit(self, trainset):
        _require_gpu()
        dev = torch.device(self.device)
        ts = self.trainset = trainset
        P = auto_strata(ts.n_users, ts.n_items, ts.n_ratings) if self.n_strata == "auto" else self.n_strata
        self.n_strata_used = P
        self.mu = float(ts.global_mean) if self.biased else 0.0
        # all_ratings(): the users ascending, each one's ratings in training order; that is the ur lists, concatenated
        u = np.repeat(np.arange(ts.n_users, dtype=np.int64), np.diff(ts.ur[0]))
        rng = np.random.RandomState(self.random_state)
        pu = rng.normal(self.init_mean, self.init_std_dev, (ts.n_users, self.n_factors))
        qi = rng.normal(self.init_mean, self.init_std_dev, (ts.n_items, self.n_factors))
        with torch.cuda.device(dev):
            lists = build_blocks(_to_device(u, torch.int64, dev), _to_device(ts.ur[1], torch.int64, dev),
                                 _to_device(ts.ur[2], torch.float64, dev), ts.n_users, ts.n_items, P)
            self.blocks = Blocks(lists, ts.n_users, ts.n_items, P)
            self.bu = torch.zeros(ts.n_users, dtype=torch.float64, device=dev)
            self.bi = torch.zeros(ts.n_items, dtype=torch.float64, device=dev)
            self.pu, self.qi = _to_device(pu, torch.float64, dev), _to_device(qi, torch.float64, dev)
            for _ in range(self.n_epochs):
                epoch(self.blocks, self.mu, self.biased, self.rates, self.bu, self.bi, self.pu, self.qi)
        return self

    def _estimate_batch(self, qu, qi_ids):
        return estimate_batch(self.mu, self.biased, self.bu, self.bi, self.pu, self.qi, qu, qi_ids)

    def estimate(self, u, i):
        """est for inner ids u, i (anything else is unknown); PredictionImpossible as surprise raises it."""
        ts = self.trainset
        qu, qi_ids = self._queries([u if ts.knows_user(u) else -1], [i if ts.knows_item(i) else -1])
        est, imp = self._estimate_batch(qu, qi_ids)
        if int(imp.item()):
            raise PredictionImpossible("User and item are unknown.")
        return float(est.item())

    def _top_n(self, owners, n, segments):
        ts = self.trainset
        return top_n(self.mu, self.biased, self.bu, self.bi, self.pu, self.qi, self._seen(), ts.global_mean, ts.rating_scale,
                     n, owners, segments)
