"""Restatement of surprise 1.0.6's NMF with biased=False (Luo et al. 2014, the multiplicative update), for the tests of
csrc/n2v_nmf.hip.  It is the definition the kernels equal bit for bit.

Parity is UNPINNED: `surprise` is not installed, the update is restated from memory, and nothing here was ever run
against surprise itself.

The model: est = qi[i] . pu[u], the dot in lane order (svd_reference.lane_dot / dot_lanes, lane_dot of the kernels).
Everything fp64, no fused multiply-add, every multiply and add rounded on its own.  One epoch reads pu and qi as they
were at its start.  For every user u, over its ratings (i, r) in Trainset.ur order (training order), num = den = +0.0:
    est = dot(qi[i], pu[u]);  num[f] = num[f] + qi[i, f] * r;  den[f] = den[f] + qi[i, f] * est
and after the list
    den[f] = den[f] + (n_ratings(u) * reg_pu) * pu[u, f];  pu'[u, f] = pu[u, f] * (num[f] / den[f])
For every item i the same with the roles swapped (pu[u, f] * r, pu[u, f] * est, reg_qi, qi'), over its ratings in
all_ratings() order: ascending inner user id.  That is NOT Trainset.ir, which is in training order.  Both passes use the
OLD tables.  No special case: a zero denominator gives 0/0 = NaN or x/0 = inf, and they propagate.

Two forms of one epoch: epoch_literal (Python floats: one global pass over all_ratings() with dense num / den tables,
then the finish, as surprise's loop runs) and epoch (one numpy row operation per rating and row).
"""
import numpy as np

import svd_reference as SV

DEFAULTS = dict(n_factors=15, n_epochs=50, biased=False, reg_pu=0.06, reg_qi=0.06, init_low=0, init_high=1, random_state=0)


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise ValueError("unknown option " + ", ".join(sorted(unknown)))
    p = dict(DEFAULTS, **kw)
    if p["biased"]:
        raise ValueError("biased=True is not restated")
    return p


def init(n_users, n_items, par):
    rng = np.random.RandomState(par["random_state"])
    pu = rng.uniform(par["init_low"], par["init_high"], (n_users, par["n_factors"]))
    qi = rng.uniform(par["init_low"], par["init_high"], (n_items, par["n_factors"]))
    return pu, qi


# ---- the lists --------------------------------------------------------------------------------------------------------

def csr(major, minor, r, n_major, order):
    """(ptr, minor, r) with the entries taken in `order` (positions into the training order) and grouped by major id,
    stably."""
    major, minor, r = np.asarray(major, np.int64)[order], np.asarray(minor, np.int64)[order], np.asarray(r, np.float64)[order]
    o = np.argsort(major, kind="stable")
    ptr = np.zeros(n_major + 1, np.int64)
    np.cumsum(np.bincount(major, minlength=n_major), out=ptr[1:])
    return ptr, minor[o].astype(np.int32), r[o]


def user_lists(u, i, r, n_users):
    """Trainset.ur: every user's (item, r) in training order."""
    return csr(u, i, r, n_users, np.arange(len(r)))


def item_lists(u, i, r, n_items):
    """Every item's (user, r) in all_ratings() order: ascending inner user id (then training order, which never decides:
    a (user, item) pair occurs once)."""
    return csr(i, u, r, n_items, SV.all_ratings_order(u))


def item_lists_ir(u, i, r, n_items):
    """Trainset.ir: every item's (user, r) in training order.  NOT what NMF sums over; here for the tests that show it."""
    return csr(i, u, r, n_items, np.arange(len(r)))


# ---- one epoch --------------------------------------------------------------------------------------------------------

def half_pass(lst, own, oth, reg, dot_fn=SV.dot_lanes):
    """The new `own` table from one row-major list (ptr, other ids, r): row k of own over its list, rows of oth."""
    ptr, ids, r = lst
    out = np.empty_like(own)
    nf = own.shape[1]
    with np.errstate(all="ignore"):
        for k in range(len(ptr) - 1):
            p = own[k]
            num, den = np.zeros(nf), np.zeros(nf)
            for e in range(ptr[k], ptr[k + 1]):
                q = oth[ids[e]]
                est = dot_fn(q, p)
                num = num + q * r[e]
                den = den + q * est
            den = den + (int(ptr[k + 1] - ptr[k]) * reg) * p
            out[k] = p * (num / den)
    return out


def epoch(ul, il, pu, qi, par, dot_fn=SV.dot_lanes):
    """(pu', qi') from the user-major and item-major lists; both passes read the old tables."""
    return half_pass(ul, pu, qi, par["reg_pu"], dot_fn), half_pass(il, qi, pu, par["reg_qi"], dot_fn)


def fit(u, i, r, n_users, n_items, par, n_epochs=None, tables=None):
    """(pu, qi) after par["n_epochs"] (or n_epochs) epochs from init() (or from `tables`)."""
    ul, il = user_lists(u, i, r, n_users), item_lists(u, i, r, n_items)
    pu, qi = init(n_users, n_items, par) if tables is None else (np.array(tables[0], np.float64), np.array(tables[1], np.float64))
    for _ in range(par["n_epochs"] if n_epochs is None else n_epochs):
        pu, qi = epoch(ul, il, pu, qi, par)
    return pu, qi


def _div(a, b):
    """Python raises on a zero divisor; the arithmetic does not."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def epoch_literal(u, i, r, n_users, n_items, pu, qi, par):
    """surprise's loop on Python floats: one pass over all_ratings() into dense user_num / user_denom / item_num /
    item_denom, then the two finishing loops.  u, i, r in training order."""
    nf = par["n_factors"]
    o = SV.all_ratings_order(u)
    u, i, r = np.asarray(u)[o].tolist(), np.asarray(i)[o].tolist(), np.asarray(r, np.float64)[o].tolist()
    pu, qi = np.asarray(pu).tolist(), np.asarray(qi).tolist()
    unum = [[0.0] * nf for _ in range(n_users)]; uden = [[0.0] * nf for _ in range(n_users)]
    inum = [[0.0] * nf for _ in range(n_items)]; iden = [[0.0] * nf for _ in range(n_items)]
    for uu, ii, rr in zip(u, i, r):
        est = SV._dot_lanes_literal(qi[ii], pu[uu])
        for f in range(nf):
            unum[uu][f] = unum[uu][f] + qi[ii][f] * rr
            uden[uu][f] = uden[uu][f] + qi[ii][f] * est
            inum[ii][f] = inum[ii][f] + pu[uu][f] * rr
            iden[ii][f] = iden[ii][f] + pu[uu][f] * est
    new_pu = [[0.0] * nf for _ in range(n_users)]; new_qi = [[0.0] * nf for _ in range(n_items)]
    for uu in range(n_users):
        n = u.count(uu)
        for f in range(nf):
            uden[uu][f] = uden[uu][f] + (n * par["reg_pu"]) * pu[uu][f]
            new_pu[uu][f] = pu[uu][f] * _div(unum[uu][f], uden[uu][f])
    for ii in range(n_items):
        n = i.count(ii)
        for f in range(nf):
            iden[ii][f] = iden[ii][f] + (n * par["reg_qi"]) * qi[ii][f]
            new_qi[ii][f] = qi[ii][f] * _div(inum[ii][f], iden[ii][f])
    return np.array(new_pu).reshape(n_users, nf), np.array(new_qi).reshape(n_items, nf)


# ---- estimate ---------------------------------------------------------------------------------------------------------

def model(pu, qi):
    """The tables in the shape svd_reference.estimate and topn_reference.svd_predictor take: (mu, bu, bi, pu, qi)."""
    return 0.0, np.zeros(len(pu)), np.zeros(len(qi)), pu, qi


def estimate(pu, qi, qu, qi_ids):
    """SVD's unbiased estimate: (est, impossible), -1 = unknown; 'User and item are unknown.' unless both are known."""
    return SV.estimate(model(pu, qi), qu, qi_ids, False)


# ---- seeded cases -----------------------------------------------------------------------------------------------------

def make_ratings(seed, n_users, n_items, n, rank=3, noise=0.3):
    """n distinct (u, i) cells of a rank-`rank` non-negative model plus noise, rounded to 1 .. 5, in a shuffled training
    order; ids are NOT renumbered by first appearance."""
    rs = np.random.RandomState(seed)
    a, b = rs.uniform(0.3, 1.3, (n_users, rank)), rs.uniform(0.3, 1.3, (n_items, rank))
    cells = rs.permutation(n_users * n_items)[:n]
    u, i = cells // n_items, cells % n_items
    r = np.clip(np.rint(1.5 * (a[u] * b[i]).sum(1) + noise * rs.normal(size=n)), 1.0, 5.0)
    return u.astype(np.int64), i.astype(np.int64), r
