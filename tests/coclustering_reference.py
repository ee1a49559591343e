"""Restatement of surprise 1.0.6's CoClustering (George and Merugu 2005), for the tests of csrc/n2v_cocl.hip.  It is the
definition the kernels equal bit for bit.

Parity is UNPINNED: `surprise` is not installed, the algorithm is restated from memory, and nothing here was ever run
against surprise itself.

Everything fp64, no fused multiply-add, every expression as written, left to right.  Users and items each belong to one
cluster; cltr_u and cltr_i start as RandomState(random_state).randint draws, users first.  user_mean / item_mean are each
row's sum in list order over its length (mean_rows: the documented deviation from numpy's pairwise mean).

averages(): int64 counts and fp64 sums per user cluster, item cluster and co-cluster; an empty one's average is the
training mean, any other sum / count.  DEVIATION from surprise, deliberate: surprise adds every sum as one chain over
all_ratings() (sums_literal, below, for the tests that show the difference); here the sums are grouped by user row.
For user u over ur[u] in list order from +0.0:  t_u = t_u + r,  s_u[ic] = s_u[ic] + r  with ic = cltr_i[i];  then over
the users in ascending inner id:  sum_cltr_u[cltr_u[u]] += t_u,  and for EVERY ic (an s_u[ic] nobody added to is +0.0)
sum_cltr_i[ic] += s_u[ic],  sum_cocltr[cltr_u[u]][ic] += s_u[ic].  On ratings whose sums are exact (multiples of 1/2)
the two orders give the same bytes.

One epoch: the averages of the current assignment; then every user takes the cluster uc with the least
    errors[uc] = sum over ur[u] in list order, from +0.0, of d * d,   d = r - est,
    est = (((avg_cocltr[uc][ic] + user_mean[u]) - avg_cltr_u[uc]) + item_mean[i]) - avg_cltr_i[ic],   ic = cltr_i[i]
then every item the same over ir[i] (training order) with uc = cltr_u[u] as the user step has just left it and the
SAME averages.  The least is numpy's argmin: the first NaN if there is one, else the first minimum; an empty list
leaves cluster 0.  After the last epoch the averages are computed once more.

estimate: the expression above with the fitted clusters when both ids are known, user_mean[u] when only the user is,
item_mean[i] when only the item is, the training mean when neither is.  Never impossible.
"""
import numpy as np

DEFAULTS = dict(n_cltr_u=3, n_cltr_i=3, n_epochs=20, random_state=0)
MAX_CLUSTERS = 64


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise ValueError("unknown option " + ", ".join(sorted(unknown)))
    return dict(DEFAULTS, **kw)


def init(n_users, n_items, par):
    rng = np.random.RandomState(par["random_state"])
    cltr_u = rng.randint(par["n_cltr_u"], size=n_users)
    cltr_i = rng.randint(par["n_cltr_i"], size=n_items)
    return cltr_u.astype(np.int64), cltr_i.astype(np.int64)


# ---- the lists --------------------------------------------------------------------------------------------------------

def lists(major, minor, r, n_major):
    """(ptr, minor, r): every major id's entries in training order (Trainset.ur / Trainset.ir)."""
    major, minor, r = np.asarray(major, np.int64), np.asarray(minor, np.int64), np.asarray(r, np.float64)
    o = np.argsort(major, kind="stable")
    ptr = np.zeros(n_major + 1, np.int64)
    np.cumsum(np.bincount(major, minlength=n_major), out=ptr[1:])
    return ptr, minor[o].astype(np.int32), r[o]


def mean_rows(lst):
    """Each row's sum in list order over its length; an empty row is NaN (eccknn.row_moments)."""
    ptr, _, r = lst
    out = np.full(len(ptr) - 1, np.nan)
    for k in range(len(ptr) - 1):
        if ptr[k + 1] > ptr[k]:
            out[k] = np.cumsum(r[ptr[k]:ptr[k + 1]])[-1] / float(ptr[k + 1] - ptr[k])
    return out


def global_mean(r):
    return float(np.cumsum(np.asarray(r, np.float64))[-1] / len(r))


# ---- the averages -----------------------------------------------------------------------------------------------------

def _finish(count, total, mean):
    with np.errstate(all="ignore"):
        return np.where(count > 0, total / np.maximum(count, 1).astype(np.float64), mean)


def sums(ul, cltr_u, cltr_i, n_cu, n_ci):
    """(count_cltr_u, count_cltr_i, count_cocltr, sum_cltr_u, sum_cltr_i, sum_cocltr), the sums grouped by user row."""
    ptr, ids, r = ul
    cu, ci, cc = np.zeros(n_cu, np.int64), np.zeros(n_ci, np.int64), np.zeros((n_cu, n_ci), np.int64)
    su, si, sc = np.zeros(n_cu), np.zeros(n_ci), np.zeros((n_cu, n_ci))
    with np.errstate(all="ignore"):
        for u in range(len(ptr) - 1):
            t, s = 0.0, np.zeros(n_ci)
            uc = int(cltr_u[u])
            for e in range(ptr[u], ptr[u + 1]):
                ic = int(cltr_i[ids[e]])
                t = t + float(r[e])
                s[ic] = s[ic] + r[e]
                cu[uc] += 1; ci[ic] += 1; cc[uc, ic] += 1
            su[uc] = su[uc] + t
            si = si + s
            sc[uc] = sc[uc] + s
    return cu, ci, cc, su, si, sc


def sums_literal(ul, cltr_u, cltr_i, n_cu, n_ci):
    """surprise's compute_averages loop on Python floats: one chain per sum over all_ratings() (ascending u, list order)."""
    ptr, ids, r = ul
    cu, ci, cc = [0] * n_cu, [0] * n_ci, [[0] * n_ci for _ in range(n_cu)]
    su, si, sc = [0.0] * n_cu, [0.0] * n_ci, [[0.0] * n_ci for _ in range(n_cu)]
    rr = np.asarray(r).tolist()
    for u in range(len(ptr) - 1):
        uc = int(cltr_u[u])
        for e in range(ptr[u], ptr[u + 1]):
            ic = int(cltr_i[ids[e]])
            cu[uc] += 1; ci[ic] += 1; cc[uc][ic] += 1
            su[uc] += rr[e]; si[ic] += rr[e]; sc[uc][ic] += rr[e]
    return (np.array(cu, np.int64), np.array(ci, np.int64), np.array(cc, np.int64).reshape(n_cu, n_ci), np.array(su), np.array(si),
            np.array(sc).reshape(n_cu, n_ci))


def averages(ul, cltr_u, cltr_i, n_cu, n_ci, mean, sums_fn=sums):
    """(avg_cltr_u, avg_cltr_i, avg_cocltr, count_cocltr)."""
    cu, ci, cc, su, si, sc = sums_fn(ul, cltr_u, cltr_i, n_cu, n_ci)
    return _finish(cu, su, mean), _finish(ci, si, mean), _finish(cc, sc, mean), cc


# ---- one epoch --------------------------------------------------------------------------------------------------------

def argmin(errors):
    """numpy's: the first NaN if there is one, else the first minimum.  Spelled out, so that the rule is on the page."""
    best = 0
    for c in range(len(errors)):
        e, b = errors[c], errors[best]
        if e != e:
            return c
        if e < b:
            best = c
    return best


def assign_users(ul, cltr_i, n_cu, avgs, user_mean, item_mean, keep=None):
    """The new cltr_u: one numpy operation over all candidates per entry, the entries in list order.  keep: a list that
    receives every row's errors."""
    ptr, ids, r = ul
    au, ai, acc = avgs[:3]
    out = np.zeros(len(ptr) - 1, np.int64)
    with np.errstate(all="ignore"):
        for u in range(len(ptr) - 1):
            errors = np.zeros(n_cu)
            for e in range(ptr[u], ptr[u + 1]):
                i = ids[e]
                ic = cltr_i[i]
                est = (((acc[:, ic] + user_mean[u]) - au) + item_mean[i]) - ai[ic]
                d = r[e] - est
                errors = errors + d * d
            out[u] = argmin(errors)
            if keep is not None:
                keep.append(errors)
    return out


def assign_items(il, cltr_u, n_ci, avgs, user_mean, item_mean, keep=None):
    ptr, ids, r = il
    au, ai, acc = avgs[:3]
    out = np.zeros(len(ptr) - 1, np.int64)
    with np.errstate(all="ignore"):
        for i in range(len(ptr) - 1):
            errors = np.zeros(n_ci)
            for e in range(ptr[i], ptr[i + 1]):
                u = ids[e]
                uc = cltr_u[u]
                est = (((acc[uc, :] + user_mean[u]) - au[uc]) + item_mean[i]) - ai
                d = r[e] - est
                errors = errors + d * d
            out[i] = argmin(errors)
            if keep is not None:
                keep.append(errors)
    return out


def epoch(ul, il, cltr_u, cltr_i, par, mean, user_mean, item_mean, sums_fn=sums):
    """(cltr_u', cltr_i', the averages the epoch used)."""
    avgs = averages(ul, cltr_u, cltr_i, par["n_cltr_u"], par["n_cltr_i"], mean, sums_fn)
    cltr_u = assign_users(ul, cltr_i, par["n_cltr_u"], avgs, user_mean, item_mean)
    cltr_i = assign_items(il, cltr_u, par["n_cltr_i"], avgs, user_mean, item_mean)
    return cltr_u, cltr_i, avgs


def fit(u, i, r, n_users, n_items, par, clusters=None, sums_fn=sums, trace=None):
    """The fitted model as a dict.  clusters: the initial (cltr_u, cltr_i) instead of init().  trace: a list that receives
    (cltr_u, cltr_i) after every epoch."""
    ul, il = lists(u, i, r, n_users), lists(i, u, r, n_items)
    mean, user_mean, item_mean = global_mean(r), mean_rows(ul), mean_rows(il)
    cltr_u, cltr_i = init(n_users, n_items, par) if clusters is None else (np.array(clusters[0], np.int64), np.array(clusters[1], np.int64))
    for _ in range(par["n_epochs"]):
        cltr_u, cltr_i, _ = epoch(ul, il, cltr_u, cltr_i, par, mean, user_mean, item_mean, sums_fn)
        if trace is not None:
            trace.append((cltr_u.copy(), cltr_i.copy()))
    au, ai, acc, cc = averages(ul, cltr_u, cltr_i, par["n_cltr_u"], par["n_cltr_i"], mean, sums_fn)
    return dict(cltr_u=cltr_u, cltr_i=cltr_i, avg_cltr_u=au, avg_cltr_i=ai, avg_cocltr=acc, count_cocltr=cc, user_mean=user_mean,
                item_mean=item_mean, mean=mean, ul=ul, il=il, n_users=n_users, n_items=n_items)


def fit_literal(u, i, r, n_users, n_items, par, trace=None):
    """surprise's fit, loop by loop on Python floats: compute_averages as one chain per sum, then per user and per candidate
    cluster a loop over ur[u], the same per item, numpy's own argmin.  (The means are mean_rows' all the same.)"""
    ul, il = lists(u, i, r, n_users), lists(i, u, r, n_items)
    mean, user_mean, item_mean = global_mean(r), mean_rows(ul).tolist(), mean_rows(il).tolist()
    cltr_u, cltr_i = init(n_users, n_items, par)
    n_cu, n_ci = par["n_cltr_u"], par["n_cltr_i"]
    ur = [[(int(ul[1][e]), float(ul[2][e])) for e in range(ul[0][k], ul[0][k + 1])] for k in range(n_users)]
    ir = [[(int(il[1][e]), float(il[2][e])) for e in range(il[0][k], il[0][k + 1])] for k in range(n_items)]
    for _ in range(par["n_epochs"]):
        au, ai, acc, _ = averages(ul, cltr_u, cltr_i, n_cu, n_ci, mean, sums_literal)
        au, ai, acc = au.tolist(), ai.tolist(), acc.tolist()
        for uu in range(n_users):
            errors = np.zeros(n_cu, np.double)
            for uc in range(n_cu):
                for ii, rr in ur[uu]:
                    ic = cltr_i[ii]
                    est = acc[uc][ic] + user_mean[uu] - au[uc] + item_mean[ii] - ai[ic]
                    errors[uc] += (rr - est) * (rr - est)
            cltr_u[uu] = np.argmin(errors)
        for ii in range(n_items):
            errors = np.zeros(n_ci, np.double)
            for ic in range(n_ci):
                for uu, rr in ir[ii]:
                    uc = cltr_u[uu]
                    est = acc[uc][ic] + user_mean[uu] - au[uc] + item_mean[ii] - ai[ic]
                    errors[ic] += (rr - est) * (rr - est)
            cltr_i[ii] = np.argmin(errors)
        if trace is not None:
            trace.append((cltr_u.copy(), cltr_i.copy()))
    au, ai, acc, cc = averages(ul, cltr_u, cltr_i, n_cu, n_ci, mean, sums_literal)
    return dict(cltr_u=cltr_u, cltr_i=cltr_i, avg_cltr_u=au, avg_cltr_i=ai, avg_cocltr=acc, count_cocltr=cc)


# ---- estimate ---------------------------------------------------------------------------------------------------------

def estimate(m, u, i):
    """The estimate of inner ids (anything outside its range is unknown), before the clip."""
    ku, ki = 0 <= u < m["n_users"], 0 <= i < m["n_items"]
    if ku and ki:
        uc, ic = m["cltr_u"][u], m["cltr_i"][i]
        with np.errstate(all="ignore"):
            return float((((m["avg_cocltr"][uc, ic] + m["user_mean"][u]) - m["avg_cltr_u"][uc]) + m["item_mean"][i]) - m["avg_cltr_i"][ic])
    if ku:
        return float(m["user_mean"][u])
    if ki:
        return float(m["item_mean"][i])
    return float(m["mean"])


def estimate_all(m, qu, qi):
    """(est, impossible): nothing is impossible."""
    return np.array([estimate(m, int(u), int(i)) for u, i in zip(qu, qi)], np.float64), np.zeros(len(qu), np.uint8)


def predictor(m, lo, hi):
    """predict(owner, item) -> (prediction, estimate, impossible) in the shape topn_reference.rankings takes."""
    def predict(owner, item):
        est = estimate(m, owner, item)
        return max(lo, min(hi, est)), est, 0
    return predict


# ---- seeded cases -----------------------------------------------------------------------------------------------------

def make_ratings(seed, n_users, n_items, n, kind="half"):
    """n distinct (u, i) cells in a shuffled training order; every user and item of the ranges need not occur.  kind
    "half": multiples of 1/2 in 0.5 .. 5, whose sums are exact; "fp64": arbitrary doubles."""
    rs = np.random.RandomState(seed)
    cells = rs.permutation(n_users * n_items)[:n]
    u, i = cells // n_items, cells % n_items
    r = rs.randint(1, 11, size=n) * 0.5 if kind == "half" else rs.normal(size=n) * 3.0 + rs.random_sample(n)
    return u.astype(np.int64), i.astype(np.int64), r


# (n_users, n_items, n_ratings, n_cltr_u, n_cltr_i, n_epochs, kind): the fits the GPU is held to after every epoch
FITS = ((70, 50, 600, 1, 1, 3, "half"), (70, 50, 600, 2, 3, 6, "fp64"), (130, 67, 1500, 3, 3, 8, "fp64"),
        (70, 50, 600, 17, 2, 6, "half"), (130, 67, 1500, 63, 64, 4, "fp64"), (130, 67, 1500, 64, 64, 4, "half"))
LIST_LENS = (0, 1, 63, 64, 65, 129, 5000)         # planted user lists of list_case()
CHAIN_USERS = (1, 63, 64, 65)


def list_case(n_cu=5, n_ci=4, seed=3):
    """Explicit assignments over lists of LIST_LENS entries: user k < 7 rated LIST_LENS[k] items of 5 000, 20 more users a
    few each, arbitrary doubles; every item is rated (user 6 rated them all).  Returns (u, i, r, n_users, n_items, cltr_u,
    cltr_i)."""
    rs = np.random.RandomState(seed)
    n_items, n_users = 5000, 27
    u, i = [], []
    for k, ln in enumerate(LIST_LENS):
        u += [k] * ln
        i += rs.permutation(n_items)[:ln].tolist()
    for k in range(len(LIST_LENS), n_users):
        ln = int(rs.randint(1, 9))
        u += [k] * ln
        i += rs.permutation(n_items)[:ln].tolist()
    u, i = np.array(u, np.int64), np.array(i, np.int64)
    o = rs.permutation(len(u))
    u, i = u[o], i[o]
    r = rs.normal(size=len(u)) * 2.0 + 3.0
    return u, i, r, n_users, n_items, rs.randint(n_cu, size=n_users).astype(np.int64), rs.randint(n_ci, size=n_items).astype(np.int64)


def edge_case(kind):
    """Small crafted inputs (u, i, r, n_users, n_items, cltr_u, cltr_i, n_cu, n_ci).
    "tie": clusters 0 and 1 of either side hold users / items with the same ratings, so their averages are equal and every
           row's errors tie between them: the first wins.
    "inf": one rating is +inf: its clusters' averages are inf, est is inf - inf = NaN there, and the first NaN wins.
    "huge": one rating is 1e308: d * d overflows for every candidate, the errors are all +inf and the first index wins."""
    if kind == "tie":
        # users 0, 1 (clusters 0, 1) rated items 0 .. 3 alike; items 0, 1 (clusters 0, 1) are rated alike by everybody
        u = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2], np.int64)
        i = np.array([0, 1, 2, 3, 0, 1, 2, 3, 2, 3], np.int64)
        r = np.array([4.0, 4.0, 2.0, 1.0, 4.0, 4.0, 2.0, 1.0, 5.0, 3.0])
        return u, i, r, 3, 4, np.array([0, 1, 2], np.int64), np.array([0, 1, 2, 2], np.int64), 3, 3
    u, i, r = make_ratings(11, 12, 9, 60, "half")
    r = r.copy()
    r[7] = np.inf if kind == "inf" else 1e308
    rs = np.random.RandomState(5)
    return u, i, r, 12, 9, rs.randint(4, size=12).astype(np.int64), rs.randint(3, size=9).astype(np.int64), 4, 3
