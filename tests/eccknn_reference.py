"""Restatement of the reference's EccenKNN (src/main_rec.py:63-329) for the tests of n2v_hip.eccknn.

Parity is UNPINNED: `surprise` is not installed and the reference's main() raises unconditionally, so nothing here was
ever run against the reference; it is restated from the text.

Two forms of the similarity:
  *_literal   the reference's `for y: for xi: for xj` loops over Python floats, line by line;
  *_numpy     one fancy-indexed update per y.  The raters of one y are distinct, so every pair (xi, xj) still receives
              its terms one y after the other, ascending — the same rounded operations in the same order.
`ri**2` is written `ri * ri`: the correctly rounded square, which libm's pow(ri, 2.0) is not guaranteed to be.

estimate / predict / rmse follow src/main_rec.py:305-329 and the documented behaviour of surprise's AlgoBase.predict
and accuracy.rmse.  DEVIATION (also in include/n2v_sim.h): a NaN similarity ranks below everything;
heapq.nlargest with NaN keys depends on the order of its comparisons.

Inner ids: first appearance in the training data (surprise's construct_trainset); -1 = unknown.
"""
import heapq
import math

import numpy as np


# ---- ids and lists ----------------------------------------------------------------------------------------------------

def inner_ids(raw):
    """(inner id per entry, raw id of every inner id) by first appearance."""
    table, out = {}, []
    for v in raw:
        if v not in table:
            table[v] = len(table)
        out.append(table[v])
    return np.array(out, dtype=np.int64), list(table)


def build_yr(x, y, r):
    """yr[y] = [(x, r), ...] in training order, keys ascending (= order of first appearance for inner ids)."""
    yr = {}
    for xi, yi, ri in zip(x, y, r):
        yr.setdefault(int(yi), []).append((int(xi), float(ri)))
    return {k: yr[k] for k in sorted(yr)}


# ---- similarities, literal --------------------------------------------------------------------------------------------

def cosine_literal(n_x, yr, min_support, w):
    prods = np.zeros((n_x, n_x), np.double)
    freq = np.zeros((n_x, n_x), np.int64)
    sqi = np.zeros((n_x, n_x), np.double)
    sqj = np.zeros((n_x, n_x), np.double)
    sim = np.zeros((n_x, n_x), np.double)
    for y, y_ratings in yr.items():
        wy = float(w[y])
        for xi, ri in y_ratings:
            for xj, rj in y_ratings:
                freq[xi, xj] += 1
                prods[xi, xj] += ri * rj * wy
                sqi[xi, xj] += ri * ri
                sqj[xi, xj] += rj * rj
    with np.errstate(all="ignore"):
        for xi in range(n_x):
            sim[xi, xi] = 1
            for xj in range(xi + 1, n_x):
                if freq[xi, xj] < min_support:
                    sim[xi, xj] = 0
                else:
                    denum = np.sqrt(sqi[xi, xj] * sqj[xi, xj])
                    sim[xi, xj] = prods[xi, xj] / denum
                sim[xj, xi] = sim[xi, xj]
    return dict(sim=sim, freq=freq, prods=prods, sqi=sqi, sqj=sqj)


def msd_literal(n_x, yr, min_support, w):
    sq_diff = np.zeros((n_x, n_x), np.double)
    freq = np.zeros((n_x, n_x), np.int64)
    sim = np.zeros((n_x, n_x), np.double)
    for y, y_ratings in yr.items():
        wy = float(w[y])
        for xi, ri in y_ratings:
            for xj, rj in y_ratings:
                d = (ri - rj) * wy
                sq_diff[xi, xj] += d * d
                freq[xi, xj] += 1
    with np.errstate(all="ignore"):
        for xi in range(n_x):
            sim[xi, xi] = 1
            for xj in range(xi + 1, n_x):
                if freq[xi, xj] < min_support:
                    sim[xi, xj] == 0          # the reference's no-op: sim starts as zeros
                else:
                    sim[xi, xj] = 1 / (sq_diff[xi, xj] / freq[xi, xj] + 1)
                sim[xj, xi] = sim[xi, xj]
    return dict(sim=sim, freq=freq, sq_diff=sq_diff)


# ---- similarities, numpy (same per-pair order) ------------------------------------------------------------------------

def _finish(sim_upper, n_x):
    iu = np.triu_indices(n_x, 1)
    sim = np.zeros((n_x, n_x), np.double)
    sim[iu] = sim_upper[iu]
    sim.T[iu] = sim_upper[iu]
    sim[np.arange(n_x), np.arange(n_x)] = 1
    return sim


def cosine_numpy(n_x, yr, min_support, w):
    prods = np.zeros((n_x, n_x), np.double)
    freq = np.zeros((n_x, n_x), np.int64)
    sqi = np.zeros((n_x, n_x), np.double)
    sqj = np.zeros((n_x, n_x), np.double)
    for y, y_ratings in yr.items():
        xs = np.array([x for x, _ in y_ratings], dtype=np.int64)
        rs = np.array([r for _, r in y_ratings], dtype=np.double)
        ix = np.ix_(xs, xs)
        sq = rs * rs
        freq[ix] += 1
        prods[ix] += (rs[:, None] * rs[None, :]) * float(w[y])
        sqi[ix] += sq[:, None]
        sqj[ix] += sq[None, :]
    with np.errstate(all="ignore"):
        full = np.where(freq < min_support, 0.0, prods / np.sqrt(sqi * sqj))
    return dict(sim=_finish(full, n_x), freq=freq, prods=prods, sqi=sqi, sqj=sqj)


def msd_numpy(n_x, yr, min_support, w):
    sq_diff = np.zeros((n_x, n_x), np.double)
    freq = np.zeros((n_x, n_x), np.int64)
    for y, y_ratings in yr.items():
        xs = np.array([x for x, _ in y_ratings], dtype=np.int64)
        rs = np.array([r for _, r in y_ratings], dtype=np.double)
        ix = np.ix_(xs, xs)
        d = (rs[:, None] - rs[None, :]) * float(w[y])
        sq_diff[ix] += d * d
        freq[ix] += 1
    with np.errstate(all="ignore"):
        full = np.where(freq < min_support, 0.0, 1 / (sq_diff / freq + 1))
    return dict(sim=_finish(full, n_x), freq=freq, sq_diff=sq_diff)


LITERAL = {"cosine": cosine_literal, "msd": msd_literal}
NUMPY = {"cosine": cosine_numpy, "msd": msd_numpy}


# ---- estimate / predict / rmse ----------------------------------------------------------------------------------------

class PredictionImpossible(Exception):
    pass


def _rank_key(t):
    s = t[0]
    return (0, 0.0) if s != s else (1, s)     # NaN below everything; -0.0 == 0.0 for Python's comparison


def estimate(sim, yr, x, y, k, min_k):
    """src/main_rec.py:305-329 on inner ids (-1 = unknown)."""
    if x < 0 or y < 0:
        raise PredictionImpossible("User and/or item is unkown.")
    neighbors = [(float(sim[x, x2]), r) for (x2, r) in yr.get(y, [])]
    k_neighbors = heapq.nlargest(k, neighbors, key=_rank_key)
    sum_sim = sum_ratings = actual_k = 0
    for (s, r) in k_neighbors:
        if s > 0:
            sum_sim += s
            sum_ratings += s * r
            actual_k += 1
    if actual_k < min_k:
        raise PredictionImpossible("Not enough neighbors.")
    with np.errstate(all="ignore"):
        est = float(np.float64(sum_ratings) / np.float64(sum_sim))     # inf / inf is NaN, not an exception
    return est, {"actual_k": actual_k}


def estimate_all(sim, yr, qx, qy, k, min_k):
    """(est, actual_k, impossible) arrays the way n2v_eccknn_estimate reports them: est 0 where impossible.  The
    neighbours with sim > 0 are counted also for an impossible estimate (they are what made it impossible)."""
    n = len(qx)
    est, ak, imp = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for q in range(n):
        x, y = int(qx[q]), int(qy[q])
        try:
            est[q], d = estimate(sim, yr, x, y, k, min_k)
            ak[q] = d["actual_k"]
        except PredictionImpossible:
            imp[q] = 1
            if x >= 0 and y >= 0:
                try:
                    ak[q] = estimate(sim, yr, x, y, k, 0)[1]["actual_k"]
                except ZeroDivisionError:
                    ak[q] = 0
    return est, ak, imp


def global_mean(r):
    s = 0.0
    for v in r:
        s += float(v)
    return s / len(r)


def predict_all(est, impossible, mean, lo, hi):
    out = np.empty(len(est))
    for q in range(len(est)):
        e = mean if impossible[q] else float(est[q])
        e = min(hi, e)
        e = max(lo, e)
        out[q] = e
    return out


def rmse(r_true, pred):
    s = 0.0
    for r, e in zip(r_true, pred):
        d = float(r) - float(e)
        s += d * d
    return math.sqrt(s / len(pred))


# ---- seeded cases -----------------------------------------------------------------------------------------------------

def make_ratings(rs, n, kind):
    if kind == "int":
        return rs.randint(1, 6, size=n).astype(np.float64)
    if kind == "half":
        return rs.randint(1, 11, size=n) * 0.5
    if kind == "fp64":
        return rs.normal(size=n) * 3.0 + rs.random_sample(n)
    raise ValueError(kind)


def make_case(seed, n_x, n_y, n_ratings, kind="int", zeros=0, plant=True):
    """Inner-id triples (x, y, r) with every x < n_x and y < n_y appearing, ids in order of first appearance, no duplicate
    (x, y); weights w[n_y] ~ N(0, 1) (negative ones included).  plant (needs n_x >= 3 and n_y >= 2): the last x rates
    only the last y and nobody else does — a y with one rater and an x that shares nothing.  zeros: that many ratings
    are set to exactly 0.0."""
    rs = np.random.RandomState(seed)
    plant = plant and n_x >= 3 and n_y >= 2
    fx, fy = (n_x - 1, n_y - 1) if plant else (n_x, n_y)
    cells = rs.permutation(fx * fy)[:min(n_ratings, fx * fy)]
    x, y = cells // fy, cells % fy
    if plant:
        x, y = np.append(x, n_x - 1), np.append(y, n_y - 1)
    # relabel by first appearance so that the arrays are valid inner ids; ids that never appear keep the tail
    def relabel(v, n):
        seen = list(dict.fromkeys(v.tolist()))
        rest = [i for i in range(n) if i not in set(seen)]
        m = np.empty(n, np.int64)
        m[np.array(seen + rest, dtype=np.int64)] = np.arange(n)
        return m[v]
    x, y = relabel(x, n_x), relabel(y, n_y)
    r = make_ratings(rs, len(x), kind)
    if zeros:
        r[rs.permutation(len(r))[:zeros]] = 0.0
    w = rs.normal(size=n_y)
    return x.astype(np.int64), y.astype(np.int64), r, w


def canon(a):
    """Bytes of an array for exact comparison.  NaNs are replaced by the one canonical NaN: IEEE 754 leaves a NaN's sign
    and payload to the implementation (0/0 is negative on x86 hosts and positive on the device)."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), np.nan, a)
    return np.ascontiguousarray(a).tobytes()
