"""Restatement of the plain k-NN baseline's similarities, surprise's `pearson` and `pearson_baseline`, and of its ALS
baselines (`baseline_als`), for the tests of n2v_hip.eccknn.KNNBasic.  The reference reaches them through
src/main_rec.py:166-169 and :181-189.

Parity is UNPINNED: scikit-surprise 1.0.6 (the reference's requirements.txt:42) is not installed and its source is not
at hand; the arithmetic below is restated from memory of that source and was never run against it.  This file is the
definition the kernels are held to, bit for bit.

The optional weight w[y] is what the reference meant to apply (it passes `i_dict=i_dict` to every similarity, :197;
surprise's functions would have rejected the keyword).  w None: the factor is not applied; w of ones gives the same bits.

Two forms of each similarity, as in tests/eccknn_reference.py:
  *_literal   the `for y: for xi: for xj` loops over Python floats;
  *_numpy     one fancy-indexed update per y: every pair still receives its terms one y after the other, ascending.
`x**2` is written `x * x`, the correctly rounded square.  The finishing formulas run on numpy fp64 scalars so that a
negative radicand and a zero divisor give the IEEE NaN / inf of the C source instead of a Python exception.
"""
import numpy as np

from eccknn_reference import _finish


def rows_of(major, minor, r, n_major):
    """rows[m] = [(minor id, r), ...] in training order, one list for every m < n_major (an empty one where m never
    appears): surprise's ur / ir."""
    rows = [[] for _ in range(n_major)]
    for m, o, v in zip(major, minor, r):
        rows[int(m)].append((int(o), float(v)))
    return rows


# ---- pearson ----------------------------------------------------------------------------------------------------------

def _pearson_pair(freq, prods, sqi, sqj, si, sj, min_support):
    if freq < min_support:
        return 0.0
    n = np.float64(freq)
    num = n * np.float64(prods) - np.float64(si) * np.float64(sj)
    denum = np.sqrt((n * np.float64(sqi) - np.float64(si) * np.float64(si)) *
                    (n * np.float64(sqj) - np.float64(sj) * np.float64(sj)))
    if denum == 0:
        return 0.0
    return float(num / denum)


def pearson_literal(n_x, yr, min_support, w=None):
    prods = np.zeros((n_x, n_x), np.double)
    freq = np.zeros((n_x, n_x), np.int64)
    sqi = np.zeros((n_x, n_x), np.double)
    sqj = np.zeros((n_x, n_x), np.double)
    si = np.zeros((n_x, n_x), np.double)
    sj = np.zeros((n_x, n_x), np.double)
    sim = np.zeros((n_x, n_x), np.double)
    for y, y_ratings in yr.items():
        for xi, ri in y_ratings:
            for xj, rj in y_ratings:
                freq[xi, xj] += 1
                prods[xi, xj] += ri * rj if w is None else ri * rj * float(w[y])
                sqi[xi, xj] += ri * ri
                sqj[xi, xj] += rj * rj
                si[xi, xj] += ri
                sj[xi, xj] += rj
    with np.errstate(all="ignore"):
        for xi in range(n_x):
            sim[xi, xi] = 1
            for xj in range(xi + 1, n_x):
                sim[xi, xj] = _pearson_pair(freq[xi, xj], prods[xi, xj], sqi[xi, xj], sqj[xi, xj], si[xi, xj], sj[xi, xj],
                                            min_support)
                sim[xj, xi] = sim[xi, xj]
    return dict(sim=sim, freq=freq, prods=prods, sqi=sqi, sqj=sqj, si=si, sj=sj)


def pearson_numpy(n_x, yr, min_support, w=None):
    prods = np.zeros((n_x, n_x), np.double)
    freq = np.zeros((n_x, n_x), np.int64)
    sqi = np.zeros((n_x, n_x), np.double)
    sqj = np.zeros((n_x, n_x), np.double)
    si = np.zeros((n_x, n_x), np.double)
    sj = np.zeros((n_x, n_x), np.double)
    for y, y_ratings in yr.items():
        xs = np.array([x for x, _ in y_ratings], dtype=np.int64)
        rs = np.array([r for _, r in y_ratings], dtype=np.double)
        ix = np.ix_(xs, xs)
        sq = rs * rs
        pr = rs[:, None] * rs[None, :]
        freq[ix] += 1
        prods[ix] += pr if w is None else pr * float(w[y])
        sqi[ix] += sq[:, None]
        sqj[ix] += sq[None, :]
        si[ix] += rs[:, None]
        sj[ix] += rs[None, :]
    with np.errstate(all="ignore"):
        n = freq.astype(np.double)
        num = n * prods - si * sj
        denum = np.sqrt((n * sqi - si * si) * (n * sqj - sj * sj))
        full = np.where(freq < min_support, 0.0, np.where(denum == 0, 0.0, num / denum))
    return dict(sim=_finish(full, n_x), freq=freq, prods=prods, sqi=sqi, sqj=sqj, si=si, sj=sj)


# ---- pearson_baseline -------------------------------------------------------------------------------------------------

def pearson_baseline_literal(n_x, yr, min_support, global_mean, bx, by, shrinkage=100, w=None):
    prods = np.zeros((n_x, n_x), np.double)
    freq = np.zeros((n_x, n_x), np.int64)
    sq_diff_i = np.zeros((n_x, n_x), np.double)
    sq_diff_j = np.zeros((n_x, n_x), np.double)
    sim = np.zeros((n_x, n_x), np.double)
    min_sprt = max(2, min_support)
    global_mean, shrinkage = float(global_mean), float(shrinkage)
    for y, y_ratings in yr.items():
        partial_bias = global_mean + float(by[y])
        for xi, ri in y_ratings:
            for xj, rj in y_ratings:
                freq[xi, xj] += 1
                diff_i = ri - (partial_bias + float(bx[xi]))
                diff_j = rj - (partial_bias + float(bx[xj]))
                prods[xi, xj] += diff_i * diff_j if w is None else diff_i * diff_j * float(w[y])
                sq_diff_i[xi, xj] += diff_i * diff_i
                sq_diff_j[xi, xj] += diff_j * diff_j
    with np.errstate(all="ignore"):
        for xi in range(n_x):
            sim[xi, xi] = 1
            for xj in range(xi + 1, n_x):
                if freq[xi, xj] < min_sprt:
                    sim[xi, xj] = 0
                else:
                    sim[xi, xj] = prods[xi, xj] / np.sqrt(sq_diff_i[xi, xj] * sq_diff_j[xi, xj])
                    f1 = np.float64(freq[xi, xj] - 1)
                    sim[xi, xj] *= f1 / (f1 + np.float64(shrinkage))
                sim[xj, xi] = sim[xi, xj]
    return dict(sim=sim, freq=freq, prods=prods, sq_diff_i=sq_diff_i, sq_diff_j=sq_diff_j)


def pearson_baseline_numpy(n_x, yr, min_support, global_mean, bx, by, shrinkage=100, w=None):
    prods = np.zeros((n_x, n_x), np.double)
    freq = np.zeros((n_x, n_x), np.int64)
    sq_diff_i = np.zeros((n_x, n_x), np.double)
    sq_diff_j = np.zeros((n_x, n_x), np.double)
    min_sprt = max(2, min_support)
    bx = np.asarray(bx, dtype=np.double)
    for y, y_ratings in yr.items():
        xs = np.array([x for x, _ in y_ratings], dtype=np.int64)
        rs = np.array([r for _, r in y_ratings], dtype=np.double)
        ix = np.ix_(xs, xs)
        d = rs - ((float(global_mean) + float(by[y])) + bx[xs])
        sq = d * d
        pr = d[:, None] * d[None, :]
        freq[ix] += 1
        prods[ix] += pr if w is None else pr * float(w[y])
        sq_diff_i[ix] += sq[:, None]
        sq_diff_j[ix] += sq[None, :]
    with np.errstate(all="ignore"):
        f1 = (freq - 1).astype(np.double)
        full = np.where(freq < min_sprt, 0.0, (prods / np.sqrt(sq_diff_i * sq_diff_j)) * (f1 / (f1 + float(shrinkage))))
    return dict(sim=_finish(full, n_x), freq=freq, prods=prods, sq_diff_i=sq_diff_i, sq_diff_j=sq_diff_j)


# ---- baselines --------------------------------------------------------------------------------------------------------

def baselines_als(ur, ir, global_mean, n_epochs=10, reg_u=15, reg_i=10):
    """(bu, bi) of surprise's baseline_als.  ur[u] = [(i, r), ...] and ir[i] = [(u, r), ...] in training order
    (rows_of); every row's sum starts at 0.0 and adds its terms in list order."""
    bu, bi = np.zeros(len(ur)), np.zeros(len(ir))
    global_mean = float(global_mean)
    with np.errstate(all="ignore"):
        for _ in range(n_epochs):
            for i, lst in enumerate(ir):
                dev_i = 0.0
                for (u, r) in lst:
                    dev_i += r - global_mean - float(bu[u])
                bi[i] = np.float64(dev_i) / np.float64(float(reg_i) + len(lst))
            for u, lst in enumerate(ur):
                dev_u = 0.0
                for (i, r) in lst:
                    dev_u += r - global_mean - float(bi[i])
                bu[u] = np.float64(dev_u) / np.float64(float(reg_u) + len(lst))
    return bu, bi


LITERAL = {"pearson": pearson_literal, "pearson_baseline": pearson_baseline_literal}
NUMPY = {"pearson": pearson_numpy, "pearson_baseline": pearson_baseline_numpy}
ACCUMULATORS = {"pearson": ("prods", "sqi", "sqj", "si", "sj"), "pearson_baseline": ("prods", "sq_diff_i", "sq_diff_j")}
