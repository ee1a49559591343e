"""TEST INFRASTRUCTURE — the definition of the centred k-NN predictors (n2v_eccknn_row_moments, n2v_eccknn_estimate_centered,
n2v_eccknn_topn_centered; n2v_hip.eccknn.KNNWithMeans / KNNWithZScore / KNNBaseline), restated in plain Python.  The product
never imports this file.

Parity is UNPINNED: scikit-surprise 1.0.6 is not installed and its source is not at hand; the rules below are restated from
memory of its KNNWithMeans, KNNWithZScore and KNNBaseline and were never run against it.  This file is the definition the
kernels are held to, bit for bit.  DEVIATION: numpy's mean / std add pairwise above 8 elements; the sums here are
sequential, in training order.

x is the side the similarity is over, y the other one; yr[y] = [(x2, r), ...] in training order (eccknn_reference.build_yr),
rows[x] = [r, ...] in training order.  Every operation is one IEEE double operation on Python floats, every parenthesis one
rounding; only a division, whose zero divisor Python refuses, goes through numpy.  The neighbours are eccknn_reference's:
heapq.nlargest under its _rank_key (higher similarity first, ties by list position, NaN last), walked in rank order.

`mutant` switches on one deliberate error; tests/test_knn_centered_host.py proves that its case table sees each of them.
"""
import heapq
import math

import numpy as np

import eccknn_reference as E
import topn_reference as T

MODES = ("means", "zscore", "baseline")
MUTANTS = ("keep_neighbour_mean", "sigma_before_division", "item_bias_first", "neighbour_biases_first",
           "too_few_is_impossible", "zero_sigma_kept")


def div(a, b):
    """a / b as IEEE has it: x / 0 is inf or NaN, not an exception."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


# ---- row moments ------------------------------------------------------------------------------------------------------

def moments(values):
    """(mean, population sigma) of one row: both sums left to right from 0.0; an empty row is 0 / 0."""
    s = 0.0
    for v in values:
        s = s + float(v)
    mu = div(s, float(len(values)))
    q = 0.0
    for v in values:
        q = q + (float(v) - mu) * (float(v) - mu)
    with np.errstate(all="ignore"):
        return mu, float(np.sqrt(np.float64(div(q, float(len(values))))))


def row_moments(rows, zero_sigma=None):
    """(mu, sd) arrays over rows; a sigma equal to 0.0 becomes zero_sigma unless that is None or NaN."""
    mu, sd = np.empty(len(rows)), np.empty(len(rows))
    for x, row in enumerate(rows):
        mu[x], sd[x] = moments(row)
        if sd[x] == 0.0 and zero_sigma is not None and zero_sigma == zero_sigma:
            sd[x] = zero_sigma
    return mu, sd


def x_rows(x, r, n_x):
    """rows[x] = the ratings of x in training order."""
    rows = [[] for _ in range(n_x)]
    for xi, ri in zip(x, r):
        rows[int(xi)].append(float(ri))
    return rows


def tables(mode, x, y, r, n_x, n_y, user_based, gm, bu=None, bi=None, mutant=None):
    """What one mode reads: a dict with mode, user_based, gm, n_x, n_y and mu / sd (means, zscore) or bx / by (baseline)."""
    tab = dict(mode=mode, user_based=bool(user_based), gm=float(gm), n_x=n_x, n_y=n_y)
    if mode == "baseline":
        tab["bx"], tab["by"] = (bu, bi) if user_based else (bi, bu)
        return tab
    rows = x_rows(x, r, n_x)
    if mode == "means":
        tab["mu"] = row_moments(rows)[0]
        return tab
    overall = moments([float(v) for v in r])[1]                  # every rating as one row, in training order
    tab["overall_sd"] = overall
    tab["mu"], tab["sd"] = row_moments(rows, None if mutant == "zero_sigma_kept" else overall)
    return tab


# ---- the estimates ----------------------------------------------------------------------------------------------------

def estimate(tab, sim, yr, x, y, k, min_k, mutant=None):
    """(est, actual_k, impossible) as n2v_eccknn_estimate_centered reports them: est 0 where impossible."""
    mode, gm, ub = tab["mode"], tab["gm"], tab["user_based"]
    known_x, known_y = 0 <= x < tab["n_x"], 0 <= y < tab["n_y"]
    if mode == "baseline":
        bx, by = tab["bx"], tab["by"]
        if not (known_x and known_y):                             # the user's bias first, the unknown side's dropped
            est = gm
            for known, b, idx in ((known_x, bx, x), (known_y, by, y)) if ub else ((known_y, by, y), (known_x, bx, x)):
                if known:
                    est = est + float(b[idx])
            return est, 0, 0
        if mutant == "item_bias_first":
            base = (gm + float(by[y])) + float(bx[x]) if ub else (gm + float(bx[x])) + float(by[y])
        else:
            base = (gm + float(bx[x])) + float(by[y]) if ub else (gm + float(by[y])) + float(bx[x])
    else:
        if not (known_x and known_y):
            return 0.0, 0, 1                                      # 'User and/or item is unkown.'
        base = float(tab["mu"][x])
    neighbors = [(float(sim[x, x2]), r, x2) for (x2, r) in yr.get(y, [])]
    k_neighbors = heapq.nlargest(k, neighbors, key=E._rank_key)
    sum_sim = sum_ratings = 0.0
    actual_k = 0
    for (s, r, x2) in k_neighbors:
        if s > 0:
            if mode == "means":
                d = r if mutant == "keep_neighbour_mean" else r - float(tab["mu"][x2])
            elif mode == "zscore":
                d = div(r - float(tab["mu"][x2]), float(tab["sd"][x2]))
            elif mutant == "neighbour_biases_first":
                d = r - (gm + (float(bx[x2]) + float(by[y])))
            else:
                d = r - ((gm + float(bx[x2])) + float(by[y]))
            sum_sim = sum_sim + s
            sum_ratings = sum_ratings + s * d
            actual_k += 1
    if actual_k < min_k:
        if mutant == "too_few_is_impossible":
            return 0.0, actual_k, 1
        sum_ratings = 0.0
    if actual_k == 0:
        return base, 0, 0
    if mode == "zscore":
        if mutant == "sigma_before_division":
            return base + div(sum_ratings * float(tab["sd"][x]), sum_sim), actual_k, 0
        return base + div(sum_ratings, sum_sim) * float(tab["sd"][x]), actual_k, 0
    return base + div(sum_ratings, sum_sim), actual_k, 0


def estimate_all(tab, sim, yr, qx, qy, k, min_k, mutant=None):
    """(est, actual_k, impossible) arrays over the queries."""
    n = len(qx)
    est, ak, imp = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for q in range(n):
        est[q], ak[q], imp[q] = estimate(tab, sim, yr, int(qx[q]), int(qy[q]), k, min_k, mutant)
    return est, ak, imp


# ---- top-N ------------------------------------------------------------------------------------------------------------

def predictor(tab, sim, yr, k, min_k, mean, lo, hi):
    """predict(owner, item) -> (prediction, estimate, impossible) for topn_reference.rankings: the anti-testset through
    estimate, the fallback and clip of eccknn_reference.predict_all, then Python's stable reversed sort."""
    def predict(owner, item):
        x, y = (owner, item) if tab["user_based"] else (item, owner)
        est, _, imp = estimate(tab, sim, yr, x, y, k, min_k)
        return float(E.predict_all([est], [imp], mean, lo, hi)[0]), est, imp
    return predict


def rankings(case, tab, sim, yr, owners, k, min_k):
    return T.rankings(case["seen"], case["n_items"], owners, predictor(tab, sim, yr, k, min_k, case["mean"], *case["scale"]))


assert math.isnan(div(0.0, 0.0)) and div(1.0, 0.0) == float("inf")
