"""TEST INFRASTRUCTURE — the definition of the k-NN sweep (n2v_eccknn_estimate_sweep, n2v_eccknn_estimate_sweep_centered,
n2v_eccknn_errors; n2v_hip.eccknn.estimate_sweep / errors / test_sweep / accuracy_sweep), restated in plain Python.  The
product never imports this file.

A cell of the sweep IS the single-cell restatement called with that (k, min_k): eccknn_reference.estimate_all for the
plain mode, knn_centered_reference.estimate_all under a centring.  Nothing here knows that the cells share a selection;
that they may is the prefix claim, which `ranked` / `selection` below restate on their own so that
tests/test_knn_sweep_host.py can check it against heapq.nlargest.  `errors` is two sequential loops.

Parity with surprise is UNPINNED, as for the two restatements this one is built from.
"""
import heapq
import math

import numpy as np

import eccknn_reference as E
import knn_centered_reference as C

MODES = (None,) + C.MODES        # None: the plain mode (EccenKNN, KNNBasic)


# ---- the cells -----------------------------------------------------------------------------------------------------------

def estimate_cell(sim, yr, qx, qy, k, min_k, tab=None):
    """(est, actual_k, impossible) arrays of one cell: the single-cell restatement, called as it stands."""
    if tab is None:
        return E.estimate_all(sim, yr, qx, qy, k, min_k)
    return C.estimate_all(tab, sim, yr, qx, qy, k, min_k)


def estimate_sweep(sim, yr, qx, qy, ks, min_ks, tab=None):
    """(est fp64 [n_k][n_m][n_q], actual_k int32 [n_k][n_q], impossible uint8 [n_k][n_m][n_q]), cell by cell.  actual_k
    does not depend on min_k: asserted, not assumed."""
    n_k, n_m, n_q = len(ks), len(min_ks), len(qx)
    est, ak, imp = np.zeros((n_k, n_m, n_q)), np.zeros((n_k, n_q), np.int32), np.zeros((n_k, n_m, n_q), np.uint8)
    for j, k in enumerate(ks):
        for m, min_k in enumerate(min_ks):
            est[j, m], a, imp[j, m] = estimate_cell(sim, yr, qx, qy, k, min_k, tab)
            if m == 0:
                ak[j] = a
            assert np.array_equal(ak[j], a), (k, min_k)
    return est, ak, imp


def errors(pred, r_true):
    """(rmse, mae) arrays over the columns of pred [n_cols][n_q]: both sums left to right from 0.0, in query order."""
    pred = np.asarray(pred, dtype=np.float64)
    pred = pred.reshape(1, -1) if pred.ndim == 1 else pred
    rmse, mae = np.empty(len(pred)), np.empty(len(pred))
    for c, col in enumerate(pred):
        sq = ab = 0.0
        for r, e in zip(r_true, col):
            d = float(r) - float(e)
            sq = sq + d * d
        for r, e in zip(r_true, col):
            ab = ab + abs(float(r) - float(e))
        rmse[c], mae[c] = math.sqrt(sq / len(col)), ab / len(col)
    return rmse, mae


# ---- the prefix claim ----------------------------------------------------------------------------------------------------

def ranked(neighbors):
    """The device order restated: a stable descending sort of (sim, ...) tuples by sim, NaN last, -0.0 tying +0.0, equal
    sims by list position."""
    return sorted(neighbors, key=E._rank_key, reverse=True)     # reverse keeps the original order of equal keys


def selection(neighbors, k):
    """What the restatements select: heapq.nlargest under eccknn_reference's key."""
    return heapq.nlargest(k, neighbors, key=E._rank_key)


# ---- the crafted case ----------------------------------------------------------------------------------------------------

N_X = 300
LENGTHS = (0, 1, 2, 3, 4, 62, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 300)   # k - 1, k, k + 1 around 3, 64, 128, 256
HUGE = 1e308


def make_case(seed=3, kind="half"):
    """A crafted similarity and rating lists, no fit: n_x = 300, one y per entry of LENGTHS.
      sim      multiples of 1/8 from about -1 to 1 (ties, zeros and non-positive values between positive ones), a tenth of
               the zeros -0.0, 3% NaN; row 0 takes four values only (long ties), row 1 is half NaN, row 2 is eight times as
               large, so that with the ratings +-1e308 planted in every list of five or more raters a product is +-inf and
               inf - inf appears in sum_ratings;
      yr       every list a random set of distinct x in random order;
      queries  x = 0, 1, 2 and two random ones for every y, then unknown x, unknown y and both (-1);
      tables   mu, sd > 0, bx, by and gm for the centred modes, random: `tab(mode, user_based)`."""
    rs = np.random.RandomState(seed)
    n_x, n_y = N_X, len(LENGTHS)
    sim = np.round(rs.normal(size=(n_x, n_x)) * 4.0) / 8.0
    sim[0] = rs.choice([0.5, 0.25, 0.0, -0.25], size=n_x)
    zeros = np.argwhere(sim == 0.0)
    for a, b in zeros[rs.permutation(len(zeros))[:len(zeros) // 10]]:
        sim[a, b] = -0.0
    sim[rs.random_sample((n_x, n_x)) < 0.03] = np.nan
    sim[1, rs.permutation(n_x)[:n_x // 2]] = np.nan
    sim[2] = sim[2] * 8.0
    yr, ptr, xs, rr = {}, [0], [], []
    for y, L in enumerate(LENGTHS):
        ids = rs.permutation(n_x)[:L]
        r = E.make_ratings(rs, L, kind)
        if L >= 5:
            r[1], r[L // 2], r[L - 1] = HUGE, -HUGE, HUGE
        if L:
            yr[y] = [(int(a), float(b)) for a, b in zip(ids, r)]
        xs.extend(ids.tolist()); rr.extend(r.tolist()); ptr.append(len(xs))
    qx, qy = [], []
    for y in range(n_y):
        qx += [0, 1, 2] + rs.randint(3, n_x, 2).tolist()
        qy += [y] * 5
    qx += [-1, 7, -1]
    qy += [5, -1, -1]
    tables = dict(gm=3.25, mu=rs.normal(size=n_x) + 3.0, sd=rs.random_sample(n_x) + 0.5, bx=rs.normal(size=n_x) * 0.3,
                  by=rs.normal(size=n_y) * 0.3)
    return dict(n_x=n_x, n_y=n_y, sim=sim, yr=yr, ptr=np.array(ptr, np.int64), yr_x=np.array(xs, np.int32),
                yr_r=np.array(rr, np.float64), qx=np.array(qx, np.int32), qy=np.array(qy, np.int32), tables=tables)


def tab(case, mode, user_based=True):
    """The restatement's table dict of one centred mode over the case's crafted tables; None for the plain mode."""
    if mode is None:
        return None
    t = case["tables"]
    out = dict(mode=mode, user_based=bool(user_based), gm=t["gm"], n_x=case["n_x"], n_y=case["n_y"])
    if mode == "baseline":
        out["bx"], out["by"] = t["bx"], t["by"]
    else:
        out["mu"], out["sd"] = t["mu"], t["sd"]
    return out


# the grids of the tests: snapshots on the 64-entry chunk borders of the sum loop, next to each other, past L for some
# lists and (1 x 1 at 40, the short lists) for all; min_ks that straddle the counts and, in the last two, exceed every k
GRIDS = {
    "borders": ((63, 64, 65, 128, 256), (1, 2, 64, 66)),
    "adjacent": ((1, 2, 3), (1, 2, 3, 4)),
    "1x1": ((40,), (1,)),
    "one-k": ((10,), (1, 3, 5, 11)),
    "one-min_k": ((1, 5, 10, 129, 255), (2,)),
    "all-impossible": ((1, 2, 3), (4, 300)),
    "16x16": ((1, 2, 3, 4, 5, 8, 16, 32, 62, 63, 64, 65, 127, 128, 129, 256),
              (1, 2, 3, 4, 5, 6, 8, 16, 32, 63, 64, 65, 128, 129, 256, 257)),
}
MAIN_GRID = ((1, 2, 3, 5, 63, 64, 65, 128, 256), (1, 2, 3, 64, 66))
