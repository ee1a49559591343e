"""TEST INFRASTRUCTURE — the definition of the SlopeOne predictor (n2v_slopeone_dev, n2v_slopeone_dev_sparse,
n2v_slopeone_estimate, n2v_slopeone_topn; n2v_hip.slopeone.SlopeOne), restated in plain Python, and the case table of
tests/test_slopeone_host.py and tests/test_gpu_slopeone.py.  The product never imports this file.

Parity is UNPINNED: scikit-surprise 1.0.6 is not installed and its source is not at hand; the rules below are restated from
memory of its SlopeOne and were never run against it.  This file is the definition the kernels are held to, bit for bit.
DEVIATION: numpy's mean adds pairwise above 8 elements; the user means here are knn_centered_reference.moments, sequential
sums in training order.

ur[u] = [(item, r), ...] in training order.  Every operation is one IEEE double operation on Python floats, one a line;
only a division, whose zero divisor Python refuses, goes through numpy (knn_centered_reference.div).

    fit:   for u ascending, for (i, ri) in ur[u], for (j, rj) in ur[u]:  freq[i][j] += 1;  acc[i][j] = acc[i][j] + (ri - rj)
           dev[i][i] = 0.0;  for i < j:  dev[i][j] = acc[i][j] / freq[i][j]  (freq 0: NaN),  dev[j][i] = -dev[i][j]
    estimate(u, i), both known:  over (j, _) in ur[u] with freq[i][j] > 0:  s = s + dev[i][j];  n += 1
           est = mu[u] if n == 0 else mu[u] + s / n;  never impossible.  Unknown u or i: impossible.

`mutant` switches on one deliberate error; tests/test_slopeone_host.py proves that the case table sees each of them.
`literal_*` is the transcription of surprise's own loops (a dict of lists, numpy's in-place operators, sum()) the
restatement is checked against.
"""
import math

import numpy as np

import eccknn_reference as E
import knn_centered_reference as C
import topn_reference as T

MUTANTS = ("mirror_summed", "freq_ge_0", "diagonal_out", "mean_of_Ri", "divide_by_len", "item_id_order")
div = C.div


# ---- the definition ---------------------------------------------------------------------------------------------------

def build_ur(u, i, r, n_users):
    ur = [[] for _ in range(n_users)]
    for uu, ii, rr in zip(u, i, r):
        ur[int(uu)].append((int(ii), float(rr)))
    return ur


def fit(u, i, r, n_users, n_items, mutant=None):
    """dict(freq int32, acc, dev fp64 [n_items][n_items], mu fp64[n_users], ur, n_users, n_items)."""
    ur = build_ur(u, i, r, n_users)
    freq = np.zeros((n_items, n_items), dtype=np.int32)
    acc = np.zeros((n_items, n_items), dtype=np.float64)
    for uu in range(n_users):
        for (a, ra) in ur[uu]:
            for (b, rb) in ur[uu]:
                d = ra - rb
                freq[a, b] += 1
                acc[a, b] = float(acc[a, b]) + d
    dev = np.zeros((n_items, n_items), dtype=np.float64)
    for a in range(n_items):
        dev[a, a] = 0.0
        for b in range(a + 1, n_items):
            dev[a, b] = div(float(acc[a, b]), float(freq[a, b]))
            if mutant == "mirror_summed":
                dev[b, a] = div(float(acc[b, a]), float(freq[b, a]))
            else:
                dev[b, a] = -float(dev[a, b])
    mu = np.array([C.moments([rr for (_, rr) in ur[uu]])[0] for uu in range(n_users)], dtype=np.float64).reshape(n_users)
    return dict(freq=freq, acc=acc, dev=dev, mu=mu, ur=ur, n_users=n_users, n_items=n_items)


def estimate(model, u, i, mutant=None):
    """(est, n_deviations, impossible) as n2v_slopeone_estimate reports them: est 0 where impossible."""
    if not (0 <= u < model["n_users"] and 0 <= i < model["n_items"]):
        return 0.0, 0, 1                                          # 'User and/or item is unkown.'
    freq, dev = model["freq"], model["dev"]
    lst = sorted(model["ur"][u]) if mutant == "item_id_order" else model["ur"][u]
    s = 0.0
    n = 0
    for (j, _) in lst:
        if mutant == "diagonal_out" and j == i:
            continue
        if freq[i, j] >= 0 if mutant == "freq_ge_0" else freq[i, j] > 0:
            s = s + float(dev[i, j])
            n += 1
    mu = float(model["mu"][u])
    if mutant == "mean_of_Ri":
        mu = C.moments([rr for (j, rr) in lst if freq[i, j] > 0])[0]
    if n == 0:
        return mu, 0, 0
    q = div(s, float(len(lst) if mutant == "divide_by_len" else n))
    return mu + q, n, 0


def estimate_all(model, qu, qi, mutant=None):
    n = len(qu)
    est, nd, imp = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for q in range(n):
        est[q], nd[q], imp[q] = estimate(model, int(qu[q]), int(qi[q]), mutant)
    return est, nd, imp


def predictor(model, mean, lo, hi):
    """predict(owner, item) -> (prediction, estimate, impossible) for topn_reference.rankings."""
    def predict(owner, item):
        est, _, imp = estimate(model, owner, item)
        return float(E.predict_all([est], [imp], mean, lo, hi)[0]), est, imp
    return predict


def rankings(case, model, owners):
    return T.rankings(case["seen"], case["n_items"], owners, predictor(model, case["mean"], *case["scale"]))


# ---- surprise's loops, transcribed ------------------------------------------------------------------------------------

def literal_fit(u, i, r, n_users, n_items):
    """(freq, dev, user_mean, ur) the way slope_one.pyx's fit forms them; np.mean replaced by the sequential mean."""
    ur = {uu: [] for uu in range(n_users)}
    for uu, ii, rr in zip(u, i, r):
        ur[int(uu)].append((int(ii), float(rr)))
    freq = np.zeros((n_items, n_items), np.int_)
    dev = np.zeros((n_items, n_items), np.double)
    with np.errstate(all="ignore"):
        for uu, u_ratings in ur.items():
            for ii, r_ui in u_ratings:
                for jj, r_uj in u_ratings:
                    freq[ii, jj] += 1
                    dev[ii, jj] += r_ui - r_uj
        for ii in range(n_items):
            dev[ii, ii] = 0
            for jj in range(ii + 1, n_items):
                dev[ii, jj] /= freq[ii, jj]
                dev[jj, ii] = -dev[ii, jj]
    user_mean = [C.moments([rr for (_, rr) in ur[uu]])[0] for uu in range(n_users)]
    return freq, dev, user_mean, ur


def literal_estimate(lit, u, i):
    """est of known (u, i) the way slope_one.pyx's estimate forms it."""
    freq, dev, user_mean, ur = lit
    Ri = [j for (j, _) in ur[u] if freq[i, j] > 0]
    est = user_mean[u]
    if Ri:
        with np.errstate(all="ignore"):
            est += sum(dev[i, j] for j in Ri) / len(Ri)
    return float(est), len(Ri)


# ---- the case table ---------------------------------------------------------------------------------------------------

TILE, YC, SC = 64, 32, 16                         # the tile kernels' constants: tile edge, dense y chunk, sparse row chunk
N_ITEMS = (1, 2, 63, 64, 65, 129)
N_USERS = (1, 31, 32, 33, 65)
LIST_LENS = (1, 63, 64, 65, 129, 130)             # the list lengths of users 0 .. 5 of the main case
BIG = 1e308


def grid_case(n_items, n_users, seed=0):
    """A table case: about 300 ratings (fewer where the grid is smaller) of halves 0.5 .. 5.0 with a few exact zeros and
    negatives, inner ids (u, i, r) in a shuffled training order; not every id need appear."""
    rs = np.random.RandomState(1000 * n_items + n_users + seed)
    cells = rs.permutation(n_items * n_users)[:300]
    u, i = cells // n_items, cells % n_items
    r = E.make_ratings(rs, len(cells), "half")
    r[rs.permutation(len(r))[:len(r) // 10]] = 0.0
    r[rs.permutation(len(r))[:len(r) // 10]] *= -1.0
    return dict(u=u.astype(np.int64), i=i.astype(np.int64), r=r, n_users=n_users, n_items=n_items)


def main_case(kind="fp64", scale=None, seed=0):
    """133 items x 40 users, about 700 ratings; inner ids (u, i, r) in a shuffled training order.  Planted:
      users 0 .. 5     lists of LIST_LENS entries, so lists cross the 64 lanes of a wavefront; users 4 and 5 rated
                       every item but 20, 129, 132 (and 128);
      items 3, 7, 100  rated 2.5 by everybody who rated them (users 4 .. 8): every deviation among them is a zero, +0.0
                       above the diagonal and -0.0 below it, inside one tile (3, 7) and across two (100);
      item 129         nobody rated it: an empty row, freq 0 and dev NaN against every item;
      user 9, item 20  rated each other alone: no estimate of user 9 for another item has a usable deviation, and
                       (9, 20) has the diagonal alone;
      items 10, 11     users 10 and 11 rate them (BIG, -BIG) and (-BIG, BIG): acc = inf + -inf, dev NaN with freq > 0;
                       the four ratings open the training order, alternating, so that no running sum overflows;
      item 132         user 12 alone rated it, among other items: user 12's estimates for the items they did not rate
                       use all of their list but this entry (0 < n < the list's length);
      items 22, 23, 24 exactly SC - 1, SC, SC + 1 raters (item 20 has 1, item 129 has 0)."""
    rs = np.random.RandomState(seed)
    n_items, n_users = 133, 40
    M = np.zeros((n_users, n_items), dtype=bool)
    special = [3, 7, 100, 10, 11, 20, 22, 23, 24, 128, 129, 132]
    ordinary = np.array([c for c in range(n_items) if c not in special])
    M[np.ix_(np.arange(12, n_users), ordinary)] = rs.random_sample((n_users - 12, len(ordinary))) < 0.05
    perm = rs.permutation(ordinary)
    M[0, perm[0]] = True
    for uu, ln in ((1, 63), (2, 64), (3, 65)):
        M[uu, perm[:ln]] = True
    M[4, :] = True
    M[4, [20, 128, 129, 132]] = False
    M[5, :] = True
    M[5, [20, 129, 132]] = False
    M[12, 132] = True
    M[6:9, [3, 7, 100]] = True
    M[9, 20] = True
    M[10:12, [10, 11]] = True
    for col, count in ((22, SC - 1), (23, SC), (24, SC + 1)):
        M[12:12 + count - 2, col] = True                          # users 4 and 5 are the other two
    assert tuple(int(M[uu].sum()) for uu in range(6)) == LIST_LENS
    uu, ii = np.nonzero(M)
    r = E.make_ratings(rs, len(uu), kind)
    r[rs.permutation(len(r))[:20]] = 0.0
    r[np.isin(ii, [3, 7, 100])] = 2.5
    big = (uu >= 10) & (uu <= 11)
    r[big] = np.where(uu[big] - 10 == ii[big] - 10, BIG, -BIG)
    order = rs.permutation(len(uu))
    first = [int(np.nonzero((uu == a) & (ii == b))[0][0]) for a, b in ((10, 10), (10, 11), (11, 10), (11, 11))]
    order = np.array(first + [k for k in order if k not in first])
    uu, ii, r = uu[order], ii[order], r[order]
    finite = r[np.abs(r) < BIG]
    scale = (float(finite.min()), float(finite.max())) if scale is None else scale
    return dict(u=uu.astype(np.int64), i=ii.astype(np.int64), r=r, n_users=n_users, n_items=n_items, scale=scale,
                mean=E.global_mean(r), seen=T.seen_sets(uu, ii, n_users))


def small_case(n_items, seed=0, scale=(2.0, 4.0)):
    """A top-N case with n_items candidates at most (63, 64, 65: around the 64 lanes of a block): 12 users, integer ratings,
    a narrow scale so that many predictions clip to equal scores; user 0 rated every item, user 1 all but two."""
    rs = np.random.RandomState(77 + n_items + seed)
    n_users = 12
    M = rs.random_sample((n_users, n_items)) < 0.2
    M[0, :] = True
    M[1, :] = True
    M[1, [0, n_items - 1]] = False
    M[2, :] = False
    M[2, n_items // 2] = True
    uu, ii = np.nonzero(M)
    order = rs.permutation(len(uu))
    uu, ii = uu[order], ii[order]
    r = E.make_ratings(rs, len(uu), "int")
    return dict(u=uu.astype(np.int64), i=ii.astype(np.int64), r=r, n_users=n_users, n_items=n_items, scale=scale,
                mean=E.global_mean(r), seen=T.seen_sets(uu, ii, n_users))


def cases():
    """[(name, case)]: what tests/test_gpu_slopeone.py compares with the device, table and estimates."""
    out = [("main", main_case())]
    out += [("grid-%d-%d" % (ni, nu), grid_case(ni, nu)) for ni in N_ITEMS for nu in N_USERS]
    out += [("small-%d" % ni, small_case(ni)) for ni in (63, 64, 65)]
    return out


def all_pairs(case):
    """Every (u, i) of the case, then unknown and out-of-range ids."""
    n_u, n_i = case["n_users"], case["n_items"]
    qu = np.repeat(np.arange(n_u), n_i).tolist() + [-1, 0, -1, n_u, 0, 2 ** 31 - 1, 3]
    qi = np.tile(np.arange(n_i), n_u).tolist() + [0, -1, -1, 0, n_i, 5, -(2 ** 31)]
    return np.array(qu, dtype=np.int64), np.array(qi, dtype=np.int64)


def outputs(case, mutant=None):
    """What the GPU test compares, as canonical bytes: the table and every estimate of all_pairs."""
    model = fit(case["u"], case["i"], case["r"], case["n_users"], case["n_items"], mutant)
    est, nd, imp = estimate_all(model, *all_pairs(case), mutant=mutant)
    return dict(dev=E.canon(model["dev"]), freq=E.canon(model["freq"]), est=E.canon(est), n=E.canon(nd), imp=E.canon(imp))


assert math.isnan(div(0.0, 0.0))
