"""TEST INFRASTRUCTURE — the definition of the top-N lists of the rating predictors (n2v_eccknn_topn, n2v_svd_topn), restated
literally, and the case table of tests/test_topn_host.py and tests/test_gpu_topn.py.  The product never imports this file.

The definition is surprise's documented recipe, `algo.test(trainset.build_anti_testset())` followed by get_top_n's
`user_ratings.sort(key=lambda x: x[1], reverse=True)`: per owner (an inner user id; one outside [0, n_users) is an unknown
user who has seen nothing) a loop over the inner items 0 .. n_items - 1 the owner has not rated, one estimate each
(eccknn_reference.estimate, or svd_reference.estimate), the training mean where the estimate is impossible, the clip of
eccknn_reference.predict_all, and Python's stable sort with reverse=True: higher score first, equal scores in ascending
inner item id, -0.0 equal to +0.0.  (No score is NaN: predict_all's min(hi, NaN) is hi.)  A list shorter than n is filled
with (-1, NaN).  Parity with surprise is UNPINNED, as for the estimates themselves: it is not installed.
"""
import numpy as np

import eccknn_reference as E
import svd_reference as SV


# ---- the definition ---------------------------------------------------------------------------------------------------

def seen_sets(u, i, n_users):
    """seen[u] = the inner items user u rated in the trainset."""
    seen = [set() for _ in range(n_users)]
    for uu, ii in zip(u, i):
        seen[int(uu)].add(int(ii))
    return seen


def anti_testset(seen, n_items, owner):
    """The candidates of one owner, ascending."""
    if not 0 <= owner < len(seen):
        return list(range(n_items))
    return [i for i in range(n_items) if i not in seen[owner]]


def knn_predictor(sim, yr, user_based, k, min_k, mean, lo, hi):
    """predict(owner, item) -> (prediction, estimate, impossible) of the k-NN classes; sim a host array, yr of build_yr."""
    def predict(owner, item):
        x, y = (owner, item) if user_based else (item, owner)
        try:
            if not (0 <= x < sim.shape[0]):
                raise E.PredictionImpossible("User and/or item is unkown.")
            est, imp = E.estimate(sim, yr, x, y, k, min_k)[0], 0
        except E.PredictionImpossible:
            est, imp = 0.0, 1
        return float(E.predict_all([est], [imp], mean, lo, hi)[0]), est, imp
    return predict


def svd_predictor(model, biased, mean, lo, hi):
    """The same for the factor model (mu, bu, bi, pu, qi); mean is the training mean, the fallback of SVD._test."""
    def predict(owner, item):
        est, imp = SV.estimate(model, [owner], [item], biased)
        return float(E.predict_all(est, imp, mean, lo, hi)[0]), float(est[0]), int(imp[0])
    return predict


def rankings(seen, n_items, owners, predict):
    """Per owner the whole ranked anti-testset [(item, prediction), ...]: every top-n list is a prefix of it."""
    out = []
    for owner in owners:
        owner = int(owner)
        user_ratings = [(i, predict(owner, i)[0]) for i in anti_testset(seen, n_items, owner)]
        user_ratings.sort(key=lambda x: x[1], reverse=True)
        out.append(user_ratings)
    return out


def lists(ranked, n):
    """(items int32 [n_owners][n], score fp64 [n_owners][n]) of rankings(); (-1, NaN) where a ranking is shorter than n."""
    items = np.full((len(ranked), n), -1, dtype=np.int32)
    score = np.full((len(ranked), n), np.nan, dtype=np.float64)
    for row, user_ratings in enumerate(ranked):
        for col, (i, s) in enumerate(user_ratings[:n]):
            items[row, col], score[row, col] = i, s
    return items, score


def segment_borders(n_items, S):
    """The first candidate of every segment but the first, as the kernels cut the range: n_items * seg // S."""
    return sorted({n_items * seg // S for seg in range(1, S)} - {0, n_items})


# ---- the case table ---------------------------------------------------------------------------------------------------

N_USERS, N_ITEMS = 70, 150
KS = (1, 40, 64, 65, 256)
NS = (1, 10, 64, 65, 256)
SEGMENTS = (1, 2, 3, 7, 64, None)                 # None: the library's default
MIN_KS = (1, 3)
INT_SCALE = (2.0, 4.0)                            # narrower than the ratings 1 .. 5: estimates are clipped at both ends


def make_case(kind="int", seed=0):
    """About 1 500 ratings of 70 users x 150 items as raw triples in a shuffled training order, with inner ids by first
    appearance.  Planted (raw ids): user "full" rated every item; user "almost" all but three; item "lonely" has one
    rater ("full"); items "p66", "p64", "p65" have that many raters, so item lists cross 64 and the two long users' lists
    do as neighbour lists of the item-based side.  kind "int": ratings 1 .. 5 and the rating scale INT_SCALE; "fp64":
    real-valued ratings, the scale their range.  w_items / w_users ~ N(0, 1) over inner ids, negative ones included."""
    rs = np.random.RandomState(seed)
    M = rs.random_sample((N_USERS, N_ITEMS)) < 0.095
    full, almost, lonely = 5, 9, 149
    M[:, lonely] = False
    for col, count in ((0, 66), (1, 64), (2, 65)):
        others = [u for u in rs.permutation(N_USERS) if u not in (full, almost)][:count - 2]
        M[:, col] = False
        M[others, col] = True
    M[full, :] = True
    M[almost, :] = True
    M[almost, [3, 77, lonely]] = False
    uu, ii = np.nonzero(M)
    order = rs.permutation(len(uu))
    uu, ii = uu[order], ii[order]
    names_u = {full: "full", almost: "almost"}
    names_i = {lonely: "lonely", 0: "p66", 1: "p64", 2: "p65"}
    raw_u = [names_u.get(int(v), "u%02d" % v) for v in uu]
    raw_i = [names_i.get(int(v), "i%03d" % v) for v in ii]
    r = E.make_ratings(rs, len(uu), kind)
    u, users = E.inner_ids(raw_u)
    i, items = E.inner_ids(raw_i)
    assert len(users) == N_USERS and len(items) == N_ITEMS
    scale = INT_SCALE if kind == "int" else (float(r.min()), float(r.max()))
    return dict(kind=kind, raw_u=raw_u, raw_i=raw_i, u=u, i=i, r=r, users=users, items=items, n_users=N_USERS,
                n_items=N_ITEMS, scale=scale, mean=E.global_mean(r), w_items=rs.normal(size=N_ITEMS),
                w_users=rs.normal(size=N_USERS), seen=seen_sets(u, i, N_USERS))


def side(case, user_based):
    """(n_x, yr, w) of one side: x the side similarities are formed over."""
    if user_based:
        return case["n_users"], E.build_yr(case["u"], case["i"], case["r"]), case["w_items"]
    return case["n_items"], E.build_yr(case["i"], case["u"], case["r"]), case["w_users"]


def svd_tables(case, n_factors, seed=0):
    """A factor model that was not trained: (mu, bu, bi, pu, qi) with biases ~ N(0, 0.7) and dots ~ N(0, 1), so that
    predictions leave the scale on both ends."""
    rs = np.random.RandomState(100 + seed + n_factors)
    f = n_factors ** -0.25
    return (case["mean"], 0.7 * rs.normal(size=case["n_users"]), 0.7 * rs.normal(size=case["n_items"]),
            f * rs.normal(size=(case["n_users"], n_factors)), f * rs.normal(size=(case["n_items"], n_factors)))


def owner_list(case):
    """Every user, then an unknown one, a subset and repeats."""
    n = case["n_users"]
    return np.array(list(range(n)) + [-1, 3, n - 1, 3, -1, 0], dtype=np.int32)
