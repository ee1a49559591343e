"""Restatement of surprise 1.0.6's SVD (the reference's `-algo svd`, src/main_rec.py:341-348) under the stratified
schedule of n2v_hip.svd, for the tests of csrc/n2v_svd.hip.  It is the definition the kernels equal bit for bit.

Parity is UNPINNED: `surprise` is not installed, the model and the update are restated from memory, and nothing here
was ever run against surprise itself.

The model: est = mu + bu[u] + bi[i] + qi[i] . pu[u] (biased) or qi[i] . pu[u].  Per rating (u, i, r), everything fp64,
no fused multiply-add, every expression left to right, puf / qif the values before the rating:
    err = r - (((mu + bu[u]) + bi[i]) + dot)             biased;  err = r - dot otherwise
    bu[u] = bu[u] + lr_bu * (err - reg_bu * bu[u]);  bi[i] = bi[i] + lr_bi * (err - reg_bi * bi[i])       biased only
    pu[u, f] = puf + lr_pu * (err * qif - reg_pu * puf);  qi[i, f] = qif + lr_qi * (err * puf - reg_qi * qif)

The schedule (P = n_strata): ub = (u * P) // n_users, ib = (i * P) // n_items, stratum s = (ib - ub) % P; an epoch is
`for s: for ub:` over the blocks (s, ub), and inside a block the ratings keep surprise's all_ratings() order (ascending
inner user id, then training order).  n_strata None is surprise's own sequence with the dot summed in ascending f;
n_strata 1 is the same sequence with the dot in lane order.

The dot in lane order (lane_dot): 64 lanes start from +0.0, lane l adds the products of the factors l, l + 64, l + 128,
l + 192 that exist, ascending; then v = v + v[lane ^ m] for m = 32, 16, 8, 4, 2, 1.  Addition commutes, so all lanes
end with the same bits; dot_lanes computes lane 0's value by halving.

Two forms of one epoch: fit_literal (Python floats, the triple loop over ratings, factors and lanes) and fit (one numpy
row operation per rating: the same rounded operations in the same order).
"""
import numpy as np

DEFAULTS = dict(n_factors=100, n_epochs=20, biased=True, init_mean=0, init_std_dev=0.1, lr_all=0.005, reg_all=0.02,
                lr_bu=None, lr_bi=None, lr_pu=None, lr_qi=None, reg_bu=None, reg_bi=None, reg_pu=None, reg_qi=None,
                random_state=0)
RATES = ("lr_bu", "lr_bi", "lr_pu", "lr_qi", "reg_bu", "reg_bi", "reg_pu", "reg_qi")
LANES = 64


def params(**kw):
    """surprise's options with lr_all / reg_all filled into the eight per-parameter values."""
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise ValueError("unknown option " + ", ".join(sorted(unknown)))
    p = dict(DEFAULTS, **kw)
    for k in RATES:
        if p[k] is None:
            p[k] = p[k[:k.index("_")] + "_all"]
        p[k] = float(p[k])
    return p


# ---- the schedule -----------------------------------------------------------------------------------------------------

def all_ratings_order(u):
    """Positions of the training ratings in surprise's all_ratings() order: by inner user id, then training order."""
    return np.argsort(np.asarray(u, np.int64), kind="stable")


def block_keys(u, i, n_users, n_items, P):
    """(s, ub) of every rating."""
    u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
    ub, ib = (u * P) // n_users, (i * P) // n_items
    return (ib - ub) % P, ub


def block_order(u, i, n_users, n_items, P):
    """u, i in all_ratings() order -> (order, blk_ptr): order[k] is the rating applied k-th in an epoch, blk_ptr
    int64[P * P + 1] the ranges of the blocks (s, ub) at s * P + ub."""
    s, ub = block_keys(u, i, n_users, n_items, P)
    key = s * P + ub
    order = np.argsort(key, kind="stable")
    ptr = np.zeros(P * P + 1, np.int64)
    np.cumsum(np.bincount(key, minlength=P * P), out=ptr[1:])
    return order, ptr


# ---- the dot ----------------------------------------------------------------------------------------------------------

def lane_dot(q, p):
    """The 64 lanes after the butterfly."""
    q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
    v = np.zeros(LANES)
    for k in range(0, len(q), LANES):
        prod = q[k:k + LANES] * p[k:k + LANES]
        v[:len(prod)] = v[:len(prod)] + prod
    lane = np.arange(LANES)
    with np.errstate(all="ignore"):
        for m in (32, 16, 8, 4, 2, 1):
            v = v + v[lane ^ m]
    return v


def dot_lanes(q, p):
    """lane_dot(q, p)[0] by halving: lane 0's additions and nothing else."""
    n = len(q)
    if n <= LANES:
        v = np.zeros(LANES)
        v[:n] = q * p
    else:
        v = np.zeros(LANES)
        for k in range(0, n, LANES):
            prod = q[k:k + LANES] * p[k:k + LANES]
            v[:len(prod)] = v[:len(prod)] + prod
    v = v[:32] + v[32:]
    v = v[:16] + v[16:]
    v = v[:8] + v[8:]
    v = v[:4] + v[4:]
    v = v[:2] + v[2:]
    return v[0] + v[1]


def dot_ascending(q, p):
    """0.0 + q0 * p0 + q1 * p1 + ..., one after the other (cumsum adds sequentially)."""
    return np.cumsum(np.concatenate(([0.0], q * p)))[-1]


def _dot_lanes_literal(q, p):
    v = [0.0] * LANES
    for f in range(len(q)):                                       # ascending f: lane f % 64 meets its factors ascending
        v[f % LANES] = v[f % LANES] + q[f] * p[f]
    for m in (32, 16, 8, 4, 2, 1):
        v = [v[l] + v[l ^ m] for l in range(LANES)]
    return v[0]


def _dot_ascending_literal(q, p):
    dot = 0.0
    for f in range(len(q)):
        dot = dot + q[f] * p[f]
    return dot


# ---- fit --------------------------------------------------------------------------------------------------------------

def global_mean(r):
    return float(np.cumsum(np.asarray(r, np.float64))[-1] / len(r))


def init(n_users, n_items, par):
    rng = np.random.RandomState(par["random_state"])
    pu = rng.normal(par["init_mean"], par["init_std_dev"], (n_users, par["n_factors"]))
    qi = rng.normal(par["init_mean"], par["init_std_dev"], (n_items, par["n_factors"]))
    return np.zeros(n_users), np.zeros(n_items), pu, qi


def sequence(u, i, r, n_users, n_items, n_strata):
    """(u, i, r) in the order one epoch applies them; u, i, r in training order."""
    u, i, r = np.asarray(u, np.int64), np.asarray(i, np.int64), np.asarray(r, np.float64)
    o = all_ratings_order(u)
    u, i, r = u[o], i[o], r[o]
    if n_strata is not None:
        o = block_order(u, i, n_users, n_items, n_strata)[0]
        u, i, r = u[o], i[o], r[o]
    return u, i, r


def fit(u, i, r, n_users, n_items, par, n_strata, n_epochs=None):
    """(mu, bu, bi, pu, qi) after par["n_epochs"] (or n_epochs) epochs; mu is 0.0 when not biased."""
    su, si, sr = sequence(u, i, r, n_users, n_items, n_strata)
    dot_fn = dot_ascending if n_strata is None else dot_lanes
    biased = bool(par["biased"])
    mu = global_mean(r) if biased else 0.0
    bu, bi, pu, qi = init(n_users, n_items, par)
    lr_bu, lr_bi, lr_pu, lr_qi, reg_bu, reg_bi, reg_pu, reg_qi = (par[k] for k in RATES)
    seq = list(zip(su.tolist(), si.tolist(), sr.tolist()))
    with np.errstate(all="ignore"):
        for _ in range(par["n_epochs"] if n_epochs is None else n_epochs):
            for uu, ii, rr in seq:
                p, q = pu[uu], qi[ii]
                dot = dot_fn(q, p)
                if biased:
                    b_u, b_i = bu[uu], bi[ii]
                    err = rr - (((mu + b_u) + b_i) + dot)
                    bu[uu] = b_u + lr_bu * (err - reg_bu * b_u)
                    bi[ii] = b_i + lr_bi * (err - reg_bi * b_i)
                else:
                    err = rr - dot
                new_p = p + lr_pu * (err * q - reg_pu * p)
                qi[ii] = q + lr_qi * (err * p - reg_qi * q)
                pu[uu] = new_p
    return mu, bu, bi, pu, qi


def fit_literal(u, i, r, n_users, n_items, par, n_strata, n_epochs=None):
    """fit() as loops over Python floats: for epoch, for stratum, for block, for rating, for factor."""
    u, i, r = np.asarray(u, np.int64), np.asarray(i, np.int64), np.asarray(r, np.float64)
    biased = bool(par["biased"])
    mu = global_mean(r) if biased else 0.0                       # training order
    o = all_ratings_order(u)
    u, i, r = u[o].tolist(), i[o].tolist(), r[o].tolist()
    bu, bi, pu, qi = init(n_users, n_items, par)
    bu, bi, pu, qi = bu.tolist(), bi.tolist(), pu.tolist(), qi.tolist()
    nf = par["n_factors"]
    lr_bu, lr_bi, lr_pu, lr_qi, reg_bu, reg_bi, reg_pu, reg_qi = (par[k] for k in RATES)

    def apply(k, dot_fn):
        uu, ii, rr = u[k], i[k], r[k]
        dot = dot_fn(qi[ii], pu[uu])
        if biased:
            err = rr - (mu + bu[uu] + bi[ii] + dot)
            bu[uu] += lr_bu * (err - reg_bu * bu[uu])
            bi[ii] += lr_bi * (err - reg_bi * bi[ii])
        else:
            err = rr - dot
        for f in range(nf):
            puf, qif = pu[uu][f], qi[ii][f]
            pu[uu][f] += lr_pu * (err * qif - reg_pu * puf)
            qi[ii][f] += lr_qi * (err * puf - reg_qi * qif)

    P = n_strata
    with np.errstate(all="ignore"):
        for _ in range(par["n_epochs"] if n_epochs is None else n_epochs):
            if P is None:
                for k in range(len(r)):
                    apply(k, _dot_ascending_literal)
                continue
            for s in range(P):
                for b in range(P):
                    for k in range(len(r)):                      # all_ratings() order inside the block
                        ub, ib = (u[k] * P) // n_users, (i[k] * P) // n_items
                        if ub == b and (ib - ub) % P == s:
                            apply(k, _dot_lanes_literal)
    return mu, np.array(bu), np.array(bi), np.array(pu).reshape(n_users, nf), np.array(qi).reshape(n_items, nf)


# ---- estimate ---------------------------------------------------------------------------------------------------------

def estimate(model, qu, qi_ids, biased, dot_fn=dot_lanes):
    """(est, impossible) arrays for inner ids, -1 = unknown; est is 0 where impossible, before any fallback or clipping."""
    mu, bu, bi, pu, qi = model
    est, imp = np.zeros(len(qu)), np.zeros(len(qu), np.uint8)
    with np.errstate(all="ignore"):
        for k, (u, i) in enumerate(zip(qu, qi_ids)):
            ku, ki = 0 <= u < len(bu), 0 <= i < len(bi)
            if biased:
                e = mu
                if ku:
                    e = e + bu[u]
                if ki:
                    e = e + bi[i]
                if ku and ki:
                    e = e + dot_fn(qi[i], pu[u])
                est[k] = e
            elif ku and ki:
                est[k] = dot_fn(qi[i], pu[u])
            else:
                imp[k] = 1                                        # 'User and item are unknown.'
    return est, imp


# ---- seeded cases -----------------------------------------------------------------------------------------------------

def make_ratings(seed, n_users, n_items, n, rank=4, noise=0.3):
    """n distinct (u, i) cells of 3 + a user offset + an item offset + half a rank-`rank` product + noise, clipped to
    [1, 5], in a shuffled training order; every id below n_users / n_items may or may not appear."""
    rs = np.random.RandomState(seed)
    a, b = rs.normal(size=(n_users, rank)), rs.normal(size=(n_items, rank))
    ou, oi = 0.6 * rs.normal(size=n_users), 0.6 * rs.normal(size=n_items)
    cells = rs.permutation(n_users * n_items)[:n]
    u, i = cells // n_items, cells % n_items
    r = np.clip(3.0 + ou[u] + oi[i] + 0.5 * (a[u] * b[i]).sum(1) / np.sqrt(rank) + noise * rs.normal(size=n), 1.0, 5.0)
    return u.astype(np.int64), i.astype(np.int64), r
