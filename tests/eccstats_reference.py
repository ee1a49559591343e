"""Restatement of the reference's eccentricity statistics (src/utils.py:53-153) for the tests of n2v_hip.eccstats.

Input: n rows (uid, id, feedback fp64, timewindow int64).  Duplicate (uid, id) rows are legal and count as rows.
Inner indices of users and items run in order of first appearance.  A group is a distinct (item, timewindow) pair;
groups are numbered in ascending (inner item, timewindow) order.

    z(x)    = x[k] - (mean(x) / std(x, ddof=0))      list_to_z_score, precedence bug kept: it is what the reference computes
    zo(x)   = (x - min) / (max - min)                list_to_zero_one
    unum[g] = rows of group g;   irg[g] = -math.log(unum[g])
    irmean[i] = (sum of irg over the item's groups) / (number of them);   ir = z(irmean)         calculate_ir_from_iu
    irz = z(irg) over groups                                                                     calculate_ir
    ws[u] = sum feedback * irz[group(row)],  fs[u] = sum feedback;  uer = ws / fs;  ue = z(uer)  calculate_ue_from_iu
    wi[i] = sum feedback * ue[user(row)],    fi[i] = sum feedback;  ier_ = wi / fi; ie = z(ier_) calculate_ie_from_iu
    ire = zo(ie * ir)                                                                            calculate_ire_from_iu
    ier = zo(q),  q = ie / ir with every +-inf replaced by 0.0                                   calculate_ier_from_iu

Order of the floating-point operations (the kernels reproduce it; the reference's pandas sums pairwise / with Kahan, so
the restatement is held to recorded reference output within a measured bound only, tests/test_eccstats_host.py):
  * a segment sum (an item's groups, a user's rows, an item's rows) starts at +0.0 and adds left to right: rows in file
    order, groups in ascending (item, timewindow) order; every product is rounded before it is added;
  * a global sum (of x, and of (x - m) * (x - m)) adds consecutive chunks of CHUNK elements left to right, each from
    +0.0, then the chunk sums left to right from +0.0; elements in ascending inner index / group number;
    var = sum / n, std = sqrt(var);
  * min / max: a NaN anywhere gives NaN (numpy's min / max; Python's min() over NaNs depends on the order, so that part
    of the reference is unpinned); -0.0 is below +0.0, so the result does not depend on the order either way.
No special case for a zero variance: the IEEE result of the formulas stands.

Two forms: `statistics_literal` (Python loops over Python floats) and `statistics_numpy` (vectorised); the host test
holds them to each other by bytes.  Nothing here imports the reference.
"""
import math

import numpy as np

CHUNK = 4096
COLUMNS = ("unum", "irg", "irmean", "ir", "irz", "ws", "fs", "uer", "ue", "wi", "fi", "ier_", "ie", "ire", "q", "ier")


def inner_ids(raw):
    """(inner id per entry, raw id of every inner id) by first appearance."""
    table, out = {}, []
    for v in raw:
        if v not in table:
            table[v] = len(table)
        out.append(table[v])
    return np.array(out, dtype=np.int64), list(table)


def groups_of(item, tw):
    """(group of every row, item of every group, timewindow of every group, unum), groups ascending (item, tw)."""
    pairs = sorted(set(zip(item.tolist(), tw.tolist())))
    number = {p: g for g, p in enumerate(pairs)}
    grp = np.array([number[p] for p in zip(item.tolist(), tw.tolist())], dtype=np.int64)
    unum = np.bincount(grp, minlength=len(pairs)).astype(np.int64)
    return grp, np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64), unum


# ---- literal -----------------------------------------------------------------------------------------------------------

def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def chunked_sum_literal(x):
    total = 0.0
    for c in range(0, len(x), CHUNK):
        s = 0.0
        for v in x[c:c + CHUNK]:
            s = s + v
        total = total + s
    return total


def z_literal(x):
    n = len(x)
    m = _div(chunked_sum_literal(x), float(n))
    dev = []
    for v in x:
        d = v - m
        dev.append(d * d)
    var = _div(chunked_sum_literal(dev), float(n))
    std = float(np.sqrt(np.float64(var)))
    shift = _div(m, std)
    return [v - shift for v in x]


def _min_max_literal(x):
    if any(v != v for v in x):
        return float("nan"), float("nan")
    key = lambda v: (v, 0 if math.copysign(1.0, v) < 0 else 1)        # -0.0 below +0.0
    return min(x, key=key), max(x, key=key)


def zo_literal(x):
    lo, hi = _min_max_literal(x)
    rng = hi - lo
    return [_div(v - lo, rng) for v in x]


def statistics_literal(uid, iid, feedback, timewindow):
    """Dict of every column in COLUMNS (float64 / int64 arrays) plus `users`, `items` (raw ids by inner index),
    `group_item`, `group_tw`, `row_group`."""
    u, users = inner_ids(uid)
    i, items = inner_ids(iid)
    f = [float(v) for v in feedback]
    tw = np.asarray(timewindow, dtype=np.int64)
    grp, g_item, g_tw, unum = groups_of(i, tw)
    n_u, n_i, n_g = len(users), len(items), len(unum)
    irg = [-math.log(int(c)) for c in unum]
    s, cnt = [0.0] * n_i, [0] * n_i
    for g in range(n_g):                                              # ascending (item, timewindow)
        s[g_item[g]] = s[g_item[g]] + irg[g]
        cnt[g_item[g]] += 1
    irmean = [_div(s[k], float(cnt[k])) for k in range(n_i)]
    ir = z_literal(irmean)
    irz = z_literal(irg)
    ws, fs = [0.0] * n_u, [0.0] * n_u
    for r in range(len(f)):                                           # file order
        ws[u[r]] = ws[u[r]] + f[r] * irz[grp[r]]
        fs[u[r]] = fs[u[r]] + f[r]
    uer = [_div(ws[k], fs[k]) for k in range(n_u)]
    ue = z_literal(uer)
    wi, fi = [0.0] * n_i, [0.0] * n_i
    for r in range(len(f)):
        wi[i[r]] = wi[i[r]] + f[r] * ue[u[r]]
        fi[i[r]] = fi[i[r]] + f[r]
    ier_ = [_div(wi[k], fi[k]) for k in range(n_i)]
    ie = z_literal(ier_)
    ire = zo_literal([ie[k] * ir[k] for k in range(n_i)])
    q = [_div(ie[k], ir[k]) for k in range(n_i)]
    q = [0.0 if math.isinf(v) else v for v in q]
    ier = zo_literal(q)
    loc = locals()
    out = {k: np.array(loc[k], dtype=np.int64 if k == "unum" else np.float64) for k in COLUMNS}
    out.update(users=users, items=items, group_item=g_item, group_tw=g_tw, row_group=grp)
    return out


# ---- vectorised --------------------------------------------------------------------------------------------------------

def chunked_sum(x):
    """np.cumsum adds one after the other.  A chunk is padded with +0.0: a sum that started at +0.0 is never -0.0, so
    adding +0.0 changes nothing."""
    x = np.asarray(x, dtype=np.float64)
    n_c = -(-len(x) // CHUNK)
    body = np.zeros(n_c * CHUNK)
    body[:len(x)] = x
    pad = np.zeros((n_c, CHUNK + 1))
    pad[:, 1:] = body.reshape(n_c, CHUNK)
    with np.errstate(all="ignore"):
        return float(np.cumsum(np.concatenate([[0.0], np.cumsum(pad, axis=1)[:, -1]]))[-1])


def z_score(x):
    x = np.asarray(x, dtype=np.float64)
    n = np.float64(len(x))
    with np.errstate(all="ignore"):
        m = np.float64(chunked_sum(x)) / n
        d = x - m
        std = np.sqrt(np.float64(chunked_sum(d * d)) / n)
        return x - (m / std)


def min_max(x):
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).any():
        return np.float64("nan"), np.float64("nan")
    lo, hi = x.min(), x.max()
    if lo == 0.0:
        lo = np.float64(-0.0) if (np.signbit(x) & (x == 0.0)).any() else np.float64(0.0)
    if hi == 0.0:
        hi = np.float64(0.0) if (~np.signbit(x) & (x == 0.0)).any() else np.float64(-0.0)
    return lo, hi


def zero_one(x):
    x = np.asarray(x, dtype=np.float64)
    lo, hi = min_max(x)
    with np.errstate(all="ignore"):
        return (x - lo) / (hi - lo)


def segment_sum(seg, values, n_seg):
    """Left to right in the order given: np.add.at is unbuffered and applies the elements one after the other."""
    out = np.zeros(n_seg)
    with np.errstate(all="ignore"):
        np.add.at(out, seg, values)
    return out


def first_appearance(raw):
    raw = np.asarray(raw)
    uniq, first, inv = np.unique(raw, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    return rank[inv.reshape(-1)], uniq[order].tolist()


def statistics_numpy(uid, iid, feedback, timewindow, log_of=None):
    """The same dict as statistics_literal.  log_of: count -> -math.log(count) cache, filled on the way."""
    u, users = first_appearance(uid)
    i, items = first_appearance(iid)
    f = np.asarray(feedback, dtype=np.float64)
    tw_values, tw_rank = np.unique(np.asarray(timewindow, dtype=np.int64), return_inverse=True)
    key = i * len(tw_values) + tw_rank.reshape(-1)
    gkeys, grp, unum = np.unique(key, return_inverse=True, return_counts=True)
    grp = grp.reshape(-1)
    g_item, g_tw = gkeys // len(tw_values), tw_values[gkeys % len(tw_values)]
    n_u, n_i = len(users), len(items)
    table = {} if log_of is None else log_of
    for c in np.unique(unum).tolist():
        if c not in table:
            table[c] = -math.log(c)
    irg = np.array([table[c] for c in unum.tolist()], dtype=np.float64)
    with np.errstate(all="ignore"):
        irmean = segment_sum(g_item, irg, n_i) / np.bincount(g_item, minlength=n_i).astype(np.float64)
        ir = z_score(irmean)
        irz = z_score(irg)
        ws, fs = segment_sum(u, f * irz[grp], n_u), segment_sum(u, f, n_u)
        uer = ws / fs
        ue = z_score(uer)
        wi, fi = segment_sum(i, f * ue[u], n_i), segment_sum(i, f, n_i)
        ier_ = wi / fi
        ie = z_score(ier_)
        ire = zero_one(ie * ir)
        q = ie / ir
        q = np.where(np.isinf(q), 0.0, q)
        ier = zero_one(q)
    unum = unum.astype(np.int64)
    loc = locals()
    out = {k: loc[k] for k in COLUMNS}
    out.update(users=users, items=items, group_item=g_item, group_tw=g_tw, row_group=grp)
    return out


def timewindow_utc(timestamps):
    """year * 100 + month of unix timestamps in UTC, by the calendar arithmetic of time.gmtime."""
    import time
    out = []
    for t in timestamps:
        st = time.gmtime(int(t))
        out.append(st.tm_year * 100 + st.tm_mon)
    return np.array(out, dtype=np.int64)


def canon(a):
    """Bytes of an array for exact comparison; every NaN becomes the one canonical NaN (as eccknn_reference.canon)."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), np.nan, a)
    return np.ascontiguousarray(a).tobytes()


def make_rows(seed, n_users, n_items, n_rows, n_windows=6, uniform_feedback=True, item_power=1.0):
    """Seeded synthetic rows: power-law items, feedback from a uniform (not exactly representable) or half stars."""
    rs = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, n_items + 1) ** item_power
    item = rs.choice(n_items, size=n_rows, p=pop / pop.sum())
    user = rs.randint(0, n_users, size=n_rows)
    fb = rs.uniform(0.1, 5.0, size=n_rows) if uniform_feedback else rs.randint(1, 11, size=n_rows) * 0.5
    tw = 201001 + rs.randint(0, n_windows, size=n_rows)
    return user.astype(np.int64), item.astype(np.int64), fb, tw.astype(np.int64)
