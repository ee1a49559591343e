"""Restatement of the nearest-neighbour ranking (csrc/n2v_knn.hip, n2v_hip/neighbors.py), numpy only.

The SCORE of a pair is not restated here: it is by definition what n2v_sim_block writes (tests/test_gpu_sim_exact.py holds
that to float64), or an exact small integer.  This module restates the ORDER (csrc/n2v_rank.h) and the host logic of
most_similar, so every comparison against it is an equality."""
import numpy as np


def order_key(scores):
    """n2v_rank.h's key of fp32 scores as int64: larger score <=> larger key, NaN lowest, -0.0 and +0.0 share one."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    u = s.view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)
    key = np.where(s == 0, 0x80000000, key)
    return np.where(np.isnan(s), 0, key)


def rank(scores_row, k, exclude=None):
    """The first k of one row in rank order: positions sorted by (order key descending, position ascending), the
    position `exclude` dropped (None, or a value outside the row, drops nothing), padded with (-1, NaN).
    Returns (cols int32 [k], vals fp32 [k])."""
    s = np.ascontiguousarray(scores_row, dtype=np.float32).reshape(-1)
    pos = np.arange(len(s))
    order = np.lexsort((pos, -order_key(s)))
    if exclude is not None:
        order = order[order != int(exclude)]
    order = order[:k]
    cols = np.full(k, -1, dtype=np.int32)
    vals = np.full(k, np.nan, dtype=np.float32)
    cols[:len(order)] = order
    vals[:len(order)] = s[order]
    return cols, vals


def rank_rows(scores, k, exclude=None):
    """rank() of every row; exclude: None or one entry per row."""
    out = [rank(row, k, None if exclude is None else exclude[i]) for i, row in enumerate(np.asarray(scores))]
    return (np.stack([c for c, _ in out]), np.stack([v for _, v in out])) if out else \
        (np.empty((0, k), np.int32), np.empty((0, k), np.float32))


def same(cols, vals, want_cols, want_vals):
    """Equality of two results: the columns, where the scores are NaN, and the bits of every other score (a NaN's sign
    and payload are not part of the contract)."""
    cols, want_cols = np.asarray(cols), np.asarray(want_cols)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    want_vals = np.ascontiguousarray(want_vals, dtype=np.float32)
    if cols.shape != want_cols.shape or vals.shape != want_vals.shape or not np.array_equal(cols, want_cols):
        return False
    nan = np.isnan(want_vals)
    return bool(np.array_equal(np.isnan(vals), nan) and np.array_equal(vals.view(np.uint32)[~nan], want_vals.view(np.uint32)[~nan]))


# ------------------------------------------------------------------------------------------------ most_similar
def mean_query(weights, rows):
    """acc = w0 * x0; acc = acc + wi * xi ...; acc / float32(count): float32 throughout, in list order."""
    acc = np.float32(weights[0]) * np.asarray(rows[0], dtype=np.float32)
    for w, x in zip(weights[1:], rows[1:]):
        acc = acc + np.float32(w) * np.asarray(x, dtype=np.float32)
    return (acc / np.float32(len(rows))).astype(np.float32)


def drop_inputs(cols, vals, input_indices, topn, labels):
    """The ranked (index, score) pairs without the input words and without empty entries, cut to topn."""
    gone = set(int(i) for i in input_indices)
    out = [(labels[int(c)], float(v)) for c, v in zip(cols, vals) if c >= 0 and int(c) not in gone]
    return out[:topn]


def most_similar(score_row, labels, input_indices, topn):
    """score_row: the fp32 scores of the query against the first len(score_row) words.  The device is asked for
    topn + len(input_indices) neighbours, then the inputs leave."""
    cols, vals = rank(score_row, topn + len(input_indices))
    return drop_inputs(cols, vals, input_indices, topn, labels)


# ------------------------------------------------------------------------------------------------ the fp64 sanity data
ARC_D = 100
ARC_N = 100
ARC_GAP = 1e-3


def arc_data(seed=5):
    """ARC_N vectors on an arc of a random plane of R^100 at angles 0.1 + 0.02 i from the query direction, each with its
    own positive length, in shuffled order; the query is the direction at angle 0.  Neighbouring cosines differ by
    about 0.02 sin(angle) >= 0.002.  Returns (vectors fp32 [ARC_N, 100], query fp32 [1, 100])."""
    rs = np.random.RandomState(seed)
    basis, _ = np.linalg.qr(rs.normal(size=(ARC_D, 2)))
    u, v = basis[:, 0], basis[:, 1]
    theta = 0.1 + 0.02 * rs.permutation(ARC_N)
    length = 0.5 + rs.random_sample(ARC_N)
    vec = (np.cos(theta)[:, None] * u[None, :] + np.sin(theta)[:, None] * v[None, :]) * length[:, None]
    return vec.astype(np.float32), (2.0 * u).astype(np.float32)[None, :]


def arc_cosines(vec, query):
    """float64 cosines of the fp32 data."""
    x, q = vec.astype(np.float64), query.astype(np.float64)[0]
    return (x @ q) / (np.linalg.norm(x, axis=1) * np.linalg.norm(q))
