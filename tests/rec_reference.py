"""TEST INFRASTRUCTURE — restatement of the reference's top_N and its metrics (src/bine_train.py:311-406) for the kernels
of csrc/n2v_rec.hip.  The product never imports this file.

The reference module does not import on Python 3 (it imports modules that do not exist, and top_N itself calls
`sorted(..., lambda x, y: cmp(...))`), so nothing can be captured from it: parity is unpinned and restated from the text.

  top_N_literal    the text of :311-406 with its dicts and loops, and the one unavoidable change: `key=` for `cmp=`.
                   `sorted(..., key=score, reverse=True)` on Python 3 is stable, so equal scores keep the order of the
                   item list; the reference's Python-2 dict order is not reproducible.
  scores / ranked_lists / user_metrics / averages
                   the same in float64 numpy on the index form the device takes (row indices, -1 = unknown vertex;
                   ground truth as a CSR of item positions), held to top_N_literal by tests/test_rec_host.py.
  score_bound / ambiguous_users
                   the forward bound of an fp64 dot product in ANY summation order, and the users whose list a device
                   with another summation order could legitimately order differently.

NaN (no reference behaviour: Python's sort is undefined on it) ranks lowest here, below -inf."""
import math

import numpy as np

U = 2.0 ** -53          # unit roundoff of fp64 (round to nearest)


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u)."""
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


# ================================================================================================ the text
def nDCG(ranked_list, ground_truth):
    dcg = 0
    idcg = IDCG(len(ground_truth))
    for i in range(len(ranked_list)):
        id = ranked_list[i]
        if id not in ground_truth:
            continue
        rank = i + 1
        dcg += 1 / math.log(rank + 1, 2)
    return dcg / idcg


def IDCG(n):
    idcg = 0
    for i in range(n):
        idcg += 1 / math.log(i + 2, 2)
    return idcg


def AP(ranked_list, ground_truth):
    hits, sum_precs = 0, 0.0
    for i in range(len(ranked_list)):
        id = ranked_list[i]
        if id in ground_truth:
            hits += 1
            sum_precs += hits / (i + 1.0)
    if hits > 0:
        return sum_precs / len(ground_truth)
    else:
        return 0.0


def RR(ranked_list, ground_list):
    for i in range(len(ranked_list)):
        id = ranked_list[i]
        if id in ground_list:
            return 1 / (i + 1.0)
    return 0


def precision_and_racall(ranked_list, ground_list):
    hits = 0
    for i in range(len(ranked_list)):
        id = ranked_list[i]
        if id in ground_list:
            hits += 1
    pre = hits / (1.0 * len(ranked_list))
    rec = hits / (1.0 * len(ground_list))
    return pre, rec


def top_N_literal(test_u, test_v, test_rate, node_list_u, node_list_v, top_n, detail=None):
    """:311-359.  `detail` (a dict) receives the ranked label lists and the five per-user numbers."""
    recommend_dict = {}
    for u in test_u:
        recommend_dict[u] = {}
        for v in test_v:
            if node_list_u.get(u) is None:
                pre = 0
            else:
                U_ = np.array(node_list_u[u]['embedding_vectors'])
                if node_list_v.get(v) is None:
                    pre = 0
                else:
                    V = np.array(node_list_v[v]['embedding_vectors'])
                    pre = U_.dot(V.T)[0][0]
            recommend_dict[u][v] = float(pre)

    precision_list = []
    recall_list = []
    ap_list = []
    ndcg_list = []
    rr_list = []
    lists = []

    for u in test_u:
        tmp_r = sorted(recommend_dict[u].items(), key=lambda x: x[1], reverse=True)[0:min(len(recommend_dict[u]), top_n)]
        tmp_t = sorted(test_rate[u].items(), key=lambda x: x[1], reverse=True)[0:min(len(test_rate[u]), len(test_rate[u]))]
        tmp_r_list = []
        tmp_t_list = []
        for (item, rate) in tmp_r:
            tmp_r_list.append(item)

        for (item, rate) in tmp_t:
            tmp_t_list.append(item)
        pre, rec = precision_and_racall(tmp_r_list, tmp_t_list)
        ap = AP(tmp_r_list, tmp_t_list)
        rr = RR(tmp_r_list, tmp_t_list)
        ndcg = nDCG(tmp_r_list, tmp_t_list)
        precision_list.append(pre)
        recall_list.append(rec)
        ap_list.append(ap)
        rr_list.append(rr)
        ndcg_list.append(ndcg)
        lists.append(tmp_r_list)
    precison = sum(precision_list) / len(precision_list)
    recall = sum(recall_list) / len(recall_list)
    # the reference divides by precison + recall unguarded; the drop-in's 0.0 is kept for 0 + 0
    f1 = 2 * precison * recall / (precison + recall) if precison + recall > 0 else 0.0
    map = sum(ap_list) / len(ap_list)
    mrr = sum(rr_list) / len(rr_list)
    mndcg = sum(ndcg_list) / len(ndcg_list)
    if detail is not None:
        detail["lists"] = lists
        detail["per_user"] = [list(t) for t in zip(precision_list, recall_list, ap_list, rr_list, ndcg_list)]
    return f1, map, mrr, mndcg


# ================================================================================================ index form
def _rows(emb, dim, idx):
    emb = np.asarray(emb, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    out = np.zeros((idx.shape[0], dim), dtype=np.float64)
    known = idx >= 0
    out[known] = emb[idx[known], :dim]
    return out, known


def scores(emb, dim, u_idx, v_idx):
    """float64 [n_users][n_items]: emb[u_idx[i], :dim] . emb[v_idx[j], :dim]; exactly 0.0 where an end is unknown (-1)."""
    A, ka = _rows(emb, dim, u_idx)
    B, kb = _rows(emb, dim, v_idx)
    with np.errstate(all="ignore"):
        S = A @ B.T
    S[~ka, :] = 0.0
    S[:, ~kb] = 0.0
    return S


def score_bound(emb, dim, u_idx, v_idx):
    """|fp64 dot in any summation order - exact dot| <= gamma(dim + 2) sum_c |a_c||b_c| (the + 2: the restatement's own
    rounding is inside the same bound)."""
    A, _ = _rows(emb, dim, u_idx)
    B, _ = _rows(emb, dim, v_idx)
    return gamma(dim + 2) * (np.abs(A) @ np.abs(B).T)


def rank_row(row, k):
    """Positions of the k best scores of one user: descending score, equal scores by ascending position (-0.0 == +0.0);
    NaN last.  numpy's stable sort of the negated row is that order (it puts NaN behind everything, +inf included)."""
    return np.argsort(-np.asarray(row, dtype=np.float64), kind="stable")[:k]


def ranked_lists(S, top_n):
    """(ranked int32 [n_users][k], score fp64 [n_users][k]), k = min(n_items, top_n)."""
    k = min(S.shape[1], top_n)
    ranked = np.stack([rank_row(row, k) for row in S]).astype(np.int32).reshape(S.shape[0], k)
    return ranked, np.take_along_axis(S, ranked.astype(np.int64), axis=1)


def discount_table(k):
    return [1 / math.log(i + 2, 2) for i in range(k)]


def user_metrics(ranked, truth_ptr, truth_pos, truth_len):
    """float64 [n_users][5] = precision, recall, AP, RR, nDCG (:361-406) in Python float arithmetic."""
    out = np.zeros((len(ranked), 5), dtype=np.float64)
    for u, lst in enumerate(ranked):
        truth = set(int(p) for p in truth_pos[truth_ptr[u]:truth_ptr[u + 1]])
        glen = int(truth_len[u])
        hits, sum_precs, rr, dcg = 0, 0.0, 0, 0
        for i, item in enumerate(lst):
            if int(item) in truth:
                hits += 1
                sum_precs += hits / (i + 1.0)
                if hits == 1:
                    rr = 1 / (i + 1.0)
                dcg += 1 / math.log(i + 2, 2)
        out[u] = (hits / (1.0 * len(lst)), hits / (1.0 * glen), sum_precs / glen if hits > 0 else 0.0, rr, dcg / IDCG(glen))
    return out


def averages(per_user):
    cols = [[float(x) for x in per_user[:, j]] for j in range(5)]
    precison, recall, m_ap, mrr, mndcg = (sum(c) / len(c) for c in cols)
    f1 = 2 * precison * recall / (precison + recall) if precison + recall > 0 else 0.0
    return f1, m_ap, mrr, mndcg


def top_N(emb, dim, u_idx, v_idx, truth_ptr, truth_pos, truth_len, top_n):
    ranked, _ = ranked_lists(scores(emb, dim, u_idx, v_idx), top_n)
    per_user = user_metrics(ranked, truth_ptr, truth_pos, truth_len)
    return averages(per_user) + (per_user,)


def ambiguous_users(S, B, top_n):
    """Users whose ranked list is not decided by the restatement alone: among the user's best k + 1 scores two
    neighbours differ by no more than the sum of their forward bounds (two exact scores, bound 0 each, may tie: the list
    order decides).  Also returns the smallest non-zero gap and the largest bound met among those scores."""
    k = min(S.shape[1], top_n)
    bad, min_gap, max_bound, tied = [], np.inf, 0.0, 0
    for u, row in enumerate(S):
        order = rank_row(row, min(S.shape[1], k + 1))
        s, b = row[order], B[u][order]
        gap, both = s[:-1] - s[1:], b[:-1] + b[1:]
        if np.any((gap <= both) & (both > 0)) or np.any(np.isnan(s)):
            bad.append(u)
        if np.any(gap > 0):
            min_gap = min(min_gap, gap[gap > 0].min())
        max_bound = max(max_bound, b.max())
        tied += bool(np.any(gap == 0))
    return bad, min_gap, max_bound, tied


# ================================================================================================ shared inputs
# (users, items, d, top_n): the real-valued cases of tests/test_gpu_rec.py; tests/test_rec_host.py proves them fit
REAL_CASES = [(300, 5000, 128, 10), (257, 1031, 100, 10), (64, 20000, 256, 50), (500, 3000, 37, 100)]
REAL_SEEDS = (0, 1, 2, 3)


def padded(table, stride, fill=np.nan):
    """The table as fp64 [n][stride] with `fill` in columns [dim, stride): padding the kernels must never read."""
    out = np.full((table.shape[0], stride), fill, dtype=np.float64)
    out[:, :table.shape[1]] = table
    return out


def real_case(users, items, d, seed):
    """Normal embeddings, 5 % of the rows of each side zeroed.  Returns (table [users + items][d], u_idx, v_idx)."""
    rs = np.random.RandomState(seed)
    table = rs.normal(size=(users + items, d))
    table[rs.choice(users, max(1, users // 20), replace=False)] = 0.0
    table[users + rs.choice(items, max(1, items // 20), replace=False)] = 0.0
    return table, np.arange(users, dtype=np.int32), np.arange(users, users + items, dtype=np.int32)


def integer_case(users=200, items=3000, d=64, seed=9):
    """Embeddings from {-3 .. 3}: every product and partial sum is exact in fp64, whatever the order."""
    rs = np.random.RandomState(seed)
    table = rs.randint(-3, 4, size=(users + items, d)).astype(np.float64)
    return table, np.arange(users, dtype=np.int32), np.arange(users, users + items, dtype=np.int32)


def random_truth(n_users, n_items, seed, max_len=12, outside=3):
    """A ground-truth CSR: per user 1..max_len distinct item positions, plus up to `outside` test items that are not
    in the item list (counted in truth_len only)."""
    rs = np.random.RandomState(seed)
    ptr, pos, lens = [0], [], []
    for _ in range(n_users):
        m = rs.randint(0, min(max_len, n_items) + 1)
        extra = rs.randint(0, outside + 1)
        if m + extra == 0:
            extra = 1
        pos.extend(sorted(rs.choice(n_items, m, replace=False).tolist()))
        ptr.append(len(pos))
        lens.append(m + extra)
    return np.array(ptr, dtype=np.int64), np.array(pos, dtype=np.int32), np.array(lens, dtype=np.int64)
