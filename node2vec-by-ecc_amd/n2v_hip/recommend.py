"""Top-N recommendation of the BiNE path on the device (csrc/n2v_rec.hip, C-ABI include/n2v_bine.h).

Reference: src/bine_train.py:311-359 (`top_N`) and :361-406 (its metrics).  Scores are fp64 dot products formed tile by
tile on the matrix cores with the per-user selection fused behind them; nothing of size users x items is stored.

Ranking rule (defined here, the reference's Python-2 dict order is not reproducible): descending score, equal scores in
ascending position of the caller's item list — `sorted(..., key=score, reverse=True)` on Python 3, whose sort is stable
also when reversed.  -0.0 ties +0.0, NaN ranks lowest.  An unknown vertex (index -1) scores exactly 0.0 against
everything, so ties are the normal case.

There is no CPU fallback.
"""
import itertools
import math

import numpy as np
import torch

from . import _lib

MAX_TOP_N = 256          # N2V_REC_MAX_TOPN
MAX_SEGMENTS = 64
ROW_BLOCK = 128          # user rows per workgroup
ITEM_TILE = 64           # items per tile; segments are ranges of whole tiles


def _require_gpu(t=None):
    if not torch.cuda.is_available():
        raise RuntimeError("n2v_hip.recommend: no GPU visible (torch.cuda.is_available() is False); no CPU fallback")
    if t is not None and not t.is_cuda:
        raise RuntimeError("n2v_hip.recommend: the embedding table must live on the device; no CPU fallback")


def _index(x, device):
    t = torch.as_tensor(x)
    if t.numel() and (int(t.min()) < -1 or int(t.max()) > 0x7fffffff):
        raise ValueError("row indices must be -1 (unknown) or non-negative int32")
    return t.to(device=device, dtype=torch.int32).contiguous()


def discount_table(k):
    """1 / math.log(i + 2, 2) for i < k: nDCG's per-rank gain (src/bine_train.py:369), Python's two-argument log."""
    return np.array([1 / math.log(i + 2, 2) for i in range(k)], dtype=np.float64)


def idcg_table(n):
    """IDCG(0..n) (src/bine_train.py:372-376): the left-to-right running sum of the discount series."""
    out = np.zeros(n + 1, dtype=np.float64)
    acc = 0
    for i in range(n):
        acc += 1 / math.log(i + 2, 2)
        out[i + 1] = acc
    return out


def top_n_lists(emb, dim, u_idx, v_idx, top_n, segments=None):
    """(ranked int32 [n_users][k], score fp64 [n_users][k]) on the device, k = min(n_items, top_n): per user position
    the k best item positions.  emb: fp64 [n][stride] device tensor, columns [0, dim) are used; u_idx / v_idx: row
    indices into emb, -1 = unknown vertex."""
    _require_gpu(emb)
    if emb.dtype != torch.float64 or emb.dim() != 2 or emb.stride(1) != 1:
        raise ValueError("emb must be a 2-d fp64 tensor with unit column stride")
    top_n = int(top_n)
    if not 1 <= top_n <= MAX_TOP_N:
        raise ValueError("top_n %d outside [1, %d]" % (top_n, MAX_TOP_N))
    segments = 0 if segments is None else int(segments)
    if not 0 <= segments <= MAX_SEGMENTS:
        raise ValueError("segments %d outside [0, %d]" % (segments, MAX_SEGMENTS))
    dev = emb.device
    u_idx, v_idx = _index(u_idx, dev), _index(v_idx, dev)
    n_users, n_items = u_idx.numel(), v_idx.numel()
    if n_users == 0 or n_items == 0:
        raise ValueError("top_n_lists: %d users x %d items: nothing to rank" % (n_users, n_items))
    if not 1 <= int(dim) <= emb.shape[1]:
        raise ValueError("dim %d outside [1, %d]" % (dim, emb.shape[1]))
    lib = _lib.load()
    S = segments or int(lib.n2v_bine_rec_segments(n_users, n_items))
    k = min(n_items, top_n)
    with torch.cuda.device(dev):
        part_score = torch.empty((n_users, S, k), dtype=torch.float64, device=dev)
        part_pos = torch.empty((n_users, S, k), dtype=torch.int32, device=dev)
        ranked = torch.empty((n_users, k), dtype=torch.int32, device=dev)
        score = torch.empty((n_users, k), dtype=torch.float64, device=dev)
        rc = lib.n2v_bine_rec_topn(emb.data_ptr(), emb.shape[0], int(dim), emb.stride(0), _lib.ptr(u_idx), n_users,
                                   _lib.ptr(v_idx), n_items, top_n, S, _lib.ptr(part_score), _lib.ptr(part_pos),
                                   _lib.ptr(ranked), _lib.ptr(score), _lib.stream_ptr(dev))
    _lib.check(rc)
    return ranked, score


def user_metrics(ranked, truth_ptr, truth_pos, truth_len):
    """fp64 [n_users][5] on the device: precision, recall, AP, RR, nDCG of every ranked list (src/bine_train.py:361-406).
    truth_ptr / truth_pos: CSR of the positions (in the item list) of each user's test items, ascending per user;
    truth_len[u] = len(test_rate[u]), which also counts test items outside the item list."""
    _require_gpu(ranked)
    dev = ranked.device
    n_users, k = ranked.shape
    tl = np.asarray(truth_len, dtype=np.int64)
    if tl.shape != (n_users,):
        raise ValueError("truth_len must have one entry per user")
    if n_users and tl.min() < 1:
        raise ZeroDivisionError("float division by zero")           # IDCG(0), src/bine_train.py:370
    ptr = np.asarray(truth_ptr, dtype=np.int64)
    pos = np.asarray(truth_pos, dtype=np.int32)
    if ptr.shape != (n_users + 1,) or ptr[0] != 0 or ptr[-1] != pos.shape[0] or np.any(np.diff(ptr) < 0):
        raise ValueError("truth_ptr is not a CSR row pointer over truth_pos")
    idcg = idcg_table(int(tl.max()))[tl]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_ptr, d_pos, d_len = to(ptr), to(pos if pos.size else np.zeros(1, np.int32)), to(tl.astype(np.int32))
    d_disc, d_idcg = to(discount_table(k)), to(idcg)
    out = torch.empty((n_users, 5), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().n2v_bine_rec_metrics(_lib.ptr(ranked.contiguous()), n_users, k, _lib.ptr(d_ptr), _lib.ptr(d_pos),
                                              _lib.ptr(d_len), _lib.ptr(d_disc), _lib.ptr(d_idcg), _lib.ptr(out),
                                              _lib.stream_ptr(dev))
    _lib.check(rc)
    return out


def averages(per_user):
    """(f1, map, mrr, ndcg) from the [n_users][5] array as the reference takes them (src/bine_train.py:352-358):
    Python's left-to-right sum(...) / len(...) in user order; F1 from the two means, 0.0 when both are 0."""
    cols = [per_user[:, j].tolist() for j in range(5)]
    n = len(cols[0])
    precison, recall, mean_ap, mrr, mndcg = (sum(c) / n for c in cols)
    f1 = 2 * precison * recall / (precison + recall) if precison + recall > 0 else 0.0
    return f1, mean_ap, mrr, mndcg


def evaluate(emb, dim, u_idx, v_idx, truth_ptr, truth_pos, truth_len, top_n):
    """top_N on the device: (f1, map, mrr, ndcg, per_user); per_user is the host copy of the [n_users][5] array."""
    ranked, _ = top_n_lists(emb, dim, u_idx, v_idx, top_n)
    per_user = user_metrics(ranked, truth_ptr, truth_pos, truth_len).cpu().numpy()
    return averages(per_user) + (per_user,)


# ------------------------------------------------------------------------------------------------ host side
def label_index(sorted_labels, labels):
    """Position of every label in the ascending array `sorted_labels`, -1 for a label that is not in it."""
    sorted_labels = np.asarray(sorted_labels)
    labels = np.asarray(labels)
    numeric = lambda x: x.dtype.kind in "iuf"
    if labels.size == 0 or sorted_labels.size == 0 or numeric(labels) != numeric(sorted_labels):
        return np.full(labels.shape, -1, dtype=np.int32)          # a string never equals a number as a dict key
    at = np.searchsorted(sorted_labels, labels)
    at_c = np.minimum(at, sorted_labels.size - 1)
    return np.where(sorted_labels[at_c] == labels, at_c, -1).astype(np.int32)


def unique_in_order(labels):
    """The labels without repeats, first occurrences in the order given: what the keys of the reference's
    recommend_dict[u] are when the item list repeats a label (src/bine_train.py:315,325)."""
    return list(dict.fromkeys(labels))


def truth_csr(test_u, test_v, test_rate):
    """(truth_ptr int64[n+1], truth_pos int32[], truth_len int64[n]) of the users `test_u` against the item list
    `test_v` (no repeated labels): per user the ascending positions in test_v of the keys of test_rate[u]; truth_len
    counts every key.  A user missing from test_rate raises KeyError, an empty test_rate[u] ZeroDivisionError, as in
    the reference."""
    test_u, test_v = list(test_u), list(test_v)
    if len(set(test_v)) != len(test_v):
        raise ValueError("the item list repeats a label; pass unique_in_order(test_v)")
    rates = [test_rate[u] for u in test_u]                         # KeyError as the reference (:335)
    lens = np.fromiter((len(r) for r in rates), dtype=np.int64, count=len(rates))
    if lens.size and lens.min() == 0:
        raise ZeroDivisionError("float division by zero")          # IDCG(0), src/bine_train.py:370
    keys = list(itertools.chain.from_iterable(rates))
    owner = np.repeat(np.arange(len(rates), dtype=np.int64), lens)
    if keys and test_v:
        va = np.asarray(test_v)
        order = np.argsort(va, kind="stable")
        at = label_index(va[order], np.asarray(keys))
        pos = np.where(at >= 0, order[np.maximum(at, 0)], -1)
    else:
        pos = np.full(len(keys), -1, dtype=np.int64)
    inside = pos >= 0
    owner, pos = owner[inside], pos[inside]
    by = np.lexsort((pos, owner))
    ptr = np.zeros(len(rates) + 1, dtype=np.int64)
    np.cumsum(np.bincount(owner, minlength=len(rates)), out=ptr[1:])
    return ptr, pos[by].astype(np.int32), lens
