"""Nearest neighbours of embedding rows on the device: the host side of csrc/n2v_knn.hip (include/n2v_sim.h,
n2v_sim_knn) and what ``KeyedVectors.most_similar`` and ``find_similar_users`` (src/utils.py:428-442) run on.

Two paths give the same arrays: "fused" forms the scores tile by tile and keeps only every query's running best-k list
(k <= 256, nothing of size n_q x n_cols is stored); "block" is the stored score block of simsel.score_block followed by
n2v_sim_rows_topk, for any k.  A pair's score has the same bits on both (one device function forms it), and both rank by
the order of csrc/n2v_rank.h: higher score first, equal scores by lower index, NaN below everything, -0.0 ties +0.0.
torch holds the buffers and reorders the few selected entries; every score and every selection is made by the HIP
kernels.  No CPU path."""
import math
import random

import numpy as np
import torch

from . import _lib, simsel

MAX_K_FUSED = 256            # N2V_SIM_KNN_MAX_K
QUERY_BLOCK = 8192           # queries per call: bounds the scratch (fused) and the stored score block (block)
BLOCK_SCORES = 1 << 28       # most scores the block path stores at once (1 GiB of fp32)
ITEM_PREFIX = "9999999"      # the reference's item labels (src/utils.py:422)
# path="auto": per-query cost of the two paths, constants measured on one MI355X (tools/knn_probe.py)
INSERT_SECONDS = 0.36e-9     # one list insertion of the fused kernel, amortised over a full grid
TILE_FLOPS = 1.0e14          # rate of the shared MFMA tile loop
BLOCK_SECONDS = 1.2e-11      # one stored score of the block path: written once, read by the selection


def _require_gpu(what):
    if not torch.cuda.is_available():
        raise RuntimeError("n2v_hip: %s needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback" % what)


def _rank_key(vals):
    """n2v_rank.h's order_key of fp32 scores as int64: larger score <=> larger key, NaN lowest, -0.0 and +0.0 equal."""
    u = vals.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)
    key = torch.where(vals == 0, torch.full_like(key, 0x80000000), key)
    return torch.where(torch.isnan(vals), torch.zeros_like(key), key)


def _fused(Q, B, k, excl, method, n_seg, cols, vals):
    lib = _lib.load()
    n_q = int(Q.shape[0])
    nbytes = int(lib.n2v_sim_knn_scratch(n_q, k, n_seg))
    if nbytes < 0:
        raise ValueError("knn: k %d or n_seg %d outside the fused kernel's range" % (k, n_seg))
    scratch = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=Q.device)
    _lib.check(lib.n2v_sim_knn(_lib.ptr(Q), n_q, _lib.ptr(B), int(B.shape[0]), int(Q.shape[1]), simsel.METHODS[method],
                               _lib.ptr(excl), k, n_seg, _lib.ptr(scratch), _lib.ptr(cols), _lib.ptr(vals),
                               _lib.stream_ptr(Q.device)))


def _block(Q, B, k, excl, method, cols, vals):
    """score_block + n2v_sim_rows_topk select the SET of the k (+ 1 where a column may have to go) best of every row;
    here it is put into rank order, the excluded column leaves, and what is missing becomes (-1, NaN)."""
    lib = _lib.load()
    n_q, n_cols = int(Q.shape[0]), int(B.shape[0])
    cols.fill_(-1)
    vals.fill_(float("nan"))
    kk = min(k + (0 if excl is None else 1), n_cols)
    if kk == 0:
        return
    scores = simsel.score_block(Q, 0, n_q, B, method)
    sc = torch.empty((n_q, kk), dtype=torch.int32, device=Q.device)
    sv = torch.empty((n_q, kk), dtype=torch.float32, device=Q.device)
    _lib.check(lib.n2v_sim_rows_topk(_lib.ptr(scores), n_q, n_cols, int(scores.stride(0)), kk, _lib.ptr(sc), _lib.ptr(sv),
                                     _lib.stream_ptr(Q.device)))
    # the set arrives in column order, so a stable descending sort by key leaves equal scores in column order
    o = torch.sort(_rank_key(sv), dim=1, descending=True, stable=True).indices
    sc, sv = torch.gather(sc, 1, o), torch.gather(sv, 1, o)
    if excl is not None:
        gone = sc == excl[:, None]
        o = torch.sort(gone.to(torch.int8), dim=1, stable=True).indices          # the excluded column last, the rest as ranked
        sc, sv, gone = torch.gather(sc, 1, o), torch.gather(sv, 1, o), torch.gather(gone, 1, o)
        sc = torch.where(gone, torch.full_like(sc, -1), sc)
        sv = torch.where(gone, torch.full_like(sv, float("nan")), sv)
    n = min(k, kk)
    cols[:, :n] = sc[:, :n]
    vals[:, :n] = sv[:, :n]


def auto_path(n_q, n_cols, k, dpad, cus=256):
    """What path="auto" takes.  The fused kernel pays for its tiles and for every insertion into its 2 * n_seg partial
    lists a query: k to fill a list, then about k * ln(c / k) replacements in a stream of c candidates in random order;
    the block path pays for every stored score.  The cheaper estimate wins; k > 256 is always "block"."""
    if k > MAX_K_FUSED:
        return "block"
    row_blocks = max(1, -(-min(n_q, QUERY_BLOCK) // 128))
    lists = 2 * min(32, max(1, -(-3 * cus // row_blocks)))          # csrc/n2v_knn.hip resolve_seg
    per_list = max(1.0, n_cols / lists)
    inserts = lists * k * (1.0 + math.log(max(1.0, per_list / k)))
    fused = inserts * INSERT_SECONDS + 2.0 * n_cols * dpad / TILE_FLOPS
    return "fused" if fused < n_cols * BLOCK_SECONDS else "block"


def knn_prepared(Q, B, k, exclude=None, method="cos", path="auto", n_seg=0, query_block=QUERY_BLOCK):
    """Q: fp32 [n_q, dpad], B: fp32 [n_cols, dpad], both as simsel.prepare returns them; exclude: None or an integer
    tensor [n_q] (an entry outside 0 .. n_cols - 1 excludes nothing).  Returns (idx int32 [n_q, k], score fp32 [n_q, k])
    in rank order, (-1, NaN) where the candidates ran out."""
    if not (Q.is_cuda and B.is_cuda):
        raise RuntimeError("n2v_hip: knn needs device tensors; there is no CPU fallback")
    k, query_block = int(k), int(query_block)
    n_q, n_cols = int(Q.shape[0]), int(B.shape[0])
    if method not in ("cos", "pearson"):
        raise ValueError("knn: method %r is not a dot product ('cos', 'pearson')" % (method,))
    if path not in ("auto", "fused", "block"):
        raise ValueError("knn: path %r, expected 'auto', 'fused' or 'block'" % (path,))
    if k < 1 or query_block < 1:
        raise ValueError("knn: k and query_block must be at least 1")
    if Q.dim() != 2 or B.dim() != 2 or Q.shape[1] != B.shape[1]:
        raise ValueError("knn: prepared operands of shapes %s and %s" % (tuple(Q.shape), tuple(B.shape)))
    if path == "auto":
        path = auto_path(n_q, n_cols, k, int(Q.shape[1]), torch.cuda.get_device_properties(Q.device).multi_processor_count)
    if path == "fused" and k > MAX_K_FUSED:
        raise ValueError("knn: the fused path keeps at most %d neighbours, k = %d" % (MAX_K_FUSED, k))
    if path == "block" and n_cols > 0:
        query_block = max(1, min(query_block, BLOCK_SCORES // n_cols))
    dev = Q.device
    excl = None if exclude is None else exclude.to(device=dev, dtype=torch.int32).contiguous()
    if excl is not None and excl.shape != (n_q,):
        raise ValueError("knn: %d exclude entries for %d queries" % (excl.numel(), n_q))
    cols = torch.empty((n_q, k), dtype=torch.int32, device=dev)
    vals = torch.empty((n_q, k), dtype=torch.float32, device=dev)
    Q, B = Q.contiguous(), B.contiguous()
    with torch.cuda.device(dev):
        for b in range(0, n_q, query_block):
            e = min(n_q, b + query_block)
            ex = None if excl is None else excl[b:e]
            if path == "fused":
                _fused(Q[b:e], B, k, ex, method, int(n_seg), cols[b:e], vals[b:e])
            else:
                _block(Q[b:e], B, k, ex, method, cols[b:e], vals[b:e])
    return cols, vals


def knn(vectors, k, queries=None, method="cos", exclude_self=None, path="auto", n_seg=0, query_block=QUERY_BLOCK):
    """The k nearest rows of `vectors` (fp32 device tensor [n, d]) for every query, by "cos" or "pearson".
    queries: None (every row queries all rows; exclude_self defaults to True), an integer tensor of row numbers
    (exclude_self defaults to False) or a separate fp32 [n_q, d] tensor (nothing can be excluded).
    path: "fused" (k <= 256), "block" (any k) or "auto" (auto_path: the cheaper by a measured cost estimate — fused for
    large matrices and small k); both give identical arrays.
    Returns (idx int32 [n_q, k], score fp32 [n_q, k]) on the device, in rank order; (-1, NaN) where fewer than k
    candidates exist."""
    if not vectors.is_cuda:
        raise RuntimeError("n2v_hip: knn needs device tensors; there is no CPU fallback")
    B = simsel.prepare(vectors, method)
    n = int(B.shape[0])
    if queries is None:
        Q = B
        excl = torch.arange(n, dtype=torch.int32, device=B.device) if exclude_self in (None, True) else None
    elif not torch.is_floating_point(queries):
        idx = queries.to(device=B.device, dtype=torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise ValueError("knn: a query index outside 0 .. %d" % (n - 1))
        Q = B[idx]
        excl = idx.to(torch.int32) if exclude_self else None
    else:
        if exclude_self:
            raise ValueError("knn: exclude_self needs queries that are rows of `vectors` (None or an index tensor)")
        if queries.dim() != 2 or queries.shape[1] != vectors.shape[1]:
            raise ValueError("knn: queries of shape %s for vectors of shape %s" % (tuple(queries.shape), tuple(vectors.shape)))
        Q = simsel.prepare(queries.to(B.device), method)
        excl = None
    return knn_prepared(Q, B, k, excl, method, path, n_seg, query_block)


# ---------------------------------------------------------------------------------------------- gensim's most_similar
def _as_list(x):
    if x is None:
        return []
    if isinstance(x, (str, bytes, np.ndarray)) or not isinstance(x, (list, tuple)):
        return [x]
    return list(x)


def query_terms(positive, negative):
    """[(weight, word or ndarray)] in list order, positives (+1) then negatives (-1); a bare word or vector is one
    positive.  ValueError when there is nothing."""
    terms = [(1.0, t) for t in _as_list(positive)] + [(-1.0, t) for t in _as_list(negative)]
    if not terms:
        raise ValueError("cannot compute similarity with no input")
    return terms


def mean_query(weighted_rows):
    """gensim's query vector, restated: acc = w0 * x0; acc = acc + wi * xi ...; acc / float32(count), all in float32."""
    acc = None
    for w, x in weighted_rows:
        t = np.float32(w) * np.asarray(x, dtype=np.float32)
        acc = t if acc is None else acc + t
    return (acc / np.float32(len(weighted_rows))).astype(np.float32)


class SimilarityIndex:
    """The unit rows of a KeyedVectors on the device (KeyedVectors.init_sims) and the queries against them."""

    def __init__(self, kv, device="cuda:0"):
        _require_gpu("most_similar")
        self.device = torch.device(device)
        self.dim = int(kv.syn0.shape[1])
        self.prepared = simsel.prepare(torch.from_numpy(kv.syn0).to(self.device), "cos")

    def unit_row(self, index):
        return self.prepared[index, :self.dim].cpu().numpy()

    def query(self, vector):
        """fp32 [1, dpad]: the host vector uploaded and passed through the device's own normalisation."""
        v = torch.from_numpy(np.ascontiguousarray(vector, dtype=np.float32).reshape(1, -1)).to(self.device)
        if v.shape[1] != self.dim:
            raise ValueError("most_similar: a vector of length %d, the vocabulary's are %d long" % (v.shape[1], self.dim))
        return simsel.prepare(v, "cos")


def most_similar(kv, positive=None, negative=None, topn=10, restrict_vocab=None):
    """gensim 3.x KeyedVectors.most_similar restated from memory (parity with gensim itself is UNPINNED): the mean of
    the positive (+1) and negative (-1) terms — a word contributes its unit row, an ndarray itself as given — is
    compared by cosine with the first `restrict_vocab` words; the input words are dropped and the `topn` best returned as
    [(label, float(score))] in n2v_rank.h's order.  topn=None: the fp32 score of every word (numpy)."""
    terms = query_terms(positive, negative)
    for _, t in terms:
        if not isinstance(t, np.ndarray) and t not in kv.vocab:
            raise KeyError("word %r not in vocabulary" % (t,))
    if topn is not None and int(topn) < 1:
        return []
    ix = kv.init_sims()
    words = [kv.vocab[t].index for _, t in terms if not isinstance(t, np.ndarray)]
    rows = [(w, t if isinstance(t, np.ndarray) else ix.unit_row(kv.vocab[t].index)) for w, t in terms]
    Q = ix.query(mean_query(rows))
    n = len(kv.index2word)
    limit = n if restrict_vocab is None else max(0, min(int(restrict_vocab), n))
    B = ix.prepared[:limit]
    if topn is None:
        if limit == 0:
            return np.empty(0, dtype=np.float32)
        return simsel.score_block(Q, 0, 1, B, "cos")[0].cpu().numpy()
    idx, score = knn_prepared(Q, B, int(topn) + len(words), method="cos")
    idx, score = idx[0].cpu().numpy(), score[0].cpu().numpy()
    drop = set(words)
    out = [(kv.index2word[i], float(s)) for i, s in zip(idx.tolist(), score) if i >= 0 and i not in drop]
    return out[:int(topn)]


# ---------------------------------------------------------------------------------------------- find_similar_users
def find_similar_users(wv_or_emb_path, ratio, target=None, seed=None, device="cuda:0"):
    """src/utils.py:428-442: the int(ratio * n_users) users nearest to `target` by cosine, the target included, in rank
    order.  Users are the labels that do not start with '9999999', in file (or vocabulary) order; target defaults to
    random.Random(seed).choice of them.  DEVIATION: the scores are the device's fp32 cosines and equal scores go by
    list order; the reference takes scipy's fp64 cosine of the parsed text and a stable sort of the same list."""
    if isinstance(wv_or_emb_path, (str, bytes)) or hasattr(wv_or_emb_path, "__fspath__"):
        from . import io as _io
        words, vecs = _io.load_word2vec_format(wv_or_emb_path)
    else:
        words, vecs = wv_or_emb_path.index2word, wv_or_emb_path.syn0
    pos = [i for i, w in enumerate(words) if not str(w).startswith(ITEM_PREFIX)]
    users = [str(words[i]) for i in pos]
    if not users:
        raise ValueError("find_similar_users: no user among %d labels" % len(words))
    target = random.Random(seed).choice(users) if target is None else str(target)
    if target not in users:
        raise KeyError("find_similar_users: user %r is not in the embedding" % (target,))
    n = int(ratio * float(len(users)))
    if n < 1:
        return []
    _require_gpu("find_similar_users")
    v = torch.from_numpy(np.ascontiguousarray(np.asarray(vecs, dtype=np.float32)[pos])).to(torch.device(device))
    q = torch.tensor([users.index(target)], dtype=torch.int64)
    idx, _ = knn(v, n, queries=q, method="cos", exclude_self=False)
    return [users[i] for i in idx[0].cpu().tolist() if i >= 0]
