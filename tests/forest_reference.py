"""The definition of the random forests of n2v_hip.forest (csrc/n2v_forest.hip), in numpy.  Every accumulated quantity is
an integer, so the kernels can equal this file bit for bit; the only rounded operations are the score of a split, the
leaf values and the averages, each in a stated order in fp64.

  bins       per feature, edges = the sorted distinct values but the first when there are at most n_bins of them, else the
             distinct values among xs[(b * n) // n_bins], b = 1 .. n_bins - 1, of the sorted column xs;  bin(x) = the number
             of edges <= x
  bootstrap  draw k of tree t is (word * n) >> 32 with word = philox4x32_10(seed; k lo, k hi, t, STREAM_BOOT)[0]; a sample's
             weight is the number of times it was drawn
  subsets    at node v of tree t feature j has the key philox4x32_10(seed; v, j, t, STREAM_FEAT)[0]; the max_features
             smallest keys are taken, equal keys by lower j
  growth     level by level, node ids breadth first, the children of a level's splitting nodes appended in node order;
             H[f][b][c] the integer sum of channel c over a node's samples with bin_f == b; (f, t) sends bin_f <= t left
  score      regressor   (S_L * S_L) / n_L + (S_R * S_R) / n_R  against  (S * S) / n
             classifier  -(((g(n_L) - s_L) + g(n_R)) - s_R)  against  -(g(n) - s), with s the sum of g(count of class c)
             from +0.0 in ascending c and g(a) = a * log(a) from a table, g(0) = 0
  choice     highest score, then lower feature, then lower bin t1; the stored threshold is the middle of the empty run after
             t1, (t1 + t_next - 1) // 2
  leaves     regressor (S / n) / 2^y_bits, classifier count_c / n; every node stores its value
"""
import math

import numpy as np

STREAM_BOOT = 0
STREAM_FEAT = 1
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(seed, c0, c1, c2, c3):
    """The four output words of Philox4x32-10 with key = seed (64 bits) and counter (c0, c1, c2, c3), as uint64 arrays of
    32-bit values; the counters broadcast.  Restated from csrc/n2v_common.h."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3)])
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def glog_table(length):
    """g(a) = a * log(a) for a < length by the host's libm log (Python's math.log), g(0) = 0."""
    return np.array([0.0] + [a * math.log(a) for a in range(1, int(length))], dtype=np.float64)


def resolve_max_features(max_features, n_features):
    """sklearn's reading of max_features: an int, a float share, "sqrt", "log2", or None for all."""
    F = int(n_features)
    if max_features is None:
        return F
    if isinstance(max_features, str):
        if max_features == "sqrt":
            return max(1, int(math.sqrt(F)))
        if max_features == "log2":
            return max(1, int(math.log2(F)))
        raise ValueError("max_features=%r: an int, a float share, 'sqrt', 'log2' or None" % (max_features,))
    if isinstance(max_features, (int, np.integer)) and not isinstance(max_features, bool):
        if not 1 <= max_features <= F:
            raise ValueError("max_features=%d outside 1 .. %d" % (max_features, F))
        return int(max_features)
    if isinstance(max_features, float) and 0.0 < max_features <= 1.0:
        return max(1, int(max_features * F))
    raise ValueError("max_features=%r: an int, a float share, 'sqrt', 'log2' or None" % (max_features,))


def bin_edges(X, n_bins):
    """A list of one fp64 edge array per feature."""
    X = np.asarray(X, dtype=np.float64)
    if np.isnan(X).any():
        raise ValueError("X holds a NaN")
    n = X.shape[0]
    out = []
    for j in range(X.shape[1]):
        xs = np.sort(X[:, j])
        u = np.unique(xs)
        if len(u) <= n_bins:
            out.append(u[1:])
        else:
            out.append(np.unique(xs[[(b * n) // n_bins for b in range(1, n_bins)]]))
    return out


def apply_bins(X, edges):
    X = np.asarray(X, dtype=np.float64)
    if np.isnan(X).any():
        raise ValueError("X holds a NaN")
    out = np.empty(X.shape, dtype=np.uint8)
    for j, e in enumerate(edges):
        out[:, j] = np.searchsorted(e, X[:, j], side="right")
    return out


def bootstrap_weights(seed, tree, n):
    k = np.arange(n, dtype=np.uint64)
    word = philox4x32_10(seed, k & _M32, k >> _S32, tree, STREAM_BOOT)[0]
    return np.bincount(((word * np.uint64(n)) >> _S32).astype(np.int64), minlength=n).astype(np.int32)


def feature_subset(seed, tree, node, n_features, m):
    j = np.arange(n_features, dtype=np.uint64)
    keys = philox4x32_10(seed, node, j, tree, STREAM_FEAT)[0]
    return np.sort(np.lexsort((j, keys))[:m])


def quantise(y, y_bits, n):
    y = np.asarray(y, dtype=np.float64)
    if not np.isfinite(y).all():
        raise ValueError("y holds a NaN or an infinity")
    yq = np.rint(y * 2.0 ** y_bits)
    if len(yq) and n * float(np.abs(yq).max()) >= 2.0 ** 53:
        raise ValueError("n * max|round(y * 2^y_bits)| reaches 2^53: lower y_bits (%d)" % y_bits)
    return yq.astype(np.int64)


def _best_regression(cnt, sm, msl):
    nL, SL = np.cumsum(cnt, 1)[:, :-1], np.cumsum(sm, 1)[:, :-1]
    n, S = cnt[0].sum(), sm[0].sum()
    nR, SR = n - nL, S - SL
    valid = (nL >= msl) & (nR >= msl)
    with np.errstate(divide="ignore", invalid="ignore"):
        sl, sr = SL.astype(np.float64), SR.astype(np.float64)
        score = (sl * sl) / nL.astype(np.float64) + (sr * sr) / nR.astype(np.float64)
    score[~valid] = -np.inf
    return score, (float(S) * float(S)) / float(n)


def _best_classification(cc, msl, g):
    cL = np.cumsum(cc, 1)[:, :-1, :]
    tot = cc[0].sum(0)
    cR = tot[None, None, :] - cL
    nL, n = cL.sum(2), int(tot.sum())
    nR = n - nL
    # sums over the classes in ascending order (cumsum adds one after the other; +0.0 + g is g)
    sL, sR, s = np.cumsum(g[cL], 2)[:, :, -1], np.cumsum(g[cR], 2)[:, :, -1], np.cumsum(g[tot])[-1]
    score = -(((g[nL] - sL) + g[nR]) - sR)
    score[~((nL >= msl) & (nR >= msl))] = -np.inf
    return score, -(g[n] - s)


def grow_tree(bins, n_bins, w, target, n_classes, tree, seed, max_depth, min_samples_split, min_samples_leaf, m_features,
              y_bits, g):
    """One tree.  target: int64 yq (regressor, n_classes == 0) or class numbers.  Returns the flat tables
    feature / threshold / left (-1 at a leaf; the right child is left + 1), value and level_ptr."""
    n, F = bins.shape
    K = int(n_classes)
    feature, threshold, left, value, level_ptr = [], [], [], [], [0]
    frontier, depth = [np.flatnonzero(w > 0)], 0
    cols = np.arange(F, dtype=np.int64)[None, :] * n_bins
    while frontier:
        first, splits = len(feature), []
        for m, idx in enumerate(frontier):
            v = first + m
            wn, b = w[idx].astype(np.int64), bins[idx].astype(np.int64)
            count = int(wn.sum())
            if K:
                tot = np.bincount(target[idx], weights=wn, minlength=K).astype(np.int64)
                value.append(tot.astype(np.float64) / float(count))
            else:
                value.append((float(int((wn * target[idx]).sum())) / float(count)) / 2.0 ** y_bits)
            feature.append(-1), threshold.append(-1), left.append(-1)
            if depth == max_depth or count < min_samples_split:
                continue
            feats = feature_subset(seed, tree, v, F, m_features) if m_features < F else np.arange(F)
            Fs = len(feats)                                  # unselected features are never scored: skip their histograms
            flat = (cols[:, :Fs] + b[:, feats]).ravel()
            if K:
                flat = flat * K + np.repeat(target[idx], Fs)
                cc = np.bincount(flat, weights=np.repeat(wn, Fs), minlength=Fs * n_bins * K).astype(np.int64).reshape(Fs, n_bins, K)
                score, parent = _best_classification(cc, min_samples_leaf, g)
                occupied = cc.sum(2) > 0
            else:
                cnt = np.bincount(flat, weights=np.repeat(wn, Fs), minlength=Fs * n_bins).astype(np.int64).reshape(Fs, n_bins)
                sm = np.bincount(flat, weights=np.repeat(wn * target[idx], Fs), minlength=Fs * n_bins).astype(np.int64).reshape(Fs, n_bins)
                score, parent = _best_regression(cnt, sm, min_samples_leaf)
                occupied = cnt > 0
            if score.shape[1] == 0:
                continue
            at = int(np.argmax(score))                       # the first maximum: lower feature, then lower bin
            fi, t1 = divmod(at, n_bins - 1)
            if not score[fi, t1] > parent:                   # -inf: no valid split
                continue
            t_next = t1 + 1 + int(np.argmax(occupied[fi, t1 + 1:]))
            feature[v], threshold[v] = int(feats[fi]), (t1 + t_next - 1) // 2
            splits.append((v, idx))
        nxt = []
        for v, idx in splits:
            left[v] = first + len(frontier) + len(nxt)
            go = bins[idx, feature[v]] <= threshold[v]
            nxt += [idx[go], idx[~go]]
        frontier, depth = nxt, depth + 1
        level_ptr.append(len(feature))
    value = np.array(value, dtype=np.float64).reshape(len(feature), K if K else 1)
    return dict(feature=np.array(feature, np.int32), threshold=np.array(threshold, np.int32), left=np.array(left, np.int32),
                value=value, level_ptr=np.array(level_ptr, np.int64))


def tree_leaves(tree, bins):
    """The leaf each row of bins ends in."""
    node = np.zeros(bins.shape[0], dtype=np.int64)
    rows = np.arange(bins.shape[0])
    while True:
        l = tree["left"][node]
        go = l >= 0
        if not go.any():
            return node
        f = np.where(go, tree["feature"][node], 0)
        right = bins[rows, f] > tree["threshold"][node]
        node = np.where(go, l + right, node)


class Forest:
    """fit / predict / predict_proba / score of the definition.  kind: "regressor" or "classifier"."""

    def __init__(self, kind, n_estimators=None, max_depth=16, min_samples_split=2, min_samples_leaf=1, max_features="default",
                 bootstrap=True, n_bins=256, y_bits=20, seed=0):
        assert kind in ("regressor", "classifier")
        self.kind = kind
        self.n_estimators = (100 if kind == "regressor" else 50) if n_estimators is None else n_estimators
        self.max_features = (1.0 if kind == "regressor" else "sqrt") if max_features == "default" else max_features
        self.max_depth, self.min_samples_split, self.min_samples_leaf = max_depth, min_samples_split, min_samples_leaf
        self.bootstrap, self.n_bins, self.y_bits, self.seed = bootstrap, n_bins, y_bits, seed

    def fit(self, X, y):
        X = np.asarray(X, dtype=np.float64)
        n, F = X.shape
        self.edges = bin_edges(X, self.n_bins)
        self.bins = apply_bins(X, self.edges)
        if self.kind == "classifier":
            self.classes_, target = np.unique(np.asarray(y), return_inverse=True)
            target, K = target.astype(np.int64).ravel(), len(self.classes_)
            if not 2 <= K <= 32:
                raise ValueError("%d classes: 2 .. 32" % K)
        else:
            target, K = quantise(y, self.y_bits, n), 0
        m = resolve_max_features(self.max_features, F)
        g = glog_table(n + 1) if K else None
        self.weights, self.trees = [], []
        for t in range(self.n_estimators):
            w = bootstrap_weights(self.seed, t, n) if self.bootstrap else np.ones(n, dtype=np.int32)
            self.weights.append(w)
            self.trees.append(grow_tree(self.bins, self.n_bins, w, target, K, t, self.seed, self.max_depth, self.min_samples_split,
                                        self.min_samples_leaf, m, self.y_bits, g))
        return self

    def _average(self, X):
        bins = apply_bins(X, self.edges)
        acc = np.zeros((bins.shape[0], self.trees[0]["value"].shape[1]))
        for tree in self.trees:
            acc = acc + tree["value"][tree_leaves(tree, bins)]
        return acc / float(len(self.trees))

    def predict(self, X):
        avg = self._average(X)
        return avg[:, 0] if self.kind == "regressor" else self.classes_[np.argmax(avg, axis=1)]

    def predict_proba(self, X):
        assert self.kind == "classifier"
        return self._average(X)

    def score(self, X, y):
        return r2_score(y, self.predict(X)) if self.kind == "regressor" else accuracy(y, self.predict(X))


def _seq_sum(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.cumsum(a)[-1]) if len(a) else 0.0


def r2_score(y, pred):
    """1 - u / v with sequential sums; with v == 0, 1 when u == 0 else 0 (sklearn's convention)."""
    y, pred = np.asarray(y, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    mean = _seq_sum(y) / float(len(y))
    u, v = _seq_sum((y - pred) * (y - pred)), _seq_sum((y - mean) * (y - mean))
    if v == 0.0:
        return 1.0 if u == 0.0 else 0.0
    return 1.0 - u / v


def accuracy(y, pred):
    return float(int((np.asarray(y) == np.asarray(pred)).sum())) / float(len(pred))
