"""Random forests on binned features (include/n2v_sim.h, n2v_forest_*): the regressor and the entropy
classifier of src/main_ecc.py:160-202 on the rows consistency.features builds.

The forest is defined by tests/forest_reference.py, in which every accumulated quantity is an integer: fp64 features go to
uint8 bins, a tree grows level by level from integer histograms, and a split's score is computed from them in a stated fp64
order.  The tables a fit gives equal that file's bit for bit, and two fits give the same bytes.  Deviations from sklearn
(binned thresholds, max_depth 16 by default, min_samples_leaf counted in draws, y rounded to 2^-y_bits, Philox streams) are
listed in DESIGN.md 4.24.  There is no CPU fallback: every step is a HIP kernel, but for the sorts and scans in between.
"""
import json
import math
import time

import numpy as np
import torch

from . import _lib

MAX_FEATURES, MAX_BINS, MAX_CLASSES, MAX_DEPTH = 4096, 256, 32, 32
BAD_NAN, BAD_BIN, BAD_CLASS, BAD_FEATURE, BAD_CHILD, BAD_TARGET = 1, 2, 4, 8, 16, 32
DEFAULT_HIST_BUDGET = 256 << 20
TABLES = ("feature", "threshold", "left", "value", "tree_ptr", "edges", "n_edges")


def feature_tile(n_bins, n_classes=0):
    """Features per histogram workgroup (n_classes 0: the regressor)."""
    return int(_lib.load().n2v_forest_feature_tile(int(n_bins), int(n_classes)))


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
    elif isinstance(max_features, (int, np.integer)) and not isinstance(max_features, bool):
        if 1 <= max_features <= F:
            return int(max_features)
        raise ValueError("max_features=%d outside 1 .. %d" % (max_features, F))
    elif isinstance(max_features, float) and 0.0 < max_features <= 1.0:
        return max(1, int(max_features * F))
    raise ValueError("max_features=%r: an int, a float share in (0, 1], 'sqrt', 'log2' or None" % (max_features,))


def _status(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def check_limits(n, n_features, n_bins, n_classes, max_depth):
    """The limits of the kernels, refused before anything is allocated."""
    if not 1 <= n < 2 ** 31:
        raise ValueError("n=%d rows: 1 .. 2^31 - 1" % n)
    if not 1 <= n_features <= MAX_FEATURES:
        raise ValueError("%d features: 1 .. %d" % (n_features, MAX_FEATURES))
    if not 2 <= n_bins <= MAX_BINS:
        raise ValueError("n_bins=%d: 2 .. %d" % (n_bins, MAX_BINS))
    if n_classes and not 2 <= n_classes <= MAX_CLASSES:
        raise ValueError("%d classes: 2 .. %d" % (n_classes, MAX_CLASSES))
    if not 0 <= max_depth <= MAX_DEPTH:
        raise ValueError("max_depth=%d: 0 .. %d" % (max_depth, MAX_DEPTH))


def check_bins(bins, n_bins):
    """ValueError if a bin of the uint8 device tensor is >= n_bins."""
    dev = _lib.call_device("forest.check_bins", "bins", bins)
    p = _lib.tensor("forest.check_bins", "bins", bins, torch.uint8, dev)
    st = _status(dev)
    _lib.check(_lib.load().n2v_forest_check_bins(p, bins.numel(), int(n_bins), st.data_ptr(), _lib.stream_ptr(dev)))
    if int(st.item()) & BAD_BIN:
        raise ValueError("a bin is >= n_bins (%d)" % n_bins)


def check_classes(cls, n_classes):
    """ValueError if a class number of the int32 device tensor lies outside 0 .. n_classes - 1."""
    dev = _lib.call_device("forest.check_classes", "cls", cls)
    p = _lib.tensor("forest.check_classes", "cls", cls, torch.int32, dev)
    st = _status(dev)
    _lib.check(_lib.load().n2v_forest_check_classes(p, cls.numel(), int(n_classes), st.data_ptr(), _lib.stream_ptr(dev)))
    if int(st.item()) & BAD_CLASS:
        raise ValueError("a class number lies outside 0 .. %d" % (n_classes - 1))


def check_tables(trees, n_features, n_bins, width):
    """ValueError, naming the cause, unless the flat tables are those of well-formed trees: shapes and tree_ptr on the host,
    every node's feature, threshold and child index by one kernel.  Runs before any launch that trusts them."""
    fn = "forest.check_tables"
    dev = _lib.call_device(fn, "feature", trees["feature"])
    tree_ptr = trees["tree_ptr"]
    _lib.tensor(fn, "tree_ptr", tree_ptr, torch.int64, dev, (None,))
    n_trees = tree_ptr.numel() - 1
    tp = tree_ptr.cpu().tolist()
    if n_trees < 1 or tp[0] != 0 or any(b - a < 1 for a, b in zip(tp, tp[1:])) or tp[-1] >= 2 ** 31:
        raise ValueError("tree_ptr does not describe trees of at least one node each")
    N = tp[-1]
    ptrs = [_lib.tensor(fn, k, trees[k], torch.int32, dev, N) for k in ("feature", "threshold", "left")]
    _lib.tensor(fn, "value", trees["value"], torch.float64, dev, (N, width))
    _lib.tensor(fn, "edges", trees["edges"], torch.float64, dev, (n_features, n_bins - 1))
    _lib.tensor(fn, "n_edges", trees["n_edges"], torch.int32, dev, n_features)
    ne = trees["n_edges"].cpu()
    if int(ne.min()) < 0 or int(ne.max()) > n_bins - 1:
        raise ValueError("a feature has more than n_bins - 1 edges: its bins would reach n_bins (%d)" % n_bins)
    st = _status(dev)
    _lib.check(_lib.load().n2v_forest_check_tree(ptrs[0], ptrs[1], ptrs[2], tree_ptr.data_ptr(), n_trees, N, int(n_features),
                                                 int(n_bins), st.data_ptr(), _lib.stream_ptr(dev)))
    bad = int(st.item())
    if bad & BAD_FEATURE:
        raise ValueError("a node names a feature outside 0 .. %d" % (n_features - 1))
    if bad & BAD_CHILD:
        raise ValueError("a child index lies outside its tree or not after its parent")
    if bad & BAD_BIN:
        raise ValueError("a threshold bin lies outside 0 .. %d" % (n_bins - 1))


def _as_device(a, dtype, dev):
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a, dtype={torch.float64: np.float64}[dtype]), device=dev)


def _seq_sum(a):
    return float(np.cumsum(a)[-1]) if len(a) else 0.0


class _Forest:
    _classifier = False

    def __init__(self, n_estimators, max_depth, min_samples_split, min_samples_leaf, max_features, bootstrap, n_bins, y_bits, seed,
                 device, hist_budget_bytes):
        if n_estimators < 1:
            raise ValueError("n_estimators=%d: at least 1" % n_estimators)
        if min_samples_leaf < 1 or min_samples_split < 0:
            raise ValueError("min_samples_leaf=%d (at least 1), min_samples_split=%d (at least 0)" % (min_samples_leaf, min_samples_split))
        if not 0 <= y_bits <= 52:
            raise ValueError("y_bits=%d: 0 .. 52" % y_bits)
        if hist_budget_bytes < 1:
            raise ValueError("hist_budget_bytes=%d: at least 1" % hist_budget_bytes)
        check_limits(1, 1, n_bins, 0, max_depth)
        self.n_estimators, self.max_depth, self.min_samples_split = int(n_estimators), int(max_depth), int(min_samples_split)
        self.min_samples_leaf, self.max_features, self.bootstrap = int(min_samples_leaf), max_features, bool(bootstrap)
        self.n_bins, self.y_bits, self.seed = int(n_bins), int(y_bits), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device, self.hist_budget_bytes = torch.device(device), int(hist_budget_bytes)
        self.trees_, self.timing_ = None, None

    def _tick(self, stage, level):
        """tools/forest_probe.py sets timing_ = {} to split a fit's time by (stage, level); it costs a synchronisation per stage."""
        if self.timing_ is not None:
            torch.cuda.synchronize(self.device)
            now = time.perf_counter()
            self.timing_[(stage, level)] = self.timing_.get((stage, level), 0.0) + now - self.timing_.get("_last", now)
            self.timing_["_last"] = now

    # ---- fit ----------------------------------------------------------------------------------------------------------------

    def _features(self, X):
        if not (isinstance(X, torch.Tensor) or isinstance(X, np.ndarray)):
            X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X must be [n, features], got %s" % (tuple(X.shape),))
        return X

    def bin_features(self, X):
        """uint8[n, F] bins of X by the fitted edges; a NaN is a ValueError."""
        lib, dev, t = _lib.load(), self.device, self.trees_
        X = self._features(X)
        check_limits(X.shape[0], X.shape[1], self.n_bins, 0, self.max_depth)
        if X.shape[1] != self.n_features_:
            raise ValueError("X has %d features, the model %d" % (X.shape[1], self.n_features_))
        X = _as_device(X, torch.float64, dev)
        bins, st = torch.empty(X.shape, dtype=torch.uint8, device=dev), _status(dev)
        _lib.check(lib.n2v_forest_bin(X.data_ptr(), X.shape[0], X.shape[1], self.n_bins, t["edges"].data_ptr(), t["n_edges"].data_ptr(),
                                      bins.data_ptr(), st.data_ptr(), _lib.stream_ptr(dev)))
        if int(st.item()) & BAD_NAN:
            raise ValueError("X holds a NaN")
        return bins

    def fit(self, X, y):
        lib, dev = _lib.load(), self.device
        if dev.type != "cuda":
            raise RuntimeError("the forests run on a GPU (device=%s); there is no CPU fallback" % dev)
        X = self._features(X)
        n, F = int(X.shape[0]), int(X.shape[1])
        if len(y) != n:
            raise ValueError("X has %d rows, y %d" % (n, len(y)))
        target, K = self._target_host(y)
        check_limits(n, F, self.n_bins, K, self.max_depth)
        m_features = resolve_max_features(self.max_features, F)
        stream = _lib.stream_ptr(dev)
        X = _as_device(X, torch.float64, dev)
        st = _status(dev)
        _lib.check(lib.n2v_forest_check_x(X.data_ptr(), n * F, st.data_ptr(), stream))
        if int(st.item()) & BAD_NAN:
            raise ValueError("X holds a NaN")
        xs = torch.sort(X.t().contiguous(), dim=1).values
        edges = torch.zeros((F, self.n_bins - 1), dtype=torch.float64, device=dev)
        n_edges = torch.empty(F, dtype=torch.int32, device=dev)
        _lib.check(lib.n2v_forest_edges(xs.data_ptr(), n, F, self.n_bins, edges.data_ptr(), n_edges.data_ptr(), stream))
        del xs
        self.n_features_, self.trees_ = F, {"edges": edges, "n_edges": n_edges}
        bins = self.bin_features(X)
        check_bins(bins, self.n_bins)
        yq, cls = self._target_device(target, n, K)
        gtab = None
        if K:
            gtab = torch.empty(n + 1, dtype=torch.float64)
            _lib.check(lib.n2v_forest_glog_table(n + 1, gtab.data_ptr()))
            gtab = gtab.to(dev)
        self.n_classes_, self.bins_, self.weights_ = K, bins, []
        parts, level_ptrs = [], []
        w = torch.ones(n, dtype=torch.int32, device=dev)
        for t in range(self.n_estimators):
            if self.bootstrap:
                w = torch.empty(n, dtype=torch.int32, device=dev)
                _lib.check(lib.n2v_forest_bootstrap(self.seed, t, n, w.data_ptr(), stream))
            self.weights_.append(w)
            tables, level_ptr = self._grow(bins, w, yq, cls, K, t, m_features, gtab)
            parts.append(tables)
            level_ptrs.append(level_ptr)
        sizes = [p[0].numel() for p in parts]
        self.trees_.update({k: torch.cat([p[i] for p in parts]) for i, k in enumerate(("feature", "threshold", "left", "value"))})
        self.trees_["tree_ptr"] = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
        self.level_ptr_ = level_ptrs
        return self

    def _grow(self, bins, w, yq, cls, K, t, m_features, gtab):
        lib, dev, stream = _lib.load(), self.device, _lib.stream_ptr(self.device)
        n, F = bins.shape
        nb, width = self.n_bins, (K if K else 1)
        cap = min(2 ** (self.max_depth + 1) - 1, 2 * n - 1)
        i32 = dict(dtype=torch.int32, device=dev)
        feature, threshold, left = (torch.full((cap,), -1, **i32) for _ in range(3))
        value = torch.zeros((cap, width), dtype=torch.float64, device=dev)
        order, seg = torch.arange(n, **i32), torch.tensor([0, n], **i32)
        first, L, depth, level_ptr = 0, 1, 0, [0]
        ptr = _lib.ptr
        while True:
            leaf_only = depth == self.max_depth
            f_count = 1 if leaf_only else F
            node_bytes = f_count * nb * (4 * K if K else 16)
            batch = max(1, self.hist_budget_bytes // node_bytes)
            seg_host = seg.cpu().tolist()
            n_pos = seg_host[L]
            split = torch.empty(L, **i32)
            self._tick("other", depth)
            for node0 in range(0, L, batch):
                node1 = min(L, node0 + batch)
                nodes = node1 - node0
                hist = torch.empty(nodes * node_bytes, dtype=torch.uint8, device=dev)
                _lib.check(lib.n2v_forest_hist(bins.data_ptr(), n, F, f_count, nb, K, order.data_ptr(), seg.data_ptr(), node0, node1,
                                               seg_host[node1] - seg_host[node0], w.data_ptr(), ptr(yq), ptr(cls), hist.data_ptr(), stream))
                self._tick("hist", depth)
                key_limit = None
                if m_features < F and not leaf_only:
                    keys = torch.empty((nodes, F), dtype=torch.int64, device=dev)
                    _lib.check(lib.n2v_forest_feature_keys(self.seed, t, first + node0, nodes, F, keys.data_ptr(), stream))
                    key_limit = torch.sort(keys, dim=1).values[:, m_features - 1].contiguous()
                best_score = torch.empty((nodes, f_count), dtype=torch.float64, device=dev)
                best_thr = torch.empty((nodes, f_count), **i32)
                node_count = torch.empty(nodes, dtype=torch.int64, device=dev)
                node_parent = torch.empty(nodes, dtype=torch.float64, device=dev)
                _lib.check(lib.n2v_forest_split(hist.data_ptr(), nodes, f_count, nb, K, self.min_samples_split, self.min_samples_leaf,
                                                int(leaf_only), ptr(gtab), 0 if gtab is None else gtab.numel(), self.seed, t,
                                                first + node0, ptr(key_limit), self.y_bits, best_score.data_ptr(), best_thr.data_ptr(),
                                                node_count.data_ptr(), node_parent.data_ptr(), feature.data_ptr(), threshold.data_ptr(),
                                                left.data_ptr(), value.data_ptr(), split[node0:].data_ptr(), stream))
                self._tick("split", depth)
            level_ptr.append(first + L)
            if leaf_only:
                break
            rank = torch.cumsum(split, 0, dtype=torch.int32)
            n_split = int(rank[-1].item())
            if n_split == 0:
                break
            if first + L + 2 * n_split > cap:
                raise RuntimeError("forest: a tree outgrew its tables")     # cannot happen: a leaf holds at least one sample
            flags = torch.empty((2, n_pos), **i32)
            _lib.check(lib.n2v_forest_route_flags(bins.data_ptr(), n, F, order.data_ptr(), seg.data_ptr(), L, n_pos, split.data_ptr(),
                                                  feature.data_ptr(), threshold.data_ptr(), first, flags.data_ptr(), stream))
            sums = torch.cumsum(flags, 1, dtype=torch.int32)
            n_next = int(sums[0, -1].item()) + int(sums[1, -1].item())
            new_order, new_seg = torch.empty(n_next, **i32), torch.empty(2 * n_split + 1, **i32)
            _lib.check(lib.n2v_forest_route_scatter(order.data_ptr(), seg.data_ptr(), L, n_pos, split.data_ptr(), rank.data_ptr(),
                                                    flags.data_ptr(), sums.data_ptr(), first, first + L, n_split, n_next, left.data_ptr(),
                                                    new_order.data_ptr(), new_seg.data_ptr(), stream))
            self._tick("route", depth)
            first, L, order, seg, depth = first + L, 2 * n_split, new_order, new_seg, depth + 1
        N = first + L
        return (feature[:N].clone(), threshold[:N].clone(), left[:N].clone(), value[:N].clone()), np.array(level_ptr, dtype=np.int64)

    # ---- predict ------------------------------------------------------------------------------------------------------------

    def _check_fitted(self):
        if self.trees_ is None or "feature" not in self.trees_:
            raise RuntimeError("the forest is not fitted")

    def predict_bins(self, bins):
        """The averaged leaf values fp64[n, width] of uint8[n, F] bins; bins and tables are checked first."""
        self._check_fitted()
        lib, dev, t = _lib.load(), self.device, self.trees_
        width = self.n_classes_ if self.n_classes_ else 1
        _lib.tensor("forest.predict_bins", "bins", bins, torch.uint8, dev, (None, self.n_features_))
        check_limits(bins.shape[0], self.n_features_, self.n_bins, self.n_classes_, self.max_depth)
        check_bins(bins, self.n_bins)
        check_tables(t, self.n_features_, self.n_bins, width)
        out = torch.empty((bins.shape[0], width), dtype=torch.float64, device=dev)
        _lib.check(lib.n2v_forest_predict(bins.data_ptr(), bins.shape[0], self.n_features_, t["feature"].data_ptr(),
                                          t["threshold"].data_ptr(), t["left"].data_ptr(), t["value"].data_ptr(), t["tree_ptr"].data_ptr(),
                                          t["tree_ptr"].numel() - 1, width, self.max_depth, out.data_ptr(), _lib.stream_ptr(dev)))
        return out

    def _average(self, X):
        self._check_fitted()
        return self.predict_bins(self.bin_features(X))

    # ---- save / load ----------------------------------------------------------------------------------------------------------

    def _params(self):
        return dict(n_estimators=self.n_estimators, max_depth=self.max_depth, min_samples_split=self.min_samples_split,
                    min_samples_leaf=self.min_samples_leaf, bootstrap=self.bootstrap, n_bins=self.n_bins, y_bits=self.y_bits,
                    seed=self.seed)

    def save(self, path):
        self._check_fitted()
        arrays = {k: self.trees_[k].cpu().numpy() for k in TABLES}
        arrays.update({"param_" + k: np.array(v) for k, v in self._params().items()})
        arrays["kind"] = np.array(type(self).__name__)
        arrays["n_classes"] = np.array(self.n_classes_)
        arrays["max_features"] = np.array(json.dumps(self.max_features))
        if self._classifier:
            arrays["classes"] = np.asarray(self.classes_)
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    @classmethod
    def load(cls, path, device="cuda:0"):
        with np.load(path, allow_pickle=False) as z:
            if str(z["kind"]) != cls.__name__:
                raise ValueError("%s holds a %s, not a %s" % (path, z["kind"], cls.__name__))
            params = {k[6:]: z[k].item() for k in z.files if k.startswith("param_")}
            self = cls(device=device, **params)
            self.max_features = json.loads(str(z["max_features"]))
            dev = self.device
            kinds = dict(feature=torch.int32, threshold=torch.int32, left=torch.int32, value=torch.float64, tree_ptr=torch.int64,
                         edges=torch.float64, n_edges=torch.int32)
            for k in TABLES:
                if torch.from_numpy(z[k]).dtype != kinds[k]:
                    raise ValueError("%s: table %s is %s, not %s" % (path, k, z[k].dtype, str(kinds[k]).replace("torch.", "")))
            self.trees_ = {k: torch.from_numpy(np.ascontiguousarray(z[k])).to(dev) for k in TABLES}
            self.n_classes_ = int(z["n_classes"])
            if self._classifier:
                self.classes_ = z["classes"]
        if self.trees_["edges"].dim() != 2 or self.trees_["edges"].shape[1] != self.n_bins - 1:
            raise ValueError("%s: edges must be [features, n_bins - 1]" % path)
        self.n_features_ = int(self.trees_["edges"].shape[0])
        check_limits(1, self.n_features_, self.n_bins, self.n_classes_, self.max_depth)
        if bool(self.n_classes_) != self._classifier or (self._classifier and len(self.classes_) != self.n_classes_):
            raise ValueError("%s: %d classes do not go with a %s" % (path, self.n_classes_, cls.__name__))
        check_tables(self.trees_, self.n_features_, self.n_bins, self.n_classes_ if self.n_classes_ else 1)
        return self


class RandomForestRegressor(_Forest):
    """sklearn's RandomForestRegressor (squared error) as defined in tests/forest_reference.py.  fit / predict / score take numpy
    arrays or device tensors; predict answers in kind.  .trees_ holds the flat tables on the device."""

    def __init__(self, n_estimators=100, max_depth=16, min_samples_split=2, min_samples_leaf=1, max_features=1.0, bootstrap=True,
                 n_bins=256, y_bits=20, seed=0, device="cuda:0", hist_budget_bytes=DEFAULT_HIST_BUDGET):
        super().__init__(n_estimators, max_depth, min_samples_split, min_samples_leaf, max_features, bootstrap, n_bins, y_bits, seed,
                         device, hist_budget_bytes)

    def _target_host(self, y):
        return y, 0

    def _target_device(self, y, n, K):
        lib, dev = _lib.load(), self.device
        y = _as_device(y if isinstance(y, torch.Tensor) else np.asarray(y, dtype=np.float64).ravel(), torch.float64, dev).reshape(-1)
        yq, top, st = torch.empty(n, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), _status(dev)
        _lib.check(lib.n2v_forest_quantise(y.data_ptr(), n, self.y_bits, yq.data_ptr(), top.data_ptr(), st.data_ptr(), _lib.stream_ptr(dev)))
        if int(st.item()) & BAD_TARGET:
            raise ValueError("y holds a NaN, an infinity or a value whose round(y * 2^y_bits) reaches 2^53: lower y_bits (%d)" % self.y_bits)
        if n * int(top.item()) >= 2 ** 53:
            raise ValueError("n * max|round(y * 2^y_bits)| reaches 2^53: lower y_bits (%d)" % self.y_bits)
        return yq, None

    def predict(self, X):
        out = self._average(X)[:, 0].contiguous()
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def score(self, X, y):
        """R^2 = 1 - u / v with sequential fp64 sums; with v == 0, 1 when u == 0 else 0 (sklearn's convention)."""
        pred = self.predict(X)
        pred = pred.cpu().numpy() if isinstance(pred, torch.Tensor) else pred
        y = (y.cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)).astype(np.float64).ravel()
        mean = _seq_sum(y) / float(len(y))
        u, v = _seq_sum((y - pred) * (y - pred)), _seq_sum((y - mean) * (y - mean))
        if v == 0.0:
            return 1.0 if u == 0.0 else 0.0
        return 1.0 - u / v


class RandomForestClassifier(_Forest):
    """sklearn's RandomForestClassifier(criterion="entropy") as defined in tests/forest_reference.py.  Labels are numbered in
    sorted order (classes_); 2 .. 32 classes."""
    _classifier = True

    def __init__(self, n_estimators=50, max_depth=16, min_samples_split=2, min_samples_leaf=1, max_features="sqrt", bootstrap=True,
                 n_bins=256, y_bits=20, seed=0, device="cuda:0", hist_budget_bytes=DEFAULT_HIST_BUDGET, criterion="entropy"):
        if criterion != "entropy":
            raise ValueError("criterion=%r: only 'entropy' is built" % (criterion,))
        super().__init__(n_estimators, max_depth, min_samples_split, min_samples_leaf, max_features, bootstrap, n_bins, y_bits, seed,
                         device, hist_budget_bytes)

    def _target_host(self, y):
        if isinstance(y, torch.Tensor):
            classes, inverse = torch.unique(y.reshape(-1), sorted=True, return_inverse=True)
            self.classes_ = classes.cpu().numpy()
        else:
            self.classes_, inverse = np.unique(np.asarray(y).ravel(), return_inverse=True)
        return inverse, len(self.classes_)

    def _target_device(self, inverse, n, K):
        cls = (inverse if isinstance(inverse, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(inverse))).to(
            device=self.device, dtype=torch.int32).contiguous()
        check_classes(cls, K)
        return None, cls

    def predict_proba(self, X):
        out = self._average(X)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def predict(self, X):
        """The first maximum of the averaged probabilities, as a label of classes_ (a numpy array)."""
        proba = self._average(X)
        best = torch.empty(proba.shape[0], dtype=torch.int32, device=self.device)
        _lib.check(_lib.load().n2v_forest_argmax(proba.data_ptr(), proba.shape[0], self.n_classes_, best.data_ptr(),
                                                 _lib.stream_ptr(self.device)))
        return self.classes_[best.cpu().numpy()]

    def score(self, X, y):
        """Accuracy."""
        pred = self.predict(X)
        y = y.cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        return float(int((y.ravel() == pred).sum())) / float(len(pred))
