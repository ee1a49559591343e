"""TEST INFRASTRUCTURE — float64 numpy restatement of the similarity + selection kernels of csrc/n2v_sim.hip
(C-ABI include/n2v_sim.h), one plain function per exported kernel, plus the forward error bounds the GPU tests
hold the kernels to.  tests/test_gpu_sim_exact.py compares the device with these; tests/test_sim_host.py compares
these with the per-pair functions of oracle/augment_oracle.py.  The product never imports this file.

Zero vectors under "cos": gensim's matutils.unitvec returns a vector of norm 0 unchanged, so its similarity with
anything is 0, not NaN (include/n2v_sim.h "COS x / sqrt(sum x^2) (gensim matutils.unitvec)"; the comment in
sim_prepare_kernel: "a zero row stays zero (similarity 0), not NaN").  gensim is not installed beside this
project, so that is taken from those two places."""
import numpy as np

COS, PEARSON, JSD = 0, 1, 2
METHODS = {"cos": COS, "pearson": PEARSON, "jsd": JSD}
U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): n successive fp32 roundings perturb a value by at most this, relatively."""
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def dpad_of(dim):
    return -(-int(dim) // 32) * 32


# ------------------------------------------------------------------------------------------------ prepare
def prepare(vec, dim, rows, method):
    """n2v_sim_prepare: vec fp32 [n_src, stride >= dim], rows None or an index array -> float64 [n_rows, dpad]."""
    method = METHODS.get(method, method)
    vec = np.asarray(vec)
    src = vec if rows is None else vec[np.asarray(rows, dtype=np.int64)]
    x = src[:, :dim].astype(np.float64)
    out = np.zeros((x.shape[0], dpad_of(dim)), dtype=np.float64)
    with np.errstate(all="ignore"):
        if method == COS:
            nrm = np.sqrt((x * x).sum(axis=1, keepdims=True))
            out[:, :dim] = np.where(nrm > 0, x / np.where(nrm > 0, nrm, 1.0), x)     # unitvec: a zero row stays as it is
        elif method == PEARSON:
            xm = x - x.mean(axis=1, keepdims=True)
            out[:, :dim] = xm / np.sqrt((xm * xm).sum(axis=1, keepdims=True))
        elif method == JSD:
            out[:, :dim] = x / x.sum(axis=1, keepdims=True)
        else:
            raise ValueError(method)
    return out


def prepare_bound(vec, dim, rows, method):
    """Absolute error bound per element of the fp32 kernel's prepared rows against prepare(), [n_rows, dim].
    Counted from the kernel's rounded operations (any summation order):
      cos      s2 = sum of dim rounded squares: relative error gamma(dim); its sqrt halves that and rounds once; the
               reciprocal and the product round once each:  rel = gamma(dim)/2 + gamma(3) + their product.
      jsd      s = sum of dim terms: |s^ - s| <= gamma(dim - 1) sum|x|, i.e. relative g = gamma(dim-1) sum|x| / |s|;
               one rounded division:  rel = g/(1-g) + u + their product.
      pearson  mean^ = fl(s^/dim) is off by e, |e| <= gamma(dim) mean|x| (sum, then one division).  Every centred entry
               moves by e: the row gains a component e * ones of length t = |e| sqrt(dim) / |x - mean| relative to the
               centred norm — t is gamma(dim) times the conditioning factor mean|x| sqrt(dim) / |x - mean| (mean|x| >=
               |mean|: the sum's error scales with sum|x|).  With o = (x-mean)/|x-mean|:
                   o^_k = (c_k - e) / (|c| sqrt(1 + t^2)) (1 + rho),
               rho = gamma(dim)/2 (norm) + gamma(4) (subtraction, sqrt, division, squares) + product, hence
                   |o^_k - o_k| <= tau + (|o_k| + tau) (rho + t^2/2),  tau = t / sqrt(dim)."""
    method = METHODS.get(method, method)
    vec = np.asarray(vec)
    src = vec if rows is None else vec[np.asarray(rows, dtype=np.int64)]
    x = src[:, :dim].astype(np.float64)
    want = prepare(vec, dim, rows, method)[:, :dim]
    with np.errstate(all="ignore"):
        if method == COS:
            a, b = gamma(dim) / 2, gamma(3)
            return (a + b + a * b) * np.abs(want)
        if method == JSD:
            g = gamma(dim - 1) * np.abs(x).sum(axis=1, keepdims=True) / np.abs(x.sum(axis=1, keepdims=True))
            g = g / (1 - g)
            return (g + U + g * U) * np.abs(want)
        xm = x - x.mean(axis=1, keepdims=True)
        cn = np.sqrt((xm * xm).sum(axis=1, keepdims=True))
        t = gamma(dim) * np.abs(x).mean(axis=1, keepdims=True) * np.sqrt(dim) / cn
        tau = t / np.sqrt(dim)
        a, b = gamma(dim) / 2, gamma(4)
        rho = a + b + a * b
        return tau + (np.abs(want) + tau) * (rho + t * t / 2)


# ------------------------------------------------------------------------------------------------ block
def rel_entr(x, y):
    """scipy.special.rel_entr's case split: x log(x/y) for x, y > 0; 0 for x == 0, y >= 0; NaN propagates; else +inf."""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    out = np.full(x.shape, np.inf)
    pos = (x > 0) & (y > 0)
    with np.errstate(all="ignore"):
        out[pos] = x[pos] * np.log(x[pos] / y[pos])
    out[(x == 0) & (y >= 0)] = 0.0
    out[np.isnan(x) | np.isnan(y)] = np.nan
    return out


def block(PA, PB, method, row_begin=0, n_rows=None, zero_diag_off=-1):
    """n2v_sim_block on prepared rows (any float type, used as float64): rows [row_begin, row_begin + n_rows) of PA
    against all rows of PB -> float64 [n_rows, n_cols]; (r, r + zero_diag_off) set to 0 when zero_diag_off >= 0."""
    method = METHODS.get(method, method)
    PA, PB = np.asarray(PA, dtype=np.float64), np.asarray(PB, dtype=np.float64)
    n_rows = PA.shape[0] - row_begin if n_rows is None else n_rows
    A = PA[row_begin:row_begin + n_rows]
    if method == JSD:
        out = np.empty((n_rows, PB.shape[0]))
        with np.errstate(all="ignore"):
            for i in range(n_rows):
                m = (A[i][None, :] + PB) / 2
                out[i] = ((rel_entr(A[i][None, :], m) + rel_entr(PB, m)) / 2).sum(axis=1)
    else:
        with np.errstate(all="ignore"):
            out = A @ PB.T
    if zero_diag_off >= 0:
        for i in range(n_rows):
            c = row_begin + i + zero_diag_off
            if c < PB.shape[0]:
                out[i, c] = 0.0
    return out


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def dot_bound(PA, PB, row_begin=0, n_rows=None):
    """|fp32 dot in ANY summation order - exact dot| <= gamma(dpad) sum_k |a_k||b_k|, plus one fp32 ulp of the exact
    value (the float64 reference is compared after the device's final rounding)."""
    PA, PB = np.abs(np.asarray(PA, dtype=np.float64)), np.abs(np.asarray(PB, dtype=np.float64))
    n_rows = PA.shape[0] - row_begin if n_rows is None else n_rows
    A = PA[row_begin:row_begin + n_rows]
    return gamma(PA.shape[1]) * (A @ PB.T)


JSD_C = 8   # see jsd_bound


def jsd_bound(PA, PB, row_begin=0, n_rows=None):
    """JSD_C u sum_k (p|log(p/m)| + q|log(q/m)| + p + q) per score, finite scores only (others: NaN/inf there).
    JSD_C = 8 counts, in units of u = 2^-24 (one rounding): logf allowed 2 ulp = 4u; the division x/y 1; the product
    x * log 1; the halving, with the rounded sum m = (p+q)/2 it stands for, 1; the accumulation 1.  The |log| terms
    carry the relative errors of the log and the product, the p + q terms the absolute error of the log that a
    relatively perturbed argument (division, m) causes."""
    PA, PB = np.asarray(PA, dtype=np.float64), np.asarray(PB, dtype=np.float64)
    n_rows = PA.shape[0] - row_begin if n_rows is None else n_rows
    A = PA[row_begin:row_begin + n_rows]
    out = np.empty((n_rows, PB.shape[0]))
    with np.errstate(all="ignore"):
        for i in range(n_rows):
            p = A[i][None, :]
            m = (p + PB) / 2
            out[i] = (np.abs(rel_entr(p, m)) + np.abs(rel_entr(PB, m)) + np.abs(p) + np.abs(PB)).sum(axis=1)
    return JSD_C * U * out


def score_bound(PA, PB, method, row_begin=0, n_rows=None):
    method = METHODS.get(method, method)
    return (jsd_bound if method == JSD else dot_bound)(PA, PB, row_begin, n_rows)


# ------------------------------------------------------------------------------------------------ global top-k
def topk_scan(S, tau, excl_keys, upper, row_begin):
    """n2v_sim_topk_scan: S = scores of rows [row_begin, row_begin + S.shape[0]) x all columns.  The SET of
    (row, col, score) with score > tau, key row * n_cols + col not excluded and, if upper, col > row."""
    n_cols = S.shape[1]
    excl = set(int(k) for k in (excl_keys if excl_keys is not None else ()))
    out = set()
    for i in range(S.shape[0]):
        r = row_begin + i
        for c in range(n_cols):
            s = S[i, c]
            if not (s > tau) or (upper and c <= r) or (r * n_cols + c) in excl:
                continue
            out.add((r, c, float(s)))
    return out


def global_topk(S, k, excl_keys, upper):
    """simsel.global_topk: the k best candidates of the full score matrix by (score desc, row, col) as a list of
    (score, row, col)."""
    cand = sorted(topk_scan(S, -np.inf, excl_keys, upper, 0), key=lambda t: (-t[2], t[0], t[1]))
    return [(s, r, c) for r, c, s in cand[:k]]


# ------------------------------------------------------------------------------------------------ row selection
def rows_count(scores, thre):
    return np.array([sum(1 for v in row if v > thre) for row in scores], dtype=np.int64)


def rows_fill(scores, thre):
    """(offsets, cols, vals): per row the columns with score > thre in column order, rows concatenated."""
    counts = rows_count(scores, thre)
    off = np.concatenate([[0], np.cumsum(counts)])[:-1]
    cols = [c for row in scores for c, v in enumerate(row) if v > thre]
    vals = [v for row in scores for v in row if v > thre]
    return off.astype(np.int64), np.array(cols, dtype=np.int32), np.array(vals, dtype=np.float32)


def rows_topk(scores, k):
    """n2v_sim_rows_topk, literally: sorted(enumerate(row), key=-score)[:k] per row, NaN first replaced by -inf
    ("NaN ranks lowest").  Python's sort is stable and compares -0.0 == +0.0.  Returns the column lists."""
    out = []
    for row in scores:
        row = [float("-inf") if v != v else float(v) for v in row]
        out.append([c for c, _ in sorted(enumerate(row), key=lambda t: -t[1])[:k]])
    return out


def order_key_select(row, k):
    """The radix select of rows_topk_kernel as first written: key = bits with the sign bit set for non-negative
    floats, all bits flipped for negative ones (so -0.0 < +0.0), NaN -> 0; everything above the k-th largest key,
    plus the first ties of it in column order.  Only tests/test_sim_host.py uses it, to show that a case separates
    this order from rows_topk's."""
    row = np.asarray(row, dtype=np.float32)
    u = row.view(np.uint32).astype(np.uint64)
    key = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    key = np.where(np.isnan(row), 0, key)
    if k == 0:
        return []
    T = np.sort(key)[::-1][k - 1]
    need_eq = k - int((key > T).sum())
    eq = np.nonzero(key == T)[0][:need_eq]
    return sorted(np.nonzero(key > T)[0].tolist() + eq.tolist())
