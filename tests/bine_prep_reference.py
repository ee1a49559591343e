"""TEST INFRASTRUCTURE — numpy fp64 restatements of the BiNE preparation kernels of csrc/n2v_bine.hip in the kernels' own
operation order, so that they match bit for bit (the library is built with -ffp-contract=off, and fp64 division and
square root are correctly rounded on both sides), and a replay of every kernel's loads and stores with each index
asserted inside the array that is actually passed (tests/test_bine_prep_host.py runs it for every case of
tests/bine_prep_cases.py before tests/test_gpu_bine_prep.py launches that case).

The integer kernels (walk lengths, walks, pools) are restated by oracle/bine_oracle.py; the replays here follow the
kernels' text instead (their binary searches, their loops), so the two also check each other.

`variant` plants an error, for the host test to show that the comparison would notice it:
  "plain_sum"   a left-to-right sum instead of lane-strided partial sums and the xor butterfly (spmv, init)
  "inf_starts"  walk counts: -inf / +inf instead of the reference's start values 0.0 / 100000.0
  "floor1"      walk counts: floor + 1 instead of ceil
  "divide"      normalise: h / mh instead of h * (1 / mh)
  "swap_words"  init: Philox words 2/3 for even columns and 0/1 for odd ones
  "norm_dim"    init: the norm from the sum of squares over the first `dim` elements in plain order"""
import math

import numpy as np

from oracle import bine_oracle as bo

LANES = np.arange(64)
BLOCK = 1024


# ------------------------------------------------------------------------------------------ fp64 building blocks
def butterfly(s):
    """wave_sum_n: s[..., lane] += s[..., lane ^ M] for M = 32, 16, 8, 4, 2, 1; every lane ends with the total."""
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[..., LANES ^ m]
    return s[..., 0]


def lane_strided_sum(p):
    """p: [..., k] terms of one row in ascending k.  Lane l adds terms l, l + 64, ... in that order from 0.0 (absent
    terms add +0.0, which changes no bit of a sum that started at +0.0), then the butterfly."""
    k = p.shape[-1]
    pad = (-k) % 64
    if pad:
        p = np.concatenate([p, np.zeros(p.shape[:-1] + (pad,))], axis=-1)
    p = p.reshape(p.shape[:-1] + (-1, 64))
    s = np.zeros(p.shape[:-2] + (64,))
    for c in range(p.shape[-2]):
        s = s + p[..., c, :]
    return butterfly(s)


def plain_sum(p):
    return np.cumsum(p, axis=-1)[..., -1] if p.shape[-1] else np.zeros(p.shape[:-1])


def block_reduce(v, is_max):
    """block_reduce over the 1024 slots of one workgroup: the halving tree."""
    sm = np.array(v, dtype=np.float64)
    assert sm.shape == (BLOCK,)
    s = BLOCK >> 1
    while s > 0:
        sm[:s] = np.fmax(sm[:s], sm[s:2 * s]) if is_max else sm[:s] + sm[s:2 * s]
        s >>= 1
    return sm[0]


def _per_thread(x, fill):
    """x[i] laid out as [trip][thread] for i = t, t + 1024, ...; absent elements hold `fill`."""
    pad = (-len(x)) % BLOCK
    return np.concatenate([x, np.full(pad, fill)]).reshape(-1, BLOCK)


# ------------------------------------------------------------------------------------------ HITS
class SpmvPlan:
    """Gather indices of one CSR, built once: entry [r][c][l] is CSR position row_ptr[r] + 64 c + l, or -1."""

    def __init__(self, row_ptr, col, w):
        self.n = len(row_ptr) - 1
        deg = np.diff(row_ptr)
        chunks = max(1, int(-(-int(deg.max() if self.n else 0) // 64)))
        k = np.arange(chunks * 64)
        idx = row_ptr[:-1, None] + k[None, :]
        self.mask = k[None, :] < deg[:, None]
        self.idx = np.where(self.mask, idx, 0)
        self.col = np.asarray(col)
        self.w = np.asarray(w)

    def __call__(self, x, variant=None):
        p = np.where(self.mask, self.w[self.idx] * x[self.col[self.idx]], 0.0)
        return plain_sum(p) if variant == "plain_sum" else lane_strided_sum(p)


def spmv(row_ptr, col, w, x, variant=None):
    return SpmvPlan(row_ptr, col, w)(x, variant)


def hits_normalise(h, a, h_last, variant=None):
    """-> (h', a', err): hits_normalise_kernel."""
    mh = np.zeros(BLOCK)
    ma = np.zeros(BLOCK)
    for hr, ar in zip(_per_thread(h, -np.inf), _per_thread(a, -np.inf)):
        mh = np.fmax(mh, hr)
        ma = np.fmax(ma, ar)
    mh, ma = block_reduce(mh, True), block_reduce(ma, True)
    with np.errstate(divide="ignore", invalid="ignore"):
        if variant == "divide":
            hv, av = h / mh, a / ma
        else:
            hv, av = h * (1.0 / mh), a * (1.0 / ma)
    err = np.zeros(BLOCK)
    for d in _per_thread(np.abs(hv - h_last), 0.0):
        err = err + d
    return hv, av, block_reduce(err, False)


def hits(row_ptr, col, w, max_iter=100, tol=1.0e-8, variant=None):
    """BineEngine.calculate_centrality in the kernels' order -> (authority, iterations)."""
    n = len(row_ptr) - 1
    plan = SpmvPlan(row_ptr, col, w)
    h = np.full(n, 1.0 / n)
    for it in range(max_iter):
        a = plan(h, variant)
        hn = plan(a, variant)
        h, a, err = hits_normalise(hn, a, h, variant)
        if err < tol:
            return a, it + 1
    raise RuntimeError("HITS: power iteration failed to converge in %d iterations" % max_iter)


def walk_counts(a, lo, hi, maxT, minT, variant=None):
    """walk_counts_kernel on a[lo:hi] -> (counts int32, scaled fp64), both of length hi - lo."""
    seg = np.asarray(a[lo:hi], dtype=np.float64)
    mx = np.full(BLOCK, -np.inf if variant == "inf_starts" else 0.0)
    mn = np.full(BLOCK, np.inf if variant == "inf_starts" else 100000.0)
    for r in _per_thread(seg, np.nan):          # fmax / fmin skip a NaN operand: an absent element changes nothing
        mx = np.fmax(mx, r)
        mn = np.fmin(mn, r)
    mx = block_reduce(mx, True)
    mn = -block_reduce(-mn, True)
    span = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (seg - mn) / span if span != 0.0 else np.zeros(len(seg))
    c = np.floor(float(maxT) * s) + 1.0 if variant == "floor1" else np.ceil(float(maxT) * s)
    return np.maximum(c.astype(np.int32), np.int32(minT)), s


# ------------------------------------------------------------------------------------------ init
def init_uniforms(n, dim, seed, variant=None):
    """x[table][row][c], c < dim: Philox counter (row, row >> 32, c >> 1, table); words 0/1 for even c, 2/3 for odd."""
    x = np.zeros((2, n, dim))
    for t in range(2):
        for r in range(n):
            for q in range((dim + 1) // 2):
                w = bo._philox(seed, r, r >> 32, q, t)
                pair = (bo._u53(w[0], w[1]), bo._u53(w[2], w[3]))
                if variant == "swap_words":
                    pair = pair[::-1]
                x[t, r, 2 * q] = pair[0]
                if 2 * q + 1 < dim:
                    x[t, r, 2 * q + 1] = pair[1]
    return x


def init_tables(x, row_stride, variant=None):
    """bine_init_kernel from its uniforms x[2][n][dim] -> (emb, ctx), each [n][row_stride] with zero padding."""
    dim = x.shape[2]
    out = np.zeros(x.shape[:2] + (row_stride,))
    out[..., :dim] = x
    if variant == "norm_dim":
        ss = plain_sum(x * x)
    elif variant == "plain_sum":
        ss = plain_sum(out * out)
    else:
        ss = lane_strided_sum(out * out)
    out[..., :dim] = x / np.sqrt(ss)[..., None]
    return out[0], out[1]


# ------------------------------------------------------------------------------------------ bounds replay
class Checked:
    """An array as a kernel sees it: every index must lie inside it."""

    def __init__(self, name, a):
        self.name, self.a, self.n = name, np.asarray(a), len(a)
        self.touched = 0

    def ok(self, i):
        i = np.asarray(i)
        if i.size:
            assert int(i.min()) >= 0 and int(i.max()) < self.n, \
                "%s[%d..%d] outside its %d elements" % (self.name, int(i.min()), int(i.max()), self.n)
            self.touched += i.size
        return i

    def __getitem__(self, i):
        return self.a[self.ok(i)]

    def __setitem__(self, i, v):
        self.a[self.ok(i)] = v


def replay_spmv(n_rows, row_ptr, col, w, x, y):
    row_ptr, col, w, x, y = (Checked(k, v) for k, v in (("row_ptr", row_ptr), ("col", col), ("w", w), ("x", x), ("y", y)))
    r = np.arange(n_rows)
    b, e = row_ptr[r], row_ptr[r + 1]
    assert (e >= b).all()
    k = np.concatenate([np.arange(bb, ee) for bb, ee in zip(b, e)]) if n_rows else np.zeros(0, np.int64)
    w.ok(k)
    x.ok(col[k])
    y.ok(r)


def replay_normalise(n, h, a, h_last, state):
    for name, v in (("h", h), ("a", a), ("h_last", h_last)):
        Checked(name, v).ok(np.arange(n))
    Checked("state", state).ok(0)


def replay_walk_counts(a, lo, hi, counts, auth_out):
    i = np.arange(lo, hi)
    Checked("a", a).ok(i)
    Checked("counts", counts).ok(i)
    if auth_out is not None:
        Checked("auth_out", auth_out).ok(i)


def replay_init(emb, ctx, n, dim, row_stride):
    assert 1 <= dim <= row_stride and row_stride % 64 == 0
    i = (np.arange(n)[:, None] * row_stride + np.arange(row_stride)[None, :]).ravel()
    Checked("emb", emb).ok(i)
    Checked("ctx", ctx).ok(i)


def replay_walk_lengths(row_ptr, cum2, walk_node, n_walks, lens):
    row_ptr, cum2, walk_node, lens = (Checked(k, v) for k, v in
                                      (("row_ptr", row_ptr), ("cum2", cum2), ("walk_node", walk_node), ("lens", lens)))
    i = np.arange(n_walks)
    node = walk_node[i].astype(np.int64)
    cum2.ok(row_ptr[node])
    cum2.ok(row_ptr[node + 1])
    lens.ok(i)


def replay_walk(row_ptr, col, cum2, walk_node, walk_off, n_walks, gw_base, seed, tokens, blocks=None):
    """bine_walk_kernel as written (its binary searches, its wave-wide search element by element), every load and
    store checked; fills `tokens` and returns the number of grid-stride trips beyond the first."""
    row_ptr, col, cum2, walk_node, walk_off, tokens = (Checked(k, v) for k, v in (
        ("row_ptr", row_ptr), ("col", col), ("cum2", cum2), ("walk_node", walk_node), ("walk_off", walk_off),
        ("tokens", tokens)))
    blocks = min((n_walks + 3) // 4, 8192) if blocks is None else blocks
    for i in range(n_walks):
        gw = gw_base + i
        off = int(walk_off[i])
        length = int(walk_off[i + 1]) - off
        cur = int(walk_node[i])
        tokens[off] = cur
        for t in range(length - 1):
            rb, re = int(row_ptr[cur]), int(row_ptr[cur + 1])
            base = int(cum2[rb])
            paths = int(cum2[re]) - base
            nxt = cur
            for trial in range(bo.MAX_TRIALS):
                r = bo._philox(seed, gw, gw >> 32, t, 1 + trial)
                pick = int(math.floor(bo._u53(r[0], r[1]) * float(paths)))
                if pick >= paths:
                    pick = paths - 1
                lo, hi = rb, re - 1
                while lo < hi:
                    mid = (lo + hi) >> 1
                    if int(cum2[mid + 1]) - base > pick:
                        hi = mid
                    else:
                        lo = mid + 1
                mid_v = int(col[lo])
                w = int(col[int(row_ptr[mid_v]) + (pick - (int(cum2[lo]) - base))])
                if w == cur:
                    continue
                nxt = w
                wb = int(row_ptr[w])
                plo, phi = 0, int(row_ptr[w + 1]) - wb
                while plo < phi:
                    pm = (plo + phi) >> 1
                    if int(col[wb + pm]) < mid_v:
                        plo = pm + 1
                    else:
                        phi = pm
                if not _any_common(col, rb, lo - rb, wb, plo):
                    break
            else:
                raise AssertionError("walk %d step %d: no proposal kept in %d trials" % (i, t, bo.MAX_TRIALS))
            cur = nxt
            tokens[off + t + 1] = cur
    return max(0, -(-n_walks // (4 * blocks)) - 1)


def _sorted_hits(col, a_lo, a_n, b_lo, b_n):
    """How many of col[a_lo : a_lo + a_n] occur in col[b_lo : b_lo + b_n], by the kernels' lower-bound search."""
    if a_n > b_n:
        a_lo, a_n, b_lo, b_n = b_lo, b_n, a_lo, a_n
    cnt = 0
    for i in range(a_n):
        x = int(col[a_lo + i])
        lo, hi = 0, b_n
        while lo < hi:
            mid = (lo + hi) >> 1
            if int(col[b_lo + mid]) < x:
                lo = mid + 1
            else:
                hi = mid
        cnt += lo < b_n and int(col[b_lo + lo]) == x
    return cnt


def _any_common(col, a_lo, a_n, b_lo, b_n):
    # the kernel stops at the first 64-element round with a hit: it reads no index that this full count does not
    return _sorted_hits(col, a_lo, a_n, b_lo, b_n) > 0


def replay_neg_pools(row_ptr, col, side_lo, side_hi, v_begin, v_end, pool_size, max_jaccard, seed, pool):
    """neg_pool_kernel as written, every load and store checked; fills `pool` (flat, row 0 = v_begin)."""
    assert 0 <= side_lo < side_hi and side_lo <= v_begin <= v_end <= side_hi and pool_size >= 1
    row_ptr, col, pool = Checked("row_ptr", row_ptr), Checked("col", col), Checked("pool", pool)
    side_n = side_hi - side_lo
    for v in range(v_begin, v_end):
        vb = int(row_ptr[v])
        vn = int(row_ptr[v + 1]) - vb
        for s in range(pool_size):
            c = v
            for trial in range(bo.POOL_TRIALS + 1):
                r = bo._philox(seed, v, s, trial, 0)
                k = int(math.floor(bo._u53(r[0], r[1]) * float(side_n)))
                if k >= side_n:
                    k = side_n - 1
                c = side_lo + k
                if c == v:
                    continue
                if trial == bo.POOL_TRIALS:
                    break
                cb = int(row_ptr[c])
                cn = int(row_ptr[c + 1]) - cb
                mult = _sorted_hits(col, vb, vn, cb, cn)
                if not (float(mult) > max_jaccard * float(vn + cn - mult)):
                    break
            if c == v:
                c = v + 1 if v + 1 < side_hi else side_lo
                if c == v:
                    c = -1
            pool[(v - v_begin) * pool_size + s] = c
