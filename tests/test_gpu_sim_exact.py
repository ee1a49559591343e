"""GPU tests: every instantiation of the similarity + selection kernels (csrc/n2v_sim.hip, C-ABI include/n2v_sim.h)
against the float64 restatement tests/sim_reference.py, through the C-ABI.

Families: "mfma" (sim_mfma_kernel, the default dot), "vector" (sim_tile_kernel<false, *>, N2V_SIM_VECTOR=1) and "jsd"
(sim_tile_kernel<true, *>), each with the block and the scan epilogue.  The case tables at the top are plain numpy and
are imported by tests/test_sim_host.py, which proves on the CPU that they hold every edge they claim and that every
set/order comparison below is decided by the reference alone (exact data, or a gap above twice the error bound).

Tolerances — all computed from the data, none fitted to the device:
  dot scores   |got - want| <= gamma(dpad) sum_k |a_k||b_k| + ulp32(want), gamma(n) = n u / (1 - n u), u = 2^-24: the
               bound of a length-dpad fp32 dot product in ANY summation order, plus the device's final rounding.
  jsd scores   8 u sum_k (p|log(p/m)| + q|log(q/m)| + p + q); the 8: logf 2 ulp = 4u, division, product, halving (with
               the rounded m it stands for) and accumulation one rounding each (sim_reference.jsd_bound).
  prepare      sim_reference.prepare_bound: counted from the sum of dim terms, the sqrt, the division/multiplication;
               pearson carries the conditioning factor mean|x| sqrt(dim) / |x - mean|.
`want` is always float64 arithmetic on the fp32 operands the kernel itself read (prepared rows are read back from the
device), so each kernel's error is separated from the previous one's.

Largest observed error / bound on an MI355X (printed by the tests, -s shows them):
  block scores   mfma 0.052, vector 0.052 (bit-identical to mfma on every case), jsd 0.25
  prepare        cos 0.27, pearson 0.08, jsd 0.74 (dim 2: two roundings against a bound of two)
The whole module takes about 7 s on the device."""
import numpy as np
import pytest

import sim_reference as R

pytestmark = pytest.mark.gpu

FAMILIES = ("mfma", "vector", "jsd")
# (family, epilogue) -> the instantiation the C-ABI launches for it; every pair is run by the tests below
INSTANTIATIONS = {
    ("mfma", "block"): "sim_mfma_kernel<false>", ("mfma", "scan"): "sim_mfma_kernel<true>",
    ("vector", "block"): "sim_tile_kernel<false, false>", ("vector", "scan"): "sim_tile_kernel<false, true>",
    ("jsd", "block"): "sim_tile_kernel<true, false>", ("jsd", "scan"): "sim_tile_kernel<true, true>",
}
SENT = np.float32(-12345.5)        # prefill of every output buffer: what the kernel must not touch keeps it
ISENT = -7


def family_method(fam, dot_method="cos"):
    return "jsd" if fam == "jsd" else dot_method


# ================================================================================================ case tables
# ---- (a)/(b) n2v_sim_block: shape, dim (-> dpad 32, 64, 96, 160, 512), row_begin, ld - n_cols, zero_diag_off kind
BLOCK_SHAPES = [(1, 1), (1, 200), (63, 65), (64, 64), (65, 63), (127, 129), (128, 128), (129, 127), (200, 257), (300, 70)]
BLOCK_CASES = [
    # n_rows, n_cols, dim, row_begin, ld_extra, zero kind, dot method
    (1, 1, 1, 0, 3, "first", "cos"),
    (1, 200, 33, 1, 128, "last", "pearson"),
    (63, 65, 65, 1, 3, "5", "cos"),
    (64, 64, 129, 0, 128, "0", "pearson"),
    (65, 63, 500, 100, 3, "off", "cos"),
    (127, 129, 33, 64, 3, "last", "cos"),
    (128, 128, 65, 0, 128, "5", "pearson"),
    (129, 127, 1, 100, 3, "none", "cos"),
    (200, 257, 129, 1, 128, "0", "cos"),
    (300, 70, 500, 64, 3, "5", "pearson"),
    (200, 257, 500, 100, 3, "last", "cos"),
    (129, 127, 65, 64, 128, "off", "pearson"),
]
A_EXTRA_ROWS = 3     # A always has rows after row_begin + n_rows: the kernel must stop at row_end, not at A's end


def zero_diag_off(kind, n_cols, row_begin):
    """first: the zero lands in column 0 (row 0, so row_begin must be 0); last: row row_begin gets it in the last
    column; none: r + off >= n_cols for every row; off: the switch is off (-1)."""
    if kind == "first":
        assert row_begin == 0
        return 0
    return {"off": -1, "0": 0, "5": 5, "last": n_cols - 1 - row_begin, "none": n_cols}[kind]


def block_case(i):
    """Inputs of BLOCK_CASES[i]: fp32 sources for the dot families (normals) and for jsd (positive, with the special
    rows), and the small-integer prepared rows of the exact layout test."""
    n_rows, n_cols, dim, rb, ld_extra, zk, dot_method = BLOCK_CASES[i]
    rs = np.random.RandomState(100 + i)
    a_rows = rb + n_rows + A_EXTRA_ROWS
    dpad = R.dpad_of(dim)
    srcA = rs.normal(size=(a_rows, dim)).astype(np.float32)
    srcB = rs.normal(size=(n_cols, dim)).astype(np.float32)
    jA = (rs.random_sample((a_rows, dim)) + 0.05).astype(np.float32)
    jB = (rs.random_sample((n_cols, dim)) + 0.05).astype(np.float32)
    special = {}
    if dim >= 2:
        if n_cols >= 2:
            jB[1] = jA[rb]
            special["identical"] = (rb, 1)                  # (row of A, row of B): score exactly 0
        jB[0, ::2] = 0.0
        special["zeros_col"] = 0                            # exact zeros: the x == 0 branch
        if n_cols >= 3:
            jB[n_cols - 1, dim // 2] = -0.2
            special["neg_col"] = n_cols - 1                 # its column is +inf
        if n_rows >= 2:
            jA[rb + 1, 1::2] = 0.0
            special["zeros_row"] = rb + 1
        if n_rows >= 3:
            jA[rb + n_rows - 1, 0] = -0.3
            special["neg_row"] = rb + n_rows - 1            # its row is +inf
    intA = rs.randint(-2, 3, size=(a_rows, dpad)).astype(np.float32)
    intB = rs.randint(-2, 3, size=(n_cols, dpad)).astype(np.float32)
    return dict(n_rows=n_rows, n_cols=n_cols, dim=dim, dpad=dpad, row_begin=rb, ld=n_cols + ld_extra,
                zoff=zero_diag_off(zk, n_cols, rb), zero_kind=zk, dot_method=dot_method, srcA=srcA, srcB=srcB,
                jsdA=jA, jsdB=jB, special=special, intA=intA, intB=intB)


# ---- (c) n2v_sim_prepare
PREP_DIMS = [1, 2, 31, 32, 33, 63, 64, 65, 100, 128, 129, 300]
PREP_NROWS = [1, 3, 4, 5, 257]
PREP_CASES = []
for _m in ("cos", "pearson", "jsd"):
    for _d in PREP_DIMS:
        if _m == "pearson" and _d == 1:
            continue                                         # a single entry is a constant row: covered by that row
        _i = len(PREP_CASES)
        PREP_CASES.append(dict(method=_m, dim=_d, stride_extra=(0, 5)[_i % 2], rows_mode=("none", "perm", "repeat")[_i % 3],
                               n_rows=PREP_NROWS[_i % 5]))


def prepare_case(i):
    """vec fp32 [n_src, stride] (NaN in the columns past dim), rows (None or int64 index), and the special output rows:
    cos row 0 all zero; pearson row 0 constant, row 1 ill-conditioned (offset 100, spread 0.01); jsd row 0 sums to 0."""
    c = PREP_CASES[i]
    method, dim, n_rows = c["method"], c["dim"], c["n_rows"]
    rs = np.random.RandomState(500 + i)
    n_src = 2 * n_rows + 3 if c["rows_mode"] == "repeat" else n_rows
    stride = dim + c["stride_extra"]
    vec = np.full((n_src, stride), np.nan, dtype=np.float32)
    vec[:, :dim] = rs.random_sample((n_src, dim)) + 0.05 if method == "jsd" else rs.normal(size=(n_src, dim))
    rows = None
    if c["rows_mode"] == "perm":
        rows = rs.permutation(n_src).astype(np.int64)
    elif c["rows_mode"] == "repeat":
        rows = rs.randint(0, n_src, size=n_rows).astype(np.int64)
        if n_rows >= 3:
            rows[-1] = rows[n_rows // 2]
    src_of = (lambda r: r) if rows is None else (lambda r: int(rows[r]))
    special = {}
    if method == "cos":
        vec[src_of(0), :dim] = 0.0
        special["zero_row"] = 0
    elif method == "pearson":
        if n_rows >= 2 and src_of(1) != src_of(0):
            vec[src_of(1), :dim] = 100.0 + 0.01 * rs.normal(size=dim)
            special["ill_row"] = 1
        vec[src_of(0), :dim] = 0.5
        special["const_row"] = 0
    elif dim >= 2:
        z = np.zeros(dim, dtype=np.float32)
        h = dim // 2
        z[:h] = 1 + np.arange(h) % 3
        z[h:2 * h] = -z[:h]
        vec[src_of(0), :dim] = z
        special["zero_sum_row"] = 0
    return dict(c, vec=vec, rows=rows, stride=stride, dpad=R.dpad_of(dim), special=special)


# ---- (d) n2v_sim_topk_scan
SCAN_N = 200
SCAN_COLS = {0: 150, 1: 200}                       # upper_triangle -> n_cols (B = the first n_cols rows of A)
SCAN_RANGES = [(0, SCAN_N), (64, 192), (1, 130), (130, 131)]
SCAN_TAUS = ("-inf", "between", "equal")
SCAN_EXCL = ("none", "one", "first_last", "corners64", "corners128", "below_tau")


def scan_operands(fam, upper):
    """Prepared rows written directly.  Dot families: integers -2..2, dpad 96, every score an exact integer.  jsd:
    positive rows of 40 entries (dpad 64).  Rows 5 and 130 repeat rows 3 and 7, so exact ties and (jsd) exact zeros
    occur off the diagonal, also in the one-row range (130, 131)."""
    rs = np.random.RandomState(900)
    if fam == "jsd":
        A = np.zeros((SCAN_N, 64), dtype=np.float32)
        x = rs.random_sample((SCAN_N, 40)) + 0.05
        A[:, :40] = x / x.sum(axis=1, keepdims=True)
    else:
        A = rs.randint(-2, 3, size=(SCAN_N, 96)).astype(np.float32)
    A[5], A[130] = A[3], A[7]
    return A, A[:SCAN_COLS[upper]].copy()


def scan_tau(fam, kind, S_range):
    """tau from the REFERENCE scores of the row range: between = the middle of the widest gap between neighbouring
    distinct scores of the middle half; equal = a value that occurs (dot: the median score; jsd: the exact 0 of
    identical rows)."""
    if kind == "-inf":
        return -np.inf
    v = np.unique(S_range[np.isfinite(S_range)])
    if kind == "equal":
        return 0.0 if fam == "jsd" else float(np.sort(S_range, axis=None)[S_range.size // 2])
    lo, hi = len(v) // 4, max(len(v) // 4 + 2, 3 * len(v) // 4)
    mid = v[lo:hi]
    j = int(np.argmax(np.diff(mid)))
    return float(np.float32((mid[j] + mid[j + 1]) / 2))


def scan_excl_pairs(kind, rb, re, n_cols, upper, tau, S_range):
    """(row, col) pairs to exclude.  Tile corners are taken relative to row_begin, where the kernels' tiles start."""
    if kind == "none":
        return []
    if kind == "first_last":
        return [(rb, 0), (re - 1, n_cols - 1)]
    if kind in ("corners64", "corners128"):
        rr, cc = ((rb + 64, rb + 127), (64, 127)) if kind == "corners64" else ((rb, rb + 127), (0, 127))
        return [(r, c) for r in rr for c in cc if r < re]
    ok = np.isfinite(S_range) if kind == "one" else ~(S_range > tau)
    if kind == "one":
        ok &= S_range > tau
    if upper:
        ok &= np.arange(n_cols)[None, :] > np.arange(rb, re)[:, None]
    idx = np.argwhere(ok)
    if len(idx) == 0:
        return []
    if kind == "one":
        i, c = idx[int(np.argmax(S_range[ok]))]
        return [(rb + int(i), int(c))]
    return [(rb + int(i), int(c)) for i, c in idx[:: max(1, len(idx) // 5)]]     # below_tau: a handful of them


def pair_keys(pairs, n_cols):
    return np.array(sorted(r * n_cols + c for r, c in pairs), dtype=np.int64)


# ---- (e) global_topk with ties at the cut, link_prediction with jsd / pearson
TIES_CONFIGS = [dict(), dict(capacity=2048, first_rows=256), dict(first_rows=1)]


def ties_case(fam):
    """A = B with every row three times (interleaved), so every score occurs at least 9 times (upper: i < j).  k is put
    inside the run of the k-th score."""
    rs = np.random.RandomState(77)
    if fam == "jsd":
        base = np.zeros((40, 32), dtype=np.float32)
        x = rs.random_sample((40, 24)) + 0.05
        base[:, :24] = x / x.sum(axis=1, keepdims=True)
    else:
        base = rs.randint(-2, 3, size=(100, 512)).astype(np.float32)
    A = np.tile(base, (3, 1))
    return A


def ties_k(S, upper, k0=150):
    """A k near k0 whose cut falls strictly inside a run of equal reference scores."""
    top = R.global_topk(S, S.size, None, upper)
    s = [t[0] for t in top]
    k = k0
    while not (s[k - 1] == s[k] and s[k - 2] == s[k - 1]):
        k += 1
    return k, top


LINKPRED_KS = [1, 5, 20]


def linkpred_case(method):
    """30 users x 20 items, 24-d positive vectors, 120 training edges.  Returns what link_prediction needs and the
    index arrays of the reference (users are the dense ids 0..29, items 30..49: labels ascend).  The seeds were picked
    on the reference's own gaps (tests/test_sim_host.py asserts them), before anything ran on a device."""
    rs = np.random.RandomState(40 if method == "jsd" else 32)
    users = np.arange(30, dtype=np.int64)
    items = np.array([int("9999999%d" % i) for i in range(20)], dtype=np.int64)
    e = np.unique(np.stack([rs.randint(0, 30, 240), rs.randint(0, 20, 240)], 1), axis=0)
    rs.shuffle(e)
    train, test = e[:120], e[120:]
    vec = (rs.random_sample((50, 24)) + 0.05).astype(np.float32)
    return dict(users=users, items=items, train_idx=train, test_idx=test, vec=vec,
                train=np.stack([users[train[:, 0]], items[train[:, 1]]], 1),
                test=np.stack([users[test[:, 0]], items[test[:, 1]]], 1))


def linkpred_reference(case, method):
    """float64 scores of users x items from the fp32 vectors, the bound of the device's scores against them (tile
    bound + the prepare bound carried through the score: dot |da||b| + |a||db| + |da||db|; jsd, whose derivative in p_k
    is log(p_k/m_k)/2, eps L with eps the relative prepare bound and L the bound's own sum — twice the first-order
    term), and the reference top-k."""
    vec = case["vec"]
    PA, PB = R.prepare(vec[:30], 24, None, method), R.prepare(vec[30:], 24, None, method)
    ea, eb = np.zeros_like(PA), np.zeros_like(PB)
    ea[:, :24], eb[:, :24] = R.prepare_bound(vec[:30], 24, None, method), R.prepare_bound(vec[30:], 24, None, method)
    S = R.block(PA, PB, method)
    if method == "jsd":
        L = R.jsd_bound(PA, PB) / (R.JSD_C * R.U)
        eps = max((ea[:, :24] / np.abs(PA[:, :24])).max(), (eb[:, :24] / np.abs(PB[:, :24])).max())
        bound = R.jsd_bound(PA, PB) * (1 + 4 * eps) + eps * L
    else:
        bound = R.dot_bound(PA, PB) * (1 + 4 * max(ea.max(), eb.max())) + R.ulp32(S) + ea @ np.abs(PB).T + np.abs(PA) @ eb.T + ea @ eb.T
    keys = pair_keys([(int(a), int(b)) for a, b in case["train_idx"]], 20)
    return S, bound, keys, R.global_topk(S, max(LINKPRED_KS), keys, False)


# ---- (f) row selection
SEL_NCOLS = [1, 5, 255, 256, 257, 600]
SEL_PAD = 7
ROW_KINDS = ("all_equal", "signed_zeros", "with_inf", "some_nan", "all_nan", "denormals", "last_bit", "normals")


def selection_rows(n_cols):
    """One row per kind of ROW_KINDS, fp32 [8, n_cols]."""
    rs = np.random.RandomState(1000 + n_cols)
    rows = np.zeros((len(ROW_KINDS), n_cols), dtype=np.float32)
    rows[0] = 0.25
    rows[1] = np.where(rs.randint(0, 2, n_cols) == 1, np.float32(0.0), np.float32(-0.0))
    rows[1, 0] = -0.0
    if n_cols > 1:
        rows[1, 1] = 0.0                                    # a -0.0 before a +0.0: the order that separates the two keys
    rows[2] = rs.randint(-2, 3, n_cols) / 2.0
    rows[2, rs.random_sample(n_cols) < 0.2] = np.inf
    rows[2, rs.random_sample(n_cols) < 0.2] = -np.inf
    rows[3] = rs.randint(-2, 3, n_cols) / 2.0
    rows[3, rs.random_sample(n_cols) < 0.15] = np.nan
    rows[3, n_cols // 2] = np.nan
    rows[4] = np.nan
    rows[5] = (rs.randint(-5, 6, n_cols).astype(np.int32).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    one = np.float32(1.0)
    rows[6] = np.where(rs.randint(0, 2, n_cols) == 1, one, np.nextafter(one, np.float32(2.0)))
    rows[7] = rs.normal(size=n_cols)
    return rows


def padded(rows, pad=SEL_PAD):
    """[n_rows, n_cols + pad] with +inf and NaN in the padding: the kernels must not read it as members."""
    out = np.empty((rows.shape[0], rows.shape[1] + pad), dtype=np.float32)
    out[:, :rows.shape[1]] = rows
    out[:, rows.shape[1]:] = np.inf
    out[:, rows.shape[1] + 1::2] = np.nan
    return out


def threshold_cases(n_cols):
    """(scores [n_rows, n_cols], thre) for rows_count / rows_fill: one row of each kind (n_rows 8), 300 rows cycling
    the kinds, and a single row (n_rows 1); thre = +-0.0, a value that occurs in the normal row, a denormal that occurs,
    the repeated value of the equal row, +-inf."""
    rows = selection_rows(n_cols)
    many = np.tile(rows, (38, 1))[:300]
    thres = [0.0, -0.0, float(rows[7, 0]), float(rows[5, n_cols // 3]), 0.25, 1.0, np.inf, -np.inf]
    out = [(rows, t) for t in thres]
    out += [(many, 0.0), (many, float(rows[7, 0])), (rows[7:8], float(rows[7, 0])), (rows[1:2], 0.0)]
    return out


# ---- every comparison that is a set or an order, with what makes it unambiguous (tests/test_sim_host.py checks each)
def selection_comparisons():
    """Yields (name, kind, payload).  kind "exact": payload = arrays whose entries must all be exactly representable
    small integers (the fp32 kernel then computes every score exactly).  kind "given": the scores are the test's own
    fp32 inputs, compared as they are — nothing is computed.  kind "gap": payload = (margin, bound) arrays: every
    margin must exceed twice its bound."""
    for fam in FAMILIES:
        for upper in (0, 1):
            A, B = scan_operands(fam, upper)
            if fam != "jsd":
                yield ("scan-%s-upper%d" % (fam, upper), "exact", (A, B))
                continue
            S, bound = R.block(A, B, "jsd"), R.jsd_bound(A, B)
            same = (A[:, None, :] == B[None, :, :]).all(axis=2)
            for rb, re in SCAN_RANGES:
                for tk in SCAN_TAUS[1:]:
                    tau = scan_tau(fam, tk, S[rb:re])
                    m = np.where(same[rb:re], np.inf, np.abs(S[rb:re] - tau))   # identical rows: exactly 0 on both sides
                    yield ("scan-jsd-upper%d-%d:%d-%s" % (upper, rb, re, tk), "gap", (m, bound[rb:re]))
    for fam in FAMILIES:
        A = ties_case(fam)
        if fam != "jsd":
            yield ("ties-%s" % fam, "exact", (A,))
            continue
        S, bound = R.block(A, A, "jsd"), R.jsd_bound(A, A)
        k, top = ties_k(S, True)
        vals = np.array([t[0] for t in top[:k + 12]])
        bnd = np.array([bound[t[1], t[2]] for t in top[:k + 12]])
        d = vals[:-1] - vals[1:]
        yield ("ties-jsd", "gap", (np.where(d == 0, np.inf, d), np.maximum(bnd[:-1], bnd[1:])))
    for method in ("jsd", "pearson"):
        S, bound, keys, top = linkpred_reference(linkpred_case(method), method)
        full = R.global_topk(S, max(LINKPRED_KS) + 1, keys, False)
        vals = np.array([t[0] for t in full])
        bnd = np.array([bound[t[1], t[2]] for t in full])
        yield ("linkpred-%s" % method, "gap", (vals[:-1] - vals[1:], np.maximum(bnd[:-1], bnd[1:])))
    for n_cols in SEL_NCOLS:
        yield ("rows-%d" % n_cols, "given", (selection_rows(n_cols),))


# ================================================================================================ device helpers
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _use_family(monkeypatch, fam):
    if fam == "vector":
        monkeypatch.setenv("N2V_SIM_VECTOR", "1")
    else:
        monkeypatch.delenv("N2V_SIM_VECTOR", raising=False)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _block(torch, A, row_begin, n_rows, B, method, zoff=-1, ld=None):
    """n2v_sim_block into a sentinel-filled [n_rows + 2, ld] buffer; returns the whole buffer."""
    from n2v_hip import _lib
    lib = _lib.load()
    n_cols = int(B.shape[0])
    ld = n_cols if ld is None else ld
    buf = torch.full((n_rows + 2, ld), float(SENT), dtype=torch.float32, device=A.device)
    _lib.check(lib.n2v_sim_block(_lib.ptr(A), row_begin, n_rows, _lib.ptr(B), n_cols, int(A.shape[1]), R.METHODS[method],
                                 zoff, _lib.ptr(buf), ld, _lib.stream_ptr(A.device)))
    return buf.cpu().numpy()


def _assert_outside_untouched(buf, n_rows, n_cols):
    mask = np.ones(buf.shape, dtype=bool)
    mask[:n_rows, :n_cols] = False
    assert (_bits(buf)[mask] == _bits(SENT)).all(), "the kernel wrote outside [n_rows, n_cols]"


def _scan(torch, A, rb, re, B, method, upper, tau, keys, capacity, pad=64):
    from n2v_hip import _lib
    lib = _lib.load()
    dev = A.device
    tau_t = torch.tensor([tau], dtype=torch.float32, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    cs = torch.full((capacity + pad,), float(SENT), dtype=torch.float32, device=dev)
    cr = torch.full((capacity + pad,), ISENT, dtype=torch.int32, device=dev)
    cc = torch.full((capacity + pad,), ISENT, dtype=torch.int32, device=dev)
    ex = None if len(keys) == 0 else _dev(torch, keys)
    _lib.check(lib.n2v_sim_topk_scan(_lib.ptr(A), rb, re, _lib.ptr(B), int(B.shape[0]), int(A.shape[1]), R.METHODS[method],
                                     upper, _lib.ptr(tau_t), _lib.ptr(ex), len(keys), _lib.ptr(cs), _lib.ptr(cr), _lib.ptr(cc),
                                     capacity, _lib.ptr(counter), _lib.stream_ptr(dev)))
    return int(counter.item()), cs.cpu().numpy(), cr.cpu().numpy(), cc.cpu().numpy()


def _ratio(err, tol):
    """largest err / tol over the finite entries (0 where both are 0)"""
    with np.errstate(all="ignore"):
        q = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    q = q[np.isfinite(err)]
    return float(q.max()) if q.size else 0.0


def _assert_scores(got, want, tol, what):
    """non-finite reference values (NaN, +-inf) must be reproduced exactly, finite ones within tol"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - want)
    bad = fin & ~(err <= tol)
    assert not bad.any(), (what, "first miss at", np.argwhere(bad)[0].tolist(), "err/bound", _ratio(err[fin], tol[fin]))
    return _ratio(err[fin], tol[fin])


# ================================================================================================ (a) + (b) block
@pytest.mark.parametrize("i", range(len(BLOCK_CASES)))
def test_block_scores_within_derived_bound(torch_cuda, monkeypatch, i):
    """(a) every family at BLOCK_CASES[i]: prepare on the device, read the prepared rows back, float64 block of THOSE
    rows, tolerance from the module docstring.  The buffer outside [n_rows, n_cols] keeps its sentinel; the zeroed
    diagonal is an exact +0.0; and the MFMA and the vector-FMA kernels, both a k-ascending fmaf chain from +0.0, agree
    bit for bit."""
    torch = torch_cuda
    from n2v_hip import simsel
    c = block_case(i)
    out = {}
    for fam in FAMILIES:
        _use_family(monkeypatch, fam)
        method = family_method(fam, c["dot_method"])
        sa, sb = (c["jsdA"], c["jsdB"]) if fam == "jsd" else (c["srcA"], c["srcB"])
        A, B = simsel.prepare(_dev(torch, sa), method), simsel.prepare(_dev(torch, sb), method)
        assert A.shape[1] == c["dpad"]
        buf = _block(torch, A, c["row_begin"], c["n_rows"], B, method, c["zoff"], c["ld"])
        _assert_outside_untouched(buf, c["n_rows"], c["n_cols"])
        got = buf[:c["n_rows"], :c["n_cols"]]
        PA, PB = A.cpu().numpy(), B.cpu().numpy()
        want = R.block(PA, PB, method, c["row_begin"], c["n_rows"], c["zoff"])
        tol = R.score_bound(PA, PB, method, c["row_begin"], c["n_rows"])
        if fam != "jsd":
            tol = tol + R.ulp32(want)
        ratio = _assert_scores(got, want, tol, (fam, BLOCK_CASES[i]))
        print("block case %d %s: max err/bound %.4f" % (i, fam, ratio))
        if c["zoff"] >= 0:
            for r in range(c["n_rows"]):
                col = c["row_begin"] + r + c["zoff"]
                if col < c["n_cols"]:
                    assert _bits(got[r, col]) == 0
        if fam == "jsd":
            sp = c["special"]
            # _assert_scores holds the device to the reference's +inf exactly; these pin the reference itself
            # (all +inf but a zeroed diagonal element) and the exact 0 of two identical rows
            if "identical" in sp:
                assert got[0, sp["identical"][1]] == 0.0 and want[0, sp["identical"][1]] == 0.0
            if "neg_row" in sp:
                assert np.isposinf(want[sp["neg_row"] - c["row_begin"]]).sum() >= c["n_cols"] - 1
            if "neg_col" in sp:
                assert np.isposinf(want[:, sp["neg_col"]]).sum() >= c["n_rows"] - 1
        out[fam] = got
    assert np.array_equal(_bits(out["mfma"]), _bits(out["vector"])), "MFMA and vector-FMA dot differ in some bit"


@pytest.mark.parametrize("fam", ["mfma", "vector"])
@pytest.mark.parametrize("i", range(len(BLOCK_CASES)))
def test_block_integer_operands_are_exact(torch_cuda, monkeypatch, i, fam):
    """(b) operands -2..2: every partial sum is an exact fp32 integer (|sum| <= 4 * 512), so the block equals the integer
    product bit for bit — a wrong lane/register mapping, wr/wc/bi/bj offset, edge guard or a dropped k-chunk cannot hide
    in a tolerance."""
    torch = torch_cuda
    c = block_case(i)
    _use_family(monkeypatch, fam)
    buf = _block(torch, _dev(torch, c["intA"]), c["row_begin"], c["n_rows"], _dev(torch, c["intB"]), "cos", c["zoff"], c["ld"])
    _assert_outside_untouched(buf, c["n_rows"], c["n_cols"])
    want = R.block(c["intA"], c["intB"], "cos", c["row_begin"], c["n_rows"], c["zoff"])
    assert np.array_equal(buf[:c["n_rows"], :c["n_cols"]].astype(np.float64), want)


# ================================================================================================ (c) prepare
@pytest.mark.parametrize("i", range(len(PREP_CASES)))
def test_prepare_within_derived_bound(torch_cuda, i):
    torch = torch_cuda
    from n2v_hip import _lib
    lib = _lib.load()
    c = prepare_case(i)
    vec = _dev(torch, c["vec"])
    rows = None if c["rows"] is None else _dev(torch, c["rows"])
    out = torch.full((c["n_rows"] + 1, c["dpad"]), float(SENT), dtype=torch.float32, device=vec.device)
    _lib.check(lib.n2v_sim_prepare(_lib.ptr(vec), c["stride"], c["dim"], _lib.ptr(rows), c["n_rows"], R.METHODS[c["method"]],
                                   _lib.ptr(out), c["dpad"], _lib.stream_ptr(vec.device)))
    buf = out.cpu().numpy()
    assert (_bits(buf[c["n_rows"]:]) == _bits(SENT)).all(), "wrote past the last row"
    got = buf[:c["n_rows"]]
    assert (_bits(got[:, c["dim"]:]) == 0).all(), "padding columns are not +0.0"
    want = R.prepare(c["vec"], c["dim"], c["rows"], c["method"])[:, :c["dim"]]
    tol = R.prepare_bound(c["vec"], c["dim"], c["rows"], c["method"])
    ratio = _assert_scores(got[:, :c["dim"]], want, np.where(np.isfinite(want), tol, 0.0), PREP_CASES[i])
    print("prepare case %d %s dim %d: max err/bound %.4f" % (i, c["method"], c["dim"], ratio))
    sp = c["special"]
    if "zero_row" in sp:
        assert (_bits(got[0]) == 0).all()
        S = _block(torch, out[:c["n_rows"]], 0, c["n_rows"], out[:c["n_rows"]], "cos")[:c["n_rows"]]
        assert (S[0] == 0).all() and (S[:, 0] == 0).all(), "a zero vector's cosine is 0 (unitvec), not NaN"
    if "const_row" in sp:
        assert np.isnan(got[0, :c["dim"]]).all() and np.isnan(want[0]).all()
    if "zero_sum_row" in sp:
        assert not np.isfinite(got[0, :c["dim"]]).any() and not np.isfinite(want[0]).any()


# ================================================================================================ (d) scan
@pytest.mark.parametrize("upper", [0, 1])
@pytest.mark.parametrize("fam", FAMILIES)
def test_topk_scan_is_the_reference_set(torch_cuda, monkeypatch, fam, upper):
    """(d) n2v_sim_topk_scan directly, every SCAN_RANGES x SCAN_TAUS x SCAN_EXCL: the counter is the number of
    qualifying pairs, the (row, col) set is the reference's, every score is bit-equal to n2v_sim_block's for that pair;
    with a capacity below the count the counter still counts everything, the kept entries are distinct members of the
    set and nothing is written past `capacity`."""
    torch = torch_cuda
    _use_family(monkeypatch, fam)
    method = family_method(fam)
    An, Bn = scan_operands(fam, upper)
    A, B = _dev(torch, An), _dev(torch, Bn)
    n_cols = Bn.shape[0]
    S = R.block(An, Bn, method)
    for rb, re in SCAN_RANGES:
        blk = _block(torch, A, rb, re - rb, B, method)[:re - rb]
        if fam != "jsd":
            assert np.array_equal(blk.astype(np.float64), S[rb:re])
        for tk in SCAN_TAUS:
            tau = scan_tau(fam, tk, S[rb:re])
            for ek in SCAN_EXCL:
                keys = pair_keys(scan_excl_pairs(ek, rb, re, n_cols, upper, tau, S[rb:re]), n_cols)
                want = {(r, c) for r, c, _ in R.topk_scan(S[rb:re], tau, keys, upper, rb)}
                what = (fam, upper, rb, re, tk, ek)
                n, cs, cr, cc = _scan(torch, A, rb, re, B, method, upper, tau, keys, capacity=max(len(want), 1) + 5)
                assert n == len(want), what
                got = list(zip(cr[:n].tolist(), cc[:n].tolist()))
                assert len(set(got)) == n and set(got) == want, what
                assert np.array_equal(_bits(cs[:n]), _bits(blk[cr[:n] - rb, cc[:n]])), what
                assert (_bits(cs[n:]) == _bits(SENT)).all() and (cr[n:] == ISENT).all() and (cc[n:] == ISENT).all(), what
                if ek == "none" and tk == "-inf" and len(want) >= 2:
                    cap = len(want) // 2
                    n2, cs, cr, cc = _scan(torch, A, rb, re, B, method, upper, tau, keys, capacity=cap)
                    assert n2 == len(want) > cap, what
                    kept = list(zip(cr[:cap].tolist(), cc[:cap].tolist()))
                    assert len(set(kept)) == cap and set(kept) <= want, what
                    assert np.array_equal(_bits(cs[:cap]), _bits(blk[cr[:cap] - rb, cc[:cap]])), what
                    assert (_bits(cs[cap:]) == _bits(SENT)).all() and (cr[cap:] == ISENT).all() and (cc[cap:] == ISENT).all(), what


# ================================================================================================ (e) global top-k
@pytest.mark.parametrize("fam,upper", [("mfma", False), ("mfma", True), ("vector", False), ("vector", True), ("jsd", True)])
def test_global_topk_with_ties_at_the_cut(torch_cuda, monkeypatch, fam, upper):
    """(e) more than k pairs share the k-th score.  Which of the tied pairs survive is not defined (the scan drops later
    ties of the running threshold), so: the multiset of scores is the reference's, every pair is a distinct valid
    candidate carrying its own score, the order is (score desc, row, col) — for the default buffer, for a 2048-entry
    one that overflows, and for first_rows=1.  jsd: scores within the derived bound, and the multiset is compared
    through the reference's value of each returned pair (gap condition, tests/test_sim_host.py)."""
    torch = torch_cuda
    from n2v_hip import simsel
    _use_family(monkeypatch, fam)
    method = family_method(fam)
    An = ties_case(fam)
    S = R.block(An, An, method)
    k, top = ties_k(S, upper)
    want_vals = sorted(t[0] for t in top[:k])
    assert sum(1 for t in top if t[0] == top[k - 1][0]) > sum(1 for t in top[:k] if t[0] == top[k - 1][0])
    A = _dev(torch, An)
    bound = R.score_bound(An, An, method)
    first = None
    for cfg in TIES_CONFIGS:
        s, r, c = simsel.global_topk(A, A, k, method, upper_triangle=upper, **cfg)
        s, r, c = s.cpu().numpy(), r.cpu().numpy().astype(np.int64), c.cpu().numpy().astype(np.int64)
        assert len(s) == k and len(set(zip(r.tolist(), c.tolist()))) == k, cfg
        assert not upper or (c > r).all()
        assert sorted(S[r, c].tolist()) == want_vals, cfg
        if fam == "jsd":
            assert (np.abs(s - S[r, c]) <= bound[r, c]).all(), cfg
        else:
            assert np.array_equal(s.astype(np.float64), S[r, c]), cfg
        order = sorted(range(k), key=lambda j: (-s[j], r[j], c[j]))
        assert order == list(range(k)), cfg
        first = s if first is None else first
        assert np.array_equal(_bits(first), _bits(s)), "the score list depends on capacity / first_rows"


@pytest.mark.parametrize("method", ["jsd", "pearson"])
def test_link_prediction_jsd_and_pearson(torch_cuda, monkeypatch, method):
    """(e) link_prediction(sim_method=...) on 30 users x 20 items against sim_reference.global_topk of the float64
    scores minus the training edges: same pairs in the same order (the reference's neighbouring scores are further
    apart than twice the bound, tests/test_sim_host.py), scores within the bound."""
    torch = torch_cuda
    from n2v_hip import csr, linkpred
    monkeypatch.delenv("N2V_SIM_VECTOR", raising=False)
    case = linkpred_case(method)
    users, items = case["users"], case["items"]
    g = csr.from_edges(np.concatenate([case["train"][:, 0], users, items[:-1]]),
                       np.concatenate([case["train"][:, 1], users, items[1:]]), None, False)
    assert g.labels.tolist() == users.tolist() + items.tolist()
    S, bound, keys, top = linkpred_reference(case, method)
    res, fin = linkpred.link_prediction(_dev(torch, case["vec"]), g, case["train"], case["test"], ks=LINKPRED_KS,
                                        sim_method=method)
    test = {(int(a), int(b)) for a, b in case["test_idx"]}
    for k in LINKPRED_KS:
        want = top[:k]
        assert [p for p, _, _ in res[k]] == [(str(users[r]), str(items[c])) for _, r, c in want], (method, k)
        for (_, s, _), (ws, r, c) in zip(res[k], want):
            assert abs(s - ws) <= bound[r, c], (method, k, r, c, s, ws)
        assert fin[k][0] == sum(1 for _, r, c in want if (r, c) in test) / k


# ================================================================================================ (f) rows
def _rows_topk_abi(torch, dev_scores, n_rows, n_cols, ld, k):
    from n2v_hip import _lib
    lib = _lib.load()
    cols = torch.full((n_rows * max(k, 1) + 8,), ISENT, dtype=torch.int32, device=dev_scores.device)
    vals = torch.full((n_rows * max(k, 1) + 8,), float(SENT), dtype=torch.float32, device=dev_scores.device)
    _lib.check(lib.n2v_sim_rows_topk(_lib.ptr(dev_scores), n_rows, n_cols, ld, k, _lib.ptr(cols), _lib.ptr(vals),
                                     _lib.stream_ptr(dev_scores.device)))
    return cols.cpu().numpy(), vals.cpu().numpy()


@pytest.mark.parametrize("n_cols", SEL_NCOLS)
def test_rows_topk_every_k(torch_cuda, n_cols):
    """(f) every k in 0..n_cols over one row of each ROW_KINDS.  At the C-ABI, ld = n_cols + 7 with +inf / NaN in the
    padding: the selected columns as a set, in column order, values bit-equal to the input (a selected -0.0 stays
    -0.0).  Through simsel.rows_topk: the ordered list.  Rows with NaN are compared as sets once k reaches into the
    NaNs, as in tests/test_gpu_sim.py.  No row mixes NaN with -inf: the reference replaces NaN by -inf and ties them,
    the kernel ranks NaN strictly below -inf; both are "NaN ranks lowest"."""
    torch = torch_cuda
    from n2v_hip import simsel
    rows = selection_rows(n_cols)
    n_rows = rows.shape[0]
    pad = padded(rows)
    dpad, dplain = _dev(torch, pad), _dev(torch, rows)
    full = R.rows_topk(rows, n_cols)
    n_real = (~np.isnan(rows)).sum(axis=1)
    for k in range(n_cols + 1):
        cols, vals = _rows_topk_abi(torch, dpad, n_rows, n_cols, pad.shape[1], k)
        assert (cols[n_rows * k:] == ISENT).all() and (_bits(vals[n_rows * k:]) == _bits(SENT)).all(), k
        ocols, ovals = simsel.rows_topk(dplain, n_cols, k)
        ocols, ovals = ocols.cpu().numpy(), ovals.cpu().numpy()
        for r in range(n_rows):
            want = full[r][:k]
            got = cols[r * k:(r + 1) * k]
            assert got.tolist() == sorted(want), (ROW_KINDS[r], n_cols, k)
            assert np.array_equal(_bits(vals[r * k:(r + 1) * k]), _bits(rows[r][got])), (ROW_KINDS[r], n_cols, k)
            if k > n_real[r]:
                assert set(ocols[r].tolist()) == set(want), (ROW_KINDS[r], n_cols, k)
            else:
                assert ocols[r].tolist() == want, (ROW_KINDS[r], n_cols, k)
                assert np.array_equal(_bits(ovals[r]), _bits(rows[r][want])), (ROW_KINDS[r], n_cols, k)


@pytest.mark.parametrize("n_cols", SEL_NCOLS)
def test_rows_count_and_fill(torch_cuda, n_cols):
    """(f) rows_count / rows_fill over the same rows with ld = n_cols + 7 (+inf / NaN padding): counts, then columns in
    order and values bit-equal at the offsets the counts give; thresholds equal to a value that occurs, +0.0 against
    -0.0 scores, +-inf (rows without a hit and rows that are all hits)."""
    torch = torch_cuda
    from n2v_hip import _lib
    lib = _lib.load()
    seen_none = seen_all = False
    for scores, thre in threshold_cases(n_cols):
        n_rows = scores.shape[0]
        pad = padded(scores)
        dev = _dev(torch, pad)
        st = _lib.stream_ptr(dev.device)
        counts = torch.full((n_rows + 2,), ISENT, dtype=torch.int64, device=dev.device)
        _lib.check(lib.n2v_sim_rows_count(_lib.ptr(dev), n_rows, n_cols, pad.shape[1], thre, _lib.ptr(counts), st))
        counts = counts.cpu().numpy()
        wc = R.rows_count(scores, thre)
        assert np.array_equal(counts[:n_rows], wc) and (counts[n_rows:] == ISENT).all(), (n_cols, thre)
        seen_none |= bool((wc == 0).any())
        seen_all |= bool((wc == n_cols).any())
        off, wcols, wvals = R.rows_fill(scores, thre)
        total = int(wc.sum())
        cols = torch.full((total + 8,), ISENT, dtype=torch.int32, device=dev.device)
        vals = torch.full((total + 8,), float(SENT), dtype=torch.float32, device=dev.device)
        _lib.check(lib.n2v_sim_rows_fill(_lib.ptr(dev), n_rows, n_cols, pad.shape[1], thre, _lib.ptr(_dev(torch, off)),
                                         _lib.ptr(cols), _lib.ptr(vals), st))
        cols, vals = cols.cpu().numpy(), vals.cpu().numpy()
        assert np.array_equal(cols[:total], wcols) and (cols[total:] == ISENT).all(), (n_cols, thre)
        assert np.array_equal(_bits(vals[:total]), _bits(wvals)) and (_bits(vals[total:]) == _bits(SENT)).all(), (n_cols, thre)
    assert seen_none and seen_all
