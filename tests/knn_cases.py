"""Case tables of tests/test_gpu_knn.py (plain numpy; tests/test_knn_host.py proves on the CPU that they hold the borders
they are there for).  The borders come from csrc/n2v_knn.hip and n2v_sim_tile.h: tile 128, wavefront 64, accumulator
block 32, k-chunk 16, lists in chunks of 64 entries."""
import numpy as np

TILE = 128
MAX_SEG = 32                 # n2v_sim_knn_max_seg()
MAX_K = 256                  # N2V_SIM_KNN_MAX_K

NQ = (1, 31, 32, 33, 64, 127, 128, 129, 257)
NCOLS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385, 1000)
DPAD = (32, 64, 96, 160, 512)
KS = (1, 2, 10, 63, 64, 65, 128, 255, 256)
SEGS = (0, 1, 2, 3, "max", "more")
EXCL = ("null", "arange", "minus1", "beyond", "col0", "col63", "col64", "col127", "col128", "last")

# hand-picked: (n_q, n_cols, dpad, k, n_seg, exclude)
_FIXED = [
    (1, 1, 32, 1, 1, "col0"),             # the only column excluded: every entry empty
    (33, 1, 64, 10, 0, "null"),           # one candidate, k = 10
    (31, 2, 32, 2, "more", "last"),
    (257, 1000, 512, 256, 3, "arange"),   # every border at once, the largest case
    (129, 1000, 96, 255, "max", "col128"),
    (128, 385, 160, 65, 2, "col127"),
    (127, 257, 32, 128, "more", "col64"),
    (64, 129, 64, 64, 2, "col63"),
    (32, 256, 96, 63, 0, "beyond"),
    (1, 255, 160, 256, 1, "minus1"),      # k above the candidates of a one-row call
    (257, 63, 32, 64, "max", "last"),     # k = n_cols + 1
    (129, 65, 512, 10, 3, "col0"),
]


def _draw():
    """48 more cases from a seeded stream: every value of every list is used, no cross-product."""
    rs = np.random.RandomState(2024)
    out = []
    for i in range(48):
        n_q, dpad, k = NQ[i % len(NQ)], DPAD[i % len(DPAD)], KS[(i // 2 + i) % len(KS)]
        n_cols = NCOLS[(5 * i + 3) % len(NCOLS)]
        seg = SEGS[(i + i // 6) % len(SEGS)]
        kinds = [e for e in EXCL if not e.startswith("col") or int(e[3:]) < n_cols]
        excl = kinds[int(rs.randint(len(kinds)))]
        if n_q * n_cols * dpad > 129 * 1000 * 160:      # keep the drawn cases small; the large corner is in _FIXED
            dpad = 32
        out.append((n_q, n_cols, dpad, k, seg, excl))
    return out


CASES = _FIXED + _draw()


def n_tiles(n_cols):
    return -(-n_cols // TILE)


def seg_value(seg, n_cols):
    """The n_seg argument of a case: "max" is the largest the export takes, "more" one more than there are column tiles."""
    if seg == "max":
        return MAX_SEG
    if seg == "more":
        return min(MAX_SEG, n_tiles(n_cols) + 1)
    return seg


def exclude_array(kind, n_q, n_cols):
    """int32 [n_q] or None."""
    if kind == "null":
        return None
    if kind == "arange":
        return np.arange(n_q, dtype=np.int32)
    if kind == "minus1":
        return np.full(n_q, -1, dtype=np.int32)
    if kind == "beyond":
        return (n_cols + np.arange(n_q) % 3 * 1000).astype(np.int32)
    col = n_cols - 1 if kind == "last" else int(kind[3:])
    return np.full(n_q, col, dtype=np.int32)


def segment_borders(n_cols, n_seg):
    """First columns of the segments 1 .. n_seg - 1 that begin inside the matrix (the kernel's t0 = n_tiles * s / n_seg)."""
    t = n_tiles(n_cols)
    return sorted(b for b in {TILE * (t * s // n_seg) for s in range(1, n_seg)} if 0 < b < n_cols)


DUP_PAIRS = ((63, 64), (127, 128))


def int_case(i):
    """Operands with entries in {-2 .. 2} as prepared rows: every score is a small integer, exact in fp32 in any order,
    with ties by the thousand.  B rows are duplicated across the wavefront border (63/64), the tile border (127/128) and
    the first border of the case's own segmentation and of n_seg 2 and 3."""
    n_q, n_cols, dpad, k, seg, excl = CASES[i]
    rs = np.random.RandomState(500 + i)
    Q = rs.randint(-2, 3, size=(n_q, dpad)).astype(np.float32)
    B = rs.randint(-2, 3, size=(n_cols, dpad)).astype(np.float32)
    dups = [p for p in DUP_PAIRS if p[1] < n_cols]
    for s in {2, 3, max(1, seg_value(seg, n_cols))}:
        dups += [(b - 1, b) for b in segment_borders(n_cols, s)[:1]]
    for a, b in dups:
        B[b] = B[a]
    return dict(n_q=n_q, n_cols=n_cols, dpad=dpad, k=k, n_seg=seg_value(seg, n_cols), exclude=exclude_array(excl, n_q, n_cols),
                Q=Q, B=B, dups=dups)


def int_scores(c):
    """The exact scores of an integer case as fp32."""
    return (c["Q"].astype(np.int64) @ c["B"].astype(np.int64).T).astype(np.float32)


# cases whose tiles can be cut into segments in more than one way: run under every n_seg of SEGS
SEG_CASES = [i for i, c in enumerate(CASES) if c[1] >= 257][:6]

# real-operand cases: (n_q, n_cols, dim, k, exclude kind); dims give dpad 32, 64, 96, 160, 512
REAL_CASES = [
    (33, 129, 20, 10, "null"),
    (129, 257, 33, 65, "col128"),
    (64, 385, 70, 256, "last"),
    (127, 1000, 100, 10, "arange"),
    (257, 255, 129, 128, "col63"),
    (32, 63, 500, 64, "minus1"),          # k = n_cols + 1: the NaN column is chosen, then an empty entry
    (1, 65, 100, 65, "col0"),
]
REAL_NAN_ROW = 5         # B row with a NaN entry: every score against it is NaN
REAL_ZERO_ROW = 7        # all-zero B row: cosine 0 (unitvec keeps it), pearson NaN (0 / 0)


def real_case(i):
    n_q, n_cols, dim, k, excl = REAL_CASES[i]
    rs = np.random.RandomState(900 + i)
    q = rs.normal(size=(n_q, dim)).astype(np.float32)
    b = rs.normal(size=(n_cols, dim)).astype(np.float32)
    b[REAL_NAN_ROW, dim // 2] = np.nan
    b[REAL_ZERO_ROW] = 0.0
    return dict(n_q=n_q, n_cols=n_cols, dim=dim, k=k, exclude=exclude_array(excl, n_q, n_cols), q=q, b=b)
