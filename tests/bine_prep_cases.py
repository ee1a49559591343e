"""TEST INFRASTRUCTURE — the case table of tests/test_gpu_bine_prep.py, shared with tests/test_bine_prep_host.py.

Nothing reaches a BiNE preparation kernel from the GPU test that is not built here: the host test replays every case
with bounds-checked indexing (tests/bine_prep_reference.py) on exactly the arrays that `*_launches` hands to the GPU
test, and shows that each case takes the branches it exists for.  Graphs come from bine.BipartiteGraph or
bine.user_edges_csr, two-hop prefixes from bo.two_hop_prefix, walk lengths from bo.walk_length on the same graph.

Left out, with the reason:
  * a CSR row of 0 entries: BipartiteGraph gives every vertex at least one rating, and no array is hand-made;
  * the `pick >= paths` clamp of the walk step and the `k >= side` clamp of the pools: unreachable.  u53 is at most
    1 - 2^-53, and for an integer p < 2^53 the exact product p - p 2^-53 lies at least half a unit in the last place
    below p (exactly representable when p is a power of two), so the rounded product is below p and floor() below p."""
import functools

import numpy as np

import bine_prep_reference as P
from oracle import bine_oracle as bo


# ------------------------------------------------------------------------------------------ graphs
def _bipartite(users, items, ratings):
    from n2v_hip import bine
    return bine.BipartiteGraph(np.asarray(users), np.asarray(items), np.asarray(ratings, dtype=np.float64))


def _wide():
    """2100 users (three trips of 1024 threads and a tail of 52), 30 items, two ratings per user."""
    rs = np.random.RandomState(11)
    users = np.repeat(np.arange(2100), 2)
    first = rs.randint(0, 30, 2100)
    items = np.stack([first, (first + 1 + rs.randint(0, 29, 2100)) % 30], 1).ravel()
    return _bipartite(users, items, rs.randint(1, 6, users.shape[0]))


def _rows():
    """Items rated by exactly 130, 65, 64, 63, 1 and 2 users; user 130 holds one entry; n = 137 (n % 4 == 1)."""
    rs = np.random.RandomState(12)
    pairs = [(u, 0) for u in range(130)] + [(u, 1) for u in range(65)] + [(u, 2) for u in range(64)] + \
            [(u, 3) for u in range(63)] + [(130, 4), (1, 5), (2, 5)]
    users, items = zip(*pairs)
    return _bipartite(users, items, rs.randint(1, 6, len(pairs)))


def _skew():
    """142 users, 12 items.  Items 0, 1, 2 hold 68 users each, laid out so that the wave-wide search for an earlier
    common neighbour swaps its ranges in both directions, needs a second 64-wide round (0 -> 1 through user 140: user
    65 is the 66th of item 0's users) and leaves early with a round to go (0 -> 2 through user 141: user 3); the other
    nine items are popularity-skewed like tests/test_gpu_bine.py's graph."""
    rs = np.random.RandomState(13)
    a = list(range(66)) + [140, 141]
    b = list(range(65, 132)) + [140, 141]
    c = [3] + list(range(66, 132)) + [141]
    pairs = [(u, 0) for u in a] + [(u, 1) for u in b] + [(u, 2) for u in c]
    for u in range(142):
        for i in np.minimum((9 * rs.random_sample(2) ** 2.5).astype(np.int64), 8):
            pairs.append((u, 3 + int(i)))
    users, items = zip(*pairs)
    return _bipartite(users, items, rs.randint(1, 6, len(pairs)))


def _deadend():
    """15 users on 6 shared items, 5 users (15..19) each alone on a private item: dead-end starts on both sides."""
    rs = np.random.RandomState(14)
    pairs = [(u, int(i)) for u in range(15) for i in rs.choice(6, 2, replace=False)] + [(15 + k, 6 + k) for k in range(5)]
    users, items = zip(*pairs)
    return _bipartite(users, items, rs.randint(1, 6, len(pairs)))


def _pair():
    return _bipartite([0, 1], [0, 0], [3.0, 4.0])                       # sides of 2 and 1


def _single_user():
    return _bipartite([0, 0, 0], [0, 1, 2], [1.0, 2.0, 5.0])            # sides of 1 and 3


def _dense():
    users, items = np.divmod(np.arange(24), 4)                          # 6 x 4, complete: every Jaccard is 1
    return _bipartite(users, items, 1.0 + (np.arange(24) % 5))


_BUILDERS = dict(wide=_wide, rows=_rows, skew=_skew, deadend=_deadend, pair=_pair, single_user=_single_user, dense=_dense)


@functools.lru_cache(maxsize=None)
def graph(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def cum2(name):
    g = graph(name)
    return bo.two_hop_prefix(g.row_ptr, g.col)


def side_range(g, side):
    return (0, g.n_u) if side == "u" else (g.n_u, g.n)


# ------------------------------------------------------------------------------------------ HITS
# user-user edges for bine.user_edges_csr: 120 random pairs heavy enough to separate the spectrum of the no longer
# bipartite matrix, then a self loop given twice and a pair repeated in both orders (the last weight wins)
def _user_edges():
    rs = np.random.RandomState(15)
    src = rs.randint(0, 142, 120).tolist() + [3, 4, 3, 9]
    dst = rs.randint(0, 142, 120).tolist() + [3, 9, 3, 4]
    return src, dst, rs.randint(4, 10, 120).astype(float).tolist() + [2.0, 1.5, 0.25, 0.75]


USER_EDGES = _user_edges()
HITS_CASES = ["wide", "rows", "skew", "skew+users"]


@functools.lru_cache(maxsize=None)
def hits_csr(name):
    """(row_ptr, col, w) of a HITS case; "+users" adds USER_EDGES through the product's own builder."""
    from n2v_hip import bine
    if name.endswith("+users"):
        g = graph(name[:-6])
        return bine.user_edges_csr(g, *USER_EDGES)[:3]
    g = graph(name)
    return g.row_ptr, g.col, g.w


def hits_vectors(name):
    """x for one spmv launch, and (h, a, h_last) for one normalise launch, of the case's size."""
    n = len(hits_csr(name)[0]) - 1
    rs = np.random.RandomState(n)
    return rs.random_sample(n) + 0.01, (rs.random_sample(n) * 7, rs.random_sample(n) * 3, rs.random_sample(n))


NORMALISE_SIZES = [1, 5, 1023, 1024, 1025, 2049]    # beside the HITS cases' own n (2130, 137, 154)


def normalise_vectors(n):
    rs = np.random.RandomState(1000 + n)
    return rs.random_sample(n) * 7, rs.random_sample(n) * 3, rs.random_sample(n)


@functools.lru_cache(maxsize=None)
def hits_expected(name):
    return P.hits(*hits_csr(name))


# ------------------------------------------------------------------------------------------ walk counts
def _counts_case(kind, m, lo=0, maxT=8, minT=1, auth=True):
    return dict(kind=kind, m=m, lo=lo, maxT=maxT, minT=minT, auth=auth)


COUNTS_CASES = [
    _counts_case("eighths9", 9, minT=0), _counts_case("eighths9", 9, minT=3), _counts_case("eighths9", 9, auth=False),
    _counts_case("above", 50), _counts_case("negative", 50, minT=0), _counts_case("equal", 40, minT=0),
    _counts_case("equal", 40, minT=3), _counts_case("random", 1, lo=5), _counts_case("eighths", 1023, lo=5, minT=0),
    _counts_case("random", 1024, lo=7, maxT=32), _counts_case("random", 1025, lo=1, auth=False),
    _counts_case("eighths", 2049, lo=3), _counts_case("random", 300, maxT=0), _counts_case("zeros", 70, lo=2),
]


def counts_id(c):
    return "%s-%d-lo%d-T%d-%d%s" % (c["kind"], c["m"], c["lo"], c["maxT"], c["minT"], "" if c["auth"] else "-noauth")


def counts_data(c):
    """-> a fp64[lo + m + 2]: the kernel reads a[lo : lo + m]; the elements around are there to stay unread."""
    rs = np.random.RandomState(c["m"] * 7 + c["lo"])
    m = c["m"]
    seg = {"eighths9": lambda: np.arange(9) / 8.0,
           "eighths": lambda: np.concatenate([[0.0, 1.0], rs.randint(0, 9, m - 2) / 8.0]),
           "above": lambda: 100001.0 + 1000.0 * rs.random_sample(m),
           "negative": lambda: -rs.random_sample(m) - 0.25,
           "equal": lambda: np.full(m, 0.37),
           "zeros": lambda: np.zeros(m),
           "random": lambda: rs.random_sample(m)}[c["kind"]]()
    return np.concatenate([np.full(c["lo"], 1.0e9), seg, np.full(2, -1.0e9)])


# ------------------------------------------------------------------------------------------ walks
def _walk_case(g, side, reps, percentage=0.15, max_len=256, seed=2024, halves=False):
    return dict(graph=g, side=side, reps=reps, percentage=percentage, max_len=max_len, seed=seed, halves=halves)


WALK_CASES = [
    _walk_case("skew", "u", 2), _walk_case("skew", "v", 6, seed=77), _walk_case("skew", "v", 4, seed=2**63 + 9, halves=True),
    _walk_case("deadend", "u", 3), _walk_case("deadend", "v", 5, halves=True), _walk_case("pair", "u", 9),
    _walk_case("pair", "v", 5), _walk_case("skew", "u", 1, percentage=0.0, max_len=5),
    _walk_case("skew", "u", 1, percentage=1.0), _walk_case("skew", "u", 1, percentage=3.5),
    _walk_case("skew", "u", 1, max_len=1),
    # more than 4 x 8192 walks: the grid-stride loop of bine_walk_kernel takes a second trip (short walks: cheap)
    _walk_case("deadend", "u", 1700, percentage=0.93, max_len=3, seed=5),
]


def walk_id(c):
    return "%s-%s-x%d-p%g-L%d-s%d%s" % (c["graph"], c["side"], c["reps"], c["percentage"], c["max_len"], c["seed"] % 1000,
                                        "-halves" if c["halves"] else "")


@functools.lru_cache(maxsize=None)
def _walk_expected(key):
    c = WALK_CASES[key]
    g, c2 = graph(c["graph"]), cum2(c["graph"])
    lo, hi = side_range(g, c["side"])
    node = np.repeat(np.arange(lo, hi, dtype=np.int32), c["reps"])
    lens = np.array([bo.walk_length(g.row_ptr, c2, int(v), i, c["percentage"], c["max_len"], c["seed"])
                     for i, v in enumerate(node)], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens.astype(np.int64))]).astype(np.int64)
    stats = {}
    tokens = np.concatenate([bo.device_walk(g.row_ptr, g.col, c2, int(v), i, int(lens[i]), c["seed"], stats)
                             for i, v in enumerate(node)]).astype(np.int32)
    return node, lens, off, tokens, stats


def walk_expected(c):
    """-> (walk_node int32, lens int32, walk_off int64, tokens int32, branch stats), computed once per process."""
    return _walk_expected(WALK_CASES.index(c))


# ------------------------------------------------------------------------------------------ pools
def _pool_case(g, side, pool_size, max_jaccard, seed=31, rows=None):
    return dict(graph=g, side=side, pool_size=pool_size, max_jaccard=max_jaccard, seed=seed, rows=rows)


POOL_CASES = [
    _pool_case("deadend", "u", 1, 0.1), _pool_case("deadend", "u", 24, 0.0), _pool_case("deadend", "v", 64, 1.0),
    _pool_case("deadend", "u", 65, 0.1), _pool_case("deadend", "v", 130, 0.1),
    _pool_case("skew", "u", 24, 0.1), _pool_case("skew", "v", 65, 0.1, seed=2**40 + 3),
    _pool_case("dense", "u", 24, 0.0), _pool_case("dense", "v", 65, 0.0),
    _pool_case("single_user", "u", 24, 0.1), _pool_case("single_user", "v", 65, 0.1),
    _pool_case("pair", "u", 130, 0.1), _pool_case("pair", "v", 1, 0.1),
    _pool_case("deadend", "u", 24, 0.1, rows=(3, 11)), _pool_case("skew", "u", 65, 0.1, rows=(5, 10)),
]


def pool_id(c):
    return "%s-%s-p%d-j%g-s%d%s" % (c["graph"], c["side"], c["pool_size"], c["max_jaccard"], c["seed"] % 1000,
                                    "-rows%d_%d" % c["rows"] if c["rows"] else "")


def pool_rows(c):
    """(side_lo, side_hi, v_begin, v_end)"""
    lo, hi = side_range(graph(c["graph"]), c["side"])
    return (lo, hi, lo + c["rows"][0], lo + c["rows"][1]) if c["rows"] else (lo, hi, lo, hi)


@functools.lru_cache(maxsize=None)
def _pool_expected(key):
    c = POOL_CASES[key]
    g = graph(c["graph"])
    lo, hi, vb, ve = pool_rows(c)
    stats = {}
    rows = [bo.neg_pool(g.row_ptr, g.col, lo, hi, v, c["pool_size"], c["max_jaccard"], c["seed"], stats)
            for v in range(vb, ve)]
    return np.array(rows, dtype=np.int32).reshape(ve - vb, c["pool_size"]), stats


def pool_expected(c):
    return _pool_expected(POOL_CASES.index(c))


# ------------------------------------------------------------------------------------------ init
INIT_DIMS = [1, 2, 63, 64, 65, 100, 511, 512]
INIT_ROWS = [1, 2, 3, 6]         # 2 n jobs, four per workgroup: 2 and 6 rows end in a workgroup with idle waves
INIT_SEED = 0x9E3779B97F4A7C15
INIT_CASES = [(n, d) for d in INIT_DIMS for n in INIT_ROWS] + [(3, 64, 128), (2, 100, 512)]   # (n, dim[, row_stride])


def init_stride(c):
    return c[2] if len(c) > 2 else next(s for s in (64, 128, 256, 512) if s >= c[1])


@functools.lru_cache(maxsize=None)
def init_uniforms(dim):
    return P.init_uniforms(max(INIT_ROWS), dim, INIT_SEED)


def init_expected(c):
    return P.init_tables(init_uniforms(c[1])[:, :c[0]], init_stride(c))


# ------------------------------------------------------------------------------------------ engine path
def _engine_case(g, seed, maxT=3, pool_size=24, max_jaccard=0.1, dim=20, walks=True):
    return dict(graph=g, seed=seed, maxT=maxT, pool_size=pool_size, max_jaccard=max_jaccard, dim=dim, walks=walks)


ENGINE_CASES = [_engine_case("skew", 2024), _engine_case("deadend", 7, maxT=4, dim=100),
                _engine_case("wide", 1, walks=False), _engine_case("rows", 1, walks=False)]


@functools.lru_cache(maxsize=None)
def _engine_expected(key):
    from n2v_hip import bine
    c = ENGINE_CASES[key]
    g, c2 = graph(c["graph"]), cum2(c["graph"])
    a, iters = hits_expected(c["graph"])
    out = dict(authority=a, iterations=iters)
    if not c["walks"]:
        return out
    counts, auth = np.zeros(g.n, np.int32), np.zeros(g.n)
    for lo, hi in ((0, g.n_u), (g.n_u, g.n)):
        counts[lo:hi], auth[lo:hi] = P.walk_counts(a, lo, hi, c["maxT"], 1)
    node = np.repeat(np.arange(g.n, dtype=np.int32), counts)
    nw_u = int(counts[:g.n_u].sum())
    walks = []
    for i, v in enumerate(node):
        seed = bine.derive_seed(c["seed"], bine.SEED_WALK_U if i < nw_u else bine.SEED_WALK_V)
        gw = i if i < nw_u else i - nw_u
        L = bo.walk_length(g.row_ptr, c2, int(v), gw, 0.15, bine.MAX_WALK_LEN, seed)
        walks.append(bo.device_walk(g.row_ptr, g.col, c2, int(v), gw, L, seed))
    pool = np.array([bo.neg_pool(g.row_ptr, g.col, *((0, g.n_u) if v < g.n_u else (g.n_u, g.n)), v, c["pool_size"],
                                 c["max_jaccard"],
                                 bine.derive_seed(c["seed"], bine.SEED_POOL_U if v < g.n_u else bine.SEED_POOL_V))
                     for v in range(g.n)], dtype=np.int32)
    emb, ctx = P.init_tables(P.init_uniforms(g.n, c["dim"], bine.derive_seed(c["seed"], bine.SEED_INIT)),
                             next(s for s in (64, 128, 256, 512) if s >= c["dim"]))
    out.update(counts=counts, auth=auth, node=node, n_walks=(nw_u, len(node) - nw_u),
               off=np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.int64),
               tokens=np.concatenate(walks).astype(np.int32), pool=pool, emb=emb, ctx=ctx)
    return out


def engine_expected(c):
    return _engine_expected(ENGINE_CASES.index(c))


# ------------------------------------------------------------------------------------------ launches
# The arguments of every C-ABI call the GPU test makes, as numpy arrays of exactly the sizes it uploads; outputs are
# pre-filled so that an element the kernel must not write can be told from one it wrote.  The host test replays these.
FILL_I, FILL_F = -7, -7.0


def spmv_launch(name):
    row_ptr, col, w = hits_csr(name)
    n = len(row_ptr) - 1
    return dict(n_rows=n, row_ptr=row_ptr, col=col, w=w, x=hits_vectors(name)[0], y=np.full(n, FILL_F))


def normalise_launch(key):
    """key: a HITS case (its n) or one of NORMALISE_SIZES"""
    h, a, h_last = hits_vectors(key)[1] if isinstance(key, str) else normalise_vectors(key)
    return dict(n=len(h), h=h.copy(), a=a.copy(), h_last=h_last, state=np.full(1, FILL_F))


def counts_launch(c):
    a = counts_data(c)
    return dict(a=a, lo=c["lo"], hi=c["lo"] + c["m"], maxT=c["maxT"], minT=c["minT"],
                counts=np.full(len(a), FILL_I, np.int32), auth_out=np.full(len(a), FILL_F) if c["auth"] else None)


def walk_launches(c):
    """-> ([launch], tokens): one launch, or two halves of which the second carries gw_base.  A launch holds the
    arguments of n2v_bine_walk_lengths (lens) and of n2v_bine_walk (walk_off, from bo.walk_length); `tokens` is the one
    array all launches of the case write into."""
    g = graph(c["graph"])
    node, lens, off, tokens, _ = walk_expected(c)
    nw = len(node)
    parts = [(0, nw // 2), (nw // 2, nw)] if c["halves"] else [(0, nw)]
    launches = [dict(row_ptr=g.row_ptr, col=g.col, cum2=cum2(c["graph"]), walk_node=node[b:e].copy(),
                     walk_off=off[b:e + 1].copy(), n_walks=e - b, gw_base=b, first=b, percentage=c["percentage"],
                     max_len=c["max_len"], seed=c["seed"], lens=np.full(e - b, FILL_I, np.int32)) for b, e in parts]
    return launches, np.full(len(tokens), FILL_I, np.int32)


def pool_launch(c):
    g = graph(c["graph"])
    lo, hi, vb, ve = pool_rows(c)
    return dict(row_ptr=g.row_ptr, col=g.col, side_lo=lo, side_hi=hi, v_begin=vb, v_end=ve, pool_size=c["pool_size"],
                max_jaccard=c["max_jaccard"], seed=c["seed"], pool=np.full((ve - vb) * c["pool_size"], FILL_I, np.int32))


def init_launch(c):
    n, dim, stride = c[0], c[1], init_stride(c)
    return dict(emb=np.full(n * stride, FILL_F), ctx=np.full(n * stride, FILL_F), n=n, dim=dim, row_stride=stride,
                seed=INIT_SEED)
