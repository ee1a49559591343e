"""TEST INFRASTRUCTURE — inputs that push the rating kernels past the thresholds of their second level, and plain numpy
models of those second levels with one deliberate error each.

The builders are numpy only and deterministic.  The models restate PARTITIONS AND INDEX ARITHMETIC, not sums
(csrc/n2v_compact.h: compact_scan_kernel; csrc/n2v_eccstats.hip: tile_scan_kernel, groups_number_kernel's gap loops,
seg_long_kernel's stride loop; csrc/n2v_eccknn.hip: sim_sparse_kernel's tile decode).  tests/test_scale_cases_host.py
asserts with them that every case below crosses the threshold it is named after and that a wrong second level changes
the result there and nowhere in the cases the suite held before; tests/test_gpu_scale_paths.py then compares the
kernels with the restatements by equality on exactly these inputs.

Cases
  scan     n_tiles in N_TILES tiles of TILE elements: the one-workgroup scans give each of SCAN_WIDTH threads
           per = ceil(n_tiles / SCAN_WIDTH) tiles.  256: per = 1 (the last one-level size); 257 and 511: per = 2 with a last
           range of one tile; 513: per = 3 and 171 full ranges; 515: per = 3 with a last range of two
  select   a keep pattern whose tiles hold 0, a few, about half or all TILE elements
  pairs    runs of equal keys at 257 tiles;  join: supports around min_count at 257 tiles
  groups   sorted (item, window) keys: groups of 1 .. 5 rows, one of 3 * TILE + 7 rows from the middle of a tile, items
           without a row before the first, between and after the last present one
  segsum   2 * 4 * LONG_BLOCKS + 3 segments of 64 / 65 elements among short ones: the queue is drained in three passes
  chain    532 999 rows, 8 200 users of 64 .. 66 rows, 3 000 items, six windows, one group of more than three tiles
  sparse   48 x 48 tiles of 64 rows, four rated rows in each: 1 176 triangle tiles to decode
"""
import functools
import math

import numpy as np

# ---- the constants of the kernels that the models restate (tests/test_scale_cases_host.py reads them from the sources) --
TILE = 2048           # n2v_eccstats.hip TILE == n2v_sim.h N2V_ECCSPLIT_TILE: rows per workgroup of the tile passes
SCAN_WIDTH = 256      # threads of tile_scan_kernel and of compact_scan_kernel
LONG_SEG = 64         # n2v_eccstats.hip: a segment of at least this many elements is queued for a wavefront
LONG_BLOCKS = 2048    # n2v_eccstats.hip: workgroups of seg_long_kernel, four wavefronts each
CHUNK = 4096          # n2v_sim.h N2V_ECCSTATS_CHUNK
TOTAL_WIDTH = 64      # total_kernel adds 64 chunk sums per round
TB = 64               # n2v_eccknn.hip: rows of a similarity tile

N_TILES = (256, 257, 511, 513, 515)
EXACT = 511           # the size that is a whole number of tiles; the others end three elements early
SCAN_PAD = 4          # sentinel words the GPU tests keep behind the scratch: an unclamped tail range lands there
SENTINEL = -7         # what those words (and every integer output) hold before a launch

N_LONG = 2 * 4 * LONG_BLOCKS + 3
MOMENT_N = (128 * CHUNK, 128 * CHUNK + 1, 129 * CHUNK + 1)
LONG_GROUP = 3 * TILE + 7
SPARSE_T, SPARSE_NY = 48, 40
SPARSE_NX = SPARSE_T * TB - 5

# the largest inputs the suite gave these paths before: 2 * TILE + 5 elements, eight queued segments, five tiles a side
OLD_ELEMENTS = 2 * TILE + 5
OLD_LONG = 8
OLD_T = 5


def n_elements(n_tiles, tile=TILE):
    return n_tiles * tile - (0 if n_tiles == EXACT else 3)


# ---------------------------------------------------------------------------------------------------------- models

def scan_ranges(n_tiles, variant=None):
    """[(lo, hi)] of the SCAN_WIDTH threads.  variant "floor": per = n_tiles // SCAN_WIDTH, and 1 where that is 0 (the
    one-tile-per-thread form that every earlier case runs); "unclamped": a thread that starts inside the array takes
    `per` tiles whether or not they exist."""
    per = -(-n_tiles // SCAN_WIDTH)
    if variant == "floor":
        per = max(n_tiles // SCAN_WIDTH, 1)
    out = []
    for t in range(SCAN_WIDTH):
        lo = min(t * per, n_tiles)
        hi = min(lo + per, n_tiles)
        if variant == "unclamped" and lo < n_tiles:
            hi = lo + per
        out.append((lo, hi))
    return out


def scan_model(counts, variant=None, beyond=SENTINEL):
    """(exclusive offsets of the n_tiles counts, total) as the two-level scan forms them: range sums, a serial scan of the
    SCAN_WIDTH range sums, then every range again from its offset.  A tile no range covers keeps its count, as the
    in-place kernel would leave it; what a range reads past the array is `beyond`."""
    counts = np.asarray(counts, dtype=np.int64)
    n_tiles = len(counts)
    ranges = scan_ranges(n_tiles, variant)
    reach = max(n_tiles, max(hi for _, hi in ranges))
    cells = np.concatenate([counts, np.full(reach - n_tiles, beyond, dtype=np.int64)])
    part = np.array([cells[lo:hi].sum() for lo, hi in ranges], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(part)])
    for (lo, hi), run in zip(ranges, start[:-1]):
        seg = cells[lo:hi].copy()
        cells[lo:hi] = run + np.concatenate([[0], np.cumsum(seg)[:-1]]) if hi > lo else seg
    return cells[:n_tiles], int(start[-1])


def tile_counts(flags, tile=TILE):
    """Set flags per tile."""
    flags = np.asarray(flags, dtype=np.int64)
    n_tiles = -(-len(flags) // tile)
    body = np.zeros(n_tiles * tile, dtype=np.int64)
    body[:len(flags)] = flags
    return body.reshape(n_tiles, tile).sum(axis=1)


def compact_model(flags, variant=None, tile=TILE):
    """(slot of every kept element, count) of the stable compaction: tile offset + kept elements before it in the tile."""
    flags = np.asarray(flags, dtype=bool)
    off, total = scan_model(tile_counts(flags, tile), variant)
    k = np.nonzero(flags)[0]
    before_tile = np.concatenate([[0], np.cumsum(tile_counts(flags, tile))])[k // tile]
    rank = np.arange(len(k)) - before_tile                                # kept elements before it in its own tile
    return off[k // tile] + rank, total


def queue_waves(n_seg):
    """Wavefronts that seg_long_kernel is launched with for n_seg segments."""
    return 4 * min((n_seg + 3) // 4, LONG_BLOCKS)


def drained(n_long, n_seg, variant=None):
    """Queue positions that some wavefront takes.  variant "first_pass": every wavefront takes one and stops."""
    n_waves = queue_waves(n_seg)
    if variant == "first_pass":
        return np.arange(min(n_long, n_waves))
    if n_long == 0:
        return np.zeros(0, dtype=np.int64)
    return np.sort(np.concatenate([np.arange(w, n_long, n_waves) for w in range(min(n_waves, n_long))]))


def drain_passes(n_long, n_seg):
    return -(-n_long // queue_waves(n_seg))


def item_gptr_model(group_item, n_items, variant=None):
    """item_gptr as groups_number_kernel writes it: the head of an item's first group fills the items since the previous
    head's, the last row fills what follows.  variant "no_gap": each writes its own item (and the end) alone; an item
    without a row keeps the sentinel."""
    group_item = np.asarray(group_item, dtype=np.int64)
    out = np.full(n_items + 1, SENTINEL, dtype=np.int64)
    prev = -1
    for g, item in enumerate(group_item.tolist()):
        if item != prev:
            out[(item if variant == "no_gap" else prev + 1):item + 1] = g
        prev = item
    out[(n_items if variant == "no_gap" else prev + 1):] = len(group_item)
    return out


def tile_start(ti, T):
    """Linear index of tile (ti, ti): the upper triangle row by row."""
    return ti * T - ti * (ti - 1) // 2


def decode(b, T, variant=None):
    """(ti, tj) of linear block b as sim_sparse_kernel finds it: a double-precision sqrt guess, clamped, then two
    correcting loops.  variant "guess": the loops left out."""
    td = float(2 * T + 1)
    ti = min(max(int((td - math.sqrt(td * td - 8.0 * float(b))) * 0.5), 0), T - 1)
    if variant is None:
        while ti + 1 < T and tile_start(ti + 1, T) <= b:
            ti += 1
        while ti > 0 and tile_start(ti, T) > b:
            ti -= 1
    return ti, ti + (b - tile_start(ti, T))


def decode_all(T, variant=None):
    return [decode(b, T, variant) for b in range(T * (T + 1) // 2)]


def guessed_rows(T):
    """The clamped sqrt guess of every block at once (np.sqrt and math.sqrt are both the correctly rounded one)."""
    b = np.arange(T * (T + 1) // 2, dtype=np.float64)
    td = float(2 * T + 1)
    return np.clip(((td - np.sqrt(td * td - 8.0 * b)) * 0.5).astype(np.int64), 0, T - 1)


# -------------------------------------------------------------------------------------------------------- builders

DENSITY = ("none", "few", "half", "all")


def keep_pattern(n_tiles, tile=TILE, seed=0):
    """(keep bool[n], density name of every tile).  Tile 5 is empty and tile 6 full, and so are the two tiles before the
    last; the last tile holds one kept element."""
    n = n_elements(n_tiles, tile)
    rs = np.random.RandomState(7000 + n_tiles + seed)
    kind = rs.randint(0, 4, size=n_tiles)
    kind[5], kind[6] = 0, 3
    kind[n_tiles - 3], kind[n_tiles - 2] = 0, 3
    keep = np.zeros(n_tiles * tile, dtype=bool)
    for t in range(n_tiles - 1):
        cell = keep[t * tile:(t + 1) * tile]
        if kind[t] == 1:
            cell[rs.choice(tile, 3, replace=False)] = True
        elif kind[t] == 2:
            cell[:] = rs.random_sample(tile) < 0.5
        elif kind[t] == 3:
            cell[:] = True
    kind[n_tiles - 1] = 1
    keep[(n_tiles - 1) * tile + int(rs.randint(0, tile - 3))] = True
    return keep[:n], [DENSITY[k] for k in kind]


SELECT_BINS = np.array([1, 2, 3, 1, 2, 3, 5, 5, 1], dtype=np.int32)    # bin 4: no user at all
SELECT_WHICH = 3


@functools.lru_cache(maxsize=None)
def select_case(n_tiles, tile=TILE):
    """(user int64[n], bins, which, keep): rows of bin `which` exactly where keep is set."""
    keep, _ = keep_pattern(n_tiles, tile)
    rs = np.random.RandomState(7100 + n_tiles)
    inside = np.nonzero(SELECT_BINS == SELECT_WHICH)[0]
    outside = np.nonzero(SELECT_BINS != SELECT_WHICH)[0]
    user = np.where(keep, inside[rs.randint(0, len(inside), size=len(keep))], outside[rs.randint(0, len(outside), size=len(keep))])
    return user.astype(np.int64), SELECT_BINS, SELECT_WHICH, keep


@functools.lru_cache(maxsize=None)
def pairs_case(n_tiles=257, tile=TILE):
    """(key unsorted int64[n], w fp64[n], n_nodes, last bool[n] over the SORTED keys): a key run ends where `last` is set,
    and the runs follow the select pattern (a tile of single keys, a tile inside one run, ...)."""
    last, _ = keep_pattern(n_tiles, tile, seed=1)
    last = last.copy()
    last[-1] = True
    n = len(last)
    run = np.concatenate([[0], np.cumsum(last)[:-1]])                     # run number of every sorted position
    n_runs = int(last.sum())
    n_nodes = n_runs + 11
    a = np.arange(n_runs, dtype=np.int64)
    key_sorted = (a * n_nodes + (a * 7 + 3) % n_nodes)[run]
    rs = np.random.RandomState(7200 + n_tiles)
    key = key_sorted[rs.permutation(n)]
    w = rs.permutation(n).astype(np.float64) + 0.25                       # every weight distinct: the survivor is named
    return key, w, n_nodes, last


@functools.lru_cache(maxsize=None)
def join_case(n_tiles=257, tile=TILE, min_count=4):
    """(v1, v2, c1, c2, min_count): both supports above min_count exactly where the keep pattern is set; elsewhere one
    of them is min_count, 0, or below."""
    keep, _ = keep_pattern(n_tiles, tile, seed=2)
    n = len(keep)
    rs = np.random.RandomState(7300 + n_tiles)
    c1, c2 = rs.randint(min_count + 1, min_count + 6, size=n), rs.randint(min_count + 1, min_count + 6, size=n)
    low = np.array([0, 1, min_count])[rs.randint(0, 3, size=n)]
    side = rs.randint(0, 2, size=n).astype(bool)
    c1 = np.where(~keep & side, low, c1)
    c2 = np.where(~keep & ~side, low, c2)
    return rs.normal(size=n), rs.normal(size=n), c1.astype(np.int64), c2.astype(np.int64), min_count


GROUP_NTW = 6
GROUP_LEAD = 3        # items 0 .. 2 have no row
GROUP_HOLE = 7        # a run of at least this many absent items in the middle
GROUP_TRAIL = 4       # absent items after the last present one
GROUP_LONG_AT = 10 * TILE + 1000


@functools.lru_cache(maxsize=None)
def groups_case(n_tiles, tile=TILE):
    """dict(key int64[n] ascending, perm int64[n], n_tw, n_items, unum int64[n_groups], group_item int64[n_groups])."""
    n = n_elements(n_tiles, tile)
    rs = np.random.RandomState(7400 + n_tiles)
    long_at, long_len = 10 * tile + 1000, 3 * tile + 7

    def short_groups(total):
        lens = rs.randint(1, 6, size=total // 2 + 8)
        lens = lens[:int(np.searchsorted(np.cumsum(lens), total)) + 1]
        lens[-1] -= lens.sum() - total
        return lens[lens > 0]

    unum = np.concatenate([short_groups(long_at), [long_len], short_groups(n - long_at - long_len)]).astype(np.int64)
    n_groups = len(unum)
    step = rs.choice([1, 2, 3, 7, 13], size=n_groups, p=[0.35, 0.3, 0.2, 0.1, 0.05]).astype(np.int64)
    step[0] = GROUP_LEAD * GROUP_NTW + 2                                  # the first key: item GROUP_LEAD, window 2
    step[n_groups // 2] = (GROUP_HOLE + 1) * GROUP_NTW
    gkey = np.cumsum(step)
    group_item = gkey // GROUP_NTW
    return dict(key=np.repeat(gkey, unum), perm=rs.permutation(n).astype(np.int64), n_tw=GROUP_NTW,
                n_items=int(group_item[-1]) + 1 + GROUP_TRAIL, unum=unum, group_item=group_item)


def groups_expected(case):
    """(row_group int32[n] by row, group_begin int64[n_groups + 1], item_gptr int64[n_items + 1], counts) in plain numpy."""
    key, perm, unum = case["key"], case["perm"], case["unum"]
    head = np.concatenate([[True], key[1:] != key[:-1]])
    row_group = np.empty(len(key), dtype=np.int32)
    row_group[perm] = np.cumsum(head) - 1
    group_begin = np.concatenate([[0], np.cumsum(unum)]).astype(np.int64)
    item_gptr = np.searchsorted(case["group_item"], np.arange(case["n_items"] + 1)).astype(np.int64)
    return row_group, group_begin, item_gptr, (len(unum), int(unum.max()))


@functools.lru_cache(maxsize=None)
def segsum_case():
    """dict(lens, ptr, a, perm, idx, g): N_LONG segments of 64 and 65 elements alternating, a short one (0, 1 or 63
    elements) after each, so the segment a queue entry names is never its position in the queue."""
    j = np.arange(N_LONG)
    short = np.where(j % 16 == 5, 63, (j // 2) % 2)
    lens = np.stack([LONG_SEG + j % 2, short], axis=1).reshape(-1).astype(np.int64)
    n = int(lens.sum())
    rs = np.random.RandomState(7500)
    n_g = 1000
    return dict(lens=lens, ptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), a=rs.uniform(0.1, 5.0, size=n),
                perm=rs.permutation(n).astype(np.int64), idx=rs.randint(0, n_g, size=n).astype(np.int32), g=rs.normal(size=n_g))


def moments_case(n):
    rs = np.random.RandomState(n % 100003)
    x = rs.uniform(-3.0, 7.0, size=n) * 10.0 ** rs.randint(-3, 4, size=n)
    x[rs.randint(0, n)] = 0.0
    x[rs.randint(0, n)] = -0.0
    return x


CHAIN_USERS, CHAIN_ITEMS, CHAIN_WINDOWS, CHAIN_ROWS = 8200, 3000, 6, 532999
CHAIN_SEED = 41


@functools.lru_cache(maxsize=None)
def chain_case():
    """(uid, id, feedback, timewindow) of CHAIN_ROWS shuffled rows: user u has 64 + u % 3 of them, items follow a
    squared uniform, LONG_GROUP rows are moved into one (item, window) group."""
    rs = np.random.RandomState(CHAIN_SEED)
    u = np.repeat(np.arange(CHAIN_USERS), LONG_SEG + np.arange(CHAIN_USERS) % 3)
    n = len(u)
    i = np.minimum((CHAIN_ITEMS * rs.random_sample(n) ** 2).astype(np.int64), CHAIN_ITEMS - 1)
    tw = 201001 + rs.randint(0, CHAIN_WINDOWS, size=n)
    planted = rs.choice(n, LONG_GROUP, replace=False)
    i[planted], tw[planted] = 7, 201003
    order = rs.permutation(n)
    return u[order].astype(np.int64), i[order], rs.uniform(0.1, 5.0, size=n), tw[order].astype(np.int64)


@functools.lru_cache(maxsize=None)
def sparse_case():
    """dict(x, y, r, w, rated): SPARSE_NX rows in SPARSE_T tiles, four rated rows per tile at offsets drawn per tile, eight
    to twelve ratings each over SPARSE_NY columns, the ratings in a shuffled (training) order."""
    rs = np.random.RandomState(7600)
    rated = np.concatenate([t * TB + np.sort(rs.choice(min(TB, SPARSE_NX - t * TB), 4, replace=False)) for t in range(SPARSE_T)])
    x, y = [], []
    for row in rated.tolist():
        ys = rs.choice(SPARSE_NY, int(rs.randint(8, 13)), replace=False)
        x += [row] * len(ys)
        y += ys.tolist()
    order = rs.permutation(len(x))
    x, y = np.array(x, dtype=np.int64)[order], np.array(y, dtype=np.int64)[order]
    return dict(x=x, y=y, r=rs.uniform(0.5, 5.0, size=len(x)), w=rs.normal(size=SPARSE_NY), rated=rated)
