"""TEST INFRASTRUCTURE — the case table of tests/test_gpu_bine_lsh_edges.py, shared with tests/test_lsh_cases_host.py.
numpy only: neither torch nor the engine is imported here.

Every graph is an edge list (user labels, item labels) for bine.BipartiteGraph.  Labels are integers, so a vertex's
id is the rank of its label and the builders place vertices at the ids they choose; the kernels hash the decimal
text of the label.

The duplicate-group family: users of one group rate the same 3 private items and nothing else, groups are disjoint.
Identical neighbour sets give identical signatures, so the deepest prefix range of every tree is exactly the group
(ties in sorted order = ascending id); disjoint sets never share a MinHash value, so no lower level adds a key.  The
group's items have the group's members as neighbours: item degrees are the group sizes, and the 3 items of a group
are a duplicate group of the item side.

What each case reaches is not claimed here but asserted, on the CPU, by tests/test_lsh_cases_host.py."""
import functools
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name graph k pool_size groups")

SET_SLOTS = 512
ITEM_BASE = 100000            # item labels: ITEM_BASE + item id (the two sides are separate label spaces anyway)


def set_home(key):
    """csrc/n2v_lsh.hip `set_home`: (key * 2654435761 mod 2^32) >> 23."""
    return ((int(key) * 2654435761) & 0xFFFFFFFF) >> 23


def _groups_graph(ids_of_groups):
    """ids_of_groups: one array of user ids per group.  Group g rates items 3g, 3g+1, 3g+2."""
    users, items = [], []
    for gi, ids in enumerate(ids_of_groups):
        for u in ids:
            for c in range(3):
                users.append(int(u))
                items.append(ITEM_BASE + 3 * gi + c)
    return np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)


BASE_SIZES = (63, 64, 65, 129, 300) + (1,) * 10


@functools.lru_cache(maxsize=None)
def base_graph():
    """631 users in duplicate groups of 63, 64, 65, 129 and 300 plus 10 singletons, 45 items; user ids permuted by a
    fixed seed so that the groups interleave."""
    n_u = sum(BASE_SIZES)
    perm = np.random.RandomState(20).permutation(n_u)
    cuts = np.cumsum((0,) + BASE_SIZES)
    return _groups_graph([np.sort(perm[cuts[i]:cuts[i + 1]]) for i in range(len(BASE_SIZES))])


WIDE_USERS, WIDE_GROUP = 2100, 260


@functools.lru_cache(maxsize=None)
def wide_graph():
    """2100 users (66 bitmap words): one duplicate group of 260, the rest singletons with one private item each.  The
    group holds EVERY id below 2100 whose home slot in the 512-slot LDS hash is 506 or above (more keys than the
    slots 506…511 can hold: the chain runs over the end of the table), four consecutive ids at the front so that two
    wavefronts of one workgroup query the same list, and random ids for the rest."""
    rs = np.random.RandomState(21)
    tail = [v for v in range(WIDE_USERS) if set_home(v) >= 506]
    chosen = set(tail) | {0, 1, 2, 3}
    rest = [v for v in rs.permutation(WIDE_USERS) if v not in chosen]
    chosen |= set(int(v) for v in rest[:WIDE_GROUP - len(chosen)])
    group = np.array(sorted(chosen))
    users, items = _groups_graph([group])
    singles = np.array([v for v in range(WIDE_USERS) if v not in chosen])
    users = np.concatenate([users, singles])
    items = np.concatenate([items, ITEM_BASE + 3 + np.arange(len(singles))])
    return users, items


COUNT_POOL = 1844             # 2100 - 256: what the 260-group's leaders have left at k = 256


@functools.lru_cache(maxsize=None)
def wide_count_graph():
    """2100 users in nine duplicate groups: one of 260 that holds every id from 2048 up (so its 256-key list sets bits
    in bitmap words 64 and 65, which only the second trip of the 64-lane popcount loop reads) and eight of 230.  With
    pool_size = 1844 the 260-group's five leaders have exactly pool_size vertices left — the count decides, and it is
    only right with words 64 and 65 in it — while the others have 1870 and draw 1844 of them."""
    rs = np.random.RandomState(25)
    high = list(range(2048, WIDE_USERS))
    low = rs.permutation(2048)
    first = np.array(sorted(high + [int(v) for v in low[:WIDE_GROUP - len(high)]]))
    rest = low[WIDE_GROUP - len(high):]
    return _groups_graph([first] + [np.sort(rest[i * 230:(i + 1) * 230]) for i in range(8)])


@functools.lru_cache(maxsize=None)
def tiny_graph():
    """41 users, k = 1, pool_size = 30: 41 > k (k + 1) + pool_size, so the kernel draws without counting, and 64 lanes
    draw from 41 vertices.  Duplicate groups of 3, 2 and 2 among singletons: at k = 1 a group's query list is its
    lowest id alone, so its other members are missing from their own lists."""
    sizes = (3, 2, 2) + (1,) * 34
    perm = np.random.RandomState(22).permutation(sum(sizes))
    cuts = np.cumsum((0,) + sizes)
    return _groups_graph([np.sort(perm[cuts[i]:cuts[i + 1]]) for i in range(len(sizes))])


@functools.lru_cache(maxsize=None)
def one_item_graph():
    """7 users on ONE item: an item side of one vertex (its row is all -1), a user side that is one duplicate group."""
    return np.arange(7, dtype=np.int64), np.full(7, ITEM_BASE, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def two_item_graph():
    """6 users on two items, three on each: every vertex has the other group, or the other item, left to draw."""
    return np.arange(6, dtype=np.int64), ITEM_BASE + np.array([0, 1, 0, 1, 0, 1], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def overlap_graph():
    """600 users drawn from 100 prototype item sets with small edits: queries reach past the duplicates, lists are
    cut at k = 6 in the middle of a range, the leader sweep has chains (a vertex listed only by followers) and
    sim(j) reaches past sim(l).  With pool_size = 10 a row touches at most 10 of the side's 19 bitmap words, so a bit
    that an epilogue leaves behind is still there for the next leader."""
    rs = np.random.RandomState(23)
    n_u, n_v, protos = 600, 200, 100
    sets = [set(rs.choice(n_v, rs.randint(3, 10), replace=False).tolist()) for _ in range(protos)]
    users, items = [], []
    for u in range(n_u):
        s = set(sets[rs.randint(protos)])
        if u % 3 == 1:
            s.add(int(rs.randint(n_v)))
        if u % 3 == 2 and len(s) > 2:
            s.discard(sorted(s)[0])
        for i in sorted(s):
            users.append(u)
            items.append(ITEM_BASE + i)
    return np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)


GRAPHS = {"base": base_graph, "wide": wide_graph, "wide_count": wide_count_graph, "tiny": tiny_graph, "one_item": one_item_graph,
          "two_items": two_item_graph, "overlap": overlap_graph}

K_SWEEP = (1, 63, 64, 65, 200, 255, 256)
TIGHT_POOLS = (374, 375, 376)          # complement of the 300-group's leaders at k = 256 is 375
ROUND_POOLS = (1, 63, 64, 65, 200)
GROUPS = (1, 2, 1024)

CASES = (
    [Case("base_k%d" % k, "base", k, 24, 1024) for k in K_SWEEP] +
    [Case("base_tight%d" % ps, "base", 256, ps, 1024) for ps in TIGHT_POOLS] +
    [Case("base_pool%d" % ps, "base", 256, ps, 1024) for ps in ROUND_POOLS if ps != 200] +
    [Case("base_groups%d" % gr, "base", 256, 200, gr) for gr in GROUPS] +      # groups1024 IS the pool_size 200 case
    [Case("base_tight375_groups1", "base", 256, 375, 1),
     Case("wide", "wide", 256, 8, 1024),
     Case("wide_count", "wide_count", 256, COUNT_POOL, 1024),
     Case("tiny", "tiny", 1, 30, 1024),
     Case("one_item", "one_item", 256, 5, 1024),
     Case("two_items", "two_items", 256, 4, 1024),
     Case("overlap", "overlap", 6, 10, 4),
     Case("overlap_groups1", "overlap", 6, 10, 1)]
)
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------ label table
@functools.lru_cache(maxsize=None)
def label_table():
    """(user labels, item labels) of a graph whose 256 users fill the first 256-thread block of the label kernel and
    whose 46 items sit behind it: byte lengths 1 … 130 mixed on both sides, the SHA-1 padding boundaries (55 / 56:
    the length no longer fits the block; 63 / 64; 119 / 120: the same with two blocks) and 130 on the item side, and
    labels whose characters take 2, 3 and 4 bytes."""
    rs = np.random.RandomState(24)
    alphabet = np.array(list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_-."))
    users, seen = [], set()
    while len(users) < 256:
        s = "".join(alphabet[rs.randint(0, len(alphabet), 1 + (len(users) * 37) % 130)])
        if s not in seen:
            seen.add(s)
            users.append(s)
    users[10], users[77], users[200] = "héllo-" + users[10][:20], "节点7", "\U0001F600" * 16 + "x"
    items = ["~" + "q" * (n - 1) for n in (1, 55, 56, 63, 64, 119, 120, 130)]
    items += ["é" * 32, "节" * 21, "é" * 60, "zé" * 40, "节" * 40, "\U0001F600" * 14]  # 64 63 120 120 120 56 bytes
    while len(items) < 46:
        s = "".join(alphabet[rs.randint(0, len(alphabet), 1 + (len(items) * 29) % 130)])
        if s not in seen and s not in items:
            items.append(s)
    edge_users = list(users)
    edge_items = [items[i % len(items)] for i in range(len(users))]
    return edge_users, edge_items
