"""No GPU: the inputs of tests/scale_cases.py cross the thresholds they claim, read from the kernels' source text, and a
wrong second level — a model in plain numpy with one deliberate error — changes the result on them while it changes
nothing on the largest inputs the suite held before (2 * tile + 5 elements, eight queued segments, five tiles a side).
Conditions on the INPUTS of tests/test_gpu_scale_paths.py, not measurements."""
import os
import re

import numpy as np
import pytest

import consistency_reference as C
import eccknn_reference as E
import eccsplit_reference as S
import eccstats_reference as R
import scale_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "node2vec-by-ecc_amd", "csrc")
BIG = [n for n in sc.N_TILES if n > sc.SCAN_WIDTH]


def _text(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr int %s = (\w+);" % name, text)
    assert m, name
    return m.group(1)


# ---- thresholds: from the source text ------------------------------------------------------------------------------------

def test_constants_are_the_kernels_own():
    stats, compact, hdr = _text(CSRC, "n2v_eccstats.hip"), _text(CSRC, "n2v_compact.h"), _text(ROOT, "include", "n2v_sim.h")
    knn = _text(CSRC, "n2v_eccknn.hip")
    assert int(_const(stats, "TILE")) == sc.TILE
    assert int(_const(stats, "LONG_SEG")) == sc.LONG_SEG
    assert int(_const(stats, "LONG_BLOCKS")) == sc.LONG_BLOCKS
    assert _const(stats, "CHUNK") == "N2V_ECCSTATS_CHUNK" and _const(compact, "COMPACT_TILE") == "N2V_ECCSPLIT_TILE"
    assert re.search(r"#define N2V_ECCSPLIT_TILE %d\b" % sc.TILE, hdr) and re.search(r"#define N2V_ECCSTATS_CHUNK %d\b" % sc.CHUNK, hdr)
    # both scans: one workgroup of SCAN_WIDTH threads, per = ceil(n_tiles / SCAN_WIDTH), SCAN_WIDTH range sums scanned by thread 0
    for text, name in ((stats, "tile_scan_kernel"), (compact, "compact_scan_kernel")):
        body = text[text.index(name + "("):]
        body = body[:body.index("\n}\n")]
        assert re.search(r"__launch_bounds__\(%d\)\s+%s\(" % (sc.SCAN_WIDTH, name), text), name
        assert "part[%d]" % sc.SCAN_WIDTH in body and "per = (n_tiles + %d) / %d;" % (sc.SCAN_WIDTH - 1, sc.SCAN_WIDTH) in body, name
        assert "for (int i = 0; i < %d; ++i)" % sc.SCAN_WIDTH in body, name
        assert re.search(r"%s<<<1, %d, 0, s>>>" % (name, sc.SCAN_WIDTH), text), name
    # the queue: LONG_BLOCKS workgroups of four wavefronts, stride = all of them
    assert "(n_seg + 3) / 4 < LONG_BLOCKS ? (n_seg + 3) / 4 : LONG_BLOCKS" in stats
    assert "n_waves = gridDim.x * 4" in stats and "w += n_waves" in stats and "len >= LONG_SEG" in stats
    # the totals: one wavefront, TOTAL_WIDTH chunk sums a round
    total = stats[stats.index("total_kernel(const double"):]
    assert "base += %d" % sc.TOTAL_WIDTH in total[:total.index("\n}\n")] and "total_kernel<0><<<1, %d, 0, s>>>" % sc.TOTAL_WIDTH in stats
    # the decode: tiles of TB rows, the guess and its two loops
    assert re.search(r"constexpr int TB = %d;" % sc.TB, knn)
    assert "(td - sqrt(td * td - 8.0 * (double)b)) * 0.5" in knn and "while (ti + 1 < T" in knn and "while (ti > 0" in knn


# ---- the two-level scans ---------------------------------------------------------------------------------------------------

def test_scan_sizes_cross_the_one_tile_per_thread_form():
    assert set(sc.N_TILES) >= {256, 257, 511, 513} and sc.EXACT in sc.N_TILES
    last = {}
    for n_tiles in sc.N_TILES:
        n = sc.n_elements(n_tiles)
        assert -(-n // sc.TILE) == n_tiles and (n % sc.TILE == 0) == (n_tiles == sc.EXACT)
        ranges = [r for r in sc.scan_ranges(n_tiles) if r[1] > r[0]]
        per = -(-n_tiles // sc.SCAN_WIDTH)
        covered = np.concatenate([np.arange(lo, hi) for lo, hi in ranges])
        assert np.array_equal(covered, np.arange(n_tiles))               # the right partition: every tile once, in order
        assert all(hi - lo == per for lo, hi in ranges[:-1])
        last[n_tiles] = (per, ranges[-1][1] - ranges[-1][0])
    assert last[256] == (1, 1)                                           # the last size of the one-level form
    assert last[257] == (2, 1) and last[511] == (2, 1) and last[515] == (3, 2)    # per >= 2, the last range shorter than per
    assert last[513] == (3, 3)                                           # 171 whole ranges of three: only the idle tail is clamped
    assert all(last[n][0] >= 2 for n in BIG)


def _differs(counts, variant):
    right, wrong = sc.scan_model(counts), sc.scan_model(counts, variant)
    return not (np.array_equal(right[0], wrong[0]) and right[1] == wrong[1])


def test_scan_model_is_an_exclusive_scan():
    rs = np.random.RandomState(1)
    for n_tiles in (1, 2, 3, 255) + sc.N_TILES + (1000,):
        counts = rs.randint(0, sc.TILE + 1, size=n_tiles)
        off, total = sc.scan_model(counts)
        assert np.array_equal(off, np.cumsum(counts) - counts) and total == counts.sum()


@pytest.mark.parametrize("what", ["select", "pairs", "join", "groups"])
def test_a_wrong_partition_shows_on_the_new_sizes_only(what):
    counts = {}
    if what == "select":
        for n_tiles in sc.N_TILES:
            counts[n_tiles] = sc.tile_counts(sc.select_case(n_tiles)[3])
    elif what == "pairs":
        counts[257] = sc.tile_counts(sc.pairs_case()[3])
    elif what == "join":
        counts[257] = sc.tile_counts(sc.keep_pattern(257, seed=2)[0])
    else:
        for n_tiles in sc.N_TILES:
            key = sc.groups_case(n_tiles)["key"]
            counts[n_tiles] = sc.tile_counts(np.concatenate([[True], key[1:] != key[:-1]]))
    for n_tiles, c in counts.items():
        assert len(c) == n_tiles and c[-1] > 0
        # per = n_tiles // 256 drops the tiles past 256 * per: seen from 257 on; 256 is where floor and ceiling still agree
        assert _differs(c, "floor") == (n_tiles > sc.SCAN_WIDTH), (what, n_tiles)
        # a tail range that is not clamped reads the words behind the scratch (the GPU tests keep SCAN_PAD sentinels
        # there and look at them afterwards): seen where the last range is shorter than per
        per = -(-n_tiles // sc.SCAN_WIDTH)
        assert _differs(c, "unclamped") == (n_tiles % per != 0), (what, n_tiles)
        over = max(hi for _, hi in sc.scan_ranges(n_tiles, "unclamped")) - n_tiles
        assert 0 <= over <= sc.SCAN_PAD and (over > 0) == (n_tiles % per != 0)
    # the old suite could not see either: at most three tiles, whatever they hold
    rs = np.random.RandomState(2)
    for n in (1, sc.TILE - 1, sc.TILE, sc.TILE + 1, sc.OLD_ELEMENTS):
        for density in (0.0, 0.01, 0.5, 1.0):
            c = sc.tile_counts(rs.random_sample(n) < density)
            assert len(c) <= 3 and not _differs(c, "floor") and not _differs(c, "unclamped")


@pytest.mark.parametrize("n_tiles", sc.N_TILES)
def test_keep_pattern_has_tiles_of_very_different_counts(n_tiles):
    user, bins, which, keep = sc.select_case(n_tiles)
    _, kind = sc.keep_pattern(n_tiles)
    c = sc.tile_counts(keep)
    assert len(user) == sc.n_elements(n_tiles) and len(c) == n_tiles
    assert set(kind) == set(sc.DENSITY)
    assert (c == 0).sum() >= 10 and (c == 3).sum() >= 10 and (c == sc.TILE).sum() >= 10 and ((c > 900) & (c < 1150)).sum() >= 10
    after_empty = np.nonzero((c[:-1] == 0) & (c[1:] == sc.TILE))[0]
    assert {5, n_tiles - 3} <= set(after_empty.tolist())                 # an all-kept tile directly after an empty one
    assert c[-1] == 1                                                    # the last tile holds a single kept element
    want = S.rows_of_bin(user, bins, which)
    assert np.array_equal(want, np.nonzero(keep)[0]) and 0 < len(want) < len(user)
    slot, total = sc.compact_model(keep)
    assert total == len(want) and np.array_equal(slot, np.arange(len(want)))


def test_pairs_and_join_cases_hold_257_tiles():
    key, w, n_nodes, last = sc.pairs_case()
    assert -(-len(key) // sc.TILE) == 257 and len(np.unique(w)) == len(w)
    ks = np.sort(key, kind="stable")
    assert np.array_equal(np.append(ks[1:] != ks[:-1], True), last)
    runs = np.diff(np.concatenate([[-1], np.nonzero(last)[0]]))
    assert runs.max() > sc.TILE and (runs == 1).sum() > sc.TILE          # a run longer than a tile, a tile of single keys
    assert 2 * len(key) < 2 ** 31 and ks.max() < n_nodes * n_nodes
    v1, v2, c1, c2, mc = sc.join_case()
    ids = C.join(v1, v2, c1, c2, mc)[0]
    assert -(-len(v1) // sc.TILE) == 257 and np.array_equal(ids, np.nonzero(sc.keep_pattern(257, seed=2)[0])[0])
    assert len(C.join(v1, v2, c1, c2, mc, variant="ge")[0]) > len(ids)   # supports of exactly min_count are present
    assert ((c1 == 0) | (c2 == 0)).any()


# ---- groups ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_tiles", sc.N_TILES)
def test_group_keys_hold_every_stated_structure(n_tiles):
    case = sc.groups_case(n_tiles)
    key, unum, gi, n_items, n_tw = case["key"], case["unum"], case["group_item"], case["n_items"], case["n_tw"]
    n = len(key)
    assert n == sc.n_elements(n_tiles) == unum.sum() and (np.diff(key) >= 0).all() and key[0] >= 0
    assert np.array_equal(np.sort(case["perm"]), np.arange(n)) and not np.array_equal(case["perm"], np.arange(n))
    head = np.concatenate([[True], key[1:] != key[:-1]])
    begin = np.nonzero(head)[0]
    assert np.array_equal(np.diff(np.append(begin, n)), unum) and np.array_equal(key[begin] // n_tw, gi)
    assert set(range(1, 6)) <= set(unum.tolist()) and sorted(set(unum.tolist()))[-2:] == [5, sc.LONG_GROUP]
    on_first = begin[(begin % sc.TILE == 0) & (begin > 0)]               # a group that starts on a tile's first row:
    assert len(on_first) >= 10                                           # ... the one before it ends on a tile's last row
    g = int(np.argmax(unum))
    assert unum[g] == sc.LONG_GROUP and begin[g] == sc.GROUP_LONG_AT and begin[g] % sc.TILE == 1000
    heads_per_tile = sc.tile_counts(head)
    no_head = np.nonzero(heads_per_tile == 0)[0]
    assert no_head.tolist() == [11, 12]                                  # two whole tiles without a head: g = base - 1 there
    assert (begin % 64 == 0).sum() >= 1000 and (begin % 64 == 63).sum() >= 1000      # heads at lane 0 and at lane 63
    # items without a row: before the first, a run in the middle, after the last; and single ones all over
    present = np.zeros(n_items, dtype=bool)
    present[gi] = True
    absent = np.nonzero(~present)[0]
    assert gi[0] == sc.GROUP_LEAD and absent[:sc.GROUP_LEAD].tolist() == list(range(sc.GROUP_LEAD))
    assert n_items - 1 - gi[-1] == sc.GROUP_TRAIL and np.diff(gi).max() > sc.GROUP_HOLE
    assert len(absent) > 1000 and (np.bincount(gi) > 1).sum() > 1000     # and items of several groups
    row_group, group_begin, item_gptr, counts = sc.groups_expected(case)
    assert np.array_equal(sc.item_gptr_model(gi, n_items), item_gptr)
    wrong = sc.item_gptr_model(gi, n_items, "no_gap")
    assert np.array_equal(np.nonzero(wrong != item_gptr)[0], absent)     # exactly the items without a row
    assert counts == (len(unum), sc.LONG_GROUP) and group_begin[-1] == n and row_group.max() == len(unum) - 1


def test_gap_fill_was_never_needed_before():
    """Ids by first appearance: every item has a row, and 'no gap fill' writes the same words."""
    for rows in (R.make_rows(7, 50, 30, 2000), R.make_rows(8, 300, 700, 20000, item_power=0.3)):
        want = R.statistics_numpy(*rows)
        gi, n_items = want["group_item"], len(want["items"])
        right = sc.item_gptr_model(gi, n_items)
        assert np.array_equal(right, np.searchsorted(gi, np.arange(n_items + 1)))
        assert np.array_equal(sc.item_gptr_model(gi, n_items, "no_gap"), right)
        assert np.bincount(gi, minlength=n_items).min() >= 1


# ---- the queue and the totals -----------------------------------------------------------------------------------------------

def test_segments_fill_the_queue_three_times():
    case = sc.segsum_case()
    lens, ptr = case["lens"], case["ptr"]
    n_seg = len(lens)
    long_seg = np.nonzero(lens >= sc.LONG_SEG)[0]
    assert len(long_seg) == sc.N_LONG == 2 * 8192 + 3 and len(long_seg) > 4 * sc.LONG_BLOCKS
    assert sc.queue_waves(n_seg) == 4 * sc.LONG_BLOCKS and sc.drain_passes(len(long_seg), n_seg) == 3
    assert lens[long_seg].tolist() == [64, 65] * (sc.N_LONG // 2) + [64]
    assert set(lens[lens < sc.LONG_SEG].tolist()) == {0, 1, 63}
    assert (long_seg[1:] != np.arange(1, sc.N_LONG)).all()               # no queue order puts segment s at position s
    assert ptr[-1] == len(case["a"]) == len(case["perm"]) == len(case["idx"]) and case["idx"].max() < len(case["g"])
    right, wrong = sc.drained(sc.N_LONG, n_seg), sc.drained(sc.N_LONG, n_seg, "first_pass")
    assert np.array_equal(right, np.arange(sc.N_LONG)) and len(wrong) == 4 * sc.LONG_BLOCKS < len(right)
    # before: eight queued segments (tests/test_gpu_eccstats.py, SEG_LENS and its items of 65 groups), one pass
    assert np.array_equal(sc.drained(sc.OLD_LONG, 8), sc.drained(sc.OLD_LONG, 8, "first_pass"))
    assert np.array_equal(sc.drained(8193, 8193 * 2), np.arange(8193)) and sc.drain_passes(8192, 8192 * 2) == 1


def test_moment_sizes_reach_the_third_round():
    rounds = lambda n: -(-(-(-n // sc.CHUNK)) // sc.TOTAL_WIDTH)
    chunks = [-(-n // sc.CHUNK) for n in sc.MOMENT_N]
    assert chunks == [128, 129, 130] and [rounds(n) for n in sc.MOMENT_N] == [2, 3, 3]
    assert rounds(64 * sc.CHUNK + 1) == 2                                # the largest case before: 65 chunks
    assert [n % sc.CHUNK for n in sc.MOMENT_N] == [0, 1, 1]              # the third round of one sum, of two; a chunk of one


# ---- the chain at workload shape --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain():
    rows = sc.chain_case()
    return rows, R.statistics_numpy(*rows)


def test_chain_case_is_the_stated_shape(chain):
    (u, i, fb, tw), want = chain
    n = len(u)
    assert n == sc.CHAIN_ROWS == 532999 and -(-n // sc.TILE) == 261 > sc.SCAN_WIDTH
    assert len(want["users"]) == sc.CHAIN_USERS and len(want["items"]) == sc.CHAIN_ITEMS and len(np.unique(tw)) == sc.CHAIN_WINDOWS
    per_user, per_item = np.bincount(u), np.bincount(i)
    assert set(per_user.tolist()) == {64, 65, 66} and len(per_user) == 8200 > 4 * sc.LONG_BLOCKS
    assert sc.drain_passes(len(per_user), len(per_user)) == 2            # the users' queue: 8 200 entries, 8 192 wavefronts
    assert per_item.min() >= 1 and 2900 <= (per_item >= sc.LONG_SEG).sum() <= 3000
    assert per_item[0] > 5 * per_item[-100:].mean()                      # the squared-uniform skew
    assert want["unum"].max() >= sc.LONG_GROUP and len(want["unum"]) > 4 * sc.CHUNK
    assert fb.min() >= 0.1 and fb.max() <= 5.0 and not np.array_equal(u, np.sort(u))
    # a tile of the sorted keys without a head
    key = np.sort(R.first_appearance(i)[0] * sc.CHAIN_WINDOWS + (tw - tw.min()))
    heads = sc.tile_counts(np.concatenate([[True], key[1:] != key[:-1]]))
    assert (heads == 0).sum() >= 2 and _differs(heads, "floor") and _differs(heads, "unclamped")


def test_chain_restatement_is_finite_everywhere(chain):
    """No user and no item drops out of the comparison as a NaN."""
    _, want = chain
    for k in R.COLUMNS:
        assert np.isfinite(want[k]).all(), k
    assert len(want["ue"]) == sc.CHAIN_USERS and all(len(want[k]) == sc.CHAIN_ITEMS for k in ("ir", "ie", "ire", "ier"))
    assert len(np.unique(want["ue"])) == sc.CHAIN_USERS and (want["ir"] != 0).all()


# ---- the sparse kernel's tile decode ----------------------------------------------------------------------------------------

def test_sparse_case_is_48_tiles_a_side():
    case = sc.sparse_case()
    x, y, rated = case["x"], case["y"], case["rated"]
    T = -(-sc.SPARSE_NX // sc.TB)
    assert T == sc.SPARSE_T == 48 and T * (T + 1) // 2 == 1176 and sc.SPARSE_NX % sc.TB == sc.TB - 5
    assert len(rated) == 4 * T and np.array_equal(np.bincount(rated // sc.TB), np.full(T, 4)) and rated.max() < sc.SPARSE_NX
    offsets = (rated % sc.TB).reshape(T, 4)
    assert len({tuple(o) for o in offsets.tolist()}) == T                # no two tiles rate the same four offsets
    assert set(np.unique(x).tolist()) == set(rated.tolist()) and len(set(zip(x.tolist(), y.tolist()))) == len(x)
    per_row = np.bincount(x)[rated]
    assert per_row.min() >= 8 and per_row.max() <= 12 and y.max() < sc.SPARSE_NY
    # co-rated pairs in every one of the 1 176 tiles
    sub = np.searchsorted(rated, x)
    freq = E.NUMPY["msd"](len(rated), E.build_yr(sub, y, case["r"]), 1, case["w"])["freq"]
    tiles = np.zeros((T, T), dtype=np.int64)
    a, b = np.nonzero(np.triu(freq, 1))
    np.add.at(tiles, (rated[a] // sc.TB, rated[b] // sc.TB), 1)
    assert (tiles[np.triu_indices(T)] > 0).all() and len(a) > 10000
    assert not np.array_equal(x, np.sort(x))                             # training order is not CSR order


def test_decode_model_and_its_sqrt_guess():
    for T in (1, 2, 3, sc.OLD_T, sc.SPARSE_T):
        want = [(ti, tj) for ti in range(T) for tj in range(ti, T)]
        assert sc.decode_all(T) == want
        assert np.array_equal(sc.guessed_rows(T), [d[0] for d in sc.decode_all(T, "guess")])
    # On this host the uncorrected guess is right for all 1 176 blocks at T = 48, and for every T up to 200: row ti starts
    # where td * td - 8 b = (2 T + 1 - 2 ti) ** 2, a perfect square far below 2 ** 53, so a correctly rounded sqrt returns
    # the integer itself and truncation cannot fall short.  There is no T <= 200 to move the case to; it stays at 48 and
    # the two correcting loops are DEFENSIVE (they guard a sqrt that is not correctly rounded).  What the case pins is the
    # decode as a whole, 1 176 blocks against the 2-D grid of the dense kernel, which has none.
    assert sc.decode_all(sc.SPARSE_T, "guess") == sc.decode_all(sc.SPARSE_T)
    for T in range(1, 201):
        rows = np.repeat(np.arange(T), T - np.arange(T))
        assert np.array_equal(sc.guessed_rows(T), rows), T
