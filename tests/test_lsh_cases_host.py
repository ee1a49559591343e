"""CPU audit of tests/lsh_cases.py: every case of tests/test_gpu_bine_lsh_edges.py reaches the path of
csrc/n2v_lsh.hip it exists for, shown by oracle/bine_lsh_oracle.py and the kernel-shaped restatement of
tests/lsh_reference.py alone.  Every audit is an assertion: a builder whose seed stops reaching its edge fails here,
before anything runs on a GPU.  The sensitivity tests show that the expected arrays change under six wrong kernels (flaws: tests/lsh_reference.py)."""
import hashlib

import numpy as np
import pytest

import lsh_cases as C
import lsh_reference as R
from oracle import bine_lsh_oracle as lo

BASE_LEN = {1, 63, 64, 65, 129, 256}
BASE_WIDTH = {1, 63, 64, 65, 129, 300}


def user_side(name, k):
    sims, owner = R.queries_of(name, k)["u"]
    return sims, owner, [v for v, s in enumerate(sims) if v not in s]


def group_of(name, size):
    """The ids of the user duplicate group of `size` members (first one of that size)."""
    g = R.graph_of(name)
    rows = {}
    for v in range(g.n_u):
        rows.setdefault(tuple(g.col[g.row_ptr[v]:g.row_ptr[v + 1]]), []).append(v)
    return [m for m in rows.values() if len(m) == size][0]


# ---- the base graph ---------------------------------------------------------------------------------------------------
def test_base_graph_is_the_validated_one():
    g = R.graph_of("base")
    assert (g.n_u, g.n_v) == (631, 45) and g.n_u % 4 != 0
    deg = np.diff(g.row_ptr)
    assert set(deg[g.n_u:].tolist()) == BASE_WIDTH and set(deg[:g.n_u].tolist()) == {3}
    order, rlo, rhi = R.ranges_of("base", "u")
    deep = rhi[:, :, -1] - rlo[:, :, -1]
    assert set(deep.ravel().tolist()) == BASE_WIDTH                   # every tree: the deepest range IS the group
    assert R.wing_widths(rlo, rhi) == BASE_WIDTH | {0}                # and disjoint groups share no shorter prefix
    big = group_of("base", 300)
    assert np.any(np.diff(big) > 1) and max(big) - min(big) > 500     # ids interleave with the other groups
    sims, owner, missing = user_side("base", 256)
    assert {len(s) for s in sims} == BASE_LEN
    assert len(np.unique(owner)) == 59 and len(missing) == 44
    assert set(missing) == set(big[256:]) and all(owner[v] == v for v in missing)
    comp = {631 - len(lo.exclusions(sims, int(l))) for l in np.unique(owner)}
    assert comp == {375, 502, 566, 567, 568, 630}


@pytest.mark.parametrize("k", C.K_SWEEP)
def test_k_sweep_cuts_where_it_claims(k):
    sims, owner, missing = user_side("base", k)
    assert max(len(s) for s in sims) == k and {len(s) for s in sims} == {min(n, k) for n in BASE_WIDTH}
    assert sum(len(s) == k for s in sims) >= 300                      # len(sim) == k: the truncated lists
    _, _, st = R.shaped_queries_of("base", "u", k)
    assert (st["hits"] > 0) == (k > 1)                                # trees 1…7 offer the same keys again
    if k % 64:
        assert st["cut_mid_chunk"] > 0                                # rank < room drops candidates inside a chunk
    else:
        assert st["cut_mid_chunk"] == 0 and st["full_chunks"] > 0     # the k-th key is lane 63 of a full chunk
    if k == 65:                                                       # full chunk, then room for exactly one
        assert any(len(s) == 65 for v, s in enumerate(sims) if v in set(group_of("base", 129)))
    if k == 200:                                                      # shorter lists go on through all 16 levels
        assert {len(s) for s in sims} == {1, 63, 64, 65, 129, 200}
    if k < 300:                                                       # k below the group: the rest miss themselves
        assert len(missing) >= 300 - k and all(owner[v] == v for v in missing)
    assert lsh_arg_limit() == 256 and max(C.K_SWEEP) == 256


def lsh_arg_limit():
    return C.SET_SLOTS // 2                                            # the ABI's `k <= kSetSlots / 2`


@pytest.mark.parametrize("pool_size", C.TIGHT_POOLS)
def test_tight_pools_meet_the_complement(pool_size):
    case = C.BY_NAME["base_tight%d" % pool_size]
    sims, owner, _ = user_side("base", 256)
    rows = R.rows_of("base", 256, pool_size)["u"]
    big = group_of("base", 300)
    leaders = sorted({int(owner[v]) for v in big})
    assert len(leaders) == 45
    _, st = R.shaped_pools_of(case, "u")
    for l in leaders:
        rest = sorted(set(range(631)) - lo.exclusions(sims, l))
        assert len(rest) == 375 and st["complements"][l] == 375
        row = rows[l]
        if pool_size == 374:                                          # complement == pool_size + 1: drawn, one left out
            assert row.min() >= 0 and len(set(row.tolist())) == 374 and set(row.tolist()) < set(rest)
            assert row.tolist() != sorted(row.tolist())
        elif pool_size == 375:                                        # every remaining vertex, ascending, no -1
            assert row.tolist() == rest
        else:                                                         # one -1
            assert row.tolist() == rest + [-1]
    assert st["all_of_it"] == (0 if pool_size == 374 else 45) and st["counted"] == 59


@pytest.mark.parametrize("pool_size", C.ROUND_POOLS)
def test_round_cut_off(pool_size):
    name = "base_groups1024" if pool_size == 200 else "base_pool%d" % pool_size
    case = C.BY_NAME[name]
    assert case.pool_size == pool_size and case.k == 256
    _, st = R.shaped_pools_of(case, "u")
    assert st["all_of_it"] == 0 and st["cut_rounds"] > 0              # a round offers more than there is room for
    assert st["rounds_max"] >= {1: 1, 63: 2, 64: 2, 65: 2, 200: 4}[pool_size]
    if pool_size == 200:
        assert st["lower_lane"] > 0 and st["earlier_round"] > 0


@pytest.mark.parametrize("groups", C.GROUPS)
def test_groups_reuse_bitmaps(groups):
    case = C.BY_NAME["base_groups%d" % groups]
    for side in "uv":
        pool, st = R.shaped_pools_of(case, side)
        if groups < 1024:
            assert st["n_lead"] > groups and st["served_max"] == -(-st["n_lead"] // groups)
        else:
            assert st["served_max"] == 1
        assert st["stale_words"] == 0                                 # every leader finds its bitmap zero
        other, _ = R.shaped_pools_of(C.BY_NAME["base_groups1024"], side)
        assert np.array_equal(pool, other)
    assert R.shaped_pools_of(case, "u")[1]["all_of_it"] == 0          # users draw, items (45) take all that is left:
    assert R.shaped_pools_of(case, "v")[1]["all_of_it"] == 15         # both epilogues run on a reused bitmap
    tight = R.shaped_pools_of(C.BY_NAME["base_tight375_groups1"], "u")[1]
    assert tight["served_max"] == 59 and 0 < tight["all_of_it"] < 59  # and both kinds of leader share ONE bitmap


# ---- the other graphs -------------------------------------------------------------------------------------------------
def test_wide_side_probes_and_wraps():
    case = C.BY_NAME["wide"]
    g = R.graph_of("wide")
    assert g.n_u >= 2100 and (g.n_u + 31) // 32 > 64
    big = group_of("wide", C.WIDE_GROUP)
    assert len(big) >= 257 and sum(C.set_home(v) >= 508 for v in big[:256]) >= 4
    sims, owner, missing = user_side("wide", 256)
    assert all(sims[v] == big[:256] for v in big) and set(missing) == set(big[256:])
    _, _, st = R.shaped_queries_of("wide", "u", 256)
    assert st["max_probe"] >= 4 and st["wrapped"] >= 1
    _, pst = R.shaped_pools_of(case, "u")
    assert pst["words"] > 64 and pst["popcount_trips"] >= 2 and pst["counted"] == pst["n_lead"]
    # the replay above IS the kernel's open addressing over the oracle's key order: same lists
    flat, sim_n, _ = R.shaped_queries_of("wide", "u", 256)
    assert R.rows_of_flat(flat, sim_n, 256) == sims


def test_wide_count_decides_in_the_second_popcount_trip():
    case = C.BY_NAME["wide_count"]
    g = R.graph_of("wide_count")
    assert (g.n_u, g.n_v) == (2100, 27) and case.pool_size == C.COUNT_POOL
    big = group_of("wide_count", C.WIDE_GROUP)
    sims, owner, missing = user_side("wide_count", 256)
    assert sum(v >= 2048 for v in big[:256]) >= 32 and len(missing) == 4
    pool, st = R.shaped_pools_of(case, "u")
    assert st["words"] == 66 and st["popcount_trips"] == 2 and st["counted"] == st["n_lead"] == 13
    leaders = sorted({int(owner[v]) for v in big})
    assert len(leaders) == 5 and all(st["complements"][l] == case.pool_size for l in leaders)      # exactly pool_size
    assert sorted(set(st["complements"].values())) == [case.pool_size, case.pool_size + 26]
    assert st["all_of_it"] == 5 and st["rounds_max"] > 64 and st["cut_rounds"] > 0
    rows = R.rows_of("wide_count", 256, case.pool_size)["u"]
    assert all(rows[l].tolist() == sorted(set(range(2100)) - set(big[:256])) for l in leaders)
    # words 64 and 65 left out of the count: those five leaders would draw instead of taking all that is left
    assert pools_differ(case, "u", "popcount_one_trip")[0]
    assert not pools_differ(C.BY_NAME["wide"], "u", "popcount_one_trip")[0]                       # `wide` cannot tell


def test_tiny_side_collides_without_counting():
    case = C.BY_NAME["tiny"]
    g = R.graph_of("tiny")
    assert g.n_u > case.k * (case.k + 1) + case.pool_size and g.n_u < 64 and g.n_u % 4 != 0
    sims, owner, missing = user_side("tiny", 1)
    assert len(missing) == 4 and all(owner[v] == v for v in missing)
    pool, st = R.shaped_pools_of(case, "u")
    assert st["counted"] == 0 and st["all_of_it"] == 0
    assert st["lower_lane"] > 0 and st["earlier_round"] > 0 and st["rounds_max"] >= 2
    rows = R.rows_of("tiny", 1, 30)["u"]
    assert any(v in rows[v].tolist() for v in missing)                # a self-missing vertex draws itself


def test_degenerate_sides():
    g = R.graph_of("one_item")
    assert g.n_v == 1 and g.n_u % 4 != 0
    exp = R.expected(C.BY_NAME["one_item"])
    assert np.all(exp["v"]["pool"] == -1) and np.all(exp["u"]["pool"] == -1)
    g = R.graph_of("two_items")
    assert g.n_v == 2 and g.n_u % 4 != 0
    exp = R.expected(C.BY_NAME["two_items"])
    assert exp["v"]["pool"].tolist() == [[g.n_u + 1, -1, -1, -1], [g.n_u, -1, -1, -1]]
    assert (exp["u"]["pool"] >= 0).any() and (exp["u"]["pool"] < 0).any()


def test_label_table():
    from n2v_hip import bine
    ul, il = C.label_table()
    g = bine.BipartiteGraph(ul, il, np.ones(len(ul)))
    labels = R.labels_of(g)
    lens = [len(s.encode("utf8")) for s in labels]
    assert g.n_u == 256 and len(labels) >= 300 and min(lens) == 1 and max(lens) == 130
    assert len(set(lens)) > 60
    for n in (55, 56, 63, 64, 119, 120):
        assert any(ln == n for ln in lens[256:]), n
    assert any(len(s) != len(s.encode("utf8")) for s in labels[256:]) and any(ord(c) > 0xFFFF for s in labels for c in s)
    assert lo.sha1_hash32(labels[300].encode("utf8")) == int.from_bytes(hashlib.sha1(labels[300].encode("utf8")).digest()[:4], "little")


# ---- both restatements agree; the leader sweep in rounds ---------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_kernel_shaped_restatement_equals_the_oracle(case):
    exp = R.expected(case)
    for side in "uv":
        e = exp[side]
        flat, sim_n, _ = R.shaped_queries_of(case.graph, side, case.k)
        assert R.rows_of_flat(flat, sim_n, case.k) == e["sims"]
        assert np.all(flat[len(e["sims"]) * case.k:] == R.GUARD)
        owner, _ = R.shaped_leaders(e["sims"])
        assert np.array_equal(owner, e["owner"])
        n_side = e["hi"] - e["lo"]
        pool, st = R.shaped_pools_of(case, side)
        rows = pool[:n_side * case.pool_size].reshape(n_side, case.pool_size)
        want = np.where(e["pool"] >= 0, e["pool"] - e["lo"], -1)
        lead = np.unique(e["owner"])
        assert np.array_equal(rows[lead], want[lead]) and np.array_equal(rows[e["owner"]], want)
        assert np.all(pool[n_side * case.pool_size:] == R.GUARD) and st["stale_words"] == 0


def test_leader_sweep_needs_three_rounds_somewhere():
    rounds = {}
    for case in C.CASES:
        for side in "uv":
            rounds[(case.name, side)] = R.shaped_leaders(R.queries_of(case.graph, case.k)[side][0])[1]
    assert rounds[("base_k256", "u")] == 2                            # duplicate groups: leaders, then their members
    assert rounds[("overlap", "u")] >= 3                              # a vertex that waits for a follower's owner
    sims, owner, missing = user_side("overlap", 6)
    _, _, st = R.shaped_queries_of("overlap", "u", 6)
    assert st["cut_mid_chunk"] > 0 and len(missing) > 0
    assert R.shaped_pools_of(C.BY_NAME["overlap"], "u")[1]["served_max"] >= 2


# ---- sensitivity -------------------------------------------------------------------------------------------------------
def pools_differ(case, side, flaw):
    """Do the rows differ after the host has given every vertex its owner's row (or the guard behind the last)?"""
    owner = R.queries_of(case.graph, case.k)[side][1]
    good, _ = R.shaped_pools_of(case, side)
    bad, st = R.shaped_pools_of(case, side, flaw=flaw)
    body = len(owner) * case.pool_size
    spread = lambda p: p[:body].reshape(len(owner), case.pool_size)[owner]
    return not (np.array_equal(spread(good), spread(bad)) and np.array_equal(good[body:], bad[body:])), st


def test_wrong_kernels_change_the_expected_arrays():
    """Which case catches which slip (flaws: tests/lsh_reference.py).  No GPU: the restatement stands for the kernel."""
    # epilogue forgets sim(j): visible where a bitmap serves a second leader AND some sim(j) reaches past sim(l)'s
    # words.  In the duplicate-group family sim(j) == sim(l), so the clear of sim(l) covers it: only `overlap` tells.
    for name in ("overlap", "overlap_groups1"):
        for side in "uv":
            differs, st = pools_differ(C.BY_NAME[name], side, "keep_sim_j")
            assert differs and st["stale_words"] > 0, (name, side)
    for name in ("base_groups1", "base_tight375_groups1"):
        assert not pools_differ(C.BY_NAME[name], "u", "keep_sim_j")[0]

    # rank <= room in the query: the key after the k-th is written behind the row
    for k in (1, 63, 65, 200, 255):
        good = R.shaped_queries_of("base", "u", k)[0]
        bad = R.shaped_queries_of("base", "u", k, "rank_le_room")[0]
        assert not np.array_equal(good, bad), k
    # … and in the pool round: the extra vertex's bit survives the epilogue and the next leader misses it
    for name in ("base_groups1", "base_pool1", "base_pool63", "base_pool64", "base_pool65", "tiny"):
        assert pools_differ(C.BY_NAME[name], "u", "rank_le_room")[0], name

    # the chunk stops at base + 63: any range of 64 or more loses the key of lane 63
    for name, k in (("base", 64), ("base", 256), ("wide", 256)):
        good, good_n, _ = R.shaped_queries_of(name, "u", k)
        bad, bad_n, _ = R.shaped_queries_of(name, "u", k, "chunk_to_63")
        assert not np.array_equal(good, bad), (name, k)
    good, good_n, _ = R.shaped_queries_of("base", "u", 63)
    bad, bad_n, _ = R.shaped_queries_of("base", "u", 63, "chunk_to_63")
    assert np.array_equal(good, bad)                                                 # k = 63 alone would not tell

    # probing without & 511: only a chain that runs over slot 511 tells.  Vertex 3 of `wide` is the last wavefront of
    # its workgroup and in the big group: its chain leaves the workgroup's LDS and the query cannot end.
    assert R.shaped_queries_of("wide", "u", 256)[2]["wrapped"] > 0 and 3 in group_of("wide", C.WIDE_GROUP)
    with pytest.raises(R.ProbeRanOff) as off:
        R.shaped_queries(*R.ranges_of("wide", "u"), 256, flaw="no_wrap")
    assert off.value.args[0] == 3
    assert R.shaped_queries_of("base", "u", 256)[2]["wrapped"] == 0                   # the base graph cannot tell
    good, bad = R.shaped_queries_of("base", "u", 256), R.shaped_queries_of("base", "u", 256, "no_wrap")
    assert np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])

    # signature rows addressed by v instead of v - v_begin: the item-side launch of the GPU test
    g, sig = R.graph_of("base"), R.signatures_of("base")
    good = R.shaped_minhash_rows(sig, g.n_u, g.n, g.n + 1)
    bad = R.shaped_minhash_rows(sig, g.n_u, g.n, g.n + 1, "v_absolute")
    assert np.array_equal(good[:g.n_v], sig[g.n_u:]) and np.all(good[g.n_v:] == R.GUARD)
    assert not np.array_equal(good, bad)
    assert np.array_equal(R.shaped_minhash_rows(sig, 0, g.n, g.n + 1), R.shaped_minhash_rows(sig, 0, g.n, g.n + 1, "v_absolute"))
