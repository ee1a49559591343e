"""No GPU: the graphs of tests/walk_edge_cases.py reach the window and list edges they claim — counted on the C oracle's
walks with the plain-Python reach analysis — and the oracle's two walks (table-driven, rebuilt per step) agree there,
since tests/test_gpu_walk_edges.py leans on both.  Conditions on the INPUTS of the GPU tests, not measurements: every
bucket must hold at least 50 steps (or tables) over the cases together, every pairing event must occur at least once."""
import numpy as np
import pytest

import walk_edge_cases as wc
from oracle import c_oracle

MIN_REACH = 50


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle(sc):
    _, case, kind, p, q, r, L = sc
    cg, info = wc.graph(case, kind)
    return cg, info, c_oracle.CsrOracle(cg.row_ptr, cg.col, cg.w, p, q), r, L


@pytest.fixture(scope="module")
def reached():
    """{scenario id: bucket counts} over the oracle's on-the-fly walks of every scenario (computed once)."""
    out = {}
    for sc in wc.SCENARIOS:
        cg, _, co, r, L = _oracle(sc)
        ow, ol, _ = co.walk(cg.start_order, r, L, mode="philox", seed=wc.SEED, on_the_fly=True)
        out[sc[0]] = wc.reach(cg, ow, ol)
    return out


def test_every_bucket_of_the_walk_kernels_is_reached(reached):
    total = {}
    for name, r in reached.items():
        print("%-22s %s" % (name, ", ".join("%s: %d" % kv for kv in sorted(r.items()))))
        for k, c in r.items():
            assert k in wc.REACH_BUCKETS, k
            total[k] = total.get(k, 0) + c
    print("all cases: " + ", ".join("%s: %d" % (k, total.get(k, 0)) for k in wc.REACH_BUCKETS))
    for k in wc.REACH_BUCKETS:
        assert total.get(k, 0) >= MIN_REACH, (k, total.get(k, 0))


def test_each_case_holds_the_edges_it_was_built_for(reached):
    """Not left to the sum: A holds the special-slot list's sizes, B the windows and strides, C the scratch fallback
    and the uncached prev row, the weighted and directed copies the general path on both sides of 256."""
    for name, r in reached.items():
        if name.startswith("A "):
            for k in ("registers m=64", "m<=64", "m 65-127", "m=128", "m>128, table in LDS (K<=256)", "K=64", "K=65"):
                assert r.get(k, 0) >= MIN_REACH, (name, k, r.get(k, 0))
    b = reached["B plain"]
    for k in ["K=%d" % K for K in (255, 256, 257, 384, 385, 512, 513, 1024, 1025)] + ["stride 1", "stride 2", "stride 3",
                                                                                      "walks prev's row"]:
        assert b.get(k, 0) >= MIN_REACH, (k, b.get(k, 0))
    c = reached["C"]
    for k in ("m>128, table in scratch (K>256)", "prev's row not cached (S>=257)", "walks cur's row", "walks prev's row"):
        assert c.get(k, 0) >= 1000, (k, c.get(k, 0))
    for name in ("B weighted", "B directed"):
        for k in ("general K=256", "general K=257", "general: table in LDS", "general: table in scratch",
                  "general: registers (K<=64)"):
            assert reached[name].get(k, 0) >= MIN_REACH, (name, k)


@pytest.mark.parametrize("sc", wc.SCENARIOS, ids=wc.SCENARIO_IDS)
def test_oracle_table_and_on_the_fly_walks_agree(sc):
    cg, _, co, r, L = _oracle(sc)
    co.preprocess()
    for mode in ("philox", "buffer"):
        U = np.random.RandomState(7).random_sample(2 * (L - 1) * r * cg.n_nodes) if mode == "buffer" else None
        tw, tl, tn = co.walk(cg.start_order, r, L, mode=mode, seed=wc.SEED, uniforms=U)
        fw, fl, fn = co.walk(cg.start_order, r, L, mode=mode, seed=wc.SEED, uniforms=U, on_the_fly=True)
        assert np.array_equal(tw, fw) and np.array_equal(tl, fl) and tn == fn, (sc[0], mode)
        assert tn == int(2 * (tl.astype(np.int64) - 1).sum())
    if sc[2] == "directed":
        assert 0.05 < float((tl < L).mean()) < 0.95        # some walks stop at a dead end, some do not


def test_builder_windows_are_reached():
    got = wc.builder_reach(wc.graph("B")[0])
    print("builder tables of B: " + ", ".join("%s: %d" % kv for kv in sorted(got.items())))
    for k in ("table K=512", "table K=513", "source row S=384", "source row S=385"):
        assert got[k] >= MIN_REACH, (k, got[k])


def test_crafted_stacks_reach_every_pairing_event():
    """Case D: the replay of Vose's loop, streamed as wave_pair streams it, equals the oracle's alias_setup bit for bit
    on every crafted row; over the rows every pairing event occurs, and the stacks take every size of the list."""
    cg, info = wc.graph("D")
    events = {name: 0 for name in wc.PAIR_EVENTS}
    ns_tables, nl_tables, k_tables = {}, {}, {}
    co = c_oracle.CsrOracle(cg.row_ptr, cg.col, cg.w, 1.0, 1.0)
    co.preprocess(first_order_shortcut=False)
    indeg = np.bincount(cg.col, minlength=cg.n_nodes)
    for name, v, wt in info["rows"]:
        J, q, ns, nl, ev = wc.replay_pairing(wt)
        norm = 0.0
        for x in wt:
            norm = norm + float(x)
        oJ, oq = c_oracle.alias_setup(np.array([float(x) / norm for x in wt]))
        assert np.array_equal(J, oJ) and np.array_equal(_bits(q), _bits(oq)), name
        # ... and the oracle's edge tables INTO v (p = q = 1, materialised) are that table
        e = int(np.nonzero(cg.col == v)[0][0])
        sl = slice(int(co.edge_off[e]), int(co.edge_off[e + 1]))
        assert np.array_equal(co.edgeJ[sl], J) and np.array_equal(_bits(co.edgeq[sl]), _bits(q)), name
        assert indeg[v] == wc.D_SOURCES
        for k, c in ev.items():
            events[k] += c
        ns_tables[ns] = ns_tables.get(ns, 0) + wc.D_SOURCES
        nl_tables[nl] = nl_tables.get(nl, 0) + wc.D_SOURCES
        k_tables[len(wt)] = k_tables.get(len(wt), 0) + wc.D_SOURCES
        if "unpopped" in name:
            assert ns == len(wt) and nl == 0 and float(len(wt)) * (1.0 / float(len(wt))) < 1.0, name
        elif name.startswith("ones"):
            assert ns == 0 and nl == len(wt), name
    print("pairing events of D: " + ", ".join("%s: %d" % (k, events[k]) for k in wc.PAIR_EVENTS))
    print("tables of D by stack size: smaller %s, larger %s" % (
        {k: ns_tables.get(k, 0) for k in (0, 1, 63, 64, 65)}, {k: nl_tables.get(k, 0) for k in (0, 1, 63, 64, 65)}))
    for k in wc.PAIR_EVENTS:
        assert events[k] >= 1, k
    for n in (0, 1, 63, 64, 65):
        assert ns_tables.get(n, 0) >= MIN_REACH and nl_tables.get(n, 0) >= MIN_REACH, (n, ns_tables.get(n), nl_tables.get(n))
    for K in (512, 513):
        assert k_tables.get(K, 0) >= MIN_REACH
    assert any(K > 512 for K in wc.D_UNPOPPED_KS) and any(K <= 512 for K in wc.D_UNPOPPED_KS)


def test_budgets_store_part_of_the_tables():
    """Case E's budgets on the CPU (the arithmetic WalkEngine.preprocess uses): a third of B's and half of A's table
    bytes leave tables on both sides of the cut, so the budgeted walk reads some tables and rebuilds others."""
    from n2v_hip.csr import degree_cut_for_budget
    for case, kind, div in (("B", "plain", 3), ("B", "directed", 3), ("A", "plain", 2)):
        cg = wc.graph(case, kind)[0]
        deg = np.diff(cg.row_ptr)
        full = int(deg[cg.col].sum()) * 32
        cut, slots = degree_cut_for_budget(cg, full // div, 32)
        stored = int((deg[cg.col] <= cut).sum())
        print("budget of %s %s: degree cut %d, %d of %d entries stored" % (case, kind, cut, stored, cg.nnz))
        assert 0 < slots * 32 <= full // div and 0.2 * cg.nnz < stored < cg.nnz
        assert wc.lanes_rounds(cg.n_nodes, 6144) * cg.n_nodes >= 6144 * 32
