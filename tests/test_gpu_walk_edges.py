"""The walk and alias-table kernels at their window and list edges (run with -m gpu): the graphs of
tests/walk_edge_cases.py — which tests/test_walk_edge_cases_host.py proves to reach the 128-entry list of the class
sweep on both sides of its halves and of its cap, the LDS windows at 256/257, 384/385, 512/513, the staging strides
1, 2, 3, and every event of the streamed Vose pairing — through every kernel that meets them, against the C oracle
(oracle/c_oracle.CsrOracle; the popularity rule against tests/popwalk_reference.py).  Everything is an equality:
J and walks are integers, q is compared by its bits."""
import functools

import numpy as np
import pytest

import walk_edge_cases as wc

pytestmark = pytest.mark.gpu

SC = {s[0]: s for s in wc.SCENARIOS}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def n2v():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import node2vec
    return node2vec


@functools.lru_cache(maxsize=2)
def _oracle(sid):
    """(graph, info, oracle with its tables, rounds, walk length) of a scenario; nobody changes them."""
    from oracle import c_oracle
    _, case, kind, p, q, r, L = SC[sid]
    cg, info = wc.graph(case, kind)
    co = c_oracle.CsrOracle(cg.row_ptr, cg.col, cg.w, p, q)
    co.preprocess(first_order_shortcut=False)
    return cg, info, co, r, L


def _engine(sid):
    from n2v_hip.engine import WalkEngine
    _, case, kind, p, q, _, _ = SC[sid]
    return WalkEngine(wc.graph(case, kind)[0], p, q)


def _uniform_args(cg, U, ol):
    """The uniform buffer as the kernels take it.  The oracle consumes it sequentially; the kernels read walk i's
    2 (L - 1) uniforms at 2 (L - 1) i unless told otherwise — the same place as long as no walk ends early."""
    import torch
    kw = dict(rng="uniforms", uniforms=torch.from_numpy(U).cuda())
    if cg.directed:
        kw["walk_uoff"] = torch.from_numpy(wc.buffer_offsets(ol)).cuda()
    return kw


def _same(got, ow, ol, what):
    w, l = got
    assert np.array_equal(l.cpu().numpy(), ol), what
    assert np.array_equal(w.cpu().numpy(), ow), what


def _subset(cg, info):
    """Start nodes that hold the case's hubs (or crafted rows), then a few ordinary ones."""
    special = info["hubs"] if "hubs" in info else (
        np.array([v for _, v, _ in info["rows"]]) if "rows" in info else np.nonzero(info["clique_of"])[0][::7])
    rest = cg.start_order[:60][~np.isin(cg.start_order[:60], special)]
    return np.concatenate([special, rest]).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("sid", wc.SCENARIO_IDS)
def test_every_slot_of_every_table(n2v, sid):
    """The wave-per-table builder's fat and thin output, every slot, against the oracle's J and q."""
    cg, _, co, _, _ = _oracle(sid)
    eng = _engine(sid)
    T = int(co.edge_off[-1])
    eng.preprocess(first_order_shortcut=False, fat=True)
    assert eng.edge_slots is None and eng.edge_fat is not None and not eng.first_order and eng.total_slots == T
    assert np.array_equal(eng.edge_off.cpu().numpy(), co.edge_off)
    assert np.array_equal(eng.slots_J(eng.node_slots).cpu().numpy()[:cg.nnz], co.nodeJ)
    assert np.array_equal(_bits(eng.slots_q(eng.node_slots).cpu().numpy()[:cg.nnz]), _bits(co.nodeq))
    eJ, eq = eng.all_edge_tables()
    assert np.array_equal(eJ[:T], co.edgeJ), "fat J"
    assert np.array_equal(_bits(eq[:T]), _bits(co.edgeq)), "fat q"
    eng.preprocess(first_order_shortcut=False, fat=False)
    assert eng.edge_fat is None
    assert np.array_equal(eng.slots_J(eng.edge_slots).cpu().numpy()[:T], co.edgeJ), "thin J"
    assert np.array_equal(_bits(eng.slots_q(eng.edge_slots).cpu().numpy()[:T]), _bits(co.edgeq)), "thin q"


def _one_table_entries(sid):
    """CSR entries whose table the one-table launch is asked for: tables of 512 and 513 slots, source rows of 384 and
    385 entries, the sizes whose slots are never popped."""
    cg, info = wc.graph(*SC[sid][1:3])
    if "rows" in info:
        vs = [v for name, v, wt in info["rows"] if "unpopped" in name or len(wt) in (512, 513)]
        return [int(np.nonzero(cg.col == v)[0][0]) for v in vs]
    hub = dict(zip(wc.B_HUBS, info["hubs"].tolist()))
    es = [int(np.nonzero(cg.col == hub[K])[0][k]) for K in (512, 513, 1024, 1025) for k in (0, -1)]
    return es + [int(cg.row_ptr[hub[S]]) + 3 for S in (384, 385)]


@pytest.mark.parametrize("sid", ["B plain", "D p=q=1", "D p=0.5 q=2"])
def test_one_table_launch(n2v, sid):
    """build_one_edge_table: one table per launch, static striding and a scratch of its own."""
    cg, _, co, _, _ = _oracle(sid)
    eng = _engine(sid)
    sizes = set()
    for e in _one_table_entries(sid):
        J, q = eng.build_one_edge_table(e)
        sl = slice(int(co.edge_off[e]), int(co.edge_off[e + 1]))
        assert np.array_equal(J, co.edgeJ[sl]), (sid, e)
        assert np.array_equal(_bits(q), _bits(co.edgeq[sl])), (sid, e)
        sizes.add(len(J))
    assert {512, 513} <= sizes
    if sid.startswith("D"):
        assert set(wc.D_UNPOPPED_KS) <= sizes


# ---------------------------------------------------------------------------------------------------- walks
@pytest.mark.parametrize("sid", wc.SCENARIO_IDS)
def test_table_driven_walks(n2v, sid):
    """Both table layouts, Philox and the uniform buffer, against the oracle's table-driven walks."""
    cg, _, co, r, L = _oracle(sid)
    eng = _engine(sid)
    eng.preprocess(first_order_shortcut=False, fat="both")
    ow, ol, _ = co.walk(cg.start_order, r, L, mode="philox", seed=wc.SEED)
    U = np.random.RandomState(11).random_sample(2 * (L - 1) * r * cg.n_nodes)
    bw, bl, _ = co.walk(cg.start_order, r, L, mode="buffer", uniforms=U)
    for layout in ("thin", "fat"):
        _same(eng.walk(eng.start_order, r, L, rng="philox", seed=wc.SEED, layout=layout), ow, ol, (sid, layout, "philox"))
        _same(eng.walk(eng.start_order, r, L, layout=layout, **_uniform_args(cg, U, bl)), bw, bl, (sid, layout, "buffer"))


@pytest.mark.parametrize("sid", wc.SCENARIO_IDS)
def test_on_the_fly_walks(n2v, sid):
    """walk_on_the_fly with no stored table against the oracle's rebuilt-per-step walks: all nodes and a subset that
    holds the hubs, Philox and the uniform buffer."""
    import torch
    cg, info, co, r, L = _oracle(sid)
    eng = _engine(sid)
    assert not eng.ready
    ow, ol, _ = co.walk(cg.start_order, r, L, mode="philox", seed=wc.SEED, on_the_fly=True)
    _same(eng.walk_on_the_fly(eng.start_order, r, L, rng="philox", seed=wc.SEED), ow, ol, (sid, "all", "philox"))
    U = np.random.RandomState(12).random_sample(2 * (L - 1) * cg.n_nodes)
    bw, bl, _ = co.walk(cg.start_order, 1, L, mode="buffer", uniforms=U, on_the_fly=True)
    _same(eng.walk_on_the_fly(eng.start_order, 1, L, **_uniform_args(cg, U, bl)), bw, bl, (sid, "all", "buffer"))
    sub = _subset(cg, info)
    starts = torch.from_numpy(sub).cuda()
    sw, sl, _ = co.walk(sub, 3, L, mode="philox", seed=wc.SEED + 1, on_the_fly=True)
    _same(eng.walk_on_the_fly(starts, 3, L, rng="philox", seed=wc.SEED + 1), sw, sl, (sid, "subset", "philox"))
    U = np.random.RandomState(13).random_sample(2 * (L - 1) * 3 * len(sub))
    bw, bl, _ = co.walk(sub, 3, L, mode="buffer", uniforms=U, on_the_fly=True)
    _same(eng.walk_on_the_fly(starts, 3, L, **_uniform_args(cg, U, bl)), bw, bl, (sid, "subset", "buffer"))
    assert not eng.ready


@pytest.mark.parametrize("sid,div", [("B plain", 3), ("B directed", 3), ("A p=4 q=0.25", 2)])
def test_budgeted_walks_wave_and_lane_kernels(n2v, sid, div):
    """Tables under a budget: a launch of a few thousand walks runs the wave-per-walk kernel, one of at least
    n2v_walk_otf_max_waves() * 32 walks the lane-per-walk kernel — L = 8 (16-byte output pieces) and L = 7 (single
    stores), Philox and the uniform buffer: its four instantiations.  Against the oracle's table-driven walks and the
    unbudgeted engine."""
    import torch
    cg, _, co, r, L = _oracle(sid)
    _, _, _, p, q, _, _ = SC[sid]
    g = n2v.Graph.from_csr(cg, p, q, rng="philox", seed=wc.SEED)
    g.preprocess_transition_probs()
    full_eng = g._engine
    full = full_eng.total_slots * 32
    assert not full_eng.partial
    max_waves = int(full_eng.lib.n2v_walk_otf_max_waves())
    n = cg.n_nodes
    R = wc.lanes_rounds(n, max_waves)
    assert n * R >= max_waves * 32 > n * (R - 1)            # the lane kernel's threshold, and not a round more
    assert n * r < min((n * r + 3) // 4, max_waves // 4) * 128  # the small launch stays with the wave kernel
    launches = [(r, L, "philox"), (R, 8, "philox"), (R, 8, "buffer"), (R, 7, "philox"), (R, 7, "buffer")]
    want = []
    for rounds, length, mode in launches:
        U = np.random.RandomState(14).random_sample(2 * (length - 1) * rounds * n) if mode == "buffer" else None
        ow, ol, _ = co.walk(cg.start_order, rounds, length, mode=mode, seed=wc.SEED, uniforms=U)
        kw = dict(rng="philox", seed=wc.SEED) if mode == "philox" else _uniform_args(cg, U, ol)
        got = full_eng.walk(full_eng.start_order, rounds, length, **kw)
        _same(got, ow, ol, (sid, "unbudgeted", rounds, length, mode))
        want.append((ow, ol, kw, got))
    g.preprocess_transition_probs(budget_bytes=full // div)
    eng = g._engine
    unstored = int((~eng.stored_mask).sum())
    assert eng.partial and 0 < eng.total_slots * 32 <= full // div and 0 < unstored < cg.nnz
    for (rounds, length, mode), (ow, ol, kw, ref) in zip(launches, want):
        got = eng.walk(eng.start_order, rounds, length, **kw)
        _same(got, ow, ol, (sid, "budgeted", rounds, length, mode))
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    if cg.directed:
        assert 0 < int((want[1][1] < 8).sum()) < n * R     # walks that stop at a dead end, and walks that do not


# ---------------------------------------------------------------------------------------------------- popularity rule
def test_popularity_rule_on_the_hub_ladder(n2v):
    """The pop on-the-fly walk (tables of up to 256 slots in LDS, beyond that in the scratch row) and the pop single
    tables (512/513: LDS table or streamed stacks) on graph B against tests/popwalk_reference.py."""
    from oracle.n2v_oracle import philox_step_uniforms
    from popwalk_reference import PopwalkOracle, csr_oracle_graph
    cg, info = wc.graph("B", "plain")
    p, q, seed = 0.5, 2.0, wc.SEED + 2
    g = n2v.Graph.from_csr(cg, p, q, rng="philox", seed=seed)
    g.popwalk = "pop"
    o = PopwalkOracle(csr_oracle_graph(cg), False, p, q, "pop")
    sub = cg.labels[_subset(cg, info)].tolist()
    want = o.simulate_walks(2, 8, nodes=sub, on_the_fly=True, step_uniforms=lambda w, t: philox_step_uniforms(seed, w, t))
    assert g.simulate_walks_on_the_fly(2, 8, nodes=sub) == want
    hub = dict(zip(wc.B_HUBS, info["hubs"].tolist()))
    for K in (255, 256, 257, 512, 513, 1024, 1025):
        v = hub[K]
        u = int(cg.col[cg.row_ptr[v] + K // 2])
        J, qq = g.get_alias_edge_pop(int(cg.labels[u]), int(cg.labels[v]))
        wJ, wq = o.get_alias_edge_pop(int(cg.labels[u]), int(cg.labels[v]))
        assert len(J) == K and np.array_equal(J, np.asarray(wJ)), K
        assert np.array_equal(_bits(qq), _bits(np.asarray(wq, dtype=np.float64))), K
