"""The popularity-biased walk on the GPU (run with -m gpu): the pop node-table kernel, the pop rule of the wave table
builder and of the on-the-fly walk, and the Graph / linkpred surface above them, against (1) the fixtures captured from
the reference (tests/golden/popwalk/*.npz) and (2) the fp64 restatement tests/popwalk_reference.py, which
tests/test_popwalk_golden.py pins to those fixtures.  No tolerances: J and walks are integers, q is compared as raw
fp64 bits, numpy's global stream must end where the reference leaves it."""
import numpy as np
import pytest

from helpers import case_weights, golden_walks, oracle_graph
from popwalk_reference import (OTF, POPWALK_CASES, PRE, PopwalkOracle, case_pq, csr_oracle_graph, load_popwalk_case,
                               simulate_walk_popularity, walk_specs)

pytestmark = pytest.mark.gpu
ERRORS = {"ZeroDivisionError": ZeroDivisionError}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _nx_graph(z):
    import networkx as nx
    G = nx.DiGraph()
    for (u, v), w in zip(z["edges"].tolist(), case_weights(z)):
        G.add_edge(int(u), int(v), weight=w)
    if not bool(z["directed"]):
        G = G.to_undirected()
    return G


@pytest.fixture(scope="module")
def n2v():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import node2vec
    return node2vec


def _graph(n2v, z, **kw):
    p, q = case_pq(z)
    return n2v.Graph(_nx_graph(z), bool(z["directed"]), p, q, **kw)


def _philox(seed):
    from oracle.n2v_oracle import philox_step_uniforms
    return lambda w, t: philox_step_uniforms(seed, w, t)


@pytest.mark.parametrize("name", POPWALK_CASES)
def test_pop_node_tables_equal_the_reference(n2v, name):
    """preprocess_transition_probs_popularity(): alias_nodes are the reference's pop tables, in the thin slots and in the
    fat slots; alias_edges are the PLAIN edge tables.  Where the reference raises, so does the call."""
    import torch
    z = load_popwalk_case(name)
    g = _graph(n2v, z)
    p, q = case_pq(z)
    if str(z["pn_error"]) or p == 0 or q == 0:
        with pytest.raises(ZeroDivisionError):
            g.preprocess_transition_probs_popularity()
        return
    assert g.preprocess_transition_probs_popularity() is None
    eng, csr = g._engine, g._csr
    nodes, ap = z["nodes"].tolist(), z["adj_ptr"]
    assert eng.pop_tables and g.alias_nodes.keys() == nodes
    for fat in ("both", True, False):
        eng.preprocess(fat=fat, pop=True)
        nq = eng.slots_q(eng.node_slots).cpu().numpy()
        nJ = eng.slots_J(eng.node_slots).cpu().numpy()
        if eng.node_fat is not None:
            fq = eng.node_fat.view(torch.float64)[:, 0].cpu().numpy()
            f32 = eng.node_fat.view(torch.int32).cpu().numpy()
        for i, v in enumerate(nodes):
            d = int(csr.dense_of([v])[0])
            sl = slice(int(csr.row_ptr[d]), int(csr.row_ptr[d + 1]))
            assert np.array_equal(csr.labels[csr.col[sl]], z["adj"][ap[i]:ap[i + 1]])
            assert np.array_equal(nJ[sl], z["pn_J"][ap[i]:ap[i + 1]]), (name, v, fat)
            assert np.array_equal(_bits(nq[sl]), _bits(z["pn_q"][ap[i]:ap[i + 1]])), (name, v, fat)
            if eng.node_fat is not None:      # fat slot = {q, record of neighbour k, record of neighbour J[k]}
                assert np.array_equal(_bits(fq[sl]), _bits(z["pn_q"][ap[i]:ap[i + 1]])), (name, v, "fat q")
                assert np.array_equal(f32[sl, 4], csr.col[sl]) and np.array_equal(f32[sl, 7], csr.col[sl][nJ[sl]])
    J0, q0 = g.alias_nodes[nodes[0]]
    assert J0.dtype == np.int64 and np.array_equal(J0, z["pn_J"][ap[0]:ap[1]])
    # the edge tables are those of preprocess_transition_probs()
    g.preprocess_transition_probs_popularity()
    popJ, popq = g._engine.all_edge_tables()
    g.preprocess_transition_probs()
    assert not g._engine.pop_tables
    J, qq = g._engine.all_edge_tables()
    assert np.array_equal(J, popJ) and np.array_equal(_bits(qq), _bits(popq))


@pytest.mark.parametrize("name", POPWALK_CASES)
def test_single_pop_tables_equal_the_reference(n2v, name):
    """get_alias_edge_pop / get_alias_edges_cur / get_alias_nodes_cur with popwalk == "pop": one table per call, no
    preprocess, every sampled table of the fixture — the hubs' (> 512 slots: the builder's scratch path) among them."""
    z = load_popwalk_case(name)
    g = _graph(n2v, z, popwalk="pop")
    ep = z["pe_ptr"]
    sizes = set()
    for i, (u, v) in enumerate(z["pe_keys"].tolist()):
        err = str(z["pe_err"][i])
        for fn in (g.get_alias_edge_pop, g.get_alias_edges_cur):
            if err:
                with pytest.raises(ERRORS[err]):
                    fn(u, v)
                continue
            J, q = fn(u, v)
            assert J.dtype == np.int64 and np.array_equal(J, z["pe_J"][ep[i]:ep[i + 1]]), (name, u, v)
            assert np.array_equal(_bits(q), _bits(z["pe_q"][ep[i]:ep[i + 1]])), (name, u, v)
        sizes.add(int(ep[i + 1] - ep[i]))
    if name == "hubs_useritem":
        assert max(sizes) > 512 and any(64 < s <= 512 for s in sizes) and any(0 < s <= 64 for s in sizes)
    nodes, ap = z["nodes"].tolist(), z["adj_ptr"]
    if not str(z["pn_error"]):
        for i, v in enumerate(nodes):
            J, q = g.get_alias_nodes_cur(v)
            assert np.array_equal(J, z["pn_J"][ap[i]:ap[i + 1]]), (name, v)
            assert np.array_equal(_bits(q), _bits(z["pn_q"][ap[i]:ap[i + 1]])), (name, v)
    else:       # the sink's in-neighbours raise (unless exempt), every other node has its table
        o = PopwalkOracle(oracle_graph(z), bool(z["directed"]), *case_pq(z), "pop")
        raised = 0
        for v in nodes:
            try:
                want = o.get_alias_node_pop(v)
            except ZeroDivisionError:
                with pytest.raises(ZeroDivisionError):
                    g.get_alias_nodes_cur(v)
                raised += 1
                continue
            J, q = g.get_alias_nodes_cur(v)
            assert np.array_equal(J, want[0]) and np.array_equal(_bits(q), _bits(want[1])), (name, v)
        assert raised > 0
    assert g._engine is not None and not g._engine.ready      # no preprocess ran
    # popwalk is read at call time
    g.popwalk = "none"
    p, q = case_pq(z)
    if p != 0 and q != 0:
        u, v = z["pe_keys"][0].tolist()
        J, qq = g.get_alias_edges_cur(u, v)
        Jn, qn = g.get_alias_edge(u, v)
        assert np.array_equal(J, Jn) and np.array_equal(_bits(qq), _bits(qn))


@pytest.mark.parametrize("name", POPWALK_CASES)
def test_walks_equal_the_reference_under_numpy_seed(n2v, name):
    """Every walk call of the fixtures — both modes, both seeds and shapes, the nodes= subset, "both" through
    linkpred.simulate_walk_popularity — with np.random.seed: identical walks, and numpy's global stream ends where
    a RandomState advanced by the recorded number of draws stands.  Where the reference raises, so does the call."""
    from n2v_hip import linkpred
    z = load_popwalk_case(name)
    for (i, seed, r, L, nd, sub, mode, both, err) in walk_specs(z):
        g = _graph(n2v, z, popwalk="pop")

        def call():
            np.random.seed(seed)
            if both:
                return linkpred.simulate_walk_popularity(g, "both", r, L, on_the_fly=(mode == OTF))
            if mode == PRE:
                g.preprocess_transition_probs_popularity()
                return g.simulate_walks(r, L, nodes=sub)
            return g.simulate_walks_on_the_fly(r, L, nodes=sub)
        if err:
            with pytest.raises(ERRORS[err]):
                call()
            continue
        walks = call()
        want = golden_walks(z, i)
        assert len(walks) == len(want) and isinstance(walks, n2v.WalkCorpus)
        assert walks == want, (name, i)
        chk = np.random.RandomState(seed)
        chk.random_sample(nd)
        assert np.random.random_sample() == chk.random_sample(), (name, i, "global stream position")
    # node2vec_walk_on_the_fly (src/node2vec.py:34-53), one walk
    specs = [s for s in walk_specs(z) if s[6] == OTF and not s[7] and not s[8] and s[5] is None]
    if specs:
        g = _graph(n2v, z, popwalk="pop")
        o = PopwalkOracle(oracle_graph(z), bool(z["directed"]), *case_pq(z), "pop")
        start = z["nodes"].tolist()[0]
        np.random.seed(77)
        assert g.node2vec_walk_on_the_fly(9, start) == o.node2vec_walk(9, start, np.random.RandomState(77).random_sample, True)


@pytest.mark.parametrize("name", ["useritem100", "karate_p025_q4", "hubs_useritem", "directed_nosink"])
def test_philox_walks_equal_the_restatement_on_the_fixture_graphs(n2v, name):
    z = load_popwalk_case(name)
    seed = 0xBEEF1234
    g = _graph(n2v, z, popwalk="pop", rng="philox", seed=seed)
    r, L = (1, 8) if name == "hubs_useritem" else (2, 15)
    for mode in (PRE, OTF):
        o = PopwalkOracle(oracle_graph(z), bool(z["directed"]), *case_pq(z), "pop")
        if mode == PRE:
            o.preprocess_transition_probs_popularity()
            g.preprocess_transition_probs_popularity()
            got = g.simulate_walks(r, L)
        else:
            got = g.simulate_walks_on_the_fly(r, L)
        want = o.simulate_walks(r, L, on_the_fly=(mode == OTF), step_uniforms=_philox(seed))
        assert got == want, (name, mode)


def _synthetic_hub_graph():
    """20k-node preferential-attachment graph (n2v_hip/synth.py), a third of the nodes relabelled as items, weights in
    quarters."""
    from n2v_hip import csr, synth
    u, v = synth.barabasi_albert_edges(20000, 5, seed=7)
    lab = np.arange(20000, dtype=np.int64)
    third = lab % 3 == 0
    lab[third] = 99999990000000 + lab[third]
    assert str(int(lab[0])).startswith("9999999") and str(int(lab[3])).startswith("9999999")
    rs = np.random.RandomState(3)
    return csr.from_edges(lab[u], lab[v], rs.randint(1, 13, len(u)) / 4.0, False)


def test_philox_walks_equal_the_restatement_on_a_20k_hub_graph(n2v):
    """Both modes on the synthetic hub graph: a subset of the starts (hubs included) against the restatement, the whole
    graph with the tables under a budget of a third against the fully stored tables."""
    import torch
    cg = _synthetic_hub_graph()
    deg = cg.degrees
    assert deg.max() > 256 and int(cg.labels[np.argmax(deg)]) >= 0
    seed = 424242
    g = n2v.Graph.from_csr(cg, 0.5, 2.0, rng="philox", seed=seed)
    hubs = cg.labels[np.argsort(-deg)[:6]].tolist()
    sub = hubs + cg.labels[cg.start_order[:600]].tolist()
    L = 8
    o = PopwalkOracle(csr_oracle_graph(cg), False, 0.5, 2.0, "pop")
    # on the fly
    g.popwalk = "pop"
    assert g.simulate_walks_on_the_fly(1, L, nodes=sub) == o.simulate_walks(1, L, nodes=sub, on_the_fly=True,
                                                                            step_uniforms=_philox(seed))
    otf_all = g.simulate_walks_on_the_fly(1, L)
    # precomputed
    g.preprocess_transition_probs_popularity()
    assert g._engine.pop_tables and not g._engine.partial
    o.preprocess_transition_probs_popularity(lazy=True)
    assert g.simulate_walks(1, L, nodes=sub) == o.simulate_walks(1, L, nodes=sub, step_uniforms=_philox(seed))
    full = g.simulate_walks(2, 20)
    fw, fl = full.walks.clone(), full.lens.clone()
    full_bytes = g._engine.total_slots * 32
    g.preprocess_transition_probs_popularity(budget_bytes=full_bytes // 3)
    eng = g._engine
    assert eng.partial and eng.pop_tables and 0 < eng.total_slots * 32 <= full_bytes // 3
    got = g.simulate_walks(2, 20)
    assert torch.equal(got.walks, fw) and torch.equal(got.lens, fl)
    assert g.simulate_walks(1, L, nodes=sub) == o.simulate_walks(1, L, nodes=sub, step_uniforms=_philox(seed))
    # the on-the-fly pop walk is another walk, and does not read the stored tables
    again = g.simulate_walks_on_the_fly(1, L)
    assert torch.equal(again.walks, otf_all.walks)
    assert not torch.equal(again.walks, g.simulate_walks(1, L).walks)


def test_mode_switching_on_one_graph_object(n2v):
    z = load_popwalk_case("useritem100")
    specs = walk_specs(z)
    pre = next(s for s in specs if s[6] == PRE and not s[7] and s[5] is None)
    otf = next(s for s in specs if s[6] == OTF and not s[7] and s[5] is None and s[1:4] == pre[1:4])
    _, seed, r, L = pre[:4]
    o = PopwalkOracle(oracle_graph(z), False, *case_pq(z), "none")
    o.preprocess_transition_probs()
    plain = o.simulate_walks(r, L, seed=seed)
    g = _graph(n2v, z)

    def run(fn):
        np.random.seed(seed)
        return fn(r, L)
    # plain -> popularity -> plain preprocess
    g.preprocess_transition_probs()
    assert run(g.simulate_walks) == plain
    eng = g._engine
    g.preprocess_transition_probs_popularity()
    assert g._engine is eng                       # the graph stays on the device; the tables change flavour
    assert run(g.simulate_walks) == golden_walks(z, pre[0])
    g.preprocess_transition_probs()
    assert run(g.simulate_walks) == plain
    # popwalk "pop" -> "none" between on-the-fly calls (stored plain tables may serve "none", never "pop")
    g.popwalk = "pop"
    assert run(g.simulate_walks_on_the_fly) == golden_walks(z, otf[0])
    g.popwalk = "none"
    assert run(g.simulate_walks_on_the_fly) == plain
    # the on-the-fly pop walk after the popularity preprocess: not the stored tables (those give pre's walks)
    g.preprocess_transition_probs_popularity()
    g.popwalk = "pop"
    assert golden_walks(z, otf[0]) != golden_walks(z, pre[0])
    assert run(g.simulate_walks_on_the_fly) == golden_walks(z, otf[0])
    assert run(g.simulate_walks) == golden_walks(z, pre[0])
    # ... and the on-the-fly PLAIN walk after the popularity preprocess must not start from the pop node tables
    g.popwalk = "none"
    assert run(g.simulate_walks_on_the_fly) == plain
    g.popwalk = "both"
    with pytest.raises(ValueError, match="popwalk"):
        g.simulate_walks_on_the_fly(r, L)


def test_p_q_1_keeps_the_plain_node_tables_for_later_steps(n2v):
    """p == q == 1: no edge tables are materialised, every record points at dst's NODE table.  After the popularity
    preprocess the first step draws from the pop tables and every later step from the plain node tables."""
    z = load_popwalk_case("useritem100")
    g = n2v.Graph(_nx_graph(z), False, 1, 1)
    o = PopwalkOracle(oracle_graph(z), False, 1, 1, "pop")
    o.preprocess_transition_probs_popularity()
    o_plain = PopwalkOracle(oracle_graph(z), False, 1, 1, "none")
    o_plain.preprocess_transition_probs()
    for fat in (None, False):
        g.preprocess_transition_probs_popularity()
        eng = g._engine
        if fat is not None:
            eng.preprocess(fat=fat, pop=True)
        assert eng.first_order and eng.pop_tables
        np.random.seed(21)
        got = g.simulate_walks(3, 25)
        assert got == o.simulate_walks(3, 25, seed=21)
        assert got != o_plain.simulate_walks(3, 25, seed=21)
        u, v = z["pe_keys"][0].tolist()
        J, q = g.alias_edges[(u, v)]
        wJ, wq = o_plain.alias_nodes[v]
        assert np.array_equal(J, wJ) and np.array_equal(_bits(q), _bits(wq))
        J, q = g.alias_nodes[v]
        wJ, wq = o.alias_nodes[v]
        assert np.array_equal(J, wJ) and np.array_equal(_bits(q), _bits(wq))


def test_errors(n2v):
    z = load_popwalk_case("directed_sink")
    g = _graph(n2v, z, popwalk="pop")
    with pytest.raises(ZeroDivisionError):          # sink neighbour: while preprocessing ...
        g.preprocess_transition_probs_popularity()
    with pytest.raises(ZeroDivisionError):          # ... on the fly when a walk gets there
        g.simulate_walks_on_the_fly(2, 10)
    g.rng = "philox"
    with pytest.raises(ZeroDivisionError):
        g.simulate_walks_on_the_fly(2, 10)
    safe = [0, 1, 2]
    o = PopwalkOracle(oracle_graph(z), True, *case_pq(z), "pop")
    assert g.simulate_walks_on_the_fly(2, 10, nodes=safe) == o.simulate_walks(2, 10, nodes=safe, on_the_fly=True,
                                                                              step_uniforms=_philox(0))
    k = load_popwalk_case("karate_p025_q4")
    for p, q, otf_ok in ((0, 2.0, False), (0.5, 0, True)):
        g = n2v.Graph(_nx_graph(k), False, p, q, popwalk="pop")
        with pytest.raises(ZeroDivisionError):
            g.preprocess_transition_probs_popularity()
        if otf_ok:                                  # q is never read by the pop rule
            o = PopwalkOracle(oracle_graph(k), False, p, q, "pop")
            np.random.seed(2)
            assert g.simulate_walks_on_the_fly(1, 12) == o.simulate_walks(1, 12, seed=2, on_the_fly=True)
            g.popwalk = "none"
        with pytest.raises(ZeroDivisionError):
            g.simulate_walks_on_the_fly(1, 12)
    g = n2v.Graph(_nx_graph(k), False, 0.25, 4.0, popwalk="both")
    with pytest.raises(ValueError, match="popwalk"):
        g.simulate_walks_on_the_fly(1, 5)
    with pytest.raises(ValueError, match="popwalk"):
        g.get_alias_nodes_cur(1)


def test_both_through_linkpred_philox(n2v):
    """simulate_walk_popularity(..., "both") in Philox mode: one WalkCorpus, the plain half first; "none" and "pop"
    are the single calls."""
    from n2v_hip import linkpred
    z = load_popwalk_case("useritem100")
    seed = 99
    for fly in (False, True):
        g = _graph(n2v, z, rng="philox", seed=seed)
        o = PopwalkOracle(oracle_graph(z), False, *case_pq(z), "none")
        for mode in ("both", "pop", "none"):
            got = linkpred.simulate_walk_popularity(g, mode, 5, 11, on_the_fly=fly)
            want = simulate_walk_popularity(o, mode, 5, 11, on_the_fly=fly, step_uniforms=_philox(seed))
            assert isinstance(got, n2v.WalkCorpus) and got == want, (fly, mode)
            assert len(got) == len(z["nodes"]) * (4 if mode == "both" else 5)


def test_shards_after_the_popularity_preprocess(n2v):
    """simulate_walks_shard after preprocess_transition_probs_popularity (only the node tables differ): the rows of
    every rank of a 2- and a 3-GPU layout equal the full call's, Philox and numpy streams."""
    import torch
    z = load_popwalk_case("useritem100")
    g = _graph(n2v, z, rng="philox", seed=5)
    g.preprocess_transition_probs_popularity()
    n, r, L = len(z["nodes"]), 3, 14
    o = PopwalkOracle(oracle_graph(z), False, *case_pq(z), "pop")
    o.preprocess_transition_probs_popularity()
    for rng in ("philox", "numpy"):
        g.rng = rng
        np.random.seed(8)
        full = g.simulate_walks(r, L)
        want = (o.simulate_walks(r, L, step_uniforms=_philox(5)) if rng == "philox" else o.simulate_walks(r, L, seed=8))
        assert full == want
        fw = full.walks.view(r, n, L)
        for world in (2, 3):
            for rank in range(world):
                np.random.seed(8)
                sh = g.simulate_walks_shard(r, L, rank, world)
                per = -(-n // world)
                b, e = min(rank * per, n), min(rank * per + per, n)
                assert torch.equal(sh.walks.view(r, e - b, L), fw[:, b:e]), (rng, world, rank)
