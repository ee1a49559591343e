"""The walk host side holds no hidden mode (run with -m gpu): which engine entry point a call of Graph uses is decided
per call and never kept on the object, so a predicate's answer and a walk's uniforms do not depend on which method ran
before; the launch wrappers know three rng names and refuse every other; preprocess reports its phases under the names
the tools read.  The graph is the 200-node, 700-edge undirected one of tests/test_gpu_mt19937.py, p = 0.5, q = 2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, Q, L = 0.5, 2.0, 36


@pytest.fixture(scope="module")
def cg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from n2v_hip import csr
    rs = np.random.RandomState(9)
    n, m = 200, 700
    src, dst = rs.randint(0, n, m), rs.randint(0, n, m)
    keep = src != dst
    return csr.from_edges(src[keep], dst[keep], None, False)          # undirected: no walk ends early


@pytest.fixture
def numpy_global_state():
    saved = np.random.get_state()
    yield
    np.random.set_state(saved)


def _fresh(cg):
    import node2vec
    g = node2vec.Graph.from_csr(cg, P, Q, rng="numpy")
    g.preprocess_transition_probs()
    return g


def test_tiled_predicate_on_a_graph_that_never_walked(cg):
    g = _fresh(cg)
    assert g._engine.edge_fat is not None and not g._engine.partial
    assert g._tiled_uniforms_ok(L) is True
    assert g._tiled_uniforms_ok(1) is False
    for knob in ("host_rng", "linear_uniforms"):
        setattr(g, knob, True)
        assert g._tiled_uniforms_ok(L) is False, knob
        g.__dict__.pop(knob)
        assert g._tiled_uniforms_ok(L) is True, knob
    g.preprocess_transition_probs(budget_bytes=g._engine.total_slots * 32 // 3)
    assert g._engine.partial and g._engine.edge_fat is not None
    assert g._tiled_uniforms_ok(L) is False


def test_numpy_mode_walks_do_not_depend_on_the_call_before(cg, numpy_global_state):
    import torch
    a, b = _fresh(cg), _fresh(cg)
    a.force_on_the_fly = True
    np.random.seed(5)
    fly = a.simulate_walks_on_the_fly(2, L)
    a.force_on_the_fly = False
    np.random.seed(5)
    after = a.simulate_walks(2, L)
    st_a = np.random.get_state()
    np.random.seed(5)
    alone = b.simulate_walks(2, L)
    st_b = np.random.get_state()
    assert bool((alone.lens == L).all())
    for other in (fly, after):
        assert torch.equal(other.lens, alone.lens) and torch.equal(other.walks, alone.walks)
    assert st_a[0] == st_b[0] and np.array_equal(st_a[1], st_b[1]) and st_a[2:] == st_b[2:]
    for g in (a, b):
        assert "_walk" not in vars(g) and "_walk_pop" not in vars(g)


def test_launch_wrappers_refuse_unknown_and_misplaced_rng_names(cg):
    from n2v_hip.engine import WalkEngine
    eng = WalkEngine(cg, P, Q)
    eng.preprocess()
    with pytest.raises(ValueError, match="rng must be"):
        eng.walk(eng.start_order, 1, 2, rng="numpy")
    with pytest.raises(ValueError, match="rng must be"):
        eng.walk_on_the_fly(eng.start_order, 1, 2, rng="numpy")
    with pytest.raises(ValueError, match="fat-table walk kernel only"):
        eng.walk_on_the_fly(eng.start_order, 1, 2, rng="uniforms_tiled")


def test_preprocess_phase_names_and_order(cg, monkeypatch):
    from n2v_hip.engine import WalkEngine
    monkeypatch.setenv("N2V_TIMING", "1")
    eng = WalkEngine(cg, P, Q)
    eng.preprocess(fat=True)
    assert list(eng.timings) == ["alloc", "node_tables", "offsets_recs", "src_of", "edge_tables_fat", "node_fat"]
    eng.preprocess(fat="both")
    assert list(eng.timings) == ["alloc", "node_tables", "offsets_recs", "src_of", "edge_tables_thin", "edge_tables_fat",
                                 "node_fat"]
    first = WalkEngine(cg, 1.0, 1.0)
    first.preprocess()
    assert first.first_order
    assert list(first.timings) == ["alloc", "node_tables", "offsets_recs", "node_fat"]
