"""The popularity-biased walk, CPU side: tests/popwalk_reference.py (a plain fp64 restatement of the reference's
popwalk="pop" and --popwalk both) equals every fixture captured from the reference itself (tests/golden/popwalk/*.npz,
written by tests/golden/make_popwalk_golden.py) bit for bit — J as integers, q as raw fp64 bits, walks as lists, the
number of uniforms drawn, the exception's type where the reference raises — plus the host-side pieces of the product
that need no GPU: the exemption flags and the argument checks."""
import numpy as np
import pytest

from helpers import golden_walks, oracle_graph
from popwalk_reference import (OTF, POPWALK_CASES, PRE, PopwalkOracle, case_pq, load_popwalk_case, restated_walks,
                               walk_specs)

ERRORS = {"ZeroDivisionError": ZeroDivisionError}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle(z):
    p, q = case_pq(z)
    return PopwalkOracle(oracle_graph(z), bool(z["directed"]), p, q, "pop")


def test_fixture_set_is_complete():
    assert set(POPWALK_CASES) >= {"useritem100", "karate_p025_q4", "hubs_useritem", "directed_nosink", "directed_sink",
                                  "karate_p0", "karate_q0"}
    z = load_popwalk_case("hubs_useritem")
    deg = np.diff(z["adj_ptr"])
    big = [int(z["nodes"][i]) for i in np.nonzero(deg >= 520)[0]]
    assert any(str(v).startswith("9999999") for v in big) and any(not str(v).startswith("9999999") for v in big)
    assert ((deg > 64) & (deg <= 512)).any() and ((deg > 0) & (deg <= 64)).any()


@pytest.mark.parametrize("name", POPWALK_CASES)
def test_restated_tables_equal_the_reference(name):
    z = load_popwalk_case(name)
    o = _oracle(z)
    nodes, ap = z["nodes"].tolist(), z["adj_ptr"]
    G = o.G
    for i, v in enumerate(nodes):
        assert sorted(G.neighbors(v)) == z["adj"][ap[i]:ap[i + 1]].tolist()
    if str(z["pn_error"]):
        with pytest.raises(ERRORS[str(z["pn_error"])]):
            o.preprocess_transition_probs_popularity()
    else:
        for i, v in enumerate(nodes):
            J, q = o.get_alias_node_pop(v)
            assert np.array_equal(J, z["pn_J"][ap[i]:ap[i + 1]]), (name, v)
            assert np.array_equal(_bits(q), _bits(z["pn_q"][ap[i]:ap[i + 1]])), (name, v)
    ep = z["pe_ptr"]
    assert len(z["pe_keys"]) > 0
    for i, (u, v) in enumerate(z["pe_keys"].tolist()):
        err = str(z["pe_err"][i])
        if err:
            with pytest.raises(ERRORS[err]):
                o.get_alias_edge_pop(u, v)
            continue
        J, q = o.get_alias_edge_pop(u, v)
        assert np.array_equal(J, z["pe_J"][ep[i]:ep[i + 1]]), (name, u, v)
        assert np.array_equal(_bits(q), _bits(z["pe_q"][ep[i]:ep[i + 1]])), (name, u, v)


@pytest.mark.parametrize("name", POPWALK_CASES)
def test_restated_walks_equal_the_reference(name):
    z = load_popwalk_case(name)
    seen = set()
    for spec in walk_specs(z):
        i, seed, r, L, nd, sub, mode, both, err = spec
        o = _oracle(z)
        rs = np.random.RandomState(seed)
        if err:
            with pytest.raises(ERRORS[err]):
                restated_walks(o, spec, rs.random_sample)
            seen.add((mode, both, "err"))
            continue
        got = restated_walks(o, spec, rs.random_sample)
        assert got == golden_walks(z, i), (name, i)
        chk = np.random.RandomState(seed)
        chk.random_sample(nd)
        assert rs.random_sample() == chk.random_sample(), (name, i, "draw count")
        assert nd == 2 * sum(len(w) - 1 for w in got)
        seen.add((mode, both, bool(sub)))
    assert len(seen) >= 2


def test_the_two_modes_are_different_walks():
    """Precomputed popularity tables + plain edge tables against get_alias_edge_pop at every step: most walks differ,
    and the precomputed mode differs from the plain walk in its first step only (same tables afterwards)."""
    z = load_popwalk_case("useritem100")
    specs = {(s[1], s[2], s[3], s[6]): s[0] for s in walk_specs(z) if not s[7] and s[5] is None}
    differ = total = 0
    for (seed, r, L, mode), i in specs.items():
        if mode == PRE:
            a, b = golden_walks(z, i), golden_walks(z, specs[(seed, r, L, OTF)])
            differ += sum(x != y for x, y in zip(a, b))
            total += len(a)
    assert total > 0 and differ > total // 2
    o = _oracle(z)
    o.preprocess_transition_probs_popularity()
    pop_edges = o.alias_edges
    o.preprocess_transition_probs()
    for k, (J, q) in o.alias_edges.items():
        assert np.array_equal(J, pop_edges[k][0]) and np.array_equal(_bits(q), _bits(pop_edges[k][1]))


def test_exemption_flags_equal_str_startswith():
    from n2v_hip.csr import popwalk_exempt_flags
    labels = [9999999, 99999990, 999999, 19999999, -9999999, 99999989999, 2**62, 0, 1, -1, 99999991234567890, 2**63 - 1,
              -2**63, 999999900000000000, 9999998, 10**18, 99999999999, 9999999 * 10**11, 9999999 * 10**11 - 1]
    rs = np.random.RandomState(1)
    labels += [int(x) for x in rs.randint(0, 2**62, size=2000)]
    labels += [int("9999999%d" % x) for x in rs.randint(0, 10**9, size=500)]
    want = [1 if str(x).startswith('9999999') else 0 for x in labels]
    got = popwalk_exempt_flags(np.array(labels, dtype=np.int64))
    assert got.dtype == np.uint8 and got.tolist() == want
    assert sum(want) > 500 and popwalk_exempt_flags(np.zeros(0, dtype=np.int64)).shape == (0,)


def test_argument_checks_without_a_gpu():
    import node2vec
    from n2v_hip import csr, linkpred
    g = node2vec.Graph.from_csr(csr.from_edges([0, 1], [1, 2]), 1, 1)
    for bad in ("both", "popular", None):
        g.popwalk = bad
        for call in (lambda: g.simulate_walks_on_the_fly(1, 3), lambda: g.node2vec_walk_on_the_fly(3, 0),
                     lambda: g.get_alias_nodes_cur(0), lambda: g.get_alias_edges_cur(0, 1)):
            with pytest.raises(ValueError, match="popwalk"):
                call()
    with pytest.raises(ValueError, match="popwalk"):
        linkpred.simulate_walk_popularity(g, "popular", 2, 3)
    for p, q in ((0, 1), (1, 0)):
        g = node2vec.Graph.from_csr(csr.from_edges([0, 1], [1, 2]), p, q)
        with pytest.raises(ZeroDivisionError):
            g.preprocess_transition_probs_popularity()
    g = node2vec.Graph.from_csr(csr.from_edges([0, 1], [1, 2]), 0, 1, )
    g.popwalk = "pop"
    with pytest.raises(ZeroDivisionError):
        g.get_alias_edge_pop(0, 1)
    with pytest.raises(KeyError):
        g.get_alias_edge_pop(0, 7)
    import main
    assert main.parse_args([]).popwalk == "none" and main.parse_args(["--popwalk", "both"]).popwalk == "both"
    with pytest.raises(SystemExit):
        main.parse_args(["--popwalk", "popular"])
