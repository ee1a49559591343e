"""TEST INFRASTRUCTURE — a plain fp64 Python restatement of the reference's popularity-biased walk
(``popwalk="pop"`` of src/node2vec.py and ``--popwalk both`` of src/main_link.py), pinned bit for bit to fixtures
captured from the reference itself (tests/golden/popwalk/*.npz, tests/test_popwalk_golden.py).

What it restates (line numbers of src/node2vec.py; pop(x) = len(G[x]), the out-degree on a DiGraph):

1. pop node table (:13-25, :213-221): over sorted(G.neighbors(cur)) the weights w * 1.0 / pop(nbr) — unless
   str(cur).startswith('9999999'), which keeps the plain weights (the test looks at cur, not at the neighbour);
2. pop edge table get_alias_edge_pop (:154-174): w / (p * pop(nbr)) for nbr == src, w / pop(nbr) otherwise; q is not
   read and there is no label exemption;
3. two modes that are NOT the same walk: precomputed (preprocess_transition_probs_popularity, :206-237) = pop NODE
   tables + the ordinary get_alias_edge tables; on the fly (:27-53 with self.popwalk == "pop") = pop node table for
   the first step, get_alias_edge_pop for every later one;
4. errors are Python's own: a neighbour of pop 0 or p == 0 divide by zero; q == 0 only matters where get_alias_edge
   runs; an unknown popwalk on the on-the-fly entry points is a ValueError here (UnboundLocalError in the reference);
5. "both" (src/main_link.py:206-219, :309-331): int(num_walks / 2) rounds plain, then as many pop, one stream.
"""
from oracle.n2v_oracle import Node2VecOracle, _per_walk_rand, alias_draw_u, alias_setup


def is_exempt(label):
    return str(label).startswith('9999999')


class _Lazy(dict):
    def __init__(self, fn):
        super().__init__()
        self._fn = fn

    def __missing__(self, key):
        self[key] = v = self._fn(key)
        return v


class PopwalkOracle(Node2VecOracle):
    def __init__(self, G, is_directed, p, q, popwalk="none"):
        super().__init__(G, is_directed, p, q)
        self.popwalk = popwalk

    def pop(self, x):
        return len(self.G.adj[x])

    # :13-25 with popwalk == "pop" / :213-221
    def get_alias_node_pop(self, cur):
        G = self.G
        if is_exempt(cur):
            unnormalized = [G.adj[cur][nbr] for nbr in sorted(G.neighbors(cur))]
        else:
            unnormalized = [G.adj[cur][nbr] * 1.0 / self.pop(nbr) for nbr in sorted(G.neighbors(cur))]
        norm_const = sum(unnormalized)
        return alias_setup([float(u) / norm_const for u in unnormalized])

    # :154-174
    def get_alias_edge_pop(self, src, dst):
        G, p = self.G, self.p
        unnormalized = []
        for dst_nbr in sorted(G.neighbors(dst)):
            pop = self.pop(dst_nbr)
            if dst_nbr == src:
                unnormalized.append(G.adj[dst][dst_nbr] / (p * pop))
            else:
                unnormalized.append(G.adj[dst][dst_nbr] / pop)
        norm_const = sum(unnormalized)
        return alias_setup([float(u) / norm_const for u in unnormalized])

    # :13-32 — read self.popwalk at call time
    def get_alias_nodes_cur(self, cur):
        if self.popwalk == "none":
            return self.get_alias_node(cur)
        if self.popwalk == "pop":
            return self.get_alias_node_pop(cur)
        raise ValueError(self.popwalk)

    def get_alias_edges_cur(self, prev, cur):
        if self.popwalk == "none":
            return self.get_alias_edge(prev, cur)
        if self.popwalk == "pop":
            return self.get_alias_edge_pop(prev, cur)
        raise ValueError(self.popwalk)

    # :206-237 — pop node tables, PLAIN edge tables.  lazy: the same tables, built when a walk first asks for them
    # (graphs whose sum of deg^2 is too much for a Python loop up front)
    def preprocess_transition_probs_popularity(self, lazy=False):
        G = self.G
        if lazy:
            self.alias_nodes = _Lazy(self.get_alias_node_pop)
            self.alias_edges = _Lazy(lambda k: self.get_alias_edge(*k))
            return
        alias_nodes = {node: self.get_alias_node_pop(node) for node in G.nodes}
        alias_edges = {}
        for (u, v) in G.edges():
            alias_edges[(u, v)] = self.get_alias_edge(u, v)
            if not self.is_directed:
                alias_edges[(v, u)] = self.get_alias_edge(v, u)
        self.alias_nodes, self.alias_edges = alias_nodes, alias_edges

    # :34-53 (on the fly, honours popwalk) and :55-79 (stored tables)
    def node2vec_walk(self, walk_length, start_node, rand, on_the_fly=False):
        G = self.G
        walk = [start_node]
        while len(walk) < walk_length:
            cur = walk[-1]
            cur_nbrs = sorted(G.neighbors(cur))
            if len(cur_nbrs) == 0:
                break
            if len(walk) == 1:
                J, q = self.get_alias_nodes_cur(cur) if on_the_fly else self.alias_nodes[cur]
            else:
                prev = walk[-2]
                J, q = self.get_alias_edges_cur(prev, cur) if on_the_fly else self.alias_edges[(prev, cur)]
            u1 = rand()
            u2 = rand()
            walk.append(cur_nbrs[alias_draw_u(J, q, u1, u2)])
        return walk


def simulate_walk_popularity(o, popwalk, num_walks, walk_length, rand=None, on_the_fly=False, step_uniforms=None):
    """src/main_link.py:206-219 (precomputed) / :309-331 (on the fly) on a PopwalkOracle: one list, the plain half
    first.  rand: the sequential stream shared by both halves; step_uniforms(w, t): a counter-based stream, where the
    walk index w restarts with every simulate_walks call, as the product's Philox counter does."""
    if popwalk not in ("none", "pop", "both"):
        raise ValueError(popwalk)
    flavours = ["none", "pop"] if popwalk == "both" else [popwalk]
    rounds = int(num_walks / 2) if popwalk == "both" else num_walks
    walks = []
    for flavour in flavours:
        if on_the_fly:
            o.popwalk = flavour
        elif flavour == "pop":
            o.preprocess_transition_probs_popularity()
        else:
            o.preprocess_transition_probs()
        walks.extend(o.simulate_walks(rounds, walk_length, rand=rand, on_the_fly=on_the_fly,
                                      step_uniforms=step_uniforms))
    return walks


def csr_oracle_graph(cg):
    """The oracle's graph over a product CsrGraph (labels, sorted rows), for graphs made without networkx."""
    from oracle.n2v_oracle import CsrBackedGraph
    return CsrBackedGraph(cg.labels, cg.row_ptr, cg.col, cg.w, cg.start_order, cg.directed)


# ---- the fixtures of tests/golden/make_popwalk_golden.py -----------------------------------------------------------
import glob  # noqa: E402
import os  # noqa: E402

import numpy as np  # noqa: E402

POPWALK_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "popwalk")
POPWALK_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(POPWALK_GOLDEN, "*.npz")))
PRE, OTF = 0, 1


def load_popwalk_case(name):
    return dict(np.load(os.path.join(POPWALK_GOLDEN, name + ".npz"), allow_pickle=False))


def case_pq(z):
    """p and q as the generator passed them: integers where they are integral (0 must divide as an int does)."""
    return tuple(int(x) if float(x) == int(x) else float(x) for x in (z["p"], z["q"]))


def walk_specs(z):
    """[(index, seed, r, L, draws, subset or None, mode, both, error name or '')]"""
    out = []
    for i, (seed, r, L, nd, has_sub, mode, both) in enumerate(z["walk_meta"].tolist()):
        sub = z["walks_%d_subset" % i].tolist() if has_sub else None
        out.append((i, seed, r, L, nd, sub, mode, bool(both), str(z["walk_err"][i])))
    return out


def restated_walks(o, spec, rand):
    """The restatement's answer to one fixture call (raises what Python raises)."""
    i, seed, r, L, nd, sub, mode, both, err = spec
    if both:
        return simulate_walk_popularity(o, "both", r, L, rand=rand, on_the_fly=(mode == OTF))
    o.popwalk = "pop"
    if mode == PRE:
        o.preprocess_transition_probs_popularity()
    return o.simulate_walks(r, L, nodes=sub, rand=rand, on_the_fly=(mode == OTF))
