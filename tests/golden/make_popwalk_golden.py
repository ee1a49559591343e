#!/usr/bin/env python3
"""Generate tests/golden/popwalk/*.npz: the reference's popularity-biased walk, captured from the reference itself.

CPU only; runs ONLY where the reference tree is mounted (the build container), through the same import of the
reference's ``src/node2vec.py`` (with the ``numpy.int = int`` shim) that make_golden.py uses.  Data only is written:
inputs and expected outputs, no reference source text.

Per graph:
* ``pn_J / pn_q``        the pop node tables (preprocess_transition_probs_popularity) in list(G.nodes()) order, slots in
                         sorted-neighbour order (``adj_ptr / adj``); ``pn_error``: the exception's type name instead;
* ``pe_keys/ptr/J/q``    get_alias_edge_pop(src, dst) for all adjacency entries (small graphs) or a seeded sample;
* ``walks_i_*``          walks under np.random.seed for both modes (``mode`` 0: preprocess_transition_probs_popularity +
                         simulate_walks; 1: simulate_walks_on_the_fly with popwalk == "pop"), two seeds, two shapes, a
                         ``nodes=`` subset call, and ``both`` (src/main_link.py:206-219 / :309-331: int(num_walks / 2)
                         plain rounds, then as many pop rounds, one stream) — with the number of uniforms consumed, or
                         the type name of the exception raised (``walk_err``).
Re-run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_popwalk_golden.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import build_graph, count_draws, karate_edges, ref  # noqa: E402  (ref = the reference's node2vec)

OUT = os.path.join(HERE, "popwalk")
PRE, OTF = 0, 1


def run_walks(G, directed, p, q, spec):
    """One walk call of the reference; returns (walks, draws) or (None, type name of the exception)."""
    seed, r, L = spec["seed"], spec["r"], spec["L"]
    sub = spec.get("nodes")
    try:
        np.random.seed(seed)
        if spec.get("both"):
            half = int(r / 2)
            if spec["mode"] == PRE:          # src/main_link.py:213-218
                g = ref.Graph(G, directed, p, q, "both")
                g.preprocess_transition_probs()
                walks = g.simulate_walks(half, L)
                g.preprocess_transition_probs_popularity()
                walks.extend(g.simulate_walks(half, L))
            else:                            # src/main_link.py:318-322, without the process pool
                g = ref.Graph(G, directed, p, q, "both")
                g.popwalk = "none"
                walks = g.simulate_walks_on_the_fly(half, L)
                g.popwalk = "pop"
                walks.extend(g.simulate_walks_on_the_fly(half, L))
        elif spec["mode"] == PRE:
            g = ref.Graph(G, directed, p, q, "pop")
            g.preprocess_transition_probs_popularity()
            walks = g.simulate_walks(r, L, nodes=sub)
        else:
            g = ref.Graph(G, directed, p, q, "pop")
            walks = g.simulate_walks_on_the_fly(r, L, nodes=sub)
    except Exception as exc:                 # noqa: BLE001 — the type name IS the expected output
        return None, type(exc).__name__
    n = count_draws(seed, np.random.get_state())
    assert n == 2 * sum(len(w) - 1 for w in walks)
    return walks, n


def std_specs(subset, shapes=((2, 12), (1, 30))):
    specs = []
    for mode in (PRE, OTF):
        for seed in (3, 11):
            for r, L in shapes:
                specs.append({"seed": seed, "r": r, "L": L, "mode": mode})
        specs.append({"seed": 5, "r": 2, "L": 9, "mode": mode, "nodes": subset})
        specs.append({"seed": 7, "r": 4, "L": 10, "mode": mode, "both": True})
    return specs


def dump_case(name, edges, weights, directed, p, q, specs, int_weights=False, edge_sample=None):
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    weights = np.asarray(weights, dtype=np.float64)
    wl = [int(w) for w in weights] if int_weights else [float(w) for w in weights]
    G = build_graph(edges, wl, directed)
    nodes = list(G.nodes())
    out = {"edges": edges, "weights": weights, "directed": np.array(directed), "int_weights": np.array(int_weights),
           "p": np.array(float(p)), "q": np.array(float(q)), "nodes": np.array(nodes, dtype=np.int64)}
    adj_ptr, adj = [0], []
    for v in nodes:
        adj.extend(sorted(G.neighbors(v)))
        adj_ptr.append(len(adj))
    out["adj_ptr"] = np.array(adj_ptr, dtype=np.int64)
    out["adj"] = np.array(adj, dtype=np.int64)

    # pop node tables: get_alias_nodes_cur with popwalk == "pop" (:13-25) is what :213-221 computes per node; the
    # whole-graph preprocess is tried first, for its exception
    g = ref.Graph(G, directed, p, q, "pop")
    J_all, q_all, err = [], [], ""
    try:
        g2 = ref.Graph(G, directed, 1.0, 1.0, "pop")      # the node tables do not depend on p, q
        g2.preprocess_transition_probs_popularity()
        for v in nodes:
            J, qq = g2.alias_nodes[v]
            Jc, qc = g.get_alias_nodes_cur(v) if len(J) else (J, qq)
            assert np.array_equal(J, Jc) and np.array_equal(np.asarray(qq).view(np.uint64), np.asarray(qc).view(np.uint64))
            J_all.extend(int(x) for x in J)
            q_all.extend(float(x) for x in qq)
    except ZeroDivisionError as exc:
        err, J_all, q_all = type(exc).__name__, [], []
    out["pn_error"] = np.array(err)
    out["pn_J"] = np.array(J_all, dtype=np.int64)
    out["pn_q"] = np.array(q_all, dtype=np.float64)

    # get_alias_edge_pop: every adjacency entry, or a seeded sample
    keys = [(u, v) for u in nodes for v in sorted(G.neighbors(u))]
    if edge_sample is not None:
        rs = np.random.RandomState(edge_sample[0])
        big = [k for k in keys if len(G[k[1]]) > 64]
        pick = rs.choice(len(keys), size=min(edge_sample[1], len(keys)), replace=False)
        pickb = rs.choice(len(big), size=min(edge_sample[2], len(big)), replace=False) if big else []
        keys = [keys[i] for i in sorted(pick)] + [big[i] for i in sorted(pickb)]
    pe_ptr, pe_J, pe_q, pe_err = [0], [], [], []
    for (u, v) in keys:
        try:
            J, qq = g.get_alias_edge_pop(u, v)
            pe_err.append("")
        except ZeroDivisionError as exc:
            J, qq = [], []
            pe_err.append(type(exc).__name__)
        pe_J.extend(int(x) for x in J)
        pe_q.extend(float(x) for x in qq)
        pe_ptr.append(len(pe_J))
    out["pe_keys"] = np.array(keys, dtype=np.int64).reshape(-1, 2)
    out["pe_ptr"] = np.array(pe_ptr, dtype=np.int64)
    out["pe_J"] = np.array(pe_J, dtype=np.int64)
    out["pe_q"] = np.array(pe_q, dtype=np.float64)
    out["pe_err"] = np.array(pe_err)

    metas, errs = [], []
    for i, spec in enumerate(specs):
        walks, n = run_walks(G, directed, p, q, spec)
        sub = spec.get("nodes")
        if walks is None:
            errs.append(n)
            walks, n = [], -1
        else:
            errs.append("")
        out["walks_%d_flat" % i] = np.array([x for w in walks for x in w], dtype=np.int64)
        out["walks_%d_ptr" % i] = np.cumsum([0] + [len(w) for w in walks]).astype(np.int64)
        out["walks_%d_subset" % i] = np.array(sub if sub else [], dtype=np.int64)
        metas.append([spec["seed"], spec["r"], spec["L"], n, 1 if sub else 0, spec["mode"], 1 if spec.get("both") else 0])
    out["walk_meta"] = np.array(metas, dtype=np.int64).reshape(-1, 7)
    out["walk_err"] = np.array(errs)

    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-22s N=%d nnz=%d pn_error=%r pe=%d walks=%d errors=%s  %d B" % (
        name, len(nodes), len(adj), err, len(keys), len(specs), sorted(set(e for e in errs if e)), os.path.getsize(path)))


def item(i):
    return int("9999999%d" % i)


def main():
    # 1. weighted undirected user-item graph, 60 users x 40 items (labels 9999999x), a few user-user edges
    rs = np.random.RandomState(2025)
    users, items = list(range(100, 160)), [item(i) for i in range(40)]
    seen, ue, uw = set(), [], []
    while len(ue) < 320:
        u, it = users[rs.randint(60)], items[min(int(40 * rs.random_sample() ** 2), 39)]
        if (u, it) not in seen:
            seen.add((u, it))
            ue.append((u, it)); uw.append(float(rs.randint(1, 11)) / 2.0)
    for k in range(25):
        a, b = users[rs.randint(60)], users[rs.randint(60)]
        if a != b and (a, b) not in seen and (b, a) not in seen:
            seen.add((a, b))
            ue.append((a, b)); uw.append(0.25 + float(rs.random_sample()))
    dump_case("useritem100", ue, uw, False, 0.5, 2.0, std_specs([items[0], 101, items[7], 150, 101]))

    # 2. karate, integer weights
    ke = karate_edges()
    dump_case("karate_p025_q4", ke, [1] * len(ke), False, 0.25, 4.0, std_specs([5, 1, 34, 12, 12, 3]), int_weights=True)

    # 3. hubs: one user-labelled (7) and one item-labelled (item(1)) hub of >= 520 neighbours (global scratch rows of
    #    the on-the-fly kernel), rows of 65-512 neighbours (its LDS window) and of <= 64 (registers)
    he, hw = [], []
    leaves = list(range(1000, 1700))
    for t in leaves[:530]:
        he.append((7, t)); hw.append(0.5 + (t * 37 % 11) / 4.0)
    for t in leaves[150:680]:
        he.append((item(1), t)); hw.append(0.25 + (t * 13 % 7) / 2.0)
    for t in leaves[::3][:120]:
        he.append((8, t)); hw.append(1.0 + (t % 5))                  # 120 neighbours
    for t in leaves[5::2][:300]:
        he.append((item(2), t)); hw.append(0.75 + (t % 3))           # 300 neighbours
    for t in leaves[1::7][:70]:
        he.append((9, t)); hw.append(2.0)                            # 70 neighbours
    he += [(7, item(1)), (7, 8), (8, item(2)), (9, item(1)), (9, 7)]
    hw += [3.0, 1.5, 0.5, 2.5, 1.0]
    for k in range(0, 690, 9):
        he.append((leaves[k], leaves[k + 5])); hw.append(1.25)       # leaf-leaf edges: common neighbours
    hub_specs = std_specs([7, item(1), 1003, 8, item(2), 9, 1500], shapes=((1, 12), (1, 6)))
    dump_case("hubs_useritem", he, hw, False, 0.5, 2.0, hub_specs, edge_sample=(5, 60, 40))

    # 4. directed, no sinks: a ring with chords, weighted
    de, dw = [], []
    for i in range(40):
        de.append((i, (i + 1) % 40)); dw.append(1.0 + (i % 4) * 0.5)
        if i % 3 == 0:
            de.append((i, (i * 7 + 3) % 40)); dw.append(0.75)
        if i % 5 == 0:
            de.append(((i + 1) % 40, i)); dw.append(2.0)
    de += [(item(3), 0), (item(3), 5), (4, item(3))]
    dw += [1.0, 2.0, 0.5]
    dump_case("directed_nosink", de, dw, True, 0.5, 2.0, std_specs([0, 5, item(3), 17]))

    # 5. directed with a sink (13): 12's row holds it, so a walk that stands on 12 after its first step — or starts on
    #    the user-labelled 12 — divides by zero; the ring 0-1-2 and the item-labelled 99999995 cannot get there.
    #    99999995 -> 13 is legal on the FIRST step (exempt: plain weights) and ends that walk at length 2.
    se = [(0, 1), (1, 2), (2, 0), (0, 2), (1, 0), (10, 11), (11, 12), (12, 13), (12, 10), (item(5), 13), (item(5), 0),
          (item(5), 1)]
    sw = [1.0, 2.0, 1.5, 0.5, 1.0, 1.0, 1.0, 2.0, 1.0, 3.0, 1.0, 0.5]
    sink_specs = std_specs([0, item(5), 1, 2, item(5), item(5)])
    sink_specs += [{"seed": 3, "r": 6, "L": 8, "mode": OTF, "nodes": [item(5), 0, item(5), 2, item(5), 1]},
                   {"seed": 4, "r": 2, "L": 6, "mode": OTF, "nodes": [0, 11]}]
    dump_case("directed_sink", se, sw, True, 0.5, 2.0, sink_specs)

    # 6. p == 0 (both modes raise) and q == 0 (legal on the fly with "pop": q is never read there)
    small = std_specs([5, 1, 34], shapes=((1, 10), (2, 5)))
    dump_case("karate_p0", ke, [1] * len(ke), False, 0, 2.0, small, int_weights=True)
    dump_case("karate_q0", ke, [1] * len(ke), False, 0.5, 0, small, int_weights=True)


if __name__ == "__main__":
    main()
