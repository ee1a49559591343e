"""TEST INFRASTRUCTURE — graphs that put the walk and alias-table kernels on their window and list edges, and a plain
Python "reach" analysis that says which branch of the kernels every step of a walk takes.

The builders are numpy only and deterministic.  The reach analysis restates the kernels' BRANCH CHOICES, not their
arithmetic (csrc/n2v_wave_table.h: dyadic_draw, wave_pair; csrc/n2v_walk_otf.hip: OtfWave::pick; csrc/n2v_tables.hip);
tests/test_walk_edge_cases_host.py asserts with it that every edge below is reached by the C oracle's walks, so that
tests/test_gpu_walk_edges.py compares the kernels with the oracle where their control flow changes.

Cases
  A  dense blocks: disjoint cliques of 65, 66, 129 and 130 nodes with pendant leaves — the class sweep's list of
     special slots at 64 (the register path's last size), 65 (second half), 128 (the cap) and 129 (fallback, LDS table);
  B  hub ladder: hubs of degree 255 ... 2049 over a sparse fringe — every LDS window of the builder and of the
     on-the-fly walk, the staging strides 1, 2, 3; weighted and directed copies for the general path;
  C  twin hubs: six pairwise adjacent hubs over the same 300 neighbours — the fallback into the global scratch row and
     the "walk prev's row" choice, thousands of times instead of a handful;
  D  crafted stacks: a directed weighted graph whose tables are alias_setup of chosen weight rows — Vose's two stacks
     at 0, 1, 63, 64, 65 entries and every event of the wave builder's streamed pairing;
  E  (no graph of its own) A and B under a table budget, walked for enough rounds to run the lane-per-walk kernel.
"""
import functools

import numpy as np

# ---- the constants of the kernels that the analysis restates ------------------------------------------------------
SPEC_CAP = 128        # n2v_wave_table.h kSpecCap
OTF_LDS_SLOTS = 256   # n2v_walk_otf.hip kLdsSlots: the table window of the on-the-fly walk
OTF_ROW = 256         # n2v_walk_otf.hip kOtfRow: the row buffers of the on-the-fly walk
STAGE_CAP = 1024      # the ints of the table window that stage_row may use (kLdsSlots * 4)
BUILDER_LDS_SLOTS = 512   # n2v_tables.hip kLdsSlots
ROW_CACHE = 384       # n2v_wave_table.h kRowCache

A_PQ = [(0.25, 4.0), (4.0, 0.25), (1.0, 1.0), (0.3, 0.7), (2.0 ** -10, 2.0 ** 20), (2.0 ** -11, 2.0 ** 21)]
A_CLIQUES = (65, 66, 129, 130)
B_HUBS = (255, 256, 257, 257, 300, 384, 385, 512, 513, 1024, 1025, 2049)
B_ADJACENT = ((1, 2), (2, 3), (5, 4), (9, 10))    # positions in B_HUBS: 256-257, 257-257, 384-300, 1024-1025
D_KS = (65, 128, 129, 193, 512, 513, 640)
D_UNPOPPED_KS = (49, 98, 103, 107, 561, 569, 644)   # K * (1.0 / K) < 1.0: every slot `smaller`, none ever popped
D_SOURCES = 9          # tables per crafted row: every stack size below is then built at least 50 times


def _csr():
    from n2v_hip import csr
    return csr


# ---------------------------------------------------------------------------------------------------- builders
def case_a():
    """Disjoint cliques of A_CLIQUES nodes; member i carries i % 3 pendant leaves; ids randomly permuted.  Returns
    (CsrGraph, info) with info["clique_of"][dense id] = clique size or 0 for a leaf."""
    rs = np.random.RandomState(1001)
    src, dst, nxt, members = [], [], 0, []
    for n in A_CLIQUES:
        ids = np.arange(nxt, nxt + n)
        nxt += n
        iu, ju = np.triu_indices(n, 1)
        src.append(ids[iu])
        dst.append(ids[ju])
        members.append(ids)
    for ids in members:
        for i, v in enumerate(ids):
            for _ in range(i % 3):
                src.append(np.array([v]))
                dst.append(np.array([nxt]))
                nxt += 1
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = rs.permutation(nxt)
    cg = _csr().from_edges(perm[src], perm[dst], None, False)
    clique_of = np.zeros(nxt, dtype=np.int64)
    for n, ids in zip(A_CLIQUES, members):
        clique_of[perm[ids]] = n
    return cg, {"clique_of": clique_of}


def _case_b_edges():
    rs = np.random.RandomState(1002)
    F = 2600
    m = F * 3 // 2
    fs, fd = rs.randint(0, F, m), rs.randint(0, F, m)
    keep = fs != fd
    src, dst = [fs[keep]], [fd[keep]]
    hubs = F + np.arange(len(B_HUBS))
    n_adj = np.zeros(len(B_HUBS), dtype=np.int64)
    for a, b in B_ADJACENT:
        src.append(np.array([hubs[a]]))
        dst.append(np.array([hubs[b]]))
        n_adj[a] += 1
        n_adj[b] += 1
    hub_edges = []
    for h, deg in enumerate(B_HUBS):
        nb = rs.choice(F, deg - int(n_adj[h]), replace=False)
        hub_edges.append((np.full(len(nb), hubs[h]), nb))
    perm = rs.permutation(F + len(B_HUBS))
    return rs, perm, src, dst, hub_edges, hubs


def case_b(kind="plain"):
    """Hubs of degree B_HUBS over a fringe of 2600 nodes of mean degree 3 among themselves, a few hub pairs adjacent.
    kind: "plain" (undirected, unweighted), "weighted" (weights randint(1, 17) / 4) or "directed" (the hubs keep their
    out-rows, a third of each hub's neighbours point back, the fringe lines keep their direction: nodes without
    out-edges exist).  Returns (CsrGraph, info) with info["hubs"] = dense ids in the order of B_HUBS."""
    rs, perm, src, dst, hub_edges, hubs = _case_b_edges()
    for hs, nb in hub_edges:
        src.append(hs)
        dst.append(nb)
        if kind == "directed":
            src.append(nb[: len(nb) // 3])
            dst.append(hs[: len(nb) // 3])
    src, dst = np.concatenate(src), np.concatenate(dst)
    if kind == "directed":        # the adjacent hub pairs point both ways
        back = [(hubs[b], hubs[a]) for a, b in B_ADJACENT if a != b]
        src = np.concatenate([src, np.array([s for s, _ in back])])
        dst = np.concatenate([dst, np.array([d for _, d in back])])
    w = None
    if kind == "weighted":
        w = rs.randint(1, 17, len(src)) / 4.0
    cg = _csr().from_edges(perm[src], perm[dst], w, kind == "directed")
    dense_hubs = cg.dense_of(perm[hubs])
    if kind != "directed":
        assert np.diff(cg.row_ptr)[dense_hubs].tolist() == list(B_HUBS)
    return cg, {"hubs": dense_hubs}


def case_c():
    """Six pairwise adjacent hubs over the same 300 neighbours (K = 305 at a hub, 6 at a neighbour)."""
    rs = np.random.RandomState(1003)
    hubs = np.arange(6)
    nbrs = 6 + np.arange(300)
    iu, ju = np.triu_indices(6, 1)
    src = np.concatenate([hubs[iu], np.repeat(hubs, 300)])
    dst = np.concatenate([hubs[ju], np.tile(nbrs, 6)])
    perm = rs.permutation(306)
    cg = _csr().from_edges(perm[src], perm[dst], None, False)
    return cg, {"hubs": cg.dense_of(perm[hubs])}


def _two_level(rs, K, nl):
    w = np.full(K, 0.5)
    w[rs.choice(K, nl, replace=False)] = 2.0
    return w


def case_d_rows():
    """[(name, weights)] of the crafted rows, in a fixed order."""
    rs = np.random.RandomState(1004)
    rows = []
    for K in D_KS:
        nls = sorted({nl for nl in (1, 63, 64, 65, K - 65, K - 64, K - 63, K - 1) if 1 <= nl <= K - 1})
        for nl in nls:
            rows.append(("two_level K=%d nl=%d" % (K, nl), _two_level(rs, K, nl)))
        rows.append(("pareto K=%d" % K, rs.pareto(1.2, K) + 0.05))
        rows.append(("ones K=%d" % K, np.ones(K)))
    for K in D_UNPOPPED_KS:
        rows.append(("ones K=%d (unpopped)" % K, np.ones(K)))
    return rows


def case_d():
    """A directed weighted graph: node v_t has the K out-neighbours (pool nodes, ascending) of crafted row t with that
    row's weights, and D_SOURCES pool nodes point at it — with p = q = 1 and no first-order shortcut the table
    (src -> v_t) is alias_setup of exactly those weights.  Pool nodes form a ring so that walks go on.  Returns
    (CsrGraph, info): info["rows"] = [(name, dense id of v_t, weights)], info["pool"] = dense ids."""
    rs = np.random.RandomState(1005)
    rows = case_d_rows()
    P = 700
    pool = np.arange(P)
    src, dst, w = [pool], [(pool + 1) % P], [np.ones(P)]
    vs = P + np.arange(len(rows))
    for t, (_, wt) in enumerate(rows):
        K = len(wt)
        nb = np.sort(rs.choice(P, K, replace=False))
        src.append(np.full(K, vs[t]))
        dst.append(nb)
        w.append(wt)
        s = rs.choice(P, D_SOURCES, replace=False)
        src.append(s)
        dst.append(np.full(D_SOURCES, vs[t]))
        w.append(np.ones(D_SOURCES))
    cg = _csr().from_edges(np.concatenate(src), np.concatenate(dst), np.concatenate(w), True)
    out = []
    for t, (name, wt) in enumerate(rows):       # labels are 0 .. n-1 already: dense id == label
        v = int(cg.dense_of([vs[t]])[0])
        b, e = int(cg.row_ptr[v]), int(cg.row_ptr[v + 1])
        assert np.array_equal(cg.w[b:e], wt), name
        out.append((name, v, wt))
    return cg, {"rows": out, "pool": cg.dense_of(pool)}


# ---------------------------------------------------------------------------------------------------- reach analysis
def _pair_counts(ow, ol):
    """Every step (prev, cur) of the walks that has a prev — the draw made at `cur` having arrived from `prev` — as
    (prev[], cur[], count[]) over the distinct pairs."""
    L = ow.shape[1]
    if L < 3:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    prev, cur = ow[:, :-2].astype(np.int64), ow[:, 1:-1].astype(np.int64)
    taken = np.arange(2, L)[None, :] < ol[:, None]          # a node was written at position t: the draw at t-1 happened
    n = int(max(ow.max(), 0)) + 1
    key, cnt = np.unique((prev * n + cur)[taken], return_counts=True)
    return key // n, key % n, cnt


def reach(cg, ow, ol):
    """Files every step with a prev of the walks (ow, ol) under the branches the on-the-fly kernel takes for it.
    Returns {bucket name: number of steps}."""
    rp, col = cg.row_ptr, cg.col
    deg = np.diff(rp)
    three_class = cg.w is None and not cg.directed      # draw_first == 2 (launch_otf)
    out = {}

    def add(name, c):
        out[name] = out.get(name, 0) + int(c)
    for p, c, cnt in zip(*_pair_counts(ow, ol)):
        K, S = int(deg[c]), int(deg[p])
        if K in (64, 65, 255, 256, 257, 384, 385, 512, 513, 1024, 1025):
            add("K=%d" % K, cnt)
        if not three_class:
            add("general: registers (K<=64)" if K <= 64 else
                "general: table in LDS" if K <= OTF_LDS_SLOTS else "general: table in scratch", cnt)
            if K in (OTF_LDS_SLOTS, OTF_LDS_SLOTS + 1):
                add("general K=%d" % K, cnt)
            continue
        rc, rprev = col[rp[c]:rp[c + 1]], col[rp[p]:rp[p + 1]]
        m = len(np.intersect1d(rc[rc != p], rprev, assume_unique=True)) + int(p in rc)
        if K <= 64:
            add("registers (K<=64)", cnt)
            if m == 64:
                add("registers m=64", cnt)
            continue
        cached = S <= OTF_ROW
        add("prev's row cached (S<=256)" if cached else "prev's row not cached (S>=257)", cnt)
        walk_cur = (cached and K <= 8 * S) or K <= S
        add("walks cur's row" if walk_cur else "walks prev's row", cnt)
        if walk_cur and cached:
            stride = None                   # nothing staged: prev's row is searched in its LDS copy
        else:
            n = S if walk_cur else K
            stride = -(-n // STAGE_CAP)
            add("stride %d" % stride, cnt)
        add("m<=64" if m <= 64 else "m 65-127" if m < SPEC_CAP else "m=128" if m == SPEC_CAP else
            "m>128, table in LDS (K<=256)" if K <= OTF_LDS_SLOTS else "m>128, table in scratch (K>256)", cnt)
    return out


REACH_BUCKETS = (
    ["K=%d" % K for K in (64, 65, 255, 256, 257, 384, 385, 512, 513, 1024, 1025)] +
    ["registers (K<=64)", "registers m=64", "m<=64", "m 65-127", "m=128", "m>128, table in LDS (K<=256)", "m>128, table in scratch (K>256)",
     "prev's row cached (S<=256)", "prev's row not cached (S>=257)", "walks cur's row", "walks prev's row",
     "stride 1", "stride 2", "stride 3",
     "general: registers (K<=64)", "general: table in LDS", "general: table in scratch", "general K=256", "general K=257"])


def builder_reach(cg):
    """The edge-table builder's windows over ALL tables of the graph: {bucket: number of tables}."""
    deg = np.diff(cg.row_ptr)
    kd = deg[cg.col]                       # table (src -> dst) has deg(dst) slots
    ks = np.repeat(deg, deg)               # and searches row(src), staged in LDS up to ROW_CACHE entries
    out = {"table K=%d" % K: int((kd == K).sum()) for K in (BUILDER_LDS_SLOTS, BUILDER_LDS_SLOTS + 1)}
    if not cg.directed:
        for S in (ROW_CACHE, ROW_CACHE + 1):
            out["source row S=%d" % S] = int((ks == S).sum())
    return out


# ---- Vose's pairing as the wave builder streams it (wave_pair) -----------------------------------------------------
PAIR_EVENTS = ("demotion on the last buffered small", "run continues across a reload of smaller", "reload of larger",
               "carried large demoted again at once", "dry with a large in hand", "carried large left at the end",
               "unpopped smalls, table <= 512", "unpopped smalls, table > 512", "unpopped larges")


def replay_pairing(weights):
    """alias_setup (src/node2vec.py:240-269) of the row `weights` (normalised by their left-to-right sum), replayed the
    way wave_pair streams the two stacks: 64 entries at a time, the pushed-back large carried in registers.  Returns
    (J, q, ns, nl, events) — events: {name in PAIR_EVENTS: count}.  Plain Python floats: the reference's roundings."""
    K = len(weights)
    norm = 0.0
    for x in weights:
        norm = norm + float(x)
    q = [float(K) * (float(x) / norm) for x in weights]
    J = [0] * K
    smaller = [k for k in range(K) if q[k] < 1.0]          # pop order: from the end
    larger = [k for k in range(K) if not (q[k] < 1.0)]
    ns, nl = len(smaller), len(larger)
    ev = {name: 0 for name in PAIR_EVENTS}
    mem_s, mem_l = ns, nl
    sbuf, lbuf = [], []
    s_pos = l_pos = 0
    carried, cs_i, cs_q = False, 0, 0.0
    l_loads = 0
    while True:
        if l_pos == len(lbuf):
            if mem_l == 0:
                break
            cnt = min(64, mem_l)
            lbuf = [larger[mem_l - 1 - i] for i in range(cnt)]
            mem_l -= cnt
            l_pos = 0
            l_loads += 1
            if l_loads > 1:
                ev["reload of larger"] += 1
        large = lbuf[l_pos]
        ql = q[large]
        l_pos += 1
        if carried:
            J[cs_i], q[cs_i] = large, cs_q
            carried = False
            ql = ql + cs_q
            ql = ql - 1.0
            if ql < 1.0:
                ev["carried large demoted again at once"] += 1
                carried, cs_i, cs_q = True, large, ql
                continue
        dry = False
        first_chain = True
        while True:
            if s_pos == len(sbuf):
                if mem_s == 0:
                    dry = True
                    break
                cnt = min(64, mem_s)
                sbuf = [smaller[mem_s - 1 - i] for i in range(cnt)]
                mem_s -= cnt
                s_pos = 0
                if not first_chain:
                    ev["run continues across a reload of smaller"] += 1
            first_chain = False
            demoted = False
            while True:
                small = sbuf[s_pos]
                ql = ql + q[small]
                ql = ql - 1.0
                J[small] = large
                s_pos += 1
                if ql < 1.0:
                    demoted = True
                    break
                if s_pos >= len(sbuf):
                    break
            if demoted:
                if s_pos == len(sbuf):
                    ev["demotion on the last buffered small"] += 1
                carried, cs_i, cs_q = True, large, ql
                break
        if dry:
            ev["dry with a large in hand"] += 1
            q[large], J[large] = ql, 0
            break
    if carried:
        ev["carried large left at the end"] += 1
        q[cs_i], J[cs_i] = cs_q, 0
    if s_pos < len(sbuf) or mem_s > 0:
        ev["unpopped smalls, table <= 512" if K <= BUILDER_LDS_SLOTS else "unpopped smalls, table > 512"] += 1
    if l_pos < len(lbuf) or mem_l > 0:
        ev["unpopped larges"] += 1
    return np.array(J, dtype=np.int64), np.array(q, dtype=np.float64), ns, nl, ev


# ---------------------------------------------------------------------------------------------------- oracle helpers
def buffer_offsets(lens):
    """Where each walk's uniforms start in a buffer consumed sequentially (the oracle's "buffer" mode): a walk of `len`
    nodes drew 2 (len - 1) of them."""
    used = 2 * (np.asarray(lens, dtype=np.int64) - 1)
    return np.concatenate([[0], np.cumsum(used)[:-1]]).astype(np.int64)


def lanes_rounds(n_starts, max_waves):
    """The fewest rounds at which a launch of the budgeted walk runs the lane-per-walk kernel (launch_otf)."""
    return -(-(int(max_waves) * 32) // int(n_starts))


# ---------------------------------------------------------------------------------------------------- scenarios
@functools.lru_cache(maxsize=None)
def graph(case, kind="plain"):
    """(CsrGraph, info) of a case, built once per process; nobody changes it."""
    return {"A": case_a, "C": case_c, "D": case_d}[case]() if case != "B" else case_b(kind)


# (id, case, kind, p, q, rounds, walk length): what both test modules walk.  A: every (p, q) of the issue — (4, 0.25)
# makes the common-neighbour class `smaller` with q ~ 0.5, so half the draws run the sweep; 0.3 / 0.7 are not dyadic
# (left-to-right sum over the runs); 2^-10 / 2^20 are the last dyadic values the launcher accepts, 2^-11 / 2^21 the
# first it does not.  D: p = q = 1 makes the tables alias_setup of the crafted rows, (0.5, 2) their classified form.
SCENARIOS = (
    [("A p=%g q=%g" % pq, "A", "plain") + pq + (2, 20) for pq in A_PQ] +
    [("B plain", "B", "plain", 0.25, 4.0, 2, 20), ("B weighted", "B", "weighted", 0.5, 2.0, 2, 20),
     ("B directed", "B", "directed", 2.0, 0.5, 2, 20), ("C", "C", "plain", 0.25, 4.0, 20, 30),
     ("D p=q=1", "D", "plain", 1.0, 1.0, 3, 20), ("D p=0.5 q=2", "D", "plain", 0.5, 2.0, 3, 20)])
SCENARIO_IDS = [s[0] for s in SCENARIOS]
SEED = 0x5EED0E
