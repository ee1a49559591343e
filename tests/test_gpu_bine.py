"""GPU parity tests of the BiNE path (include/n2v_bine.h) against oracle/bine_oracle.py.

Bit-exact: walk lengths, walks, negative pools (all integer work, Philox-driven).  fp64 rounding: HITS
scores, initial rows, and the sequential training mode against the numpy restatement of
src/bine_train.py:243-309,452-504 (tolerance 1e-9 relative: numpy's BLAS dot and the wave butterfly sum in a
different order; exp/log differ by <= 1 ulp).  Multi-wave parallel runs are checked against the sequential mode
through their loss trajectories; every training kernel variant, the parallel ones included, is pinned to the
restatement by tests/test_gpu_bine_exact.py.  The reference's own BiNE code cannot run (oracle header): parity unpinned at
the bit level, closed statistically by tests/test_bine_host.py."""
import numpy as np
import pytest

from oracle import bine_oracle as bo

pytestmark = pytest.mark.gpu


def make_graph(seed=3, n_u=300, n_v=120, per_user=6, labels=True):
    from n2v_hip import bine
    rs = np.random.RandomState(seed)
    users = np.repeat(np.arange(n_u), per_user)
    # skewed item popularity so that hubs and multiplicities > 1 occur
    items = np.minimum((n_v * rs.random_sample(users.shape[0]) ** 2.5).astype(np.int64), n_v - 1)
    ratings = rs.randint(1, 6, size=users.shape[0]).astype(float)
    if labels:
        return bine.BipartiteGraph(["u%d" % u for u in users], ["i%d" % i for i in items], ratings)
    return bine.BipartiteGraph(users, items, ratings)


@pytest.fixture(scope="module")
def eng():
    from n2v_hip import bine
    g = make_graph()
    e = bine.BineEngine(g, device="cuda:0", seed=2024)
    e.calculate_centrality()
    e.generate_walks(percentage=0.15, maxT=8, minT=1)
    e.build_negative_pools(pool_size=24, max_jaccard=0.1)
    e.build_occurrences()
    return e


def test_hits_matches_networkx111_restatement(eng):
    g = eng.g
    a, iters = bo.hits_nx111(g.row_ptr, g.col, g.w)
    got = eng.authority.cpu().numpy()
    assert eng.hits_iterations == iters
    assert np.allclose(got, a, rtol=1e-10, atol=1e-14)
    for lo, hi in ((0, g.n_u), (g.n_u, g.n)):
        counts, auth = bo.walk_counts(a, lo, hi, 8, 1)
        dev = eng.counts[lo:hi].cpu().numpy()
        safe = np.abs(8 * auth - np.round(8 * auth)) > 1e-9     # away from a ceil() boundary
        assert np.array_equal(dev[safe], counts[safe])
        assert np.allclose(eng.auth_scaled[lo:hi].cpu().numpy(), auth, rtol=1e-9, atol=1e-12)


def test_walks_bit_exact(eng):
    from n2v_hip import bine
    g = eng.g
    cum2 = bo.two_hop_prefix(g.row_ptr, g.col)
    assert np.array_equal(eng.cum2.cpu().numpy(), cum2)
    off = eng.walk_off.cpu().numpy()
    tok = eng.tokens.cpu().numpy()
    node = eng.walk_node.cpu().numpy()
    counts = eng.counts.cpu().numpy()
    assert np.array_equal(node, np.repeat(np.arange(g.n), counts))
    nw_u, nw_v = eng.n_walks
    assert nw_u == counts[: g.n_u].sum() and nw_v == counts[g.n_u:].sum()
    rs = np.random.RandomState(0)
    check = np.concatenate([np.arange(40), rs.randint(0, nw_u + nw_v, 400), np.arange(nw_u - 20, nw_u + 20)])
    lens_seen = []
    for i in check:
        side_seed = bine.derive_seed(2024, bine.SEED_WALK_U if i < nw_u else bine.SEED_WALK_V)
        gw = i if i < nw_u else i - nw_u
        L = bo.walk_length(g.row_ptr, cum2, node[i], gw, 0.15, bine.MAX_WALK_LEN, side_seed)
        assert off[i + 1] - off[i] == L
        assert tok[off[i]:off[i + 1]].tolist() == bo.device_walk(g.row_ptr, g.col, cum2, node[i], gw, L, side_seed)
        lens_seen.append(L)
    assert max(lens_seen) > 10
    # every step moves to a different vertex of the same side that shares a neighbour
    tw = eng.tok_walk.cpu().numpy()
    assert np.array_equal(tw, np.repeat(np.arange(nw_u + nw_v), np.diff(off)))
    for i in check[:100]:
        w = tok[off[i]:off[i + 1]]
        for x, y in zip(w[:-1], w[1:]):
            assert x != y and (x < g.n_u) == (y < g.n_u)
            assert set(g.col[g.row_ptr[x]:g.row_ptr[x + 1]]) & set(g.col[g.row_ptr[y]:g.row_ptr[y + 1]])


def test_walk_lengths_geometric_full_population(eng):
    lens = np.diff(eng.walk_off.cpu().numpy())
    # dead-end starts aside, P(len = k) = 0.15 * 0.85^(k-1): compare the mean (1/0.15) within 5 %
    assert abs(lens.mean() - 1 / 0.15) < 0.35


def test_negative_pools_bit_exact(eng):
    from n2v_hip import bine
    g = eng.g
    pool = eng.pool.cpu().numpy()
    for v in [0, 1, 17, g.n_u - 1, g.n_u, g.n_u + 3, g.n - 1]:
        lo, hi, k = (0, g.n_u, bine.SEED_POOL_U) if v < g.n_u else (g.n_u, g.n, bine.SEED_POOL_V)
        want = bo.neg_pool(g.row_ptr, g.col, lo, hi, v, 24, 0.1, bine.derive_seed(2024, k))
        assert pool[v].tolist() == want
    assert ((pool[: g.n_u] < g.n_u).all() and (pool[g.n_u:] >= g.n_u).all())
    assert (pool != np.arange(g.n)[:, None]).all()


def test_init_rows(eng):
    from n2v_hip import bine
    eng.init_embeddings(d=20)
    emb, ctx = eng.emb.cpu().numpy(), eng.ctx.cpu().numpy()
    assert emb.shape[1] == 64 and (emb[:, 20:] == 0).all() and (ctx[:, 20:] == 0).all()
    e0, c0 = bo.init_rows(12, 20, bine.derive_seed(2024, bine.SEED_INIT))
    assert np.allclose(emb[:12, :20], e0, rtol=1e-14, atol=0)
    assert np.allclose(ctx[:12, :20], c0, rtol=1e-14, atol=0)
    assert np.allclose((emb ** 2).sum(1), 1.0, rtol=1e-14)


@pytest.mark.parametrize("d,ns", [(16, 4), (100, 4), (200, 6)])
def test_sequential_training_matches_numpy_restatement(d, ns):
    from n2v_hip import bine
    g = make_graph(seed=5, n_u=40, n_v=25, per_user=4)
    e = bine.BineEngine(g, device="cuda:0", seed=7)
    e.calculate_centrality()
    e.generate_walks(maxT=4)
    e.build_negative_pools(pool_size=12, max_jaccard=0.2)
    e.build_occurrences()
    e.init_embeddings(d=d)
    emb = e.emb[:, :d].cpu().numpy().copy()
    ctx = e.ctx[:, :d].cpu().numpy().copy()
    iters = 3
    lam, losses = bo.train(g.edge_u, g.edge_v, g.edge_w, emb, ctx, e.occ_ptr.cpu().numpy(), e.occ_pos.cpu().numpy(),
                           e.tokens.cpu().numpy(), e.tok_walk.cpu().numpy(), e.walk_off.cpu().numpy(),
                           e.pool.cpu().numpy(), 5, ns, 0.01, 0.01, 0.1, 0.01, iters,
                           bine.derive_seed(7, bine.SEED_OCC), bine.derive_seed(7, bine.SEED_NEG))
    got = e.train(max_iter=iters, ws=5, ns=ns, mode="sequential")
    assert np.allclose(got, losses, rtol=1e-9)
    assert e.lam == pytest.approx(lam, rel=1e-15)
    assert np.allclose(e.emb[:, :d].cpu().numpy(), emb, rtol=1e-9, atol=1e-12)
    assert np.allclose(e.ctx[:, :d].cpu().numpy(), ctx, rtol=1e-9, atol=1e-12)
    assert (e.emb[:, d:] == 0).all() and (e.ctx[:, d:] == 0).all()


@pytest.mark.parametrize("pmode", ["atomic", "store"])
def test_parallel_mode_tracks_sequential_mode(eng, pmode):
    """Hogwild ordering changes which update sees which, not what is computed: after the same number of
    iterations the losses of the two modes agree closely and the embeddings stay close."""
    eng.init_embeddings(d=32)
    e0, c0 = eng.emb.clone(), eng.ctx.clone()
    seq = eng.train(max_iter=4, mode="sequential")
    es = eng.emb.clone()
    eng.emb.copy_(e0)
    eng.ctx.copy_(c0)
    par = eng.train(max_iter=4, mode=pmode)
    assert np.allclose(seq, par, rtol=2e-3 if pmode == "atomic" else 1e-2)
    assert eng.lam > 0
    rel = ((eng.emb - es).norm() / (es - e0).norm()).item()
    assert rel < (0.2 if pmode == "atomic" else 0.35), rel
    # deterministic sampling: a second parallel run processes the same occurrences (loss differs only by
    # update order)
    eng.emb.copy_(e0)
    eng.ctx.copy_(c0)
    par2 = eng.train(max_iter=4, mode=pmode)
    assert np.allclose(par, par2, rtol=2e-3 if pmode == "atomic" else 1e-2)


def test_vectors_accessor_and_walk_lists(eng):
    eng.init_embeddings(d=32)
    vu, vv = eng.vectors("u"), eng.vectors("v")
    assert vu.shape == (eng.g.n_u, 32) and vv.shape == (eng.g.n_v, 32)
    wl = eng.walks_as_lists("v")
    assert len(wl) == eng.n_walks[1] and all(str(x).startswith("i") for x in wl[0])


def test_replica_merge_matches_single_table_run():
    """Multi-GPU scheme (BineEngine.train_sharded) with the replicas simulated in one process: two engines with
    identical state pass over the two halves of the rating list, the sum of their changes is applied to both —
    the loss trajectory follows the single-table run."""
    from n2v_hip import bine
    g = make_graph(seed=11, n_u=400, n_v=150, per_user=6)

    def fresh():
        e = bine.BineEngine(g, device="cuda:0", seed=5)
        e.calculate_centrality()
        e.generate_walks(maxT=6)
        e.build_negative_pools(pool_size=16, max_jaccard=0.1)
        e.build_occurrences()
        e.init_embeddings(d=48)
        return e

    single = fresh()
    want = single.train(max_iter=5, mode="atomic")
    reps = [fresh(), fresh()]
    assert torch_equal(reps[0].emb, reps[1].emb) and torch_equal(reps[0].tokens, single.tokens)
    half = g.n_ratings // 2
    ranges = [(0, half), (half, g.n_ratings)]
    for r in reps:
        r.reset_schedule(0.01)
    bases = [reps[0].emb.clone(), reps[0].ctx.clone()]
    got = []
    for it in range(5):
        for r, rg in zip(reps, ranges):
            r.train_pass(it, mode="atomic", e_range=rg)
        for k, name in enumerate(("emb", "ctx")):
            total = bases[k] + sum(getattr(r, name) - bases[k] for r in reps)
            for r in reps:
                getattr(r, name).copy_(total)
            bases[k] = total.clone()
        loss = sum(r.state[1] for r in reps)
        for r in reps:
            r.state[1] = loss
            got.append(r.finish_iteration()[0])
    assert np.allclose(got[0::2], got[1::2], rtol=0, atol=0)        # replicas stay in lockstep
    assert np.allclose(got[0::2], want, rtol=5e-3)
    assert reps[0].state[0].item() == single.state[0].item()       # same learning-rate decisions


def torch_equal(a, b):
    import torch
    return bool(torch.equal(a, b))


def test_two_rank_probe_over_gloo(tmp_path):
    """Two ranks of tools/bine_probe.py under torch.distributed.run sharing the one GPU (merges over gloo through
    host memory — the rehearsal path of n2v_hip.dist; on a multi-GPU node the same code runs over RCCL)."""
    import json
    import os
    import subprocess
    import sys
    from helpers import ROOT
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    port = 29300 + os.getpid() % 300
    base = [os.path.join(ROOT, "tools", "bine_probe.py"), "--users", "3000", "--items", "2000", "--ratings", "60000",
            "--dim", "64", "--iters", "4", "--maxT", "8", "--pool", "32", "--mode", "atomic"]
    one = subprocess.run([sys.executable] + base, capture_output=True, text=True, timeout=600, env=env)
    assert one.returncode == 0, one.stderr[-3000:]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port)] + base + ["--backend", "gloo"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert two.returncode == 0, two.stderr[-3000:]
    j1 = json.loads(one.stdout.strip().splitlines()[-1])
    j2 = json.loads(two.stdout.strip().splitlines()[-1])
    assert j2["n_gpus"] == 2 and j1["walks"] == j2["walks"]
    # 1e-2: LSH clusters share one pool (src/bine_lsh.py:49-51), so negatives collide across the two shards more often than
    # independent pools did (0.5 % apart on this graph)
    assert np.allclose(j1["train"]["losses"], j2["train"]["losses"], rtol=1e-2)
    # the overlapped merge (the other rank's changes arrive one pass late): same walks, a loss curve close to the
    # synchronous one on this graph — the pass's own loss is reduced at once, only the tables lag
    port2 = 29600 + os.getpid() % 300
    three = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", str(port2)] + base +
                           ["--backend", "gloo", "--overlap-merge"], capture_output=True, text=True, timeout=600, env=env)
    assert three.returncode == 0, three.stderr[-3000:]
    j3 = json.loads(three.stdout.strip().splitlines()[-1])
    assert j3["n_gpus"] == 2 and j3["walks"] == j1["walks"]
    print("BiNE losses 1 GPU %s | 2 ranks sync %s | 2 ranks overlapped %s" % (j1["train"]["losses"], j2["train"]["losses"], j3["train"]["losses"]))
    assert np.allclose(j1["train"]["losses"], j3["train"]["losses"], rtol=2e-2)


def test_drop_in_train_flow(tmp_path):
    """The reference's call sequence (src/bine_train.py:600-612): GraphUtils -> construct_training_graph ->
    train(args, gul); vectors_u.dat / vectors_v.dat in its text format; top_N on held-out ratings."""
    import bine_train as bt
    rs = np.random.RandomState(1)
    lines, test_rate = [], {}
    for u in range(120):
        # popularity-skewed choices: one connected graph with a clear HITS spectral gap
        liked = np.unique(np.minimum((80 * rs.random_sample(10) ** 2).astype(np.int64), 79))
        for k, i in enumerate(liked):
            if k == 0 and len(liked) > 3:
                test_rate.setdefault("u%d" % u, {})["i%d" % i] = 5.0      # held out
            else:
                lines.append("u%d\ti%d\t%d\n" % (u, i, rs.randint(3, 6)))
    f = tmp_path / "ratings_train.dat"
    f.write_text("".join(lines))
    gul = bt.GraphUtils(str(tmp_path), device="cuda:0", seed=3)
    gul.construct_training_graph(str(f))
    items = sorted({i for d in test_rate.values() for i in d} & set(gul.node_v))
    test_rate = {u: {i: r for i, r in d.items() if i in items} for u, d in test_rate.items()}
    test_rate = {u: d for u, d in test_rate.items() if d and u in set(gul.node_u)}
    args = bt.default_args(d=32, max_iter=30, maxT=8, model_path=str(tmp_path), save=True,
                           test_rates=(list(test_rate), items, test_rate))
    node_list_u, roc, ap = bt.train(args, gul)
    assert (roc, ap) == (0, 0) and len(node_list_u) == len(gul.node_u)
    assert node_list_u["u7"]["embedding_vectors"].shape == (1, 32)
    rows = (tmp_path / "vectors_u.dat").read_text().splitlines()
    assert len(rows) == len(gul.node_u) and rows[0].split()[0] == gul.node_u[0] and len(rows[0].split()) == 33
    assert np.allclose([float(x) for x in rows[0].split()[1:]], node_list_u[gul.node_u[0]]["embedding_vectors"][0])
    assert len((tmp_path / "vectors_v.dat").read_text().splitlines()) == len(gul.node_v)
    f1, m_ap, mrr, ndcg = bt.train.last["metrics"]
    assert 0 <= f1 <= 1 and 0 <= m_ap <= 1 and 0 <= mrr <= 1 and 0 <= ndcg <= 1
    assert len(bt.train.last["losses"]) >= 1 and gul.authority_u and len(gul.walks_u) == gul.engine.n_walks[0]
    assert gul.edge_list[0] == ("u0", lines[0].split("\t")[1], float(lines[0].split("\t")[2]))


def test_hits_raises_like_networkx_when_it_does_not_converge():
    """networkx 1.11 raises after max_iter power iterations; two equal disconnected halves never separate."""
    from n2v_hip import bine
    users = ["u%d" % (k // 2) for k in range(40)]
    items = ["i%d" % (2 * (k // 20) + k % 2) for k in range(40)]      # users 0-9 on items 0/1, users 10-19 on items 2/3
    w = [1.0 + (k // 20) * 1e-9 for k in range(40)]
    e = bine.BineEngine(bine.BipartiteGraph(users, items, w), device="cuda:0")
    with pytest.raises(bine.BineConvergenceError):
        e.calculate_centrality(max_iter=5, tol=1e-30)


def test_config5_size_properties():
    """BASELINE config 5's shape at full size (500k users, 500k items, 2e7 ratings, d = 256) through properties
    that do not need the oracle: walk counts follow the authority rule, every walk starts at its vertex, stays on
    its side and moves between vertices that share a neighbour, lengths are geometric, pools avoid the vertex
    itself, the occurrence index is a permutation grouped by vertex, and the two parallel training variants agree."""
    import torch
    from scipy import stats
    from n2v_hip import bine, synth
    u, i, r = synth.bipartite_powerlaw_ratings(500_000, 500_000, 20_000_000)
    g = bine.BipartiteGraph(u, i, r)
    e = bine.BineEngine(g, device="cuda:0", seed=42)
    e.calculate_centrality()
    e.generate_walks(0.15, 32, 1)
    auth, counts = e.auth_scaled, e.counts.long()
    want = torch.clamp(torch.ceil(32 * auth), min=1).long()
    assert (auth.min() == 0) and (auth[: g.n_u].max() == 1) and (auth[g.n_u:].max() == 1)
    assert torch.equal(counts, want)
    off, tok, node = e.walk_off, e.tokens.long(), e.walk_node.long()
    assert torch.equal(tok[off[:-1]], node)
    lens = (off[1:] - off[:-1])
    side_tok = tok >= g.n_u
    assert torch.equal(side_tok, side_tok[off[:-1]][e.tok_walk.long()])            # a walk never changes side
    inner = torch.ones_like(tok, dtype=torch.bool)
    inner[off[1:-1]] = False
    inner[0] = False                                                                # positions that have a predecessor
    assert (tok[1:][inner[1:]] != tok[:-1][inner[1:]]).all()                        # never stays put
    # geometric lengths: P(len = k) = 0.15 * 0.85^(k-1) over the walks whose start is not a dead end
    deg2 = (e.cum2[e.row_ptr[1:]] - e.cum2[e.row_ptr[:-1]]) - (e.row_ptr[1:] - e.row_ptr[:-1])
    live = (deg2[node] > 0)
    ll = lens[live].cpu().numpy()
    assert (lens[~live] == 1).all()
    ks = np.arange(1, 40)
    obs = np.array([(ll == k).sum() for k in ks], dtype=np.float64)
    exp = len(ll) * 0.15 * 0.85 ** (ks - 1)
    assert stats.chi2.sf(((obs - exp) ** 2 / exp).sum(), len(ks) - 1) > 1e-4
    # sampled steps connect vertices with a common neighbour
    rs = np.random.RandomState(0)
    pos = np.nonzero(inner.cpu().numpy())[0]
    tk = tok.cpu().numpy()
    for p in rs.choice(pos, 3000, replace=False):
        a, b = int(tk[p - 1]), int(tk[p])
        ra, rb = g.col[g.row_ptr[a]:g.row_ptr[a + 1]], g.col[g.row_ptr[b]:g.row_ptr[b + 1]]
        assert np.intersect1d(ra, rb, assume_unique=True).size > 0, (a, b)
    e.build_negative_pools(200)
    pool = e.pool.long()
    ids = torch.arange(g.n, device=pool.device)[:, None]
    assert (pool != ids).all() and ((pool >= g.n_u) == (ids >= g.n_u)).all()
    e.build_occurrences()
    assert torch.equal(torch.sort(e.occ_pos).values, torch.arange(tok.numel(), device=tok.device))
    grouped = tok[e.occ_pos]
    assert (grouped[1:] >= grouped[:-1]).all()
    assert torch.equal(e.occ_ptr[1:] - e.occ_ptr[:-1], torch.bincount(tok, minlength=g.n))
    e.init_embeddings(256)
    e0, c0 = e.emb.clone(), e.ctx.clone()
    a = e.train(max_iter=2, mode="atomic")
    e.emb.copy_(e0)
    e.ctx.copy_(c0)
    b = e.train(max_iter=2, mode="store")
    assert e.mode_used == "store" and np.allclose(a, b, rtol=1e-3)
    assert torch.isfinite(e.emb).all() and torch.isfinite(e.ctx).all() and (e.emb[:, 256:].numel() == 0)


def test_add_user_edges_changes_only_the_hits_input(tmp_path):
    """main()'s second stage (src/bine_train.py:614-622): similarity edges between users join the graph hits()
    sees; authority scores equal the networkx-1.11 restatement on that augmented graph; walks still move on the
    bipartite projections."""
    import bine_train as bt
    from n2v_hip import bine
    g = make_graph(seed=9, n_u=150, n_v=60, per_user=5)
    gul = bt.GraphUtils(str(tmp_path), device="cuda:0", seed=4)
    gul.graph = g
    gul.engine = bine.BineEngine(g, device="cuda:0", seed=4)
    args = bt.default_args(d=16, max_iter=3, maxT=4, user_edges_mode="ratio", user_edges_ratio=0.05)
    bt.run(args, gul)
    eng = gul.engine
    n_added = bt.train.last["user_edges_added"]
    k = int(g.n_u * 0.05)
    assert 0 < n_added <= g.n_u * k and "first_stage" in bt.train.last
    rp, col, w = (t.cpu().numpy() for t in eng.hits_csr)
    assert len(col) == len(g.col) + 2 * n_added - int(((np.repeat(np.arange(g.n), np.diff(rp)) == col)).sum())
    uu = (np.repeat(np.arange(g.n), np.diff(rp)) < g.n_u) & (col < g.n_u)
    assert uu.sum() > 0 and (w[uu] == 1.0).all()
    a, iters = bo.hits_nx111(rp, col, w)
    assert eng.hits_iterations == iters and np.allclose(eng.authority.cpu().numpy(), a, rtol=1e-10, atol=1e-14)
    a0, _ = bo.hits_nx111(g.row_ptr, g.col, g.w)
    assert not np.allclose(a[: g.n_u] / a[: g.n_u].max(), a0[: g.n_u] / a0[: g.n_u].max(), atol=1e-3)
    tok = eng.tokens.cpu().numpy()
    off = eng.walk_off.cpu().numpy()
    for i in range(0, eng.n_walks[0], 7):          # user walks: every step shares an ITEM
        wlk = tok[off[i]:off[i + 1]]
        for x, y in zip(wlk[:-1], wlk[1:]):
            assert set(g.col[g.row_ptr[x]:g.row_ptr[x + 1]]) & set(g.col[g.row_ptr[y]:g.row_ptr[y + 1]])
    # the other similarities of src/bine_train.py:55-71 run on the same kernels; an unknown one is refused
    n_p = bt.add_user_edge(args, gul, sim_method="pearson")
    assert 0 < n_p <= g.n_u * k
    with pytest.raises(ValueError):
        bt.add_user_edge(args, gul, sim_method="manhattan")
