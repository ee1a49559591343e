"""GPU tests: every instantiation of bine_train_kernel against the float64 restatement of oracle/bine_oracle.py.

n2v_bine_train_pass dispatches to 24 kernels: VPL 1/2/4/8 (row stride 64..512) x NT 5/8 (ns <= 4 or 5..7) x mode
SEQUENTIAL / PARALLEL / PARALLEL_STORE.  The eight (d, ns) cases below cover the eight (VPL, NT) pairs, and each
case runs in all three modes against one restatement run:

  * SEQUENTIAL: the whole pass on one wavefront, the reference's update order by construction;
  * PARALLEL and PARALLEL_STORE, deterministic by construction: the pass is launched one rating at a time, or one
    16-rating range at a time.  Ratings are handed out in chunks of kChunk = 16 through the counter in state[6]
    (zeroed before every launch, as the header requires), so such a range is taken whole by one wavefront and the
    parallel code paths (agent-scope loads, the prefetch of the next context row, the LDS parking of context rows and
    their (final - loaded) commits, whole-row stores, the user row carried across a chunk) must reproduce the
    sequential update order.

Tolerances are those of tests/test_gpu_bine.py's sequential test: rows at rtol 1e-9 / atol 1e-12 (numpy's dot and
the wave butterfly sum in another order; exp/log within an ulp; (final - loaded) + loaded rounds once more), losses at
rtol 1e-9, the learning rate at rel 1e-15.  state[5] counts the rows the reference's access pattern moves: an exact
integer that pins the number of targets of every skip_gram call.  Each case also asserts that the edge it exists for
occurred in the restatement's data.  Multi-wave parallel runs are covered by the trajectory tests of
tests/test_gpu_bine.py."""
import numpy as np
import pytest

from oracle import bine_oracle as bo

pytestmark = pytest.mark.gpu

ALPHA, BETA, GAMMA, LAM = 0.01, 0.01, 0.1, 0.01
ITERS = 2
KCHUNK = 16

# (d, ns, data): `data` sets ws, the walks (percentage, maxT, minT) and the Jaccard pool size; `edge` is the
# restatement counter that must be non-zero for the case to prove anything
CASES = [
    (16, 4, dict(), "capped"),                                            # VPL 1, NT 5; > 10 occurrences
    (64, 7, dict(pool_size=3), "negs_cut"),                               # VPL 1, NT 8; pool_size < ns
    (100, 0, dict(minT=0, percentage=0.5), "empty"),                      # VPL 2, NT 5; ns = 0, minT = 0
    (128, 5, dict(ws=31, percentage=0.02, maxT=2), "window63"),           # VPL 2, NT 8; a 63-token window
    (256, 4, dict(), "repeat_context"),                                   # VPL 4, NT 5 (BASELINE config 5); z c z
    (200, 7, dict(), "neg_in_window"),                                    # VPL 4, NT 8; negatives in the window
    (300, 4, dict(ws=31, percentage=0.02, maxT=2), "window63"),           # VPL 8, NT 5
    (512, 7, dict(ws=31, percentage=0.02, maxT=2), "window63"),           # VPL 8, NT 8
]
CASE_IDS = ["d%d-ns%d" % (d, ns) for d, ns, _, _ in CASES]
# (mode, span): span None = one whole sequential pass, else launches of `span` ratings
RUNS = [("sequential", None), ("atomic", 1), ("atomic", KCHUNK), ("store", 1), ("store", KCHUNK)]
RUN_IDS = ["sequential", "atomic-1", "atomic-16", "store-1", "store-16"]


def seeds(e):
    from n2v_hip import bine
    return bine.derive_seed(e.seed, bine.SEED_OCC), bine.derive_seed(e.seed, bine.SEED_NEG)


def restate(e, emb0, ctx0, ws, ns, iters, e_range=None):
    """The restatement on the engine's own walks, occurrences and pools, from the rows emb0 / ctx0 (torch, padded)."""
    d = e.dim
    emb = emb0[:, :d].cpu().numpy().copy()
    ctx = ctx0[:, :d].cpu().numpy().copy()
    g = e.g
    e0, e1 = e_range if e_range is not None else (0, g.n_ratings)
    first = g.first[e0:e1] if e_range is not None else None
    stats = {}
    so, sn = seeds(e)
    lam, losses = bo.train(g.edge_u[e0:e1], g.edge_v[e0:e1], g.edge_w[e0:e1], emb, ctx, e.occ_ptr.cpu().numpy(),
                           e.occ_pos.cpu().numpy(), e.tokens.cpu().numpy(), e.tok_walk.cpu().numpy(),
                           e.walk_off.cpu().numpy(), e.pool.cpu().numpy(), ws, ns, ALPHA, BETA, GAMMA, LAM, iters, so, sn,
                           first=first, stats=stats)
    return dict(emb=emb, ctx=ctx, lam=lam, losses=losses, stats=stats)


def run_device(e, emb0, ctx0, ws, ns, n_iters, mode, span, e_range=None):
    """Runs n_iters passes from emb0 / ctx0.  span None: e.train (one launch per pass); else launches of `span`
    ratings, each with the work counter zeroed.  Returns (losses, lam, state[5])."""
    e.emb.copy_(emb0)
    e.ctx.copy_(ctx0)
    if span is None:
        losses = e.train(max_iter=n_iters, alpha=ALPHA, beta=BETA, gamma=GAMMA, lam=LAM, ws=ws, ns=ns, mode=mode,
                         e_range=e_range)
    else:
        e.reset_schedule(LAM)
        lo, hi = e_range if e_range is not None else (0, e.g.n_ratings)
        for it in range(n_iters):
            for a in range(lo, hi, span):
                e.state[6] = 0.0
                e.train_pass(it, ALPHA, BETA, GAMMA, ws, ns, mode, e_range=(a, min(a + span, hi)))
            e.finish_iteration()
        losses = e.losses
    return list(losses), float(e.state[0].item()), float(e.state[5].item())


def check(e, want, got):
    losses, lam, rows_ref = got
    d = e.dim
    emb, ctx = e.emb.cpu().numpy(), e.ctx.cpu().numpy()
    assert len(losses) == len(want["losses"])
    np.testing.assert_allclose(losses, want["losses"], rtol=1e-9, atol=0)
    assert lam == pytest.approx(want["lam"], rel=1e-15)
    np.testing.assert_allclose(emb[:, :d], want["emb"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(ctx[:, :d], want["ctx"], rtol=1e-9, atol=1e-12)
    assert (emb[:, d:] == 0).all() and (ctx[:, d:] == 0).all(), "padding columns moved"
    assert rows_ref == want["stats"]["rows_ref"]


_prepared = {}


def prepared(k):
    """Engine, starting rows and restatement of CASES[k], built once per module."""
    if k not in _prepared:
        from n2v_hip import bine
        from test_gpu_bine import make_graph
        d, ns, data, _ = CASES[k]
        g = make_graph(seed=5, n_u=40, n_v=25, per_user=4)
        e = bine.BineEngine(g, device="cuda:0", seed=7)
        e.calculate_centrality()
        e.generate_walks(percentage=data.get("percentage", 0.15), maxT=data.get("maxT", 4), minT=data.get("minT", 1))
        e.build_negative_pools(pool_size=data.get("pool_size", 12), max_jaccard=0.2)
        e.build_occurrences()
        e.init_embeddings(d=d)
        emb0, ctx0 = e.emb.clone(), e.ctx.clone()
        ws = data.get("ws", 5)
        want = restate(e, emb0, ctx0, ws, ns, ITERS)
        _prepared[k] = (e, emb0, ctx0, ws, ns, want)
    return _prepared[k]


def test_cases_cover_every_instantiation():
    pairs = {(next(s for s in (64, 128, 256, 512) if s >= d) // 64, 5 if ns <= 4 else 8) for d, ns, _, _ in CASES}
    assert pairs == {(v, t) for v in (1, 2, 4, 8) for t in (5, 8)}
    assert {m for m, _ in RUNS} == {"sequential", "atomic", "store"}


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_case_exercises_its_edge(k):
    e, _, _, ws, ns, want = prepared(k)
    st = want["stats"]
    edge = CASES[k][3]
    if edge == "window63":
        assert ws == 31 and st["max_window"] == 63, st
    else:
        assert st[edge] > 0, (edge, st)
    assert st["occurrences"] > 0 and len(want["losses"]) == ITERS
    if edge == "empty":
        assert (e.occ_ptr[1:] == e.occ_ptr[:-1]).any()


@pytest.mark.parametrize("run", range(len(RUNS)), ids=RUN_IDS)
@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_train_kernel_matches_restatement(k, run):
    e, emb0, ctx0, ws, ns, want = prepared(k)
    mode, span = RUNS[run]
    got = run_device(e, emb0, ctx0, ws, ns, len(want["losses"]), mode, span)
    assert e.mode_used == mode
    check(e, want, got)


@pytest.mark.parametrize("e_range", [(2, 37), (17, 150)])
def test_sequential_shard_range_matches_restatement_of_the_slice(e_range):
    """A range that starts and ends inside one user's run of ratings (make_graph groups ratings by user): the
    skip-gram blocks follow `first`, the KL updates start and stop mid-user."""
    e, emb0, ctx0, ws, ns, _ = prepared(0)
    g = e.g
    e0, e1 = e_range
    assert g.edge_u[e0 - 1] == g.edge_u[e0] and g.edge_u[e1 - 1] == g.edge_u[e1]
    want = restate(e, emb0, ctx0, ws, ns, ITERS, e_range=e_range)
    assert want["stats"]["blocks"] > 0
    got = run_device(e, emb0, ctx0, ws, ns, len(want["losses"]), "sequential", None, e_range=e_range)
    check(e, want, got)


@pytest.mark.parametrize("d,ns", [(16, 4), (64, 7)])
def test_short_lsh_pools_match_restatement(d, ns):
    """LSH pools of sides smaller than pool_size: a valid prefix, then -1.  An occurrence draws min(ns, valid) slots
    of the prefix (random.sample(negs, min(num_negs, len(negs))), src/bine_graph_utils.py:185)."""
    from n2v_hip import bine
    from test_gpu_bine_lsh import clustered_graph
    g = clustered_graph(60, 20, 5)
    e = bine.BineEngine(g, device="cuda:0", seed=11)
    e.calculate_centrality()
    e.generate_walks(percentage=0.15, maxT=4, minT=1)
    e.build_negative_pools(pool_size=64)
    pool = e.pool.cpu().numpy()
    assert (pool < 0).any()
    e.build_occurrences()
    e.init_embeddings(d=d)
    emb0, ctx0 = e.emb.clone(), e.ctx.clone()
    want = restate(e, emb0, ctx0, 5, ns, ITERS)
    assert want["stats"]["short_pool"] > 0
    for mode, span in (("sequential", None), ("store", 1)):
        got = run_device(e, emb0, ctx0, 5, ns, len(want["losses"]), mode, span)
        check(e, want, got)
