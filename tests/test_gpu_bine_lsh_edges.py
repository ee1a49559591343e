"""GPU edge cases of the MinHash-LSH pool kernels (csrc/n2v_lsh.hip) against oracle/bine_lsh_oracle.py, bit for bit:
signatures, every query list with its order, the owners and every pool row, on the cases of tests/lsh_cases.py.
Everything is integer and compared with array_equal.  tests/test_lsh_cases_host.py shows on the CPU which path of
which kernel each case reaches (chunks exactly full, k = 256, probe chains over the end of the LDS set, bitmaps
serving many leaders, rounds cut at every boundary, complements of pool_size - 1 / pool_size / pool_size + 1, …) and
that the expected arrays change under six plausible slips of the kernels; run it first.  All inputs reach the
kernels through BineEngine, apart from one n2v_lsh_minhash call over the item rows alone."""
import functools

import numpy as np
import pytest

import lsh_cases as C
import lsh_reference as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def engine_of(graph):
    from n2v_hip import bine
    return bine.BineEngine(R.graph_of(graph), device="cuda:0", seed=R.ENGINE_SEED)


def run(case):
    e = engine_of(case.graph)
    e._build_lsh_pools(case.pool_size, case.k, groups=case.groups)
    return e


def assert_equals_oracle(e, case):
    exp = R.expected(case)
    sig_dev = e.lsh["signatures"].cpu().numpy().view(np.uint32)
    pool = e.pool.cpu().numpy()
    assert pool.shape == (e.g.n, case.pool_size)
    for side in "uv":
        want = exp[side]
        a, b = want["lo"], want["hi"]
        assert np.array_equal(sig_dev[a:b], want["sig"]), (case.name, side)
        sim = e.lsh[side]["sim"].cpu().numpy()
        sim_n = e.lsh[side]["sim_n"].cpu().numpy()
        assert sim.shape == (b - a, case.k)
        assert np.array_equal(sim_n, [len(s) for s in want["sims"]]), (case.name, side)
        for i, s in enumerate(want["sims"]):
            assert sim[i, :len(s)].tolist() == s, (case.name, side, i)
        assert np.array_equal(e.lsh[side]["owner"].cpu().numpy(), want["owner"]), (case.name, side)
        assert e.lsh[side]["clusters"] == len(np.unique(want["owner"]))
        rows = pool[a:b]
        bad = np.nonzero((rows != want["pool"]).any(axis=1))[0]
        assert bad.size == 0, (case.name, side, bad[:8].tolist(), want["owner"][bad[:8]].tolist())


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_lsh_pools_equal_restatement_at_the_edges(case):
    assert_equals_oracle(run(case), case)


def test_groups_settings_give_identical_pools():
    """59 / 15 leaders per side through 1, 2 or 59 / 15 bitmaps: the same rows, and the oracle's."""
    pools = []
    for groups in C.GROUPS:
        case = C.BY_NAME["base_groups%d" % groups]
        e = run(case)
        pools.append(e.pool.cpu().numpy().copy())
    assert np.array_equal(pools[0], pools[1]) and np.array_equal(pools[0], pools[2])
    side = R.expected(case)
    assert np.array_equal(pools[0], np.concatenate([side["u"]["pool"], side["v"]["pool"]]))


def test_self_missing_vertex_draws_itself():
    """k below the size of a duplicate group: its later members are not in their own lists, lead themselves, and
    their own id is a candidate like any other (the reference's `total_list` holds it too)."""
    case = C.BY_NAME["tiny"]
    e = run(case)
    sim = e.lsh["u"]["sim"].cpu().numpy()
    owner = e.lsh["u"]["owner"].cpu().numpy()
    pool = e.pool.cpu().numpy()
    missing = [v for v in range(e.g.n_u) if sim[v, 0] != v]
    assert len(missing) == 4 and all(owner[v] == v for v in missing)
    assert any(v in pool[v].tolist() for v in missing)
    assert np.array_equal(pool[:e.g.n_u], R.expected(case)["u"]["pool"])


def test_label_table_equals_hashlib():
    import hashlib
    from n2v_hip import bine
    ul, il = C.label_table()
    g = bine.BipartiteGraph(ul, il, np.ones(len(ul)))
    e = bine.BineEngine(g, device="cuda:0", seed=1)
    hv = e.label_hashes().cpu().numpy().view(np.uint32)
    want = np.array([int.from_bytes(hashlib.sha1(s.encode("utf8")).digest()[:4], "little") for s in R.labels_of(g)],
                    dtype=np.uint32)
    assert hv.shape == want.shape and np.array_equal(hv, want)


def test_minhash_of_the_item_rows_alone():
    """n2v_lsh_minhash(v_begin = n_u, v_end = n): row v - v_begin of the output, nothing behind row n_v.  The buffer
    has n + 1 rows, so a kernel that wrote row v would still write inside it — and be seen."""
    import torch
    from n2v_hip import _lib
    e = engine_of("base")
    g, p = e.g, _lib.ptr
    hv = e.label_hashes()
    a, b = e.minhash_permutations()
    pa = torch.from_numpy(a.view(np.int64)).to(e.device)
    pb = torch.from_numpy(b.view(np.int64)).to(e.device)
    out = torch.full((g.n + 1, 128), R.GUARD, dtype=torch.int32, device=e.device)
    _lib.check(e.lib.n2v_lsh_minhash(p(e.row_ptr), p(e.col), p(hv), p(pa), p(pb), g.n_u, g.n, p(out), e._stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    sig = R.signatures_of("base")
    assert np.array_equal(got[:g.n_v].view(np.uint32), sig[g.n_u:])
    assert np.all(got[g.n_v:] == R.GUARD)
    assert np.array_equal(got[:g.n_v], e.minhash_signatures(hv).cpu().numpy()[g.n_u:])


def test_k_above_256_is_refused_before_launch():
    """The LDS set holds 512 slots for at most 256 keys: k = 257 must fail in the argument check."""
    import torch
    from n2v_hip import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n = 8
    order = torch.arange(n, dtype=torch.int32, device=dev).repeat(8, 1).contiguous()
    rlo = torch.arange(n, dtype=torch.int32, device=dev).view(n, 1, 1).repeat(1, 8, 16).contiguous()
    rhi = rlo + 1
    sim = torch.full((n, 257), R.GUARD, dtype=torch.int32, device=dev)
    sim_n = torch.full((n,), R.GUARD, dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)
    p = _lib.ptr
    for k in (257, 0, -1, 1 << 20):
        assert lib.n2v_lsh_forest_query(p(order), p(rlo), p(rhi), n, k, p(sim), p(sim_n), st) != 0
        msg = lib.n2v_last_error().decode()
        assert "n2v_lsh_forest_query: bad size" in msg and "k %d" % k in msg and "k <= 256" in msg
    torch.cuda.synchronize()
    assert bool((sim == R.GUARD).all()) and bool((sim_n == R.GUARD).all())
    # the same launch at k = 256 is taken: every vertex finds itself
    assert lib.n2v_lsh_forest_query(p(order), p(rlo), p(rhi), n, 256, p(sim), p(sim_n), st) == 0
    torch.cuda.synchronize()
    assert sim_n.tolist() == [1] * n and sim.view(-1)[::256][:n].tolist() == list(range(n))
    # and the engine passes the refusal on
    e = engine_of("two_items")
    e._build_lsh_pools(4, 256)
    before = e.pool.clone()
    with pytest.raises(_lib.N2VError, match="k 257; k <= 256"):
        e.build_negative_pools(pool_size=4, k=257)
    assert torch.equal(e.pool, before)
