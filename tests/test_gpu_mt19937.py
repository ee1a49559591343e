"""The MT19937 stream kernels (csrc/n2v_mt19937.hip: mt_fill_kernel<0 | 1 | 2>, mt_jump_kernel) against the numpy
restatement in tests/mt19937_reference.py (itself held to numpy by tests/test_mt19937_host.py), at their edges.

The entry points are called directly: start states come from the restated raw sequence, never from the jump code, so
strides that are not whole blocks, streams of a single double, trailing streams without output and every `pos` from 0
to 624 are reachable at a few thousand doubles.  Every output buffer lies inside a larger one filled with a sentinel
bit pattern (no uniform in [0, 1) has it), and the whole buffer is compared: every stream double at the position the
restated layout gives, every other element — the holes of the tiled layout and both guards — untouched.  All
comparisons are exact: uint64 views of doubles, uint32 states."""
import collections

import numpy as np
import pytest

import mt19937_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0xFFF8DEADBEEF0001)      # a NaN: never a uniform
SENTINEL32 = np.uint32(0xA5C3F00D)
FRONT = 64                                    # guard doubles in front of the output: keeps it 64-byte aligned
KEY = np.random.RandomState(20240229).get_state()[1].copy()

# pairs_per_walk on both sides of every ring size of mt_fill_kernel<2> (2^r doubles, the smallest 2^r >= 8 * pairs + 320),
# on both sides of the switch to mt_fill_kernel<1> (r > 12), and two more sizes of the latter
RING_OF = {1: 9, 2: 9, 24: 9, 25: 10, 88: 10, 89: 11, 216: 11, 217: 12, 472: 12, 473: None, 499: None, 1000: None}
MODE2 = tuple(p for p, r in RING_OF.items() if r is not None)
MODE1 = tuple(p for p, r in RING_OF.items() if r is None)

Case = collections.namedtuple("Case", "pairs pos wps ns kind final")   # pairs 0: linear output


def ring_rule(pairs):
    """fill_common's choice: ring exponent of mt_fill_kernel<2>, None for mt_fill_kernel<1>."""
    dpw, r = 2 * pairs, 0
    while (1 << r) < 4 * dpw + 320:
        r += 1
    return r if r <= 12 else None


def family(pairs):
    return "linear" if pairs == 0 else ("mode2" if ring_rule(pairs) is not None else "mode1")


def long_stride(pairs):
    """Whole blocks that hold two groups of four segments (16 * pairs words each): wherever such a stream starts, one
    whole group lies inside it."""
    return 624 * -(-32 * max(pairs, 1) // 624)


def n_doubles(c):
    half = (c.wps // 2) & ~1                  # an even number of words strictly inside a stream (wps > 2)
    if c.kind == "one":
        return 1
    if c.kind == "stream_end":                # the last stream is full
        return c.ns * c.wps // 2
    if c.kind == "mid":                       # ends inside the last stream, not on a block end
        assert 0 < half < c.wps
        words = (c.ns - 1) * c.wps + half
        if (c.pos + words) % 624 == 0:
            words += 2
        assert words < c.ns * c.wps
        return words // 2
    if c.kind == "block_end":                 # pos + 2n is a whole number of blocks, inside the last stream
        words = (c.pos + c.ns * c.wps - 2) // 624 * 624 - c.pos
        assert (c.ns - 1) * c.wps < words < c.ns * c.wps and words % 2 == 0
        return words // 2
    if c.kind == "trailing2":                 # the last two streams have no output at all
        words = (c.ns - 3) * c.wps + (half if c.wps > 2 else 2)
        assert (c.ns - 3) * c.wps < words <= (c.ns - 2) * c.wps
        return words // 2
    raise ValueError(c.kind)


def _table():
    cases = []
    odd = (1, 311, 623)
    # every layout with a stride that holds whole groups: block-aligned, and with 2 added under an odd pos
    for i, p in enumerate((0,) + MODE2 + MODE1):
        cases.append(Case(p, (0, 624, 312)[i % 3], long_stride(p), 3, "mid", True))
        cases.append(Case(p, odd[i % 3], long_stride(p) + 2, 4, ("stream_end", "mid")[i % 2], True))
    # every pos, every short stride and every kind of n against every family
    edges = [(0, 2, 5, "stream_end"), (624, 2, 5, "trailing2"), (1, 624, 4, "mid"), (311, 626, 3, "one"),
             (0, 626, 4, "block_end"), (624, 1248, 3, "block_end"), (623, 1248, 5, "trailing2"), (311, 624, 3, "stream_end"),
             (623, 2, 4, "stream_end")]
    for p in (0, 25, 473):
        for j, (pos, wps, ns, kind) in enumerate(edges):
            cases.append(Case(p, pos, wps, ns, kind, j != 2))       # one case per family without a final_state
    # a stream boundary on a segment boundary inside a group (312 = 78 segments of 4 doubles, 19.5 groups)
    cases.append(Case(2, 0, 624, 4, "mid", True))
    # the same for the element-wise kernel: streams of exactly one segment (946 doubles), so every boundary is a segment
    # edge and three in four are not the edge of a four-segment group
    cases.append(Case(473, 0, 2 * 946, 5, "mid", True))
    # the other MODE 2 sizes at a short, unaligned stride: boundaries inside segments
    for p in (1, 24, 88, 89, 216, 217, 472):
        cases.append(Case(p, 1, 626, 5, "trailing2", True))
    # more than 64 segments (the second tile row) at the largest MODE 2 size and in MODE 1
    cases.append(Case(472, 0, long_stride(472), 9, "stream_end", True))
    cases.append(Case(473, 1, long_stride(473) + 2, 9, "mid", True))
    # many streams: once linear, once tiled
    cases.append(Case(0, 1, 626, 65, "mid", True))
    cases.append(Case(24, 623, 624, 64, "stream_end", True))
    return cases


CASES = _table()
CASE_IDS = ["%s-p%d-pos%d-w%d-s%d-%s%s" % (family(c.pairs), c.pairs, c.pos, c.wps, c.ns, c.kind, "" if c.final else "-nofinal")
            for c in CASES]


def geometry(c):
    """Per stream with output: (first double, one past its last double)."""
    n = n_doubles(c)
    return [(k * c.wps // 2, min(n, (k + 1) * c.wps // 2)) for k in range(c.ns) if k * c.wps // 2 < n]


# ---------------------------------------------------------------------------------------------------- coverage (host)
def test_case_table_is_valid_and_unique():
    assert len(set(CASES)) == len(CASES)
    for c in CASES:
        n = n_doubles(c)
        assert 0 <= c.pos <= 624 and c.wps >= 2 and c.wps % 2 == 0 and 1 <= n and 2 * n <= c.ns * c.wps, c
        assert n <= 80000, c                                       # nothing needs more than that


def test_ring_rule_matches_the_table():
    """The table's ring sizes are the library's rule (2^r >= 4 * dpw + 320, r <= 12) recomputed here."""
    for p, r in RING_OF.items():
        assert ring_rule(p) == r, (p, r)
    for lo, hi in ((24, 25), (88, 89), (216, 217), (472, 473)):
        assert hi == lo + 1 and ring_rule(lo) != ring_rule(hi)
    assert {RING_OF[p] for p in MODE2} == {9, 10, 11, 12} and len(MODE1) >= 3


def test_every_axis_value_meets_every_family():
    for fam in ("linear", "mode2", "mode1"):
        mine = [c for c in CASES if family(c.pairs) == fam]
        assert {c.pos for c in mine} >= {0, 1, 311, 623, 624}, fam
        assert {c.wps for c in mine} >= {2, 624, 626, 1248}, fam
        assert {c.kind for c in mine} == {"one", "mid", "stream_end", "block_end", "trailing2"}, fam
        assert any(not c.final for c in mine) and any(3 <= c.ns <= 5 for c in mine)
        assert any(c.pos % 2 == 1 and c.wps % 624 != 0 for c in mine), fam            # odd pos, unaligned stride
        assert any(c.pos == 624 and c.wps == 2 for c in mine), fam
        for c in mine:
            if c.kind == "trailing2":
                assert len(geometry(c)) <= c.ns - 2
            if c.kind == "block_end":
                assert (c.pos + 2 * n_doubles(c)) % 624 == 0
            if c.kind == "mid":
                assert (c.pos + 2 * n_doubles(c)) % 624 != 0 and 2 * n_doubles(c) % c.wps != 0
    many = [c for c in CASES if c.ns >= 64]
    assert sorted(family(c.pairs) for c in many) == ["linear", "mode2"]
    assert {family(c.pairs) for c in CASES} == {"linear", "mode2", "mode1"}
    assert {c.pairs for c in CASES} == {0} | set(RING_OF)


@pytest.mark.parametrize("pairs", MODE2 + MODE1)
def test_each_tiled_size_has_its_stream_edges(pairs):
    """From the restated geometry alone: a whole four-segment group inside one stream, a group cut by a stream
    boundary, a stream with a ragged first and a ragged last group; a block-aligned long stride and one with 2 added."""
    dpw, G = 2 * pairs, 8 * pairs
    mine = [c for c in CASES if c.pairs == pairs]
    whole = cut = ragged = False
    for c in mine:
        for k, (lo, hi) in enumerate(geometry(c)):
            first = -(-lo // G)
            whole |= (first + 1) * G <= hi
            cut |= k > 0 and lo % G != 0
            ragged |= lo % G != 0 and hi % G != 0 and (first + 1) * G <= hi
    assert whole and cut and ragged, (pairs, whole, cut, ragged)
    assert {long_stride(pairs), long_stride(pairs) + 2} <= {c.wps for c in mine}
    assert long_stride(pairs) // 2 >= 2 * G


def test_stream_boundaries_fall_inside_segments_and_inside_groups():
    for fam, sizes in (("mode2", MODE2), ("mode1", MODE1)):
        in_segment = in_group = second_row = False
        for c in CASES:
            if c.pairs not in sizes:
                continue
            dpw, G = 2 * c.pairs, 8 * c.pairs
            for k, (lo, hi) in enumerate(geometry(c)):
                in_segment |= k > 0 and lo % dpw != 0
                in_group |= k > 0 and lo % dpw == 0 and lo % G != 0
                second_row |= hi > 64 * dpw
        assert in_segment and in_group and second_row, fam


# ---------------------------------------------------------------------------------------------------------- the fills
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from n2v_hip import _lib
    return _lib, _lib.load(), torch.device("cuda:0")


@pytest.fixture()
def numpy_global_state():
    saved = np.random.get_state()
    yield
    np.random.set_state(saved)


def _first_difference(got, want, front, size):
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    where = "front guard" if i < front else ("back guard" if i >= front + size else "output[%d]" % (i - front))
    kind = "sentinel overwritten" if want[i] == SENTINEL else ("left unwritten" if got[i] == SENTINEL else "wrong value")
    return "%d elements differ; first at %s: %s (got %016x, want %016x)" % (len(bad), where, kind, int(got[i]), int(want[i]))


def run_fill(dev, c):
    import torch
    _lib, lib, d = dev
    n = n_doubles(c)
    x = ref.raw_words(KEY, c.ns * c.wps + 624)
    states = np.stack([x[k * c.wps:k * c.wps + 624] for k in range(c.ns)])          # window_after(KEY, k * wps)
    want = ref.doubles_of_words(x[c.pos:c.pos + 2 * n])
    if c.pairs:
        where, size = ref.tiled_layout(n, c.pairs)
        back = 64 * 2 * c.pairs + 8                 # one more group of 64 segments
    else:
        where, size, back = np.arange(n), n, 1024
    total = FRONT + size + back
    buf = torch.full((total,), int(SENTINEL.view(np.int64)), dtype=torch.int64, device=d)
    fin = torch.full((16 + 625 + 16,), int(SENTINEL32.view(np.int32)), dtype=torch.int32, device=d)
    states_d = torch.from_numpy(states.view(np.int32)).to(d)
    out_ptr = buf.data_ptr() + 8 * FRONT
    fin_ptr = fin.data_ptr() + 4 * 16 if c.final else None
    assert out_ptr % 64 == 0
    with torch.cuda.device(d):
        if c.pairs:
            rc = lib.n2v_mt19937_fill_tiled(states_d.data_ptr(), c.ns, c.pos, c.wps, n, c.pairs, out_ptr, fin_ptr,
                                            _lib.stream_ptr(d))
        else:
            rc = lib.n2v_mt19937_fill(states_d.data_ptr(), c.ns, c.pos, c.wps, n, out_ptr, fin_ptr, _lib.stream_ptr(d))
        _lib.check(rc)
        torch.cuda.synchronize(d)
    got = buf.cpu().numpy().view(np.uint64)
    expect = np.full(total, SENTINEL, dtype=np.uint64)
    expect[FRONT + where] = want.view(np.uint64)
    if not np.array_equal(got, expect):
        pytest.fail(_first_difference(got, expect, FRONT, size))
    f = fin.cpu().numpy().view(np.uint32)
    assert (f[:16] == SENTINEL32).all() and (f[16 + 625:] == SENTINEL32).all(), "final_state guard"
    if not c.final:
        assert (f == SENTINEL32).all()
        return
    k = (2 * n - 1) // c.wps                                     # the last stream with output
    key_k, pos_k = ref.state_after(states[k], c.pos, n - k * c.wps // 2)
    assert int(f[16 + 624]) == pos_k, (int(f[16 + 624]), pos_k)
    assert np.array_equal(f[16:16 + 624], key_k), "final_state key"
    if c.wps % 624 == 0:
        rs = np.random.RandomState(0)
        rs.set_state(("MT19937", KEY, c.pos, 0, 0.0))
        assert np.array_equal(rs.random_sample(n).view(np.uint64), want.view(np.uint64))
        st = rs.get_state()
        assert int(f[16 + 624]) == st[2] and np.array_equal(f[16:16 + 624], st[1]), "final_state vs numpy"


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_fill_equals_the_restated_stream(dev, k):
    run_fill(dev, CASES[k])


# ------------------------------------------------------------------------------------------------------ the jump kernel
JUMP_STRIDES = (1, 2, 7, 624, 626, 1001, 1872, 2496, 19937, 19938, 19939, 40000)
JUMP_STREAMS = (2, 3, 4, 5, 8, 9, 64, 65)


@pytest.mark.parametrize("stride", JUMP_STRIDES)
def test_device_jump_equals_the_raw_sequence(dev, stride):
    """Round 0 of a stride below 19938 is a bare power of x (one set bit: only the kernel's tail loop runs); later
    rounds and longer strides are reduced polynomials of thousands of set bits (the eight-at-a-time loop).  19937 is
    the longest sequence the kernel's LDS buffer is sized for."""
    import torch
    from n2v_hip import mt19937
    x = ref.raw_words(KEY, (max(JUMP_STREAMS) - 1) * stride)
    for ns in JUMP_STREAMS:
        got = mt19937.jump_states_device(KEY, stride, ns, "cuda:0")
        torch.cuda.synchronize()
        got = got.cpu().numpy().view(np.uint32)
        assert got.shape == (ns, 624)
        want = np.stack([x[k * stride:k * stride + 624] for k in range(ns)])
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (stride, ns, bad[:8].tolist())


# ------------------------------------------------------------------------------------------------- the product's path
# (n, streams and words per stream global_uniforms_device ends up with, who derives the start states): 10 streams for
# 9 * 4096 doubles become 8 once the stride is rounded up to 16 blocks, which the host still jumps
PRODUCT_PATHS = [(5 * 4096, 6, 624 * 11, "host"), (9 * 4096, 8, 624 * 16, "host"), (17 * 4096, 14, 624 * 16, "device")]


@pytest.mark.parametrize("tiled_pairs", [None, 79, 499])
@pytest.mark.parametrize("n,n_streams,wps,jump", PRODUCT_PATHS, ids=["%d-%s%d" % (p[0], p[3], p[1]) for p in PRODUCT_PATHS])
def test_global_uniforms_device_state_and_out_buffer(dev, numpy_global_state, monkeypatch, n, n_streams, wps, jump, tiled_pairs):
    """Several streams with the state read back from the kernel, linear and tiled: start states by the host jump (up to
    HOST_JUMP_STREAMS streams) and by the device jump (beyond) — the path taken is observed, not inferred; an `out=`
    buffer longer than needed is written in its first `need` elements only."""
    import torch
    from n2v_hip import mt19937
    _, _, d = dev
    assert (jump == "device") == (n_streams > mt19937.HOST_JUMP_STREAMS) and n_streams > 1
    calls = []
    host_jump, device_jump = mt19937.jump_states, mt19937.jump_states_device
    monkeypatch.setattr(mt19937, "jump_states", lambda key, stride, ns: (calls.append(("host", stride, ns)),
                                                                       host_jump(key, stride, ns))[1])
    monkeypatch.setattr(mt19937, "jump_states_device", lambda key, stride, ns, dv: (calls.append(("device", stride, ns)),
                                                                                  device_jump(key, stride, ns, dv))[1])
    pos = 311
    rs = np.random.RandomState(0)
    rs.set_state(("MT19937", KEY, pos, 0, 0.0))
    want = rs.random_sample(n)
    st_want = rs.get_state()
    assert np.array_equal(want.view(np.uint64), ref.doubles(KEY, pos, n).view(np.uint64))
    if tiled_pairs:
        where, need = ref.tiled_layout(n, tiled_pairs)
    else:
        where, need = np.arange(n), n
    extra = 64 * 2 * (tiled_pairs or 8)
    for from_device in (True, False):
        del calls[:]
        buf = torch.full((need + extra,), int(SENTINEL.view(np.int64)), dtype=torch.int64, device=d)
        np.random.set_state(("MT19937", KEY, pos, 0, 0.0))
        got = mt19937.global_uniforms_device(n, d, state_from_device=from_device, tiled_pairs=tiled_pairs,
                                             out=buf.view(torch.float64))
        torch.cuda.synchronize(d)
        st = np.random.get_state()
        # the start states came from where the table says; without the read-back the host then advances the global state
        assert calls[0] == (jump, wps, n_streams), calls
        assert len(calls) == (1 if from_device else 2) and all(c[0] == "host" and c[2] == 2 for c in calls[1:]), calls
        assert got.numel() == need and got.data_ptr() == buf.data_ptr()
        expect = np.full(need + extra, SENTINEL, dtype=np.uint64)
        expect[where] = want.view(np.uint64)
        have = buf.cpu().numpy().view(np.uint64)
        if not np.array_equal(have, expect):
            pytest.fail(_first_difference(have, expect, 0, need))
        assert st[2] == st_want[2] and np.array_equal(st[1], st_want[1]), from_device


# ----------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def walk_graph():
    import node2vec
    from n2v_hip import csr
    rs = np.random.RandomState(9)
    n, m = 200, 700
    src, dst = rs.randint(0, n, m), rs.randint(0, n, m)
    keep = src != dst
    cg = csr.from_edges(src[keep], dst[keep], None, False)          # undirected: no walk ends early
    g = node2vec.Graph.from_csr(cg, 0.5, 2.0, rng="numpy")
    g.preprocess_transition_probs()
    saved = np.random.get_state()
    g.simulate_walks(1, 3)               # selects the table-driven walk kernel, which _tiled_uniforms_ok asks about
    np.random.set_state(saved)
    return g


@pytest.mark.parametrize("L", [473, 474, 500])
def test_long_walks_read_the_tiled_uniforms_like_numpy(dev, numpy_global_state, walk_graph, L):
    """L - 1 = 472 pairs is the last size of the ring fill, 473 and 499 run the element-wise fill; the walk kernel
    reads the tiled layout at those sizes.  Against the same walk fed by numpy's own random_sample on the host, and
    by the linear device fill."""
    import torch
    g = walk_graph
    for k in ("host_rng", "linear_uniforms"):
        g.__dict__.pop(k, None)
    assert g._engine.edge_fat is not None and g._tiled_uniforms_ok(L)
    res = {}
    try:
        for mode in ("tiled", "host", "linear"):
            for k in ("host_rng", "linear_uniforms"):
                g.__dict__.pop(k, None)
            if mode == "host":
                g.host_rng = True
            if mode == "linear":
                g.linear_uniforms = True
            assert g._tiled_uniforms_ok(L) == (mode == "tiled")
            np.random.seed(31)
            c = g.simulate_walks(1, L)
            st = np.random.get_state()
            res[mode] = (c.walks.clone(), c.lens.clone(), st[1].copy(), int(st[2]))
    finally:
        for k in ("host_rng", "linear_uniforms"):      # the graph is shared by the module
            g.__dict__.pop(k, None)
    assert bool((res["host"][1] == L).all())                         # every walk drew its 2 (L - 1) uniforms
    chk = np.random.RandomState(31)
    chk.random_sample(2 * (L - 1) * res["host"][0].shape[0])
    assert res["host"][3] == chk.get_state()[2] and np.array_equal(res["host"][2], chk.get_state()[1])
    for mode in ("tiled", "linear"):
        assert torch.equal(res[mode][1], res["host"][1]), (L, mode)
        assert torch.equal(res[mode][0], res["host"][0]), (L, mode)
        assert res[mode][3] == res["host"][3] and np.array_equal(res[mode][2], res["host"][2]), (L, mode)
