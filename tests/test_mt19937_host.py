"""CPU tests of the MT19937 stream code: the restatement in tests/mt19937_reference.py is held to numpy itself, and
the host half of csrc/n2v_mt19937.hip / n2v_hip/mt19937.py (GF(2) jump-ahead, jump polynomials, state bookkeeping, the
tiled index map, argument checks) is held to the restatement.  Needs the built library, no GPU: every call here is host
arithmetic or is rejected before a launch.  Every comparison is exact (uint32 states, uint64 views of doubles)."""
import ctypes as C

import numpy as np
import pytest

import mt19937_reference as ref

POSITIONS = (0, 1, 311, 312, 623, 624)
# one value per kind: a draw that ends before the first block ends (where pos allows), exactly on a block end, one word
# past it, and several blocks further on
STRIDES = (1, 2, 7, 624, 626, 1001, 624 * 3, 624 * 4, 19937, 19938, 19939, 40000)


def _key(seed):
    return np.random.RandomState(seed).get_state()[1].copy()


def _n_edges(pos):
    """n: inside the first block, ending exactly on a block end (pos + 2n == 624 k), one word over (625), several
    blocks on — whichever exist for this parity of pos."""
    out = {1, 5, 312 * 3 + 7, 312 * 5}
    for target in (624, 625, 624 * 2, 624 * 2 + 1, 624 * 4, 624 * 4 + 1):
        if target > pos and (target - pos) % 2 == 0:
            out.add((target - pos) // 2)
    return sorted(out)


@pytest.fixture(scope="module")
def lib():
    from n2v_hip import _lib
    return _lib.load()


@pytest.mark.parametrize("pos", POSITIONS)
def test_restatement_equals_numpy_random_sample(pos):
    key = _key(11)
    ends = set()
    for n in _n_edges(pos):
        rs = np.random.RandomState(0)
        rs.set_state(("MT19937", key, pos, 0, 0.0))
        want = rs.random_sample(n)
        got = ref.doubles(key, pos, n)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (pos, n)
        st = rs.get_state()
        k2, p2 = ref.state_after(key, pos, n)
        assert p2 == st[2] and np.array_equal(k2, st[1]), (pos, n)
        ends.add(pos + 2 * n)
    assert min(ends) < 624 or pos >= 623                            # a draw that stays inside the first block
    assert {624 * 2 + pos % 2, 624 * 4 + pos % 2} <= ends           # ends exactly on a block end (odd pos: one word over)
    assert pos == 624 or 624 + pos % 2 in ends                      # the first block's end: the last draw without a twist
    assert max(ends) >= 624 * 5                                     # several blocks on


def test_restated_window_equals_numpy_key_after_twists():
    key = _key(12)
    for b in (1, 2, 3, 7):
        rs = np.random.RandomState(0)
        rs.set_state(("MT19937", key, 624, 0, 0.0))
        rs.random_sample(312 * b)                                   # b twists, pos back at 624
        st = rs.get_state()
        assert st[2] == 624 and np.array_equal(ref.window_after(key, 624 * b), st[1]), b
    assert np.array_equal(ref.window_after(key, 0), key)


@pytest.mark.parametrize("stride", STRIDES)
def test_host_jump_equals_the_raw_sequence(stride):
    from n2v_hip import mt19937
    key = _key(13)
    x = ref.raw_words(key, 8 * stride)
    for ns in (1, 2, 3, 5, 9):
        got = mt19937.jump_states(key, stride, ns)
        assert got.shape == (ns, 624) and got.dtype == np.uint32
        for k in range(ns):
            assert np.array_equal(got[k], x[k * stride:k * stride + 624]), (stride, ns, k)


@pytest.mark.parametrize("stride,family", [(624, True), (1248, True), (624 * 8, True), (1, False), (7, False), (626, False),
                                           (624 * 3, False), (19937, False), (19938, False), (40000, False)])
def test_jump_polynomials_are_well_formed_and_advance_the_window(lib, stride, family):
    blocks = stride // 624
    assert family == (stride % 624 == 0 and blocks & (blocks - 1) == 0)    # the library's rule for its family path
    rounds = 4
    polys = np.full((rounds, 19968), 0xFFFFFFFF, dtype=np.uint32)
    assert lib.n2v_mt19937_jump_polys_host(stride, rounds, polys.ctypes.data_as(C.c_void_p)) == 0
    key = _key(14)
    x = ref.raw_words(key, max(19938, stride << (rounds - 1)))
    for r in range(rounds):
        n = int(polys[r, 0])
        assert 1 <= n <= 19938
        p = polys[r, 1:1 + n].astype(np.int64)
        assert (np.diff(p) > 0).all() and p[0] >= 0 and p[-1] < 19938, (stride, r)
        want = x[stride << r:(stride << r) + 624]
        assert np.array_equal(ref.apply_positions(x, p), want), (stride, r)
        if (stride << r) < 19938:
            assert p.tolist() == [stride << r]                     # a bare power of x: one set bit


@pytest.mark.parametrize("pos", POSITIONS)
def test_advance_global_state_equals_random_sample(pos):
    from n2v_hip import mt19937
    key = _key(15)
    saved = np.random.get_state()
    try:
        for n in _n_edges(pos):
            np.random.set_state(("MT19937", key, pos, 0, 0.0))
            np.random.random_sample(n)
            want = np.random.get_state()
            np.random.set_state(("MT19937", key, pos, 0, 0.0))
            mt19937.advance_global_state(n)
            got = np.random.get_state()
            assert got[2] == want[2] and np.array_equal(got[1], want[1]), (pos, n)
            k2, p2 = ref.state_after(key, pos, n)
            assert got[2] == p2 and np.array_equal(got[1], k2), (pos, n)
        np.random.set_state(("MT19937", key, pos, 0, 0.0))
        mt19937.advance_global_state(0)
        got = np.random.get_state()
        assert got[2] == pos and np.array_equal(got[1], key)
    finally:
        np.random.set_state(saved)


@pytest.mark.parametrize("pairs", [1, 2, 24, 25, 472, 473, 1000])
def test_tiled_index_and_size_equal_the_literal_layout(pairs):
    from n2v_hip import mt19937
    dpw = 2 * pairs
    for n in (1, dpw - 1, dpw, 3 * dpw + 1, 64 * dpw - 1, 64 * dpw, 64 * dpw + 1, 65 * dpw + 3, 128 * dpw):
        where, size = ref.tiled_layout(n, pairs)
        assert mt19937.tiled_size(n, pairs) == size, (pairs, n)
        assert np.array_equal(mt19937.tiled_index(np.arange(n), pairs), where), (pairs, n)
        assert len(np.unique(where)) == n and where.max() < size


def _err(lib):
    return lib.n2v_last_error().decode()


def test_rejected_arguments_return_an_error(lib):
    """Every call fails its argument check before anything is launched or dereferenced: the pointers are host
    buffers that only have to be non-null (and, for the tiled output, 64-byte aligned or not)."""
    key = _key(16)
    kp = key.ctypes.data_as(C.c_void_p)
    out = np.zeros((9, 624), dtype=np.uint32)
    op = out.ctypes.data_as(C.c_void_p)
    for args in ((None, 624, 2, op), (kp, 624, 2, None), (kp, 624, 0, op), (kp, -1, 2, op)):
        assert lib.n2v_mt19937_jump_host(*args) != 0, args
        assert "n2v_mt19937_jump_host" in _err(lib)
    polys = np.zeros((33, 19968), dtype=np.uint32)
    pp = polys.ctypes.data_as(C.c_void_p)
    for args in ((0, 1, pp), (624, 0, pp), (624, 33, pp), (624, 1, None)):
        assert lib.n2v_mt19937_jump_polys_host(*args) != 0, args
        assert "n2v_mt19937_jump_polys_host" in _err(lib)
    # 5 streams need 3 rounds; 9 need 4
    for ns, rounds in ((5, 2), (9, 3), (2, 0), (0, 1)):
        assert lib.n2v_mt19937_jump_device(op, ns, pp, rounds, None) != 0, (ns, rounds)
        assert "n2v_mt19937_jump_device" in _err(lib)
    assert lib.n2v_mt19937_jump_device(None, 2, pp, 1, None) != 0
    assert lib.n2v_mt19937_jump_device(op, 2, None, 1, None) != 0

    raw = np.zeros(64, dtype=np.float64)
    base = raw.ctypes.data
    aligned = base + (-base) % 64
    bad = [dict(pos=-1), dict(pos=625), dict(wps=625), dict(wps=0), dict(wps=-2), dict(ns=0), dict(n=-1),
           dict(ns=3, wps=624, n=937),                  # 3 * 624 words hold 936 doubles
           dict(states=None), dict(out=None)]
    for tiled in (False, True):
        name = "n2v_mt19937_fill_tiled" if tiled else "n2v_mt19937_fill"
        cases = list(bad)
        if tiled:
            cases += [dict(pairs=0), dict(pairs=-1), dict(pairs=(1 << 24) + 1), dict(out=aligned + 8),
                      dict(wps=1 << 33, ns=1, pairs=1)]           # a stream of 2^32 doubles: beyond the 32-bit in-stream split
        for kw in cases:
            a = dict(states=op, ns=3, pos=0, wps=624, n=10, pairs=3, out=aligned)
            a.update(kw)
            if tiled:
                rc = lib.n2v_mt19937_fill_tiled(a["states"], a["ns"], a["pos"], a["wps"], a["n"], a["pairs"], a["out"], None, None)
            else:
                rc = lib.n2v_mt19937_fill(a["states"], a["ns"], a["pos"], a["wps"], a["n"], a["out"], None, None)
            assert rc != 0, (name, kw)
            assert _err(lib).startswith(name + ":"), (name, kw, _err(lib))
    assert not raw.any() and not out.any()
    # the accepted edge that launches nothing: zero doubles
    assert lib.n2v_mt19937_fill(op, 1, 624, 2, 0, None, None, None) == 0
    assert lib.n2v_mt19937_fill_tiled(op, 1, 0, 2, 0, 1, None, None, None) == 0
