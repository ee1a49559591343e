"""GPU tests: the second level of the rating kernels — the paths that only do something once a first-level count passes
a threshold (csrc/n2v_compact.h and csrc/n2v_eccstats.hip: the one-workgroup scans past 256 tiles, a group longer than
a tile, item_gptr over items without rows, the long-segment queue past its 8 192 wavefronts, the third round of the
totals; csrc/n2v_eccknn.hip: the sparse kernel's decode of 1 176 triangle tiles) — through the C-ABI unless a test says
otherwise, on the inputs of tests/scale_cases.py, which tests/test_scale_cases_host.py shows to cross every threshold.

Exact comparisons only: integers with array_equal, fp64 by bytes after canon.  Every output buffer starts as a sentinel;
the scratch of the scans has sentinel words behind it that must come back untouched.  All inputs are well formed."""
import numpy as np
import pytest

import consistency_reference as C
import eccknn_reference as E
import eccsplit_reference as S
import eccstats_reference as R
import scale_cases as sc
from test_gpu_consistency import c_join
from test_gpu_eccknn_sparse import assert_same, c_dense, c_sparse
from test_gpu_eccsplit import c_pairs, c_select, pairs_numpy, tile
from test_gpu_eccstats import ISENT, SENT, _L, _dev, _full, c_moments, c_segsum, check

pytestmark = pytest.mark.gpu

assert ISENT == sc.SENTINEL


# ---- 1: the two-level scans ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_tiles", sc.N_TILES)
def test_select_past_256_tiles(n_tiles):
    assert tile() == sc.TILE
    user, bins, which, keep = sc.select_case(n_tiles)
    got = c_select(user, bins, which, pad=sc.SCAN_PAD)
    assert np.array_equal(got, S.rows_of_bin(user, bins, which))
    assert len(got) == int(keep.sum())


def test_pairs_at_257_tiles():
    key, w, n_nodes, last = sc.pairs_case()
    want_key, want_w = pairs_numpy(key, w, n_nodes)
    got_key, got_w = c_pairs(key, w, n_nodes)                            # two slots per kept element
    assert len(got_key) == 2 * int(last.sum()) and np.array_equal(got_key, want_key)
    assert got_w.tobytes() == want_w.tobytes()


def test_join_at_257_tiles():
    cs = sc.join_case()
    ids, o1, o2 = c_join(*cs)
    want = C.join(*cs)
    assert np.array_equal(ids, want[0]) and len(ids) > 0
    assert o1.tobytes() == want[1].tobytes() and o2.tobytes() == want[2].tobytes()


def c_groups(key_sorted, perm, n_tw, n_items):
    """n2v_eccstats_groups alone -> numpy (row_group, group_begin, unum, item_gptr, counts), everything a sentinel first."""
    import torch
    L = _L(); lib = L.load()
    dk, dp = _dev(key_sorted, np.int64), _dev(perm, np.int64)
    n = len(key_sorted)
    n_scratch = int(lib.n2v_eccstats_groups_scratch(n))
    scratch = _full(n_scratch + sc.SCAN_PAD, ISENT, torch.int64)
    row_group, group_begin = _full(n, ISENT, torch.int32), _full(n + 1, ISENT, torch.int64)
    unum, item_gptr, counts = _full(n, ISENT, torch.int64), _full(n_items + 1, ISENT, torch.int64), _full(2, ISENT, torch.int64)
    L.check(lib.n2v_eccstats_groups(L.ptr(dk), L.ptr(dp), n, n_tw, n_items, L.ptr(scratch), L.ptr(row_group), L.ptr(group_begin),
                                    L.ptr(unum), L.ptr(item_gptr), L.ptr(counts), L.stream_ptr(dk.device)))
    torch.cuda.synchronize()
    assert n_scratch == -(-n // sc.TILE) and (scratch[n_scratch:] == ISENT).all()
    return tuple(t.cpu().numpy() for t in (row_group, group_begin, unum, item_gptr, counts))


@pytest.mark.parametrize("n_tiles", sc.N_TILES)
def test_groups_past_256_tiles_long_group_and_item_gaps(n_tiles):
    case = sc.groups_case(n_tiles)
    want_rg, want_begin, want_gptr, (n_groups, largest) = sc.groups_expected(case)
    row_group, group_begin, unum, item_gptr, counts = c_groups(case["key"], case["perm"], case["n_tw"], case["n_items"])
    assert counts.tolist() == [n_groups, largest] == [len(case["unum"]), sc.LONG_GROUP]
    assert row_group.dtype == np.int32 and np.array_equal(row_group, want_rg)       # row_group[perm[k]]: the group of k
    assert np.array_equal(unum[:n_groups], case["unum"]) and (unum[n_groups:] == ISENT).all()
    assert np.array_equal(group_begin[:n_groups + 1], want_begin) and (group_begin[n_groups + 1:] == ISENT).all()
    assert np.array_equal(item_gptr, want_gptr), np.nonzero(item_gptr != want_gptr)[0][:8]


# ---- 2: the long-segment queue and the totals ---------------------------------------------------------------------------

def test_segsum_queue_of_three_passes():
    case = sc.segsum_case()
    lens = case["lens"]
    n_seg = len(lens)
    seg = np.repeat(np.arange(n_seg), lens)
    ptr, a, g = _dev(case["ptr"], np.int64), _dev(case["a"], np.float64), _dev(case["g"], np.float64)
    perm, idx = _dev(case["perm"], np.int64), _dev(case["idx"], np.int32)
    # perm, idx and g: both sums
    av = case["a"][case["perm"]]
    wv = av * case["g"][case["idx"][case["perm"]]]
    s, w = c_segsum(ptr, a, perm=perm, idx=idx, g=g)
    s, w = s.cpu().numpy(), w.cpu().numpy()
    want_s, want_w = R.segment_sum(seg, av, n_seg), R.segment_sum(seg, wv, n_seg)
    assert R.canon(s) == R.canon(want_s), np.nonzero(s != want_s)[0][:8]            # a sentinel: a dropped queue entry
    assert R.canon(w) == R.canon(want_w), np.nonzero(w != want_w)[0][:8]
    # mean = 1, no g, no perm: the elements in place; an empty segment's mean is 0 / 0
    m, none = c_segsum(ptr, a, mean=True)
    with np.errstate(all="ignore"):
        want_m = R.segment_sum(seg, case["a"], n_seg) / lens.astype(np.float64)
    m = m.cpu().numpy()
    assert none is None and R.canon(m) == R.canon(want_m), np.nonzero(m != want_m)[0][:8]
    assert np.isnan(want_m).sum() == (lens == 0).sum() > 0


@pytest.mark.parametrize("n", sc.MOMENT_N)
def test_moments_third_round_of_the_totals(n):
    x = sc.moments_case(n)
    s = c_moments(_dev(x, np.float64)).cpu().numpy()
    m = np.float64(R.chunked_sum(x)) / np.float64(n)
    d = x - m
    ssd = np.float64(R.chunked_sum(d * d))
    lo, hi = R.min_max(x)
    want = np.array([R.chunked_sum(x), m, ssd, ssd / n, np.sqrt(ssd / n), lo, hi, n], dtype=np.float64)
    assert R.canon(s) == R.canon(want), (s, want)


# ---- 3: the whole chain once at workload shape --------------------------------------------------------------------------

def test_chain_at_workload_shape():
    """261 tiles, 8 200 queued user segments, a group of more than three tiles: check() of tests/test_gpu_eccstats.py
    through the C-ABI, then the module (its own torch.empty scratch) against the same restatement."""
    from n2v_hip import eccstats as M
    u, i, fb, tw = sc.chain_case()
    want, got = check(u, i, fb, tw)
    assert got["largest"] >= sc.LONG_GROUP and len(want["users"]) == sc.CHAIN_USERS and len(want["items"]) == sc.CHAIN_ITEMS
    for k in R.COLUMNS:
        assert np.isfinite(got[k]).all(), k
    st = M.item_statistics(u, i, fb, tw, intermediates=True)
    assert st.items == want["items"] and st.users == want["users"]
    for k in M.MODES + ("ue",):
        assert R.canon(getattr(st, k)) == R.canon(want[k]), k
    for k in M.INTERMEDIATES:
        assert R.canon(st.intermediates[k]) == R.canon(want[k]), k


# ---- 4: the sparse kernel's tile decode ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sparse_want():
    """{name: full n_x x n_x matrices}: the restatement on the 192 rated rows as their own problem, scattered back; 1.0
    on the diagonal; zeros elsewhere.  A pair's result depends on its two rows alone."""
    case = sc.sparse_case()
    rated, n_x = case["rated"], sc.SPARSE_NX
    sub = np.searchsorted(rated, case["x"])
    out = {}
    for name in ("cosine", "msd"):
        small = E.NUMPY[name](len(rated), E.build_yr(sub, case["y"], case["r"]), 1, case["w"])
        full = {}
        for key, v in small.items():
            m = np.zeros((n_x, n_x), dtype=v.dtype)
            m[np.ix_(rated, rated)] = v
            full[key] = m
        full["sim"][np.arange(n_x), np.arange(n_x)] = 1.0
        out[name] = full
    return out


@pytest.mark.parametrize("name", ["cosine", "msd"])
def test_sparse_decode_of_1176_tiles(sparse_want, name):
    case = sc.sparse_case()
    n_x, n_y = sc.SPARSE_NX, sc.SPARSE_NY
    want = sparse_want[name]
    got = c_sparse(case["x"], case["y"], case["r"], case["w"], n_x, n_y, name, 1)
    assert set(got) == set(want) == ({"sim", "freq", "prods", "sqi", "sqj"} if name == "cosine" else {"sim", "freq", "sq_diff"})
    for key, v in got.items():                                           # every cell written
        assert v.shape == (n_x, n_x) and not (v == (ISENT if key == "freq" else SENT)).any(), key
    assert_same(got, want, (name, "restatement"))
    assert_same(got, c_dense(case["x"], case["y"], case["r"], case["w"], n_x, n_y, name, 1), (name, "dense kernel"))
