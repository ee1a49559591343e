"""CPU tests around the fused k-NN kernel (csrc/n2v_knn.hip) and n2v_hip/neighbors.py: the ranking restatement against a
brute-force sort, the case tables of tests/test_gpu_knn.py against the borders they claim, the C-ABI surface and its
argument checks (no GPU is touched), the host logic of most_similar, and the separation of the fp64 sanity data."""
import functools
import os
import re

import numpy as np
import pytest

import knn_cases as K
import knn_reference as R
from helpers import ROOT

CSRC = os.path.join(ROOT, "node2vec-by-ecc_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the restatement
def _brute(row, k, exclude):
    """Python's sort with an explicit comparison: NaN below everything, -0.0 == +0.0, equal scores by position."""
    def cmp(a, b):
        (pa, sa), (pb, sb) = a, b
        na, nb = sa != sa, sb != sb
        if na != nb:
            return 1 if na else -1
        if not na and sa != sb:
            return -1 if sa > sb else 1
        return pa - pb
    cand = [(p, float(s)) for p, s in enumerate(row) if p != exclude]
    top = sorted(cand, key=functools.cmp_to_key(cmp))[:k]
    return [p for p, _ in top] + [-1] * (k - len(top)), [s for _, s in top] + [float("nan")] * (k - len(top))


def test_rank_restatement_equals_a_brute_force_sort():
    rs = np.random.RandomState(3)
    specials = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, 1.5, -1.5, np.float32(1e-45), -np.float32(1e-45)], np.float32)
    for trial in range(40):
        n = int(rs.randint(1, 40))
        row = specials[rs.randint(0, len(specials), size=n)]
        if trial % 3 == 0:
            row = np.where(rs.random_sample(n) < 0.5, row, rs.normal(size=n).astype(np.float32)).astype(np.float32)
        for k in (1, 2, n, n + 3):
            for exclude in (None, 0, n - 1, n + 5, -1):
                cols, vals = R.rank(row, k, exclude)
                bc, bv = _brute(row, k, exclude)
                assert cols.tolist() == bc, (row, k, exclude)
                assert R.same(cols, vals, np.array(bc, np.int32), np.array(bv, np.float32))
    # the properties by hand: NaN last, the zeros tie (position decides), duplicates in position order
    cols, vals = R.rank(np.array([0.5, np.nan, 0.5, -1.0, 2.0, -0.0, 0.0], np.float32), 8)
    assert cols.tolist() == [4, 0, 2, 5, 6, 3, 1, -1] and np.signbit(vals[3]) and not np.signbit(vals[4])
    assert np.isnan(vals[6]) and np.isnan(vals[7])
    cols, _ = R.rank(np.array([1.0], np.float32), 2, exclude=0)
    assert cols.tolist() == [-1, -1]
    assert not R.same([1, 2], [1.0, 2.0], [1, 2], [1.0, np.float32(2.0000002)]) and R.same([1], [np.nan], [1], [-np.nan])
    assert not R.same([0], [0.0], [0], [-0.0])


# ------------------------------------------------------------------------------------------------ the case tables
def test_case_tables_cover_the_borders_of_the_kernel():
    t = K.CASES
    assert 55 <= len(t) <= 70 and len(set(t)) == len(t)
    assert {c[0] for c in t} == {1, 31, 32, 33, 64, 127, 128, 129, 257}
    assert {c[1] for c in t} == {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385, 1000}
    assert {c[2] for c in t} == {32, 64, 96, 160, 512}
    assert {c[3] for c in t} == {1, 2, 10, 63, 64, 65, 128, 255, 256}
    assert {c[4] for c in t} == {0, 1, 2, 3, "max", "more"}
    assert {c[5] for c in t} == {"null", "arange", "minus1", "beyond", "col0", "col63", "col64", "col127", "col128", "last"}
    src = open(os.path.join(CSRC, "n2v_knn.hip")).read() + open(os.path.join(CSRC, "n2v_sim_tile.h")).read()
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    for pattern, value in ((r"SIM_MT = (\d+)", K.TILE), (r"MAX_SEG = (\d+)", K.MAX_SEG), (r"SIM_MKC = (\d+)", 16), (r"SB = (\d+)", 32)):
        assert int(re.search(pattern, src).group(1)) == value, pattern
    assert int(re.search(r"#define N2V_SIM_KNN_MAX_K (\d+)", hdr).group(1)) == K.MAX_K == max(K.KS)
    all_empty = more_than_tiles = k_above = dup_seg = 0
    for i in range(len(t)):
        c = K.int_case(i)
        assert c["Q"].shape == (c["n_q"], c["dpad"]) and c["B"].shape == (c["n_cols"], c["dpad"])
        for M in (c["Q"], c["B"]):
            assert np.array_equal(M, np.round(M)) and np.abs(M).max() <= 2 and 4 * c["dpad"] < 2 ** 24
        assert 0 <= c["n_seg"] <= K.MAX_SEG and 1 <= c["k"] <= K.MAX_K
        ex = c["exclude"]
        hit = np.zeros(c["n_q"], bool) if ex is None else (ex >= 0) & (ex < c["n_cols"])
        if t[i][5] in ("null", "minus1", "beyond"):
            assert not hit.any()
        if t[i][5].startswith("col") or t[i][5] == "last":
            assert hit.all()
        cand = c["n_cols"] - hit.astype(int)
        all_empty += int((cand == 0).all())
        k_above += int((c["k"] > cand).any())
        more_than_tiles += int(c["n_seg"] > K.n_tiles(c["n_cols"]))
        for a, b in c["dups"]:
            assert np.array_equal(c["B"][a], c["B"][b]) and b == a + 1
        own = K.segment_borders(c["n_cols"], max(1, c["n_seg"]))
        dup_seg += int(bool(own) and (own[0] - 1, own[0]) in c["dups"])
        if c["n_cols"] > 128:
            assert (63, 64) in c["dups"] and (127, 128) in c["dups"]
        S = K.int_scores(c)
        assert S.dtype == np.float32 and np.array_equal(S, np.round(S)) and np.abs(S).max() <= 4 * 512
    assert all_empty >= 1 and k_above >= 5 and more_than_tiles >= 8 and dup_seg >= 8
    # ties by the thousand: in the largest case the scores of a row take far fewer values than there are columns
    S = K.int_scores(K.int_case(3))
    assert S.shape == (257, 1000) and max(len(np.unique(r)) for r in S) < 400
    assert len(K.SEG_CASES) >= 4 and all(K.n_tiles(t[i][1]) >= 3 for i in K.SEG_CASES)
    # real operands: every dpad of the table and the song2vec one (128), the NaN and the zero row inside every B, one case with k above the non-NaN candidates
    assert {-(-c[2] // 32) * 32 for c in K.REAL_CASES} == {32, 64, 96, 128, 160, 512}
    for i, rc in enumerate(K.REAL_CASES):
        c = K.real_case(i)
        assert np.isnan(c["b"][K.REAL_NAN_ROW]).sum() == 1 and (c["b"][K.REAL_ZERO_ROW] == 0).all()
        assert np.isfinite(np.delete(c["b"], K.REAL_NAN_ROW, axis=0)).all() and np.isfinite(c["q"]).all()
    assert any(c[3] > c[1] - 1 for c in K.REAL_CASES) and any(c[3] <= 256 < c[1] for c in K.REAL_CASES)


# ------------------------------------------------------------------------------------------------ the C-ABI
NEW = ("n2v_sim_knn_max_k", "n2v_sim_knn_max_seg", "n2v_sim_knn_scratch", "n2v_sim_knn")


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes
    from n2v_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "n2v_sim.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, "%s is not declared" % name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params), name
        assert hasattr(lib, name), "libn2v_hip.so does not export %s" % name
    L = _lib.load()
    assert L.n2v_sim_knn_max_k() == 256 and L.n2v_sim_knn_max_seg() == 32
    # bytes of 2 * n_seg lists of k (score, position) pairs a query; refusals are -1
    assert L.n2v_sim_knn_scratch(100, 10, 3) == 100 * 6 * 10 * 8 and L.n2v_sim_knn_scratch(0, 1, 1) == 0
    assert L.n2v_sim_knn_scratch(1, 256, 32) == 64 * 256 * 8
    for bad in ((-1, 1, 1), (1, 0, 1), (1, 257, 1), (1, 1, -1), (1, 1, 33)):
        assert L.n2v_sim_knn_scratch(*bad) == -1, bad
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "n2v_knn.hip" in mk and "n2v_sim_tile.h" in mk
    # one tile loop: the MFMA chain is written once, in the shared header, and both kernels call it
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("n2v_sim.hip", "n2v_knn.hip", "n2v_sim_tile.h")}
    assert {f: s.count("__builtin_amdgcn_mfma_f32_32x32x2f32(") for f, s in src.items()} == \
        {"n2v_sim.hip": 0, "n2v_knn.hip": 0, "n2v_sim_tile.h": 4}
    assert src["n2v_sim.hip"].count("n2v::sim_mfma_tile(") == 1 and src["n2v_knn.hip"].count("n2v::sim_mfma_tile(") == 1
    assert not re.findall(r"hipLaunchKernelGGL\(\(?sim_", src["n2v_knn.hip"])


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Every call below returns before the first HIP call: no GPU is needed (and none is touched)."""
    from n2v_hip import _lib
    lib = _lib.load()
    p = 64      # a non-NULL, 16-byte aligned "pointer" that is never dereferenced: each call fails its checks first

    def knn(Q=p, n_q=3, B=p, n_cols=5, dpad=32, method=0, exclude=None, k=2, n_seg=1, scratch=p, cols=p, vals=p):
        return lib.n2v_sim_knn(Q, n_q, B, n_cols, dpad, method, exclude, k, n_seg, scratch, cols, vals, None)

    for kw, msg in ((dict(method=2), "not a dot product"), (dict(method=-1), "not a dot product"), (dict(method=3), "not a dot product"),
                    (dict(k=0), "k 0 outside"), (dict(k=257), "k 257 outside"), (dict(k=-1), "outside"),
                    (dict(n_q=-1), "bad sizes"), (dict(n_cols=-1), "bad sizes"), (dict(dpad=16), "bad sizes"),
                    (dict(dpad=0), "bad sizes"), (dict(dpad=48), "bad sizes"), (dict(n_cols=2 ** 31), "too many columns"),
                    (dict(n_seg=-1), "n_seg"), (dict(n_seg=33), "n_seg"),
                    (dict(Q=p + 8), "16-byte aligned"), (dict(B=p + 4), "16-byte aligned"), (dict(scratch=p + 2), "4-byte aligned"),
                    (dict(Q=None), "null pointer"), (dict(B=None), "null pointer"), (dict(scratch=None), "null pointer"),
                    (dict(cols=None), "null pointer"), (dict(vals=None), "null pointer")):
        assert knn(**kw) == -1, kw
        assert msg in lib.n2v_last_error().decode(), (kw, lib.n2v_last_error())
    # nothing to do is no error, and needs no pointer
    assert knn(n_q=0, Q=None, B=None, scratch=None, cols=None, vals=None) == 0


# ------------------------------------------------------------------------------------------------ most_similar's host logic
def test_query_formation_on_hand_computed_vectors():
    from n2v_hip import neighbors as N
    a, b, c = np.array([1.0, 0.0, 0.5], np.float32), np.array([0.0, 2.0, 0.25], np.float32), np.array([0.5, 0.5, 0.5], np.float32)
    assert N.mean_query([(1.0, a)]).tolist() == [1.0, 0.0, 0.5]
    assert N.mean_query([(1.0, a), (1.0, b), (-1.0, c)]).tolist() == [np.float32(0.5) / np.float32(3), np.float32(1.5) / np.float32(3), np.float32(0.25) / np.float32(3)]
    assert N.mean_query([(1.0, a), (1.0, b), (-1.0, c)]).dtype == np.float32
    # float32 throughout and in list order: (big + 1) - big loses the 1, big - big + 1 would not
    big, one = np.array([2.0 ** 24], np.float32), np.array([1.0], np.float32)
    assert N.mean_query([(1.0, big), (1.0, one), (-1.0, big)]).tolist() == [0.0]
    assert N.mean_query([(1.0, big), (-1.0, big), (1.0, one)]).tolist() == [np.float32(1) / np.float32(3)]
    rs = np.random.RandomState(0)
    rows = [rs.normal(size=7).astype(np.float32) for _ in range(4)]
    w = [1.0, 1.0, -1.0, -1.0]
    assert np.array_equal(N.mean_query(list(zip(w, rows))), R.mean_query(w, rows))
    # positives then negatives; a bare word or vector is one positive; nothing is a ValueError
    assert N.query_terms("x", None) == [(1.0, "x")] and N.query_terms(["x", "y"], ["z"]) == [(1.0, "x"), (1.0, "y"), (-1.0, "z")]
    t = N.query_terms(a, ("z",))
    assert len(t) == 2 and t[0][1] is a and t[1] == (-1.0, "z")
    with pytest.raises(ValueError, match="no input"):
        N.query_terms(None, [])
    # the filter: inputs and empty entries leave, then the cut
    labels = ["a", "b", "c", "d", "e"]
    got = R.drop_inputs(np.array([2, 0, 4, -1]), np.array([0.9, 0.8, 0.7, np.nan], np.float32), [0], 5, labels)
    assert got == [("c", float(np.float32(0.9))), ("e", float(np.float32(0.7)))]
    assert R.most_similar(np.array([0.1, 0.9, 0.5, 0.9, np.nan], np.float32), labels, [1], 2) == [("d", float(np.float32(0.9))), ("c", 0.5)]


def test_auto_path_reproduces_the_measured_decisions():
    """path="auto" is a cost estimate with three measured constants; it must decide every shape that was measured on
    an MI355X (256 CUs) the way the measurement went, and never take the fused kernel above its k."""
    from n2v_hip import neighbors as N
    measured = [(5000, 10, 128, "block"), (20000, 10, 64, "block"), (30000, 10, 128, "block"), (50000, 10, 128, "block"),
                (70000, 10, 128, "fused"), (100000, 10, 128, "fused"), (799000, 10, 128, "fused"),
                (50000, 100, 128, "block"), (100000, 100, 128, "block")]
    for n, k, dpad, want in measured:
        assert N.auto_path(n, n, k, dpad, 256) == want, (n, k)
    assert N.auto_path(10 ** 7, 10 ** 7, 257, 128) == "block" and N.auto_path(10 ** 7, 10 ** 7, 256, 128) == "fused"
    assert N.auto_path(1, 0, 1, 32) == "block"


def test_most_similar_argument_errors_and_no_cpu_fallback(monkeypatch):
    import torch
    from n2v_hip import neighbors as N
    from n2v_hip.sgns import KeyedVectors
    from n2v_hip.word2vec import LabelKeyedVectors
    rs = np.random.RandomState(1)
    kv = KeyedVectors(np.arange(5), np.array([5, 4, 3, 2, 1]), rs.normal(size=(5, 4)).astype(np.float32))
    lkv = LabelKeyedVectors(["a", "b", "c"], [3, 2, 1], rs.normal(size=(3, 4)).astype(np.float32))
    for v in (kv, lkv):
        for name in ("init_sims", "most_similar", "similar_by_word", "similar_by_vector"):
            assert callable(getattr(v, name))
    with pytest.raises(KeyError):
        kv.most_similar(positive=["nobody"])
    with pytest.raises(KeyError):
        lkv.similar_by_word("z")
    with pytest.raises(ValueError, match="no input"):
        kv.most_similar()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for call in (lambda: kv.most_similar(positive=["0"]), lambda: lkv.similar_by_word("a"),
                 lambda: kv.similar_by_vector(np.ones(4, np.float32)), lambda: kv.init_sims()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.knn(torch.zeros(3, 4), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.find_similar_users(kv, 1.0, target="0")


def test_main_ecc_similar_flags_are_checked_by_the_parser(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "node2vec-by-ecc_amd"))
    import main_ecc
    a = main_ecc.parse_args(["-input", "r.csv", "-out", str(tmp_path)])
    assert a.similar_emb is None and a.similar_ratio is None and a.similar_name == "cosine_onetenth"
    a = main_ecc.parse_args(["-input", "r.csv", "-out", str(tmp_path), "-similar-emb", "e.emb", "-similar-ratio", "0.1",
                             "-similar-target", "7"])
    assert (a.similar_emb, a.similar_ratio, a.similar_target) == ("e.emb", 0.1, "7")
    for argv in (["-similar-emb", "e.emb"], ["-similar-ratio", "0.1"]):
        with pytest.raises(SystemExit):
            main_ecc.parse_args(["-input", "r.csv", "-out", str(tmp_path)] + argv)
    with pytest.raises(SystemExit):
        main_ecc.parse_args(["-input", "r.csv", "-save-bins", "b", "-similar-emb", "e.emb", "-similar-ratio", "0.1"])


# ------------------------------------------------------------------------------------------------ the fp64 sanity data
def test_arc_data_is_separated_by_far_more_than_the_fp32_error():
    import sim_reference as S
    vec, query = R.arc_data()
    assert vec.shape == (R.ARC_N, R.ARC_D) and vec.dtype == np.float32 and query.shape == (1, R.ARC_D)
    cos = np.sort(R.arc_cosines(vec, query))[::-1]
    gaps = cos[:-1] - cos[1:]
    assert gaps.min() >= R.ARC_GAP, gaps.min()
    # 10^-3 is over 100 times the fp32 bound sim_reference derives for a dot product of unit rows at dpad 128 (sum |a||b|
    # <= 1), and the smallest gap is more than twice that bound plus the two normalisations' (d + 3 roundings each): no
    # pair of neighbours can change places
    dot = float(S.gamma(S.dpad_of(R.ARC_D)))
    assert S.dpad_of(R.ARC_D) == 128 and 100 * dot < R.ARC_GAP, dot
    assert 2 * (dot + 2 * float(S.gamma(R.ARC_D + 3))) < gaps.min()
    assert len(set(np.argsort(-R.arc_cosines(vec, query)).tolist())) == R.ARC_N
