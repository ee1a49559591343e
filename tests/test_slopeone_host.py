"""CPU tests of the SlopeOne predictor: the restatement tests/slopeone_reference.py against a table worked out by hand and
against a literal transcription of surprise's loops on seeded trainsets, proof that the case table of the GPU test sees
each of the restatement's deliberate errors, the constructor, the -algo slopeone flags of main_rec.py, the "no CPU
fallback" errors, the table limit and the four new C-ABI symbols.  No GPU."""
import os
import re

import numpy as np
import pytest

import eccknn_reference as E
import slopeone_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the toy of Lemire and Maclachlan's paper, in training order -------------------------------------------------------
#   u0: i0 = 5, i1 = 3          u1: i0 = 3, i1 = 4, i2 = 2          u2: i1 = 2, i2 = 5
U = [0, 1, 2, 0, 1, 1, 2]
I = [0, 0, 1, 1, 1, 2, 2]
R = [5.0, 3.0, 2.0, 3.0, 4.0, 2.0, 5.0]


def test_restatement_by_hand():
    m = S.fit(U, I, R, 3, 3)
    assert m["freq"].tolist() == [[2, 2, 1], [2, 3, 2], [1, 2, 2]]
    assert m["acc"].tolist() == [[0.0, 1.0, 1.0], [-1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]]
    assert m["dev"].tolist() == [[0.0, 0.5, 1.0], [-0.5, 0.0, -0.5], [-1.0, 0.5, 0.0]]
    assert m["mu"].tolist() == [4.0, 3.0, 3.5] and m["ur"][1] == [(0, 3.0), (1, 4.0), (2, 2.0)]
    assert S.estimate(m, 2, 0) == (3.5 + (0.5 + 1.0) / 2.0, 2, 0)       # ur[2] = [(1, 2), (2, 5)]: dev[0][1], then dev[0][2]
    assert S.estimate(m, 0, 2) == (4.0 + (-1.0 + 0.5) / 2.0, 2, 0)
    assert S.estimate(m, 0, 0) == (4.0 + (0.0 + 0.5) / 2.0, 2, 0)       # a rated item: the diagonal counts
    for u, i in ((-1, 0), (0, -1), (3, 0), (0, 3), (-1, -1)):
        assert S.estimate(m, u, i) == (0.0, 0, 1)
    # two items nobody co-rated: freq 0, dev NaN, and an estimate that can use nothing is the user's mean
    m = S.fit([0, 1], [0, 1], [2.0, 4.0], 2, 2)
    assert m["freq"].tolist() == [[1, 0], [0, 1]] and np.isnan(m["dev"][0, 1]) and np.isnan(m["dev"][1, 0])
    assert S.estimate(m, 0, 1) == (2.0, 0, 0) and S.estimate(m, 0, 0) == (2.0 + 0.0 / 1.0, 1, 0)
    # equal ratings: +0.0 above the diagonal, -0.0 below it; a mirror summed on its own would be +0.0 there too
    m = S.fit([0, 0], [0, 1], [3.0, 3.0], 1, 2)
    assert not np.signbit(m["dev"][0, 1]) and np.signbit(m["dev"][1, 0]) and not np.signbit(m["acc"][1, 0])
    assert not np.signbit(S.fit([0, 0], [0, 1], [3.0, 3.0], 1, 2, "mirror_summed")["dev"][1, 0])


@pytest.mark.parametrize("name", ["main", "grid-65-33", "grid-2-65", "grid-129-1", "small-64"])
def test_restatement_equals_surprises_loops_transcribed(name):
    case = dict(S.cases())[name]
    args = (case["u"], case["i"], case["r"], case["n_users"], case["n_items"])
    m, lit = S.fit(*args), S.literal_fit(*args)
    assert np.array_equal(m["freq"], lit[0]) and E.canon(m["dev"]) == E.canon(lit[1])
    assert m["mu"].tolist() == lit[2] or E.canon(m["mu"]) == E.canon(np.array(lit[2]))
    n_nan = 0
    for u in range(case["n_users"]):
        for i in range(case["n_items"]):
            got, want = S.estimate(m, u, i), S.literal_estimate(lit, u, i)
            assert got[2] == 0 and got[1] == want[1] and E.canon(np.array([got[0]])) == E.canon(np.array([want[0]])), (u, i)
            n_nan += got[0] != got[0]
    assert (n_nan > 0) == (name == "main")                         # the planted inf - inf, compared as NaN


def test_the_main_case_holds_what_it_claims():
    case = S.main_case()
    m = S.fit(case["u"], case["i"], case["r"], case["n_users"], case["n_items"])
    dev, freq = m["dev"], m["freq"]
    assert tuple(len(m["ur"][u]) for u in range(6)) == S.LIST_LENS
    for a, b in ((3, 7), (3, 100), (7, 100)):                      # one diagonal tile, and two tiles
        assert freq[a, b] > 0 and dev[a, b] == 0.0 and not np.signbit(dev[a, b]) and np.signbit(dev[b, a])
    assert 3 // S.TILE == 7 // S.TILE != 100 // S.TILE
    assert freq[129].max() == 0 and np.isnan(dev[129, :129]).all() and np.isnan(dev[:129, 129]).all() and dev[129, 129] == 0.0
    assert freq[10, 11] > 0 and np.isnan(dev[10, 11]) and np.isnan(dev[11, 10])
    assert freq.diagonal()[[129, 20, 22, 23, 24]].tolist() == [0, 1, S.SC - 1, S.SC, S.SC + 1]
    assert S.estimate(m, 9, 5) == (float(m["mu"][9]), 0, 0) and S.estimate(m, 9, 20)[1:] == (1, 0)
    n12 = len(m["ur"][12])
    assert n12 > 2 and S.estimate(m, 12, 5)[1] == n12 - 1
    assert (case["r"] == 0.0).any() and (case["r"] < 0).any() and np.isnan(S.estimate(m, 5, 10)[0])


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_the_case_table_catches_every_deliberate_error(mutant):
    seen_by = []
    for name, case in S.cases():
        if name.startswith("grid") and name != "grid-65-33":
            continue                                              # one grid case is enough here; the GPU test runs all
        base, changed = S.outputs(case), S.outputs(case, mutant)
        if any(base[k] != changed[k] for k in base):
            seen_by.append(name)
    assert seen_by, "no case of the table sees the mutant %s" % mutant


def test_rankings_of_the_restatement():
    m = S.fit(U, I, R, 3, 3)
    case = dict(seen=[{0, 1}, {0, 1, 2}, {1, 2}], n_items=3, mean=E.global_mean(R), scale=(1.0, 4.0))
    ranked = S.rankings(case, m, [0, 1, 2, -1])
    assert ranked[0] == [(2, 3.75)] and ranked[1] == [] and ranked[2] == [(0, 4.0)]      # 4.25 clipped
    assert ranked[3] == [(i, case["mean"]) for i in range(3)]                            # unknown: the training mean


# ---- the class and the flags ---------------------------------------------------------------------------------------------

def test_constructor_and_limits():
    from n2v_hip import eccknn, slopeone
    assert issubclass(slopeone.SlopeOne, eccknn.TopN) and slopeone.MAX_TABLE == 1 << 31
    for form in eccknn.FORMS:
        assert slopeone.SlopeOne(sim_options={"form": form}).form == form
    assert slopeone.SlopeOne().form == "auto"
    with pytest.raises(ValueError, match="form 'tiles'"):
        slopeone.SlopeOne(sim_options={"form": "tiles"})
    with pytest.raises(ValueError, match="no similarity"):
        slopeone.SlopeOne(sim_options={"name": "msd"})
    for text in ("surprise", "UNPINNED", "tests/slopeone_reference.py", "no CPU fallback"):
        assert text in slopeone.__doc__
    assert slopeone.check_items(46340) == 46340
    for bad in (46341, 0, 1 << 31):
        with pytest.raises(ValueError, match="n_items"):
            slopeone.check_items(bad)


def test_no_cpu_fallback_and_the_table_limit_comes_first(monkeypatch):
    import torch
    from n2v_hip import eccknn, slopeone
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ts = eccknn.Trainset.from_ratings(U, I, R)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        slopeone.SlopeOne().fit(ts)
    ok = torch.zeros((3, 3), dtype=torch.float64), torch.zeros((3, 3), dtype=torch.int32)
    ur = tuple(torch.as_tensor(a) for a in ts.ur)
    q = torch.zeros(1, dtype=torch.int32)
    for call in (lambda: slopeone.deviations(torch.zeros((3, 3), dtype=torch.float64), torch.zeros((3, 3), dtype=torch.uint8)),
                 lambda: slopeone.deviations_sparse(tuple(torch.as_tensor(a) for a in ts.ir), 3),
                 lambda: slopeone.estimate_batch(ok[0], ok[1], ur, torch.zeros(3, dtype=torch.float64), q, q),
                 lambda: slopeone.top_n(ok[0], ok[1], ur, torch.zeros(3, dtype=torch.float64), None, 3.0, (1, 5), 10)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="outside"):              # the option checks still come first
        slopeone.top_n(ok[0], ok[1], ur, torch.zeros(3, dtype=torch.float64), None, 3.0, (1, 5), 257)

    # n_items^2 > 2^31: a ValueError from host arithmetic, before the GPU is asked for and before anything is allocated
    class Wide:
        n_items, n_users = 46341, 2
    with pytest.raises(ValueError, match="46341"):
        slopeone.SlopeOne(sim_options={"form": "sparse"}).fit(Wide)
    wide = torch.empty((1, 46341), dtype=torch.float64, device="meta")
    with pytest.raises(ValueError, match="46341"):
        slopeone.deviations(wide, wide)
    with pytest.raises(ValueError, match="exceeds the dense limit"):
        slopeone.SlopeOne(sim_options={"form": "dense"}).fit(type("T", (), dict(n_items=40000, n_users=60000)))


def test_main_rec_flags(capsys):
    import main_rec
    a = main_rec.parse_args("-input r.csv -algo slopeone".split())
    assert (a.algo, a.form, a.topn, a.cv, a.test_ratio, a.seed) == ("slopeone", "auto", None, 0, 0.2, 0)
    a = main_rec.parse_args("-input r.csv -algo slopeone -form sparse -topn 10 -threshold 4 -save-recs o.csv -cv 3 "
                            "-test-ratio 0.3 -seed 7".split())
    assert (a.form, a.topn, a.threshold, a.save_recs, a.cv, a.test_ratio, a.seed) == ("sparse", 10, 4.0, "o.csv", 3, 0.3, 7)
    for flag in ("-k 20", "-mink 2", "-sim msd", "-shrinkage 50", "-weights w.csv", "-mode ir", "-item-based", "-factors 8",
                 "-epochs 3", "-lr 0.1", "-reg 0.1", "-strata 2", "-unbiased"):
        with pytest.raises(SystemExit):
            main_rec.parse_args(("-input r.csv -algo slopeone %s" % flag).split())
        assert "%s does not go with -algo slopeone" % flag.split()[0] in capsys.readouterr().err, flag
    with pytest.raises(SystemExit):
        main_rec.parse_args("-input r.csv -algo bogus".split())
    assert "slopeone" in capsys.readouterr().err and "-algo slopeone" in main_rec.__doc__
    # the other algorithms keep -shrinkage's default
    assert main_rec.parse_args("-input r.csv -algo knn".split()).shrinkage == 100
    assert main_rec.parse_args("-input r.csv -algo knn -shrinkage 50".split()).shrinkage == 50.0


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------

NEW = {"n2v_slopeone_dev": 8, "n2v_slopeone_dev_sparse": 10, "n2v_slopeone_estimate": 15, "n2v_slopeone_topn": 23}


def test_symbols_are_declared_bound_and_exported():
    from n2v_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    section = hdr[hdr.index("SlopeOne: surprise's"):hdr.index("int n2v_slopeone_dev(")]
    assert "UNPINNED" in section and "tests/slopeone_reference.py" in section and "UNPINNED" in S.__doc__
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(n2v_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SIGNATURES)
    for name, count in NEW.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(",") + 1 == count, name
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW)
    assert "n2v_slopeone.hip" in open(os.path.join(ROOT, "node2vec-by-ecc_amd", "csrc", "Makefile")).read()


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Every call below returns before the first HIP call: no GPU is needed (and none is touched)."""
    from n2v_hip import _lib
    lib = _lib.load()
    one = 8     # a non-NULL "pointer" that is never dereferenced: each call fails its argument checks first

    def dense(n_items=5, n_users=7, inp=one, dev=one, freq=one):
        return lib.n2v_slopeone_dev(inp, one, n_items, n_users, dev, freq, None, None)

    def sparse(n_items=5, n_users=7, n=4, ptr=one, ys=one, dev=one, freq=one):
        return lib.n2v_slopeone_dev_sparse(ptr, ys, one, n_items, n_users, n, dev, freq, None, None)

    def est(n_items=5, n_users=7, n=4, n_q=3, dev=one, freq=one, mu=one, out=one):
        return lib.n2v_slopeone_estimate(dev, freq, n_items, one, one, n_users, n, mu, one, one, n_q, out, one, one, None)

    def top(n_items=5, n_users=7, n=4, n_owners=3, top_n=10, segments=0, dev=one, items=one):
        return lib.n2v_slopeone_topn(dev, one, n_items, one, one, n_users, n, one, one, one, 4, one, n_owners, 3.0, 1.0, 5.0,
                                     top_n, segments, one, one, items, one, None)

    for call, kw, msg in ((dense, dict(n_items=0), "n_items=0"), (dense, dict(n_users=0), "n_users=0"),
                          (dense, dict(n_items=46341, n_users=1), "n_items^2"), (dense, dict(n_items=1 << 40), "n_items^2"),
                          (dense, dict(n_items=40000, n_users=60000), "dense limit"), (dense, dict(inp=None), "null"),
                          (dense, dict(dev=None), "null"), (dense, dict(freq=None), "null"),
                          (sparse, dict(n_items=0), "n_items=0"), (sparse, dict(n_users=1 << 31), "n_users"),
                          (sparse, dict(n=-1), "n=-1"), (sparse, dict(n_items=46341), "n_items^2"), (sparse, dict(ptr=None), "null"),
                          (sparse, dict(ys=None), "null"), (sparse, dict(freq=None), "null"),
                          (est, dict(n_q=0), "n_q"), (est, dict(n_items=0), "n_items=0"), (est, dict(n_items=46341), "n_items^2"),
                          (est, dict(n=-1), "n=-1"), (est, dict(dev=None), "null"), (est, dict(freq=None), "null"),
                          (est, dict(mu=None), "null"), (est, dict(out=None), "null"),
                          (top, dict(n_items=46341), "n_items^2"), (top, dict(n_owners=0), "n_owners"), (top, dict(top_n=257), "top_n 257"),
                          (top, dict(top_n=0), "top_n 0"), (top, dict(segments=65), "segments"), (top, dict(dev=None), "null"),
                          (top, dict(items=None), "null")):
        assert call(**kw) != 0, kw
        assert msg in lib.n2v_last_error().decode(), (kw, lib.n2v_last_error())
