"""CPU tests around the sparse form of the EccenKNN similarity: the host rule that picks a form, the -form option of
main_rec.py, and the new symbols' place in the header and the ctypes table.  What the kernels compute is
tests/test_gpu_eccknn_sparse.py's business."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_choose_form_truth_table():
    from n2v_hip import eccknn
    lim = 1 << 31
    assert eccknn.MAX_DENSE == lim and eccknn.FORMS == ("auto", "dense", "sparse")
    inside, at, past = (6040, 3706), (1 << 16, 1 << 15), (1 << 16, (1 << 15) + 1)
    for n_x, n_y in (inside, at):
        assert eccknn.choose_form(n_x, n_y, "auto") == "dense"
        assert eccknn.choose_form(n_x, n_y, "dense") == "dense"
        assert eccknn.choose_form(n_x, n_y, "sparse") == "sparse"
    assert eccknn.choose_form(*past, "auto") == "sparse"
    assert eccknn.choose_form(*past, "sparse") == "sparse"
    with pytest.raises(ValueError, match="dense limit"):
        eccknn.choose_form(*past, "dense")
    assert eccknn.choose_form(40000, 5000000, "auto") == "sparse"          # the 30Music layout
    assert eccknn.choose_form(140000, 27000, "auto") == "sparse"           # MovieLens-20M
    # the limit is an argument: the rule, not the constant
    assert eccknn.choose_form(10, 10, "auto", limit=100) == "dense"
    assert eccknn.choose_form(10, 11, "auto", limit=100) == "sparse"
    with pytest.raises(ValueError, match="dense limit of 100 elements"):
        eccknn.choose_form(10, 11, "dense", limit=100)
    for bad in ("bogus", "", None, "Dense"):
        with pytest.raises(ValueError, match="allowed values"):
            eccknn.choose_form(10, 10, bad)


def test_eccenknn_validates_form_without_a_gpu():
    from n2v_hip import eccknn
    assert eccknn.EccenKNN(sim_options={"name": "msd"}).form == "auto"
    assert eccknn.EccenKNN(sim_options={"name": "cosine", "form": "sparse"}).form == "sparse"
    with pytest.raises(ValueError, match="bogus"):
        eccknn.EccenKNN(sim_options={"name": "msd", "form": "bogus"})


def test_main_rec_form_option():
    import main_rec
    assert main_rec.parse_args(["-input", "r.csv"]).form == "auto"
    for form in ("auto", "dense", "sparse"):
        assert main_rec.parse_args(["-input", "r.csv", "-form", form]).form == form
    with pytest.raises(SystemExit):
        main_rec.parse_args(["-input", "r.csv", "-form", "bogus"])
    assert "-form auto|dense|sparse" in main_rec.__doc__


def test_sparse_symbols_are_declared_and_bound():
    from n2v_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "n2v_sim.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(n2v_[a-z0-9_]+)\s*\(", hdr))
    new = {"n2v_eccknn_sparse_chunk", "n2v_eccknn_csr_check", "n2v_eccknn_sim_sparse"}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    # (that each binding has the header's parameters, type by type: tests/test_host_logic.py)
    for bit, macro in ((1, "N2V_ECCKNN_CSR_BAD_PTR"), (2, "N2V_ECCKNN_CSR_BAD_Y"), (4, "N2V_ECCKNN_CSR_UNSORTED")):
        assert re.search(r"#define %s %d\b" % (macro, bit), hdr)
    from n2v_hip import eccknn
    assert [b for b, _ in eccknn.CSR_BAD] == [1, 2, 4]
