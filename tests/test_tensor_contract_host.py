"""The device-tensor contract of the rating modules, the part that needs no GPU: the table of tests/tensor_contract_cases.py
is complete, the one helper every wrapper hands its tensors through (n2v_hip._lib.tensor) refuses what it must, with and
without `python -O`, and the NoLaunch proxy lets through exactly the entry points that take no pointer."""
import fnmatch
import importlib
import inspect
import os
import subprocess
import sys

import pytest

import tensor_contract_cases as TC


# ---- completeness -----------------------------------------------------------------------------------------------------

def test_the_cases_load_without_torch():
    code = "import sys; sys.path.insert(0, %r); import tensor_contract_cases as TC; " \
           "assert 'torch' not in sys.modules and 'n2v_hip' not in sys.modules; print(len(TC.malformed_rows()))"
    out = subprocess.run([sys.executable, "-c", code % os.path.dirname(os.path.abspath(__file__))], capture_output=True, text=True)
    assert out.returncode == 0 and int(out.stdout) > 500, out.stderr


def test_every_function_that_hands_a_tensor_to_the_library_is_in_the_table():
    found = {}
    for short in TC.MODULES:
        found.update(TC.functions_that_hand_over(importlib.import_module("n2v_hip." + short)))
    assert len(found) >= 30 and {"eccknn.predict", "svd.Blocks.__init__", "nmf.epoch"} <= set(found)    # the search itself works
    assert sorted(set(found) - set(TC.TABLE)) == [], "a wrapper outside the contract's table"
    for name, row in TC.TABLE.items():
        mod, label = name.split(".", 1)
        obj = importlib.import_module("n2v_hip." + mod)
        for part in label.split("."):
            obj = getattr(obj, part)                                # a row names something that exists
        params = inspect.signature(obj).parameters
        for arg in row["args"]:
            assert TC.root(arg.path) in params, (name, arg.path)
            assert arg.dtype in ("int32", "int64", "float64", "uint8") and arg.rank in (1, 2), (name, arg)
            assert set(arg.flags) <= set("owcf")
        for via in row.get("via", ()):
            assert via in TC.PUBLIC, (name, via)
        assert row["args"] or row.get("note"), name                 # a row without tensors says why
    assert not [n for n in TC.PUBLIC if n.split(".")[-1].startswith("_") and not n.endswith("__init__")]
    # what the issue names as written in place is marked so
    written = {(n, a.path) for n in TC.PUBLIC for a in TC.TABLE[n]["args"] if "w" in a.flags}
    assert written == {("svd.epoch", p) for p in ("bu", "bi", "pu", "qi")} | {("nmf.epoch", "pu_out"), ("nmf.epoch", "qi_out")} \
        | {("coclustering.assign", "cltr_u"), ("coclustering.assign", "cltr_i")}


def test_the_malformed_rows_cover_every_tensor_argument():
    rows = TC.malformed_rows()
    assert len(rows) == len(set(rows))
    for name in TC.PUBLIC:
        for arg in TC.TABLE[name]["args"]:
            kinds = {m for n, p, m in rows if (n, p) == (name, arg.path)}
            if "c" in arg.flags:
                assert not kinds
                continue
            assert {"dtype", "cpu", "strided", "other_device"} <= kinds, (name, arg.path)
            assert ("none" in kinds) == ("o" not in arg.flags) and ("longer" in kinds) == ("shorter" in kinds) == (arg.tie is not None)
    tied = {TC.root(p) for n, p, m in rows if m == "longer"}
    assert {"w", "qx", "qy", "bu", "bi", "pu", "qi", "seen", "lists", "yr", "avgs", "mask", "r_true", "cltr_u", "user_mean"} <= tied


# ---- the helper alone --------------------------------------------------------------------------------------------------------

def test_the_helper_returns_the_pointer_or_names_what_is_wrong():
    import torch
    from n2v_hip import _lib
    cpu = torch.device("cpu")
    ok = torch.arange(6, dtype=torch.int32)
    assert _lib.tensor("mod.fn", "qx", ok, torch.int32, cpu) == ok.data_ptr()
    assert _lib.tensor("mod.fn", "qx", ok, torch.int32, cpu, 6) == ok.data_ptr()
    assert _lib.tensor("mod.fn", "qx", ok, torch.int32, cpu, (None,)) == ok.data_ptr()
    two = torch.zeros((3, 4), dtype=torch.float64)
    assert _lib.tensor("mod.fn", "pu", two, torch.float64, cpu, (3, None)) == two.data_ptr()
    assert _lib.tensor("mod.fn", "pu", two, torch.float64, cpu, (None, 4)) == two.data_ptr()
    carved = torch.zeros(20, dtype=torch.float64)[3:9]
    assert _lib.tensor("mod.fn", "w", carved, torch.float64, cpu, 6) == carved.data_ptr()      # an offset view is contiguous
    empty = torch.zeros(0, dtype=torch.float64)
    assert _lib.tensor("mod.fn", "w", empty, torch.float64, cpu, 0) == empty.data_ptr()
    assert _lib.tensor("mod.fn", "w", None, torch.float64, cpu, 6, optional=True) is None
    bad = [("qx", torch.arange(6), torch.int32, None),                                 # torch's default integer
           ("qx", ok.to(torch.int64), torch.int32, None), ("ptr", ok, torch.int64, None),
           ("w", torch.zeros(6, dtype=torch.float32), torch.float64, None), ("mask", ok, torch.uint8, None),
           ("mask", torch.zeros(6, dtype=torch.bool), torch.uint8, None),             # bool has uint8's bytes and is refused
           ("qx", torch.arange(12, dtype=torch.int32)[::2], torch.int32, None),
           ("pu", two.t(), torch.float64, None), ("pu", two.t().contiguous().t(), torch.float64, (3, 4)),
           ("qx", ok, torch.int32, 5), ("qx", ok, torch.int32, 7), ("qx", ok, torch.int32, (None, None)),
           ("qx", ok.view(6, 1), torch.int32, 6), ("qx", ok.view(6, 1), torch.int32, (None,)),
           ("pu", two, torch.float64, (4, 3)), ("pu", two, torch.float64, (3, 5)), ("pu", two.view(-1), torch.float64, (3, 4)),
           ("pu", two, torch.float64, 12), ("w", None, torch.float64, 6)]
    for name, t, dtype, shape in bad:
        with pytest.raises(ValueError, match=r"^mod\.fn: %s\b" % name):
            _lib.tensor("mod.fn", name, t, dtype, cpu, shape)
    with pytest.raises(ValueError, match=r"^mod\.fn: qx\b.* on meta"):                 # another device than the call's
        _lib.tensor("mod.fn", "qx", torch.empty(6, dtype=torch.int32, device="meta"), torch.int32, cpu)
    for junk in ([3, 1, 2], 7, "qx", (ok,), __import__("numpy").arange(6, dtype="int32")):
        with pytest.raises(TypeError, match=r"^mod\.fn: qx\b"):
            _lib.tensor("mod.fn", "qx", junk, torch.int32, cpu, optional=True)
        with pytest.raises(TypeError, match=r"^mod\.fn: qx\b"):
            _lib.call_device("mod.fn", "qx", junk)
    # the device of a call is a GPU's: a CPU tensor's address never reaches a kernel
    for t in (ok, torch.empty(6, device="meta")):
        with pytest.raises(ValueError, match=r"^mod\.fn: sim\b"):
            _lib.call_device("mod.fn", "sim", t)
    with pytest.raises(ValueError, match=r"^mod\.fn: sim is required"):
        _lib.call_device("mod.fn", "sim", None)
    # ptr(), for tensors a wrapper allocated itself: a ValueError, not an assert
    assert _lib.ptr(None) is None and _lib.ptr(ok) == ok.data_ptr()
    with pytest.raises(ValueError, match="non-contiguous"):
        _lib.ptr(two.t())


def test_the_helper_launches_and_synchronises_nothing():
    """It reads dtype, device, dim(), shape, numel() and is_contiguous() alone: a meta tensor has nothing else to read, and
    a forbidden read (item(), min(), cpu(), data of any kind) raises on it."""
    import torch
    from n2v_hip import _lib
    meta = torch.device("meta")
    t = torch.empty((5, 3), dtype=torch.float64, device=meta)
    _lib.tensor("mod.fn", "pu", t, torch.float64, meta, (5, None))
    for shape, dtype in (((5, 4), torch.float64), ((5, 3), torch.float32), (15, torch.float64)):
        with pytest.raises(ValueError, match=r"^mod\.fn: pu\b"):
            _lib.tensor("mod.fn", "pu", t, dtype, meta, shape)
    source = inspect.getsource(_lib.tensor) + inspect.getsource(_lib.call_device)
    for word in (".item(", ".min(", ".max(", ".cpu(", ".any(", ".all(", ".tolist(", "synchronize"):
        assert word not in source, word


def test_the_helper_is_the_same_under_python_O():
    script = ("import torch; from n2v_hip import _lib; c = torch.device('cpu'); t = torch.arange(6)\n"
              "for f in (lambda: _lib.tensor('f', 'qx', t, torch.int32, c), lambda: _lib.ptr(t[::2]), lambda: _lib.call_device('f', 'qx', t)):\n"
              "    try: f(); print('accepted')\n    except ValueError as e: print('ValueError', e)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "node2vec-by-ecc_amd")] + sys.path))
    plain, optimised = (subprocess.run([sys.executable] + flag + ["-c", script + "print(__debug__)"], capture_output=True,
                                       text=True, env=env) for flag in ([], ["-O"]))
    assert plain.returncode == 0 and optimised.returncode == 0, plain.stderr + optimised.stderr
    assert plain.stdout.splitlines()[-1] == "True" and optimised.stdout.splitlines()[-1] == "False"
    assert plain.stdout.splitlines()[:-1] == optimised.stdout.splitlines()[:-1]
    lines = plain.stdout.splitlines()[:-1]
    assert len(lines) == 3 and all(line.startswith("ValueError") for line in lines), lines
    assert "f: qx" in lines[0] and "non-contiguous" in lines[1] and "f: qx" in lines[2]


# ---- the proxy ---------------------------------------------------------------------------------------------------------------

def test_the_proxy_lets_through_exactly_the_pointer_free_entry_points():
    from n2v_hip import _lib
    passes = TC.pass_through(_lib.SIGNATURES)
    free = sorted(name for name, (_, args) in _lib.SIGNATURES.items() if not any(a is _lib.C.c_void_p for a in args))
    assert passes == free and 10 <= len(passes) < len(_lib.SIGNATURES) // 4
    for name in passes:                                             # integers in, a constant or a text out: no memory is named
        res, args = _lib.SIGNATURES[name]
        assert all(a in (_lib.C.c_int64, _lib.C.c_int32) for a in args) and res is not _lib.C.c_void_p, name
    for pattern in ("n2v_*_max_*", "n2v_topn_segments", "n2v_*_scratch", "n2v_abi_version", "n2v_last_error"):
        hits = fnmatch.filter(_lib.SIGNATURES, pattern)
        assert hits and set(hits) <= set(passes), pattern
    for name in ("n2v_eccknn_csr_check", "n2v_svd_blocks_check", "n2v_nmf_lists_check", "n2v_eccknn_estimate", "n2v_eccknn_predict",
                 "n2v_svd_epoch", "n2v_cocl_assign", "n2v_slopeone_topn"):
        assert name not in passes

    class Lib:                                                      # stands for the loaded library
        def __getattr__(self, name):
            return lambda *a: ("real", name, a)
    proxy = TC.NoLaunch(Lib(), _lib.SIGNATURES)
    assert proxy.n2v_topn_segments(3, 4) == ("real", "n2v_topn_segments", (3, 4)) and proxy.calls == []
    with pytest.raises(AssertionError, match="library called: n2v_eccknn_predict"):
        proxy.n2v_eccknn_predict(0, 0, 0, 0, 0.0, 0.0, 0.0, 0, 0, 0)
    assert proxy.calls == ["n2v_eccknn_predict"]
    with pytest.raises(AttributeError):
        proxy.n2v_no_such_entry
