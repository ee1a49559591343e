"""The replica-merge kernels (csrc/n2v_merge.hip: merge_snapshot / _hot_apply / _flush / _pack_rows kernels and
tsum_kernel) against the fp32-exact numpy restatement in tests/merge_reference.py (itself held to torch, and its case
tables measured against deliberate errors, by tests/test_merge_host.py), at their edges.

Every buffer of a case — tables, weights, row lists, every wire — is uploaded with guard rows on both sides that hold a
sentinel bit pattern, and is compared WHOLE after every step: the addressed rows with the restatement's bits (uint32 /
uint16 views, so -0 is not +0; where the restatement holds a NaN the device must hold a NaN, whatever its sign and
payload), everything else — cold rows of a hot apply, rows outside a list, wire rows after a list, the guards — with
the bits it had."""
import types

import numpy as np
import pytest

import merge_reference as ref
from merge_reference import F32, U16

pytestmark = pytest.mark.gpu

INVALID = -1                                   # N2V_ERR_INVALID of include/n2v_hip.h


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from n2v_hip import _lib, merge
    return types.SimpleNamespace(torch=torch, lib=_lib, hip=merge.HipMergeOps(), merge=merge)


def _up(torch, a):
    if a.dtype == U16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(a).cuda()


def _down(torch, t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(U16)
    return t.cpu().numpy()


class _Hip:
    """HipMergeOps behind the restatement's method set (the fused entry points take a list of tables)."""

    def __init__(self, dev):
        self.d = dev
        for name in ("snapshot", "hot_apply", "flush", "pack_rows"):
            setattr(self, name, getattr(dev.hip, name))

    def _tsum(self, call, tabs, wire):
        arr = self.d.hip.tsum_tables([t for t, _, _ in tabs], [b for _, b, _ in tabs], [r for _, _, r in tabs])
        call(arr, int(wire.shape[1]), wire, self.d.lib.stream_ptr(wire.device))

    def tsum_pack(self, tabs, wire):
        self._tsum(self.d.hip.tsum_pack, tabs, wire)

    def tsum_apply(self, tabs, wire):
        self._tsum(self.d.hip.tsum_apply, tabs, wire)


def device_run(dev, run, B, *args):
    """As merge_reference.numpy_run, on the device: [(step, {buffer: whole array, guards included})]."""
    torch = dev.torch
    full = {k: _up(torch, g.full) for k, g in B.items() if g is not None}
    views = {k: (None if g is None else full[k][g.g:full[k].shape[0] - g.g]) for k, g in B.items()}
    out = []
    run(_Hip(dev), views, *args, lambda step: out.append((step, {k: _down(torch, t) for k, t in full.items()})))
    return out


def _check(expect, got, what):
    bad = ref.results_differ(expect, got)
    assert not bad, (what, bad[:4])


@pytest.mark.parametrize("case", ref.merge_cases(), ids=lambda c: c.id)
def test_snapshot_hot_apply_flush_equal_the_restatement(dev, case):
    B, expect = ref.build_merge(case)
    _check(expect, device_run(dev, ref.run_merge, B, case.n_hot()), case.id)


@pytest.mark.parametrize("case", ref.tsum_cases(), ids=lambda c: c.id)
def test_tsum_pack_and_apply_equal_the_restatement(dev, case):
    B, expect = ref.build_tsum(case)
    got = device_run(dev, ref.run_tsum, B, len(case.counts), sum(case.counts))
    _check(expect, got, case.id)
    if sum(case.counts) == 0:                  # no table, or only empty ones: OK, and no byte changes
        start = {k: g.full for k, g in B.items() if g is not None}
        assert not ref.results_differ([("pack", start), ("apply", start)], got, exact=True)


@pytest.mark.parametrize("case", ref.pack_cases(), ids=lambda c: c.id)
def test_per_table_tsum_path_equals_the_restatement_and_the_fused_kernels(dev, case):
    """n2v_merge_pack_rows + n2v_merge_hot_apply with xs aliasing x (both __restrict__) and w == 1."""
    B, expect = ref.build_pack(case)
    apply = case.kind != "repeat"
    got = device_run(dev, ref.run_per_table, B, case.n, apply)
    _check(expect, got, case.id)
    fused = device_run(dev, ref.run_pack_as_tsum, B, case.n, apply)
    _check(expect, fused, case.id + " fused")
    # the two device paths against each other: the same bits, and NaNs at the same places
    assert not ref.results_differ(got, fused) and not ref.results_differ(fused, got), case.id


@pytest.mark.parametrize("stride", [64, 512])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_tiered_sum_merger_at_the_product_strides_equals_the_restatement(dev, stride, bf16):
    """TieredSumMerger's fused path over a three-tier plan (the stand-in all-reduce of two identical replicas doubles
    the wire) against NumpyMergeOps driven by the same plan, at the row strides of d <= 64 and d > 256."""
    torch, merge = dev.torch, dev.merge

    class Doubling:
        world, rank = 2, 0
        wire_dtype = torch.bfloat16 if bf16 else torch.float32

        def all_reduce_async(self, t):
            t.mul_(2)
            return None

    n = 300
    counts = (np.random.default_rng(2).random(n) ** 6 * 40000 + 1).astype(np.int64)
    plan = merge.SumTierPlan(counts, 6.0e4, 2, 10, 5, torch.device("cuda"), theta=30.0, n_tiers=3, ratio=4)
    assert all(0 < plan.rows_ge[i][2].numel() < plan.rows_ge[i][1].numel() < n for i in range(2))
    lists = [[None] + [plan.rows_ge[i][lv].cpu().numpy() for lv in (1, 2)] for i in range(2)]
    rng = np.random.default_rng(stride + bf16)
    tabs = [rng.standard_normal((n, stride)).astype(F32) for _ in range(2)]
    base = [t.copy() for t in tabs]
    dtabs = [torch.from_numpy(t).cuda() for t in tabs]
    fused = merge.TieredSumMerger(dtabs, plan, Doubling())
    assert fused.fused
    ops = ref.NumpyMergeOps()
    for step, level in enumerate([2, 2, 1, 2, 0, 1, 2, 0]):
        for i in range(2):
            d = (rng.standard_normal((n, stride)) * 0.01).astype(F32)
            dtabs[i] += torch.from_numpy(d).cuda()
            tabs[i] = ref.f32_add(tabs[i], d)
        fused.merge(level)
        args = [(tabs[i], base[i], lists[i][level]) for i in range(2)]
        total = sum(n if a[2] is None else len(a[2]) for a in args)
        wire = np.zeros((total, stride), U16 if bf16 else F32)
        ops.tsum_pack(args, wire)
        wire[...] = ref.bf16_round(ref.f32_mul(ref.bf16_to_f32(wire), F32(2))) if bf16 else ref.f32_mul(wire, F32(2))
        ops.tsum_apply(args, wire)
        for i in range(2):
            assert not len(ref.bits_differ(tabs[i], dtabs[i].cpu().numpy())), (step, level, i)
            assert not len(ref.bits_differ(base[i], fused.base[i].cpu().numpy())), (step, level, i)
        assert not len(ref.bits_differ(wire, _down(torch, fused.wire[:total]))), (step, level)
    assert fused.n_merges == [2, 2, 4]


# ------------------------------------------------------------------------------------------- rejected arguments
def _rejected_calls(p, bf16):
    """name -> [(what, arguments)]: every call must be refused before anything is launched.  p: device pointers of
    small valid buffers (3 rows of stride 8), so that each call has exactly ONE thing wrong."""
    x, xs, base, w, pos, rows, cold, hotw, tab = p["x"], p["xs"], p["base"], p["w"], p["pos"], p["rows"], p["cold"], p["hotw"], p["tab"]
    s, st = 8, p["stream"]
    out = {"n2v_merge_snapshot": [], "n2v_merge_hot_apply": [], "n2v_merge_flush": [], "n2v_merge_pack_rows": [],
           "n2v_tsum_pack": [], "n2v_tsum_apply": []}
    snap = [x, xs, base, 3, s, w, pos, cold, cold, hotw, bf16, st]
    happ = [x, xs, base, s, w, rows, 3, hotw, bf16, st]
    flus = [x, xs, base, 3, s, w, pos, cold, bf16, st]
    pack = [x, base, s, rows, 3, cold, bf16, st]

    def but(args, at, value):
        a = list(args)
        a[at] = value
        return a

    out["n2v_merge_snapshot"] += [("negative count", but(snap, 3, -1)), ("stride 0", but(snap, 4, 0))] + \
        [("NULL " + n, but(snap, i, None)) for i, n in ((0, "x"), (1, "xs"), (2, "base"), (5, "w"))] + \
        [("no hot_pos and no cold_wire", but(but(snap, 6, None), 8, None)), ("hot_pos without hot_wire", but(snap, 9, None))]
    out["n2v_merge_hot_apply"] += [("negative count", but(happ, 6, -1)), ("stride 0", but(happ, 3, 0))] + \
        [("NULL " + n, but(happ, i, None)) for i, n in ((0, "x"), (1, "xs"), (2, "base"), (4, "w"), (5, "hot_rows"), (7, "hot_sum"))]
    out["n2v_merge_flush"] += [("negative count", but(flus, 3, -1)), ("stride 0", but(flus, 4, 0))] + \
        [("NULL " + n, but(flus, i, None)) for i, n in ((0, "x"), (1, "xs"), (2, "base"), (5, "w"))]
    out["n2v_merge_pack_rows"] += [("negative count", but(pack, 4, -1)), ("stride 0", but(pack, 2, 0))] + \
        [("NULL " + n, but(pack, i, None)) for i, n in ((0, "x"), (1, "base"), (3, "rows"), (5, "wire"))]
    for name in ("n2v_tsum_pack", "n2v_tsum_apply"):
        good = lambda n_rows=3, table=x, b=base: tab(table, b, rows, n_rows)
        out[name] += [("n_tabs 5", [good(), 5, s, cold, bf16, st]), ("n_tabs -1", [good(), -1, s, cold, bf16, st]),
                      ("stride 0", [good(), 1, 0, cold, bf16, st]), ("NULL tabs", [None, 1, s, cold, bf16, st]),
                      ("negative row count", [good(n_rows=-1), 1, s, cold, bf16, st]),
                      ("rows but NULL table", [good(table=None), 1, s, cold, bf16, st]),
                      ("rows but NULL base", [good(b=None), 1, s, cold, bf16, st]),
                      ("NULL wire with rows", [good(), 1, s, None, bf16, st])]
    return out


@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
def test_rejected_arguments_are_refused_by_name_and_change_nothing(dev, bf16):
    torch, lib = dev.torch, dev.lib.load()
    g = torch.Generator(device="cuda").manual_seed(5)
    wdt = torch.bfloat16 if bf16 else torch.float32
    t = {k: torch.randn(3, 8, device="cuda", generator=g) for k in ("x", "xs", "base")}
    t["w"] = torch.rand(3, device="cuda", generator=g)
    t["pos"] = torch.tensor([0, -1, 1], dtype=torch.int32, device="cuda")
    t["rows"] = torch.tensor([2, 0, 1], dtype=torch.int64, device="cuda")
    t["cold"] = torch.randn(3, 8, device="cuda", generator=g).to(wdt)
    t["hotw"] = torch.randn(3, 8, device="cuda", generator=g).to(wdt)
    before = {k: _down(torch, v).copy() for k, v in t.items()}
    p = {k: v.data_ptr() for k, v in t.items()}
    p["stream"] = dev.lib.stream_ptr(t["x"].device)
    keep = []

    def tab(table, base, rows, n_rows):
        arr = (dev.hip._TsumTable * 1)()
        arr[0].table, arr[0].base, arr[0].rows, arr[0].n_rows = table, base, rows, n_rows
        keep.append(arr)
        return arr

    p["tab"] = tab
    n = 0
    for name, calls in _rejected_calls(p, bf16).items():
        for what, args in calls:
            rc = getattr(lib, name)(*args)
            assert rc == INVALID, (name, what, rc)
            assert lib.n2v_last_error().decode().startswith(name + ":"), (name, what, lib.n2v_last_error())
            n += 1
    assert n == 8 + 8 + 6 + 6 + 8 + 8
    # zero counts with NULL pointers are fine
    st = p["stream"]
    assert lib.n2v_merge_snapshot(None, None, None, 0, 8, None, None, None, None, None, bf16, st) == 0
    assert lib.n2v_merge_hot_apply(None, None, None, 8, None, None, 0, None, bf16, st) == 0
    assert lib.n2v_merge_flush(None, None, None, 0, 8, None, None, None, bf16, st) == 0
    assert lib.n2v_merge_pack_rows(None, None, 8, None, 0, None, bf16, st) == 0
    for fn in (lib.n2v_tsum_pack, lib.n2v_tsum_apply):
        assert fn(None, 0, 8, None, bf16, st) == 0
        assert fn(tab(None, None, None, 0), 1, 8, None, bf16, st) == 0
    torch.cuda.synchronize()
    for k, v in t.items():
        assert np.array_equal(before[k].view(np.uint8), _down(torch, v).view(np.uint8)), k


def test_wire_types_and_host_tensors_are_refused(dev):
    torch, hip = dev.torch, dev.hip
    x, base = torch.zeros(3, 8, device="cuda"), torch.zeros(3, 8, device="cuda")
    rows = torch.arange(3, device="cuda")
    w = torch.ones(3, device="cuda")
    half = torch.zeros(3, 8, device="cuda", dtype=torch.float16)
    with pytest.raises(TypeError):
        hip.pack_rows(x, base, rows, half)
    with pytest.raises(TypeError):
        hip.hot_apply(x, x, base, w, rows, half)
    with pytest.raises(TypeError):
        hip.snapshot(x, x.clone(), base, w, None, None, half, None)
    with pytest.raises(TypeError):
        hip.flush(x, x.clone(), base, w, None, half)
    c = torch.zeros(3, 8)
    wire = torch.zeros(3, 8)
    for call in (lambda: hip.pack_rows(c, c.clone(), torch.arange(3), wire),
                 lambda: hip.hot_apply(c, c, c.clone(), torch.ones(3), torch.arange(3), wire),
                 lambda: hip.snapshot(c, c.clone(), c.clone(), torch.ones(3), None, None, wire, None),
                 lambda: hip.flush(c, c.clone(), c.clone(), torch.ones(3), None, None),
                 lambda: hip.tsum_tables([c], [c.clone()], [None])):
        with pytest.raises(RuntimeError):
            call()
    assert not x.any() and not base.any()
