"""The numpy restatement of the replica-merge kernels (tests/merge_reference.py: NumpyMergeOps) without a GPU:
its bfloat16 rounding against torch's, the whole restatement against TorchMergeOps on CPU tensors on every case the
device tests run (tests/test_gpu_merge_exact.py), and what those cases can tell apart — every deliberate error of
merge_reference.MUTANTS must change the result of at least one case, so the coverage of the case tables is derived
here and not asserted by hand."""
import numpy as np
import pytest
import torch

import merge_reference as ref
from merge_reference import F32, U16, U32


def _torch(a):
    """A CPU tensor on the memory of a numpy array (uint16: as bfloat16)."""
    if a is None:
        return None
    return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16) if a.dtype == U16 else torch.from_numpy(a)


def _bf16_bits(t):
    return t.view(torch.int16).numpy().view(U16)


class TorchTsum(ref.TorchMergeOps):
    """n2v_tsum_pack / n2v_tsum_apply as TieredSumMerger's per-table path restates them: pack_rows per table into its
    piece of the wire, hot_apply with xs aliasing x and a weight of one."""

    def _each(self, tabs):
        o = 0
        for t, b, rows in tabs:
            rows = torch.arange(t.shape[0]) if rows is None else rows
            yield t, b, rows, o, o + rows.numel()
            o += rows.numel()

    def tsum_pack(self, tabs, wire):
        for t, b, rows, lo, hi in self._each(tabs):
            if hi > lo:
                self.pack_rows(t, b, rows, wire[lo:hi])

    def tsum_apply(self, tabs, wire):
        for t, b, rows, lo, hi in self._each(tabs):
            if hi > lo:
                self.hot_apply(t, t, b, torch.ones(t.shape[0]), rows, wire[lo:hi])


def torch_run(run, B, *args):
    """As merge_reference.numpy_run, with TorchMergeOps on CPU tensors that share the copies' memory."""
    B = {k: (None if g is None else g.copy()) for k, g in B.items()}
    out = []
    run(TorchTsum(), {k: (None if g is None else _torch(g.v)) for k, g in B.items()}, *args,
        lambda step: out.append((step, {k: g.full.copy() for k, g in B.items() if g is not None})))
    return out


def test_float64_steps_are_float32_operations_subnormals_included():
    """The restatement's arithmetic keeps what a flushing device would lose: subnormal differences and products, the
    sign of zero, overflow to inf."""
    f = lambda *bits: np.array(bits, U32).view(F32)
    assert ref.f32_sub(f(0x00800001, 0x80000000, 0x00000000, 0x7f7fffff), f(0x00800000, 0x00000000, 0x00000000, 0xff7fffff)) \
        .view(U32).tolist() == [0x00000001, 0x80000000, 0x00000000, 0x7f800000]
    assert ref.f32_mul(f(0x3e000000, 0x00000000), f(0x00000008, 0xbf800000)).view(U32).tolist() == [0x00000001, 0x80000000]
    a, b = f(0x3f800000), f(0x33800000)            # 1 + 2^-24: the tie goes to even, 1 + 3 * 2^-25 rounds up
    assert ref.f32_add(a, b).view(U32).tolist() == [0x3f800000]
    assert ref.f32_add(a, f(0x33c00000)).view(U32).tolist() == [0x3f800001]
    # torch's CPU float32 gives the same on random operands, products and sums
    rng = np.random.default_rng(0)
    p, q = (rng.integers(0, 2**32, 200000, dtype=np.uint64).astype(U32).view(F32) for _ in range(2))
    for mine, theirs in ((ref.f32_add, torch.add), (ref.f32_sub, torch.sub), (ref.f32_mul, torch.mul)):
        assert not len(ref.bits_differ(theirs(torch.from_numpy(p), torch.from_numpy(q)).numpy(), mine(p, q)))


def test_bf16_round_equals_torch_on_every_non_nan_pattern():
    rng = np.random.default_rng(7)
    bits = np.concatenate([rng.integers(0, 2**32, 1 << 20, dtype=np.uint64).astype(U32), ref.EDGE_BITS,
                           ref.PAIR_BITS.reshape(-1), ref.MISC_BITS])
    assert len(bits) >= 10**6
    f = bits.view(F32)
    mine, theirs = ref.bf16_round(f), _bf16_bits(torch.from_numpy(f).to(torch.bfloat16))
    nan = np.isnan(f)
    assert nan.sum() > 1000 and np.array_equal(mine[~nan], theirs[~nan])
    assert ref._is_nan16(mine[nan]).all() and ref._is_nan16(theirs[nan]).all()
    # the hand-picked ones, spelled out
    spelled = {0x3f808000: 0x3f80, 0x3f818000: 0x3f82, 0x3f807fff: 0x3f80, 0x3f808001: 0x3f81, 0x3f817fff: 0x3f81,
               0x3f818001: 0x3f82, 0x3fff8000: 0x4000, 0x7f7f8000: 0x7f80, 0x7f7f7fff: 0x7f7f, 0xff7f8000: 0xff80,
               0x00008000: 0x0000, 0x00008001: 0x0001, 0x00018000: 0x0002, 0x007fffff: 0x0080, 0x80000000: 0x8000}
    got = ref.bf16_round(np.array(list(spelled), U32).view(F32))
    assert got.tolist() == list(spelled.values())
    # and back: every bfloat16 pattern survives the round trip
    allh = np.arange(1 << 16, dtype=np.uint32).astype(U16)
    keep = ~ref._is_nan16(allh)
    assert np.array_equal(ref.bf16_round(ref.bf16_to_f32(allh))[keep], allh[keep])


def test_case_tables_hold_every_shape_and_edge_the_kernels_have():
    mc, tc, pc = ref.merge_cases(), ref.tsum_cases(), ref.pack_cases()
    for cases in (mc, tc, pc):
        assert len({c.id for c in cases}) == len(cases)
    shapes = {(n, s, b) for n in ref.ROWS for s in ref.STRIDES for b in (False, True)}
    assert shapes <= {(c.n, c.stride, c.bf16) for c in mc} and shapes <= {(c.n, c.stride, c.bf16) for c in pc}
    assert {(h, p, l, b) for h in ref.HOT_MODES for p in (0, 1) for l in (0, 1) for b in (0, 1)} <= \
        {(c.hot, c.prev, c.last, c.bf16) for c in mc}
    for s in ref.STRIDES:                          # each stride meets a hot tier, a late sum and both value classes
        mine = [c for c in mc if c.stride == s]
        assert {c.values for c in mine} == {"randn", "edge"} and any(c.n_hot() for c in mine)
        assert any(c.prev and c.n_hot() < c.n for c in mine) and any(c.last and c.n_hot() < c.n for c in mine)
    assert {len(c.counts) for c in tc} == {0, 1, 2, 3, 4}
    for counts in ((1, 1, 1, 1), (1, 2, 3), (3, 0, 2), (0, 5), (5, 0), (0, 0, 4, 0), (257, 1, 0, 6)):
        for b in (False, True):
            assert {c.listed for c in tc if c.counts == counts and c.bf16 == b} >= \
                {tuple(bool((f + st * t) % 2) for t in range(len(counts))) for f in (0, 1) for st in (0, 1)}
    assert {(c.stride, c.bf16) for c in tc if 0 in c.counts and len(set(c.listed)) == 2} == \
        {(s, b) for s in ref.STRIDES for b in (False, True)}
    assert {c.kind for c in pc} == {"perm", "subset", "repeat"}
    # the value classes reach the arithmetic: over the "edge" cases every pattern is some change x - xs of a hot row
    # and of a cold row, every tie / overflow / subnormal / NaN pattern is some wire operand, every weight is used
    seen = {"hot": set(), "cold": set(), "sum": set(), "w": set()}
    for c in mc:
        if c.values != "edge":
            continue
        B, _ = ref.build_merge(c)
        d = ref.f32_sub(B["x"].v, B["xs"].v).view(U32)
        hot = (B["hot_pos"].v >= 0) if B["hot_pos"] is not None else np.zeros(c.n, bool)
        seen["hot"].update(d[hot].reshape(-1).tolist())
        seen["cold"].update(d[~hot].reshape(-1).tolist())
        seen["w"].update(B["w"].v.tolist())
        for k in ("prev", "last", "hot_sum"):
            if B[k] is not None and not c.bf16:
                seen["sum"].update(B[k].v.view(U32).reshape(-1).tolist())
    finite = [int(e) for e in ref.EDGE_BITS if (int(e) & 0x7fffffff) <= 0x7f800000]
    assert set(finite) <= seen["hot"] and set(finite) <= seen["cold"] and set(finite) <= seen["sum"]
    assert {0x00000001, 0x80000001, 0x00007fff, 0x00010000} <= seen["hot"] & seen["cold"]      # subnormal differences
    assert any(np.isnan(np.array([v], U32).view(F32)[0]) for v in seen["hot"])
    assert seen["w"] == set(ref.W_CYCLE.tolist())


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_numpy_restatement_equals_torch_restatement_on_every_case(bf16):
    n = 0
    for case in ref.merge_cases():
        if case.bf16 == bf16:
            B, expect = ref.build_merge(case)
            assert not ref.results_differ(expect, torch_run(ref.run_merge, B, case.n_hot())), case.id
            n += 1
    for case in ref.tsum_cases():
        if case.bf16 == bf16:
            B, expect = ref.build_tsum(case)
            assert not ref.results_differ(expect, torch_run(ref.run_tsum, B, len(case.counts), sum(case.counts))), case.id
            n += 1
    for case in ref.pack_cases():
        if case.bf16 == bf16:
            B, expect = ref.build_pack(case)
            apply = case.kind != "repeat"
            assert not ref.results_differ(expect, torch_run(ref.run_per_table, B, case.n, apply)), case.id
            # one table through the fused entry points: the same bits, NaNs included (both are this restatement)
            fused = ref.numpy_run(ref.run_pack_as_tsum, B, ref.NumpyMergeOps(), case.n, apply)
            assert not ref.results_differ(expect, fused, exact=True), case.id
            n += 1
    assert n > 200


def _all_runs():
    """(kind, case, buffers, expected, rerun(ops))."""
    for c in ref.merge_cases():
        B, e = ref.build_merge(c)
        yield "merge", c, B, e, lambda ops, B=B, c=c: ref.numpy_run(ref.run_merge, B, ops, c.n_hot())
    for c in ref.tsum_cases():
        B, e = ref.build_tsum(c)
        yield "tsum", c, B, e, lambda ops, B=B, c=c: ref.numpy_run(ref.run_tsum, B, ops, len(c.counts), sum(c.counts))
    for c in ref.pack_cases():
        B, e = ref.build_pack(c)
        yield "pack", c, B, e, lambda ops, B=B, c=c: ref.numpy_run(ref.run_per_table, B, ops, c.n, c.kind != "repeat")


def _in_guard(B, buffer, index):
    g = B[buffer]
    return not g.g <= index[0] < g.full.shape[0] - g.g


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_of_the_restatement_changes_some_case(mutant):
    """A mutant that reads or writes outside even the guards (IndexError) does not count: a comparison has to see it."""
    caught, in_guard = [], []
    for kind, case, B, expect, rerun in _all_runs():
        try:
            diff = ref.results_differ(expect, rerun(ref.NumpyMergeOps(mutant)), exact=True)
        except IndexError:
            continue
        if diff:
            caught.append((kind, case))
            if any(_in_guard(B, k, i) for _, k, i in diff):
                in_guard.append((kind, case))
    assert caught, mutant
    kinds = {k for k, _ in caught}
    if mutant == "pick_first_match":               # matters only with an empty table — and the tables have those
        assert kinds == {"tsum"} and all(0 in c.counts for _, c in caught)
    if mutant == "ncol_over":                      # seen by the sentinels, in every family of kernels
        assert {k for k, _ in in_guard} == {"merge", "tsum", "pack"}
    if mutant == "row_guard":                      # by the sentinel rows of the tables; for a row list, by the wire row
        assert "merge" in {k for k, _ in in_guard} and kinds == {"merge", "tsum", "pack"}       # after the last one
    if mutant in ("ncol_trunc", "ncol_over"):      # exactly the strides with a partial last 64-lane step
        assert {c.stride for _, c in caught} == {s for s in ref.STRIDES if s % 64}
    if mutant in ("bf16_trunc", "bf16_away"):
        assert all(c.bf16 for _, c in caught) and kinds == {"merge", "tsum", "pack"}
        # not by luck: the tie with an even kept mantissa alone tells "away", its lower neighbour alone "trunc"
        one = np.array([0x3f808000 if mutant == "bf16_away" else 0x3f80ffff], U32).view(F32)
        assert ref.bf16_round(one, mutant[5:]) != ref.bf16_round(one)
    if mutant == "contract":                       # every case that has the step at all
        assert {c for k, c in caught if k == "merge"} == {c for c in ref.merge_cases() if c.has_two_step()}
