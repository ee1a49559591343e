"""CPU tests of the walk engine's host arithmetic (n2v_hip/engine.py): the memory plan of the alias tables
(plan_tables), the rng names of a walk launch (rng_mode) and the frame of a launch with its check of a caller's output
buffers (walk_frame).  Nothing is launched: these are pure functions so that no GPU test has to hand a kernel an
undersized buffer, or fake the free memory, to reach them."""
import numpy as np
import pytest
import torch

from n2v_hip import _lib, csr, engine
from n2v_hip.csr import degree_cut_for_budget

GIB = 1 << 30
AMPLE = 64 * GIB


@pytest.fixture(scope="module")
def star_path():
    """A star (centre 0, leaves 1-4) and a path 5 - 6 - 7, undirected: degrees 4, 1, 1, 1, 1, 1, 2, 1.
    nnz = 12 entries; T = sum over entries of deg(dst): 0 -> leaf 4 x 1, leaf -> 0 4 x 4, 5 -> 6 and 7 -> 6 2 x 2,
    6 -> 5 and 6 -> 7 2 x 1 = 26 slots."""
    src = np.array([0, 0, 0, 0, 5, 6])
    dst = np.array([1, 2, 3, 4, 6, 7])
    cg = csr.from_edges(src, dst, None, False)
    assert cg.nnz == 12 and engine.edge_table_slots(cg) == 26
    return cg, 12, 26


def plan(cg, free, fat="auto", budget_bytes=None, first_order=False):
    return engine.plan_tables(cg, first_order, fat, budget_bytes, free)


def test_plan_with_ample_memory_is_fat_only(star_path):
    cg, nnz, T = star_path
    assert plan(cg, AMPLE) == (T, False, None, False, True)
    assert engine.plan_tables(cg, False, "auto", None, AMPLE, edge_slots=T) == plan(cg, AMPLE)


def test_plan_at_the_fat_reserve_is_thin_only(star_path):
    """free = 8 GiB: (nnz + T) * 32 < free - 8 GiB = 0 fails, the thin tables fit beside the 1 GiB reserve."""
    cg, nnz, T = star_path
    assert plan(cg, 8 * GIB) == (T, False, None, True, False)


def test_plan_without_room_for_thin_tables_budgets_itself(star_path):
    """free = 1 GiB: T * 16 > 0 bytes beside the reserve, the automatic budget is max(0, free - 8 GiB) = 0."""
    cg, nnz, T = star_path
    cut, total = degree_cut_for_budget(cg, 0, 32)
    assert total == 0
    assert plan(cg, GIB) == (0, True, cut, False, True)          # partial forces fat; no MemoryError


def test_plan_under_a_budget(star_path):
    cg, nnz, T = star_path
    assert plan(cg, AMPLE, budget_bytes=32 * T) == (T, False, None, False, True)
    got = plan(cg, AMPLE, budget_bytes=0)
    assert got.partial and got.total == 0 and got.want_fat and not got.want_thin
    # between the two: 320 bytes hold the tables of the destinations of degree 1 (6 slots) and 2 (4 slots), not 4's 16
    assert degree_cut_for_budget(cg, 320, 32) == (3, 10)
    assert plan(cg, AMPLE, budget_bytes=320) == (10, True, 3, False, True)
    assert plan(cg, AMPLE, fat=False, budget_bytes=320) == (10, True, 3, False, True)      # also over fat=False
    assert plan(cg, AMPLE, budget_bytes=32 * T - 1).partial


def test_plan_raises_when_the_layout_asked_for_does_not_fit(star_path):
    cg, nnz, T = star_path
    with pytest.raises(MemoryError):
        plan(cg, GIB, fat=True)
    with pytest.raises(MemoryError):
        plan(cg, GIB, fat=False)


def test_plan_both_layouts_need_48_bytes_a_slot(star_path):
    cg, nnz, T = star_path
    assert plan(cg, GIB + 48 * T, fat="both") == (T, False, None, True, True)
    with pytest.raises(MemoryError):
        plan(cg, GIB + 48 * T - 1, fat="both")
    assert plan(cg, GIB + 48 * T - 1, fat=True) == (T, False, None, False, True)           # 32 T alone does fit there


def test_plan_first_order_stores_no_edge_tables(star_path):
    """total == nnz (the node tables stand in), never partial, and nothing is asked of `free` from the 1 GiB reserve
    up — below it the comparison `need > free - 1 GiB` fails for need = 0 as it always has."""
    cg, nnz, T = star_path
    for free in (GIB, 8 * GIB, AMPLE):
        for fat in ("auto", True, False, "both"):
            for budget in (None, 0, 32 * T):
                got = plan(cg, free, fat=fat, budget_bytes=budget, first_order=True)
                assert got.total == nnz and not got.partial and got.stored_degree_cut is None, (free, fat, budget)
    assert plan(cg, AMPLE, first_order=True)[3:] == (False, True)
    assert plan(cg, 8 * GIB, first_order=True)[3:] == (True, False)


def test_edge_table_slots_directed():
    """0 -> 1, 0 -> 2, 1 -> 2, 2 -> 0: out-degrees 2, 1, 1; sum over entries of deg(dst) = 1 + 1 + 1 + 2."""
    cg = csr.from_edges(np.array([0, 0, 1, 2]), np.array([1, 2, 2, 0]), None, True)
    assert engine.edge_table_slots(cg) == 5


def test_rng_mode():
    for tiled_ok in (False, True):
        assert engine.rng_mode("philox", tiled_ok) == _lib.RNG_PHILOX
        assert engine.rng_mode("uniforms", tiled_ok) == _lib.RNG_UNIFORMS
    assert engine.rng_mode("uniforms_tiled", True) == _lib.RNG_UNIFORMS_TILED
    assert len({_lib.RNG_PHILOX, _lib.RNG_UNIFORMS, _lib.RNG_UNIFORMS_TILED}) == 3
    for name in ("numpy", "", None, "Philox"):
        with pytest.raises(ValueError, match="rng must be"):
            engine.rng_mode(name, True)
    with pytest.raises(ValueError, match="the tiled uniform layout is read by the fat-table walk kernel only"):
        engine.rng_mode("uniforms_tiled", False)


def test_walk_frame_defaults_and_allocation():
    pos_count, n_local, walks, lens = engine.walk_frame(10, 3, None, 2, 5, None, "cpu")
    assert (pos_count, n_local) == (7, 14)
    assert walks.shape == (14, 5) and walks.dtype == torch.int32 and lens.shape == (14,) and lens.dtype == torch.int32
    assert engine.walk_frame(10, 3, 4, 2, 5, None, "cpu")[:2] == (4, 8)
    with pytest.raises(ValueError, match="walk_length"):
        engine.walk_frame(10, 0, None, 1, 0, None, "cpu")


def test_walk_frame_checks_a_callers_buffers():
    L, n_local = 5, 8
    big_w = torch.empty((3 * n_local, L), dtype=torch.int32)
    big_l = torch.empty(3 * n_local, dtype=torch.int32)
    w, l = big_w[n_local:2 * n_local], big_l[n_local:2 * n_local]          # slices of a larger buffer go through
    got = engine.walk_frame(10, 3, 4, 2, L, (w, l), "cpu")
    assert got[:2] == (4, n_local) and got[2] is w and got[3] is l
    bad = {
        "walks of the wrong shape": (big_w[:n_local - 1], l),
        "walks too narrow": (torch.empty((n_local, L - 1), dtype=torch.int32), l),
        "walks int64": (torch.empty((n_local, L), dtype=torch.int64), l),
        "walks non-contiguous": (torch.empty((n_local, 2 * L), dtype=torch.int32)[:, ::2], l),
        "lens one short": (w, big_l[:n_local - 1]),
        "lens int64": (w, torch.empty(n_local, dtype=torch.int64)),
    }
    for what, out in bad.items():
        with pytest.raises(ValueError, match="must be a contiguous int32 tensor"):
            engine.walk_frame(10, 3, 4, 2, L, out, "cpu")
            pytest.fail("accepted: " + what)
