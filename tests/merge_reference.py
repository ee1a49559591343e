"""TEST INFRASTRUCTURE — restatements of the replica-merge kernels (csrc/n2v_merge.hip, declared in
include/n2v_hip.h "replica merges"), same arguments and semantics.

TorchMergeOps works on tensors of any device.  The CPU tests run the merge PROTOCOL (n2v_hip.sgns.ReplicaMerger:
tiers, one-interval delay of the cold rows, collectives over gloo) with these ops injected; tests/test_gpu_sgns.py
checks the HIP kernels against them bit for bit.

NumpyMergeOps is the fp32-exact restatement the kernels are pinned to at their edges (tests/test_merge_host.py holds
it to TorchMergeOps and derives what the case tables below can tell apart; tests/test_gpu_merge_exact.py holds the
kernels to it).  Every arithmetic step is evaluated in float64 on the float32 operands and rounded once to float32,
which for a single +, - or * is the float32 operation itself (53 >= 2 * 24 + 2); base + w * S is two such steps.  It
addresses memory as the kernels do — element offsets from the pointer it was given — so that a restatement with a
wrong guard writes where the kernel would: into the guard rows that every buffer of a case carries.

The product never imports this file: without a GPU its own ops raise."""
import collections
import functools
import zlib

import numpy as np
import torch


class TorchMergeOps:
    @staticmethod
    def _wire(t, like):
        return t.to(like.dtype)

    def snapshot(self, x, xs, base, w, hot_pos, sum_prev, cold_wire, hot_wire):
        d = x - xs
        n = x.shape[0]
        hot = (hot_pos >= 0) if hot_pos is not None else torch.zeros(n, dtype=torch.bool, device=x.device)
        cold = ~hot
        if hot.any():
            hot_wire[hot_pos[hot].long()] = d[hot].to(hot_wire.dtype)
            if cold_wire is not None:
                cold_wire[hot] = 0
        if cold.any():
            if sum_prev is not None:
                base[cold] = base[cold] + w[cold, None] * sum_prev[cold].float()
            cold_wire[cold] = d[cold].to(cold_wire.dtype)
            nx = base[cold] + d[cold]
            x[cold] = nx
            xs[cold] = nx

    def pack_rows(self, x, base, rows, wire):
        wire[: rows.numel()] = (x[rows] - base[rows]).to(wire.dtype)

    def hot_apply(self, x, xs, base, w, hot_rows, hot_sum):
        b = base[hot_rows] + w[hot_rows, None] * hot_sum.float()
        base[hot_rows] = b
        x[hot_rows] = b
        xs[hot_rows] = b

    def flush(self, x, xs, base, w, hot_pos, sum_last):
        n = x.shape[0]
        cold = (hot_pos < 0) if hot_pos is not None else torch.ones(n, dtype=torch.bool, device=x.device)
        if sum_last is not None and cold.any():
            base[cold] = base[cold] + w[cold, None] * sum_last[cold].float()
        x.copy_(base)
        xs.copy_(base)


# ----------------------------------------------------------------------------------------- the numpy restatement
F32, F64, U16, U32 = np.float32, np.float64, np.uint16, np.uint32
MUTANTS = ("bf16_trunc", "bf16_away", "contract", "hot_cold_not_zeroed", "snapshot_no_xs", "cold_drop_d",
           "flush_folds_hot", "tsum_apply_no_table", "pick_gt", "pick_first_match", "pos_j", "ncol_trunc", "ncol_over",
           "row_guard")


def _is_nan16(h):
    return (h & U16(0x7fff)) > U16(0x7f80)


def bf16_round(f, mode="even"):
    """float32 array -> bfloat16 bit patterns (uint16), round to nearest even on the bit pattern; a NaN gives some
    NaN.  mode "trunc" / "away" (half away from zero) are the wrong roundings of the sensitivity checks."""
    u = np.ascontiguousarray(f, dtype=F32).view(U32).astype(np.uint64)
    if mode == "even":
        r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    elif mode == "away":
        r = (u + 0x8000) >> 16
    else:
        r = u >> 16
    return np.where((u & 0x7fffffff) > 0x7f800000, 0x7fc0, r & 0xffff).astype(U16)


def bf16_to_f32(h):
    return (np.ascontiguousarray(h, dtype=U16).astype(U32) << 16).view(F32)


def _fl32(op, a, b):
    with np.errstate(all="ignore"):
        return op(np.asarray(a, dtype=F32).astype(F64), np.asarray(b, dtype=F32).astype(F64)).astype(F32)


def f32_sub(a, b):
    return _fl32(np.subtract, a, b)


def f32_add(a, b):
    return _fl32(np.add, a, b)


def f32_mul(a, b):
    return _fl32(np.multiply, a, b)


def _mem(a):
    """(the whole allocation `a` is a view of, flat; element offset of a's first element in it): what a pointer is."""
    if a is None:
        return None, 0
    root = a
    while isinstance(root.base, np.ndarray):
        root = root.base
    assert root.dtype == a.dtype and root.flags.c_contiguous and a.flags.c_contiguous
    off = (a.__array_interface__["data"][0] - root.__array_interface__["data"][0]) // a.itemsize
    return root.reshape(-1), off


def _at(A, start, k=None):
    """A[start : start + k] (k None: the element), never clipped: outside the allocation is an IndexError."""
    if A is None or start < 0 or start + (1 if k is None else k) > A.size:
        raise IndexError("outside the allocation")
    return A[start] if k is None else A[start:start + k]


class NumpyMergeOps:
    """The six entry points as literal per-row loops (one iteration = one wavefront's row, the columns as one vector).
    Wire buffers are float32, or uint16 holding bfloat16 bits.  `mutant`: one deliberate error of MUTANTS — only for
    the sensitivity checks, never an expectation."""

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.m = mutant

    # -- the shared steps
    def _ncol(self, stride):                                  # for (c = lane; c < stride; c += 64)
        return {"ncol_trunc": stride & ~63, "ncol_over": (stride + 63) & ~63}.get(self.m, stride)

    def _n(self, n):                                          # if (r >= n) return
        return n + 1 if self.m == "row_guard" else n

    def _load(self, W, i, k):
        v = _at(W, i, k)
        return bf16_to_f32(v) if W.dtype == U16 else v

    def _store(self, W, i, v):
        mode = {"bf16_trunc": "trunc", "bf16_away": "away"}.get(self.m, "even")
        at = _at(W, i, len(v))                                # a NULL wire: IndexError
        at[:] = bf16_round(v, mode) if W.dtype == U16 else v

    def _axpy(self, b, w, s):                                 # b + w * s: two roundings (-ffp-contract=off)
        if self.m == "contract":
            with np.errstate(all="ignore"):
                return (b.astype(F64) + F64(w) * s.astype(F64)).astype(F32)
        return f32_add(b, f32_mul(w, s))

    # -- the weighted merges
    def snapshot(self, x, xs, base, w, hot_pos, sum_prev, cold_wire, hot_wire):
        n, stride = x.shape
        (X, xo), (XS, so), (B, bo), (W, wo) = _mem(x), _mem(xs), _mem(base), _mem(w)
        (HP, po), (SP, spo), (CW, co), (HW, ho) = _mem(hot_pos), _mem(sum_prev), _mem(cold_wire), _mem(hot_wire)
        nc = self._ncol(stride)
        for r in range(self._n(n)):
            hp = int(_at(HP, po + r)) if hot_pos is not None else -1
            wr = _at(W, wo + r)
            o = r * stride
            d = f32_sub(_at(X, xo + o, nc), _at(XS, so + o, nc))
            if hp >= 0:
                self._store(HW, ho + hp * stride, d)
                if cold_wire is not None and self.m != "hot_cold_not_zeroed":
                    self._store(CW, co + o, np.zeros(nc, F32))
            else:
                b = _at(B, bo + o, nc).copy()
                if sum_prev is not None:
                    b = self._axpy(b, wr, self._load(SP, spo + o, nc))
                    _at(B, bo + o, nc)[:] = b
                self._store(CW, co + o, d)
                nx = b if self.m == "cold_drop_d" else f32_add(b, d)
                _at(X, xo + o, nc)[:] = nx
                if self.m != "snapshot_no_xs":
                    _at(XS, so + o, nc)[:] = nx

    def hot_apply(self, x, xs, base, w, hot_rows, hot_sum):
        stride = x.shape[1]
        (X, xo), (XS, so), (B, bo), (W, wo) = _mem(x), _mem(xs), _mem(base), _mem(w)
        (R, ro), (HS, ho) = _mem(hot_rows), _mem(hot_sum)
        nc = self._ncol(stride)
        for j in range(self._n(len(hot_rows))):
            r = int(_at(R, ro + j))
            o = r * stride
            b = self._axpy(_at(B, bo + o, nc), _at(W, wo + r), self._load(HS, ho + j * stride, nc))
            _at(B, bo + o, nc)[:] = b
            _at(X, xo + o, nc)[:] = b
            _at(XS, so + o, nc)[:] = b

    def flush(self, x, xs, base, w, hot_pos, sum_last):
        n, stride = x.shape
        (X, xo), (XS, so), (B, bo), (W, wo) = _mem(x), _mem(xs), _mem(base), _mem(w)
        (HP, po), (SL, lo) = _mem(hot_pos), _mem(sum_last)
        nc = self._ncol(stride)
        for r in range(self._n(n)):
            cold = hot_pos is None or int(_at(HP, po + r)) < 0 or self.m == "flush_folds_hot"
            wr = _at(W, wo + r)
            o = r * stride
            b = _at(B, bo + o, nc).copy()
            if cold and sum_last is not None:
                b = self._axpy(b, wr, self._load(SL, lo + o, nc))
                _at(B, bo + o, nc)[:] = b
            _at(X, xo + o, nc)[:] = b
            _at(XS, so + o, nc)[:] = b

    # -- the tiered pure sums
    def pack_rows(self, x, base, rows, wire):
        stride = x.shape[1]
        (X, xo), (B, bo), (R, ro), (WI, io) = _mem(x), _mem(base), _mem(rows), _mem(wire)
        nc = self._ncol(stride)
        for j in range(self._n(len(rows))):
            o = int(_at(R, ro + j)) * stride
            self._store(WI, io + j * stride, f32_sub(_at(X, xo + o, nc), _at(B, bo + o, nc)))

    def _tsum(self, tabs, wire, apply):
        """tabs: [(table, base, rows or None)]; wire [sum of the list lengths][stride], the lists back to back."""
        if not tabs:
            return
        stride = tabs[0][0].shape[1]
        first = [0]
        for t, _, rows in tabs:
            first.append(first[-1] + (t.shape[0] if rows is None else len(rows)))
        mem = [(_mem(t), _mem(b), _mem(rows)) for t, b, rows in tabs]
        WI, io = _mem(wire)
        nc = self._ncol(stride)
        for j in range(self._n(first[-1]) if first[-1] else 0):
            t = 0
            for u in range(1, len(tabs)):                     # the unrolled chain: the LAST table that begins at or before j
                hit = j > first[u] if self.m == "pick_gt" else j >= first[u]
                if self.m == "pick_first_match":
                    hit = hit and first[u] > first[t]
                if hit:
                    t = u
            (X, xo), (B, bo), (R, ro) = mem[t]
            k = j if self.m == "pos_j" else j - first[t]
            o = (int(_at(R, ro + k)) if tabs[t][2] is not None else k) * stride
            if apply:
                b = f32_add(_at(B, bo + o, nc), self._load(WI, io + j * stride, nc))
                _at(B, bo + o, nc)[:] = b
                if self.m != "tsum_apply_no_table":
                    _at(X, xo + o, nc)[:] = b
            else:
                self._store(WI, io + j * stride, f32_sub(_at(X, xo + o, nc), _at(B, bo + o, nc)))

    def tsum_pack(self, tabs, wire):
        self._tsum(tabs, wire, False)

    def tsum_apply(self, tabs, wire):
        self._tsum(tabs, wire, True)


def bits_differ(expect, got):
    """Indices at which `got` is not `expect`, as bit patterns (so -0 is not +0) — except where `expect` is a NaN:
    there `got` must be a NaN, whatever its sign and payload.  float32, or uint16 holding bfloat16; integers exactly."""
    assert expect.shape == got.shape and expect.dtype == got.dtype, (expect.shape, got.shape, expect.dtype, got.dtype)
    if expect.dtype == F32:
        same = np.where(np.isnan(expect), np.isnan(got), expect.view(U32) == got.view(U32))
    elif expect.dtype == U16:
        same = np.where(_is_nan16(expect), _is_nan16(got), expect == got)
    else:
        same = expect == got
    return np.argwhere(~same)


# ------------------------------------------------------------------------------------------------ the case tables
# Shared by the host tests (restatement against torch, and what the tables can tell apart) and the device tests.
STRIDES = (1, 2, 63, 64, 65, 100, 128, 192, 256, 512)         # sgns._row_stride gives 64 .. 512; the ABI takes any >= 1
ROWS = (1, 3, 4, 5, 8, 257)                                   # 4 rows per 256-thread block
SENTINEL = np.array([0xA5C3F00D], U32).view(F32)[0]           # guard rows; no NaN, so it is compared by bits
SENTINEL16 = U16(0xA5C3)
W_CYCLE = np.array([0.3, 1.0, 0.0, 0.125, 0.7], F32)          # non-dyadic first: a one-row case has it

# float32 patterns whose bfloat16 rounding decides something
EDGE_BITS = np.array(
    [0x3f808000, 0x3f818000,                                  # ties: kept mantissa even / odd
     0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,          # their neighbours, one ulp either side
     0x3fff8000,                                              # the carry runs into the exponent
     0x7f7f8000, 0x7f7f7fff,                                  # -> inf, -> max
     0xbf808000, 0xbf818000, 0xbfff8000, 0xff7f8000, 0xff7f7fff, 0xbf807fff, 0xbf818001,
     0x00000000, 0x80000000,
     0x00000001, 0x00007fff, 0x00008000, 0x00008001,          # below / at / above half a bfloat16 subnormal step
     0x00018000, 0x80018000, 0x80008000, 0x80008001,
     0x007fffff, 0x007f8000, 0x00800000,                      # the largest subnormals round to the smallest normal
     0x7f800000, 0xff800000,
     0x7fc00000, 0x7f800001, 0xffc12345, 0x7fffffff], U32)    # NaN: quiet, signalling with a payload below bit 16, ...
# (a, b) whose float32 difference a - b decides something
PAIR_BITS = np.array(
    [(e, 0) for e in EDGE_BITS] + [(e, 0x80000000) for e in EDGE_BITS[:20]] +
    [(e, e) for e in EDGE_BITS[:31]] +                        # equal operands (infinities: inf - inf): change +0 / NaN
    [(0x80000000, 0x00000000), (0x80000000, 0x80000000), (0x00000000, 0x80000000),
     (0x00800001, 0x00800000), (0x00800000, 0x00800001),      # differences of one float32 subnormal ulp
     (0x3f800000, 0x3f800000), (0x00c00000, 0x00bf8001),      # 0x7fff subnormal ulps: below half a bfloat16 step
     (0x00c00000, 0x00bf8000), (0x00c00000, 0x00bf7fff), (0x00c00000, 0x00be8000), (0x80c00000, 0x80be8000),
     (0x00810000, 0x00800000),                                # exactly one bfloat16 subnormal step
     (0x7f800000, 0xff800000), (0xff800000, 0xff800000), (0x7fc00000, 0x3f800000), (0x3f800000, 0xffc12345),
     (0x7f7fffff, 0xff7fffff)], U32)                          # the difference overflows
MISC_BITS = np.array([0x00000000, 0x80000000, 0x7f7fffff, 0xff7fffff, 0x00000001, 0x00800000, 0x3f800000, 0x80800001], U32)


class Guarded:
    """An array with guard rows (2-D) or guard elements (1-D) on both sides; `v` is the part a kernel is given."""

    def __init__(self, data, fill, guard):
        data = np.ascontiguousarray(data)
        self.g = int(guard)
        self.full = np.empty((data.shape[0] + 2 * self.g,) + data.shape[1:], data.dtype)
        self.full[...] = fill
        self.full[self.g:self.g + data.shape[0]] = data

    @property
    def v(self):
        return self.full[self.g:self.full.shape[0] - self.g]

    def copy(self):
        c = Guarded.__new__(Guarded)
        c.g, c.full = self.g, self.full.copy()
        return c


def guard_rows(stride):
    """At least two rows and at least 64 elements: one row too many and one 64-lane step too many stay inside."""
    return max(2, -(-64 // stride))


def _table(a, stride):
    a = np.asarray(a)
    fill = SENTINEL16 if a.dtype == U16 else SENTINEL
    return Guarded(a.reshape(-1, stride), fill, guard_rows(stride))


def _vector(a):
    a = np.asarray(a)
    # guards of inputs the kernels only read: a cold row (-1), row 0, the float sentinel
    fill = {np.dtype(np.int32): -1, np.dtype(np.int64): 0}.get(a.dtype, SENTINEL)
    return Guarded(a, fill, 16)


def _randn(rng, k, scale=1.0):
    return (rng.standard_normal(k) * scale).astype(F32)


def _pair_fill(rng, k, values):
    """(a, b): the operands of a change a - b, k elements each."""
    a = _randn(rng, k)
    b = f32_sub(a, _randn(rng, k, 0.01))
    if values == "edge":
        i = (np.arange(k) + int(rng.integers(len(PAIR_BITS)))) % len(PAIR_BITS)
        a, b = PAIR_BITS[i, 0].copy().view(F32), PAIR_BITS[i, 1].copy().view(F32)
    return a, b


def _base_fill(rng, k, values):
    b = _randn(rng, k)
    if values == "edge" and k > 1:                            # element 0 stays plain: see _needs_two_roundings
        at = np.arange(1, k, 3)
        b[at] = MISC_BITS[(at + int(rng.integers(8))) % len(MISC_BITS)].view(F32)
    return b


def _sum_fill(rng, k, values, bf16):
    """A summed change as it comes back on the wire (float32, or bfloat16 bits)."""
    s = _randn(rng, k)
    if values == "edge" and k > 1:
        at = np.arange(1, k, 2)
        s[at] = EDGE_BITS[(at + int(rng.integers(64))) % len(EDGE_BITS)].view(F32)
    if not bf16:
        return s
    h = bf16_round(s)
    return np.where(np.isnan(s), (s.view(U32) >> 16).astype(U16), h)      # keep the NaN patterns' upper halves


def _unsorted(rng, pool, k):
    """k distinct entries of `pool`, not in ascending order where k >= 2 allows it."""
    while True:
        r = rng.permutation(pool)[:k].astype(np.int64)
        if k < 2 or np.any(np.diff(r) < 0):
            return r


def _snapshots(B):
    return {k: g.full.copy() for k, g in B.items() if g is not None}


def _views(B):
    return {k: (None if g is None else g.v) for k, g in B.items()}


def results_differ(a, b, exact=False):
    """a, b: [(step, {buffer: whole array})] of two runs of a case -> [(step, buffer, first index)] that differ."""
    assert [s for s, _ in a] == [s for s, _ in b]
    out = []
    for (step, ea), (_, eb) in zip(a, b):
        assert ea.keys() == eb.keys()
        for k in ea:
            bad = np.argwhere(ea[k].view(U32 if ea[k].dtype == F32 else ea[k].dtype) !=
                              eb[k].view(U32 if eb[k].dtype == F32 else eb[k].dtype)) if exact else bits_differ(ea[k], eb[k])
            if len(bad):
                out.append((step, k, tuple(int(i) for i in bad[0])))
    return out


# ---- n2v_merge_snapshot -> n2v_merge_hot_apply -> n2v_merge_flush
HOT_MODES = ("null", "none", "some", "some_unsorted", "all", "all_nocold")


class MergeCase(collections.namedtuple("MergeCase", "n stride bf16 hot prev last values")):
    """hot: hot_pos NULL | given, no row hot | some rows hot, list ascending | list not ascending | every row hot |
    every row hot and cold_wire NULL.  prev / last: cold_sum_prev / cold_sum_last given."""

    @property
    def id(self):
        return "n%d-s%d-%s-%s-%s%s-%s" % (self.n, self.stride, "bf16" if self.bf16 else "f32", self.hot,
                                         "p" if self.prev else "", "l" if self.last else "", self.values)

    def n_hot(self):
        return {"null": 0, "none": 0, "all": self.n, "all_nocold": self.n}.get(self.hot, (self.n + 1) // 2)

    def has_two_step(self):
        """Some element goes through base + w * S."""
        cold = self.n - self.n_hot()
        return self.n_hot() > 0 or (cold > 0 and (self.prev or self.last))


def merge_cases():
    rng = np.random.default_rng(1)
    out = []
    for stride in STRIDES:                                    # every shape with both wires, the rest drawn
        for n in ROWS:
            for bf16 in (False, True):
                out.append(MergeCase(n, stride, bf16, HOT_MODES[int(rng.integers(6))], bool(rng.integers(2)),
                                     bool(rng.integers(2)), ("randn", "edge")[int(rng.integers(2))]))
    for bf16 in (False, True):                                # every combination of the rest at one odd shape
        for hot in HOT_MODES:
            for prev in (False, True):
                for last in (False, True):
                    for values in ("randn", "edge"):
                        out.append(MergeCase(5, 65, bf16, hot, prev, last, values))
    for bf16 in (False, True):                                # every edge pattern somewhere in a hot and in a cold row
        out.append(MergeCase(8, 100, bf16, "some_unsorted", True, True, "edge"))
        out.append(MergeCase(257, 2, bf16, "some", True, True, "edge"))
    return list(dict.fromkeys(out))


def run_merge(ops, v, n_hot, snap):
    ops.snapshot(v["x"], v["xs"], v["base"], v["w"], v["hot_pos"], v["prev"], v["cold_wire"], v["hot_wire"])
    snap("snapshot")
    if n_hot:
        ops.hot_apply(v["x"], v["xs"], v["base"], v["w"], v["hot_rows"], v["hot_sum"])
        snap("hot_apply")
    ops.flush(v["x"], v["xs"], v["base"], v["w"], v["hot_pos"], v["last"])
    snap("flush")


def numpy_run(run, B, ops, *args):
    """Runs a case on copies of its buffers B -> [(step, {buffer: whole array, guards included})]."""
    B = {k: (None if g is None else g.copy()) for k, g in B.items()}
    out = []
    run(ops, _views(B), *args, lambda step: out.append((step, _snapshots(B))))
    return out


@functools.lru_cache(maxsize=None)
def build_merge(case):
    """-> (buffers, expected results).  The buffers are drawn again until the run has at least one element where
    base + w * S rounded once differs from the two roundings (where the case has such a step at all)."""
    n, stride, k = case.n, case.stride, case.n * case.stride
    n_hot = case.n_hot()
    for attempt in range(64):
        rng = np.random.default_rng([zlib.crc32(case.id.encode()), attempt])
        x, xs = _pair_fill(rng, k, case.values)
        wire = lambda rows: _table(_sum_fill(rng, rows * stride, case.values, case.bf16), stride)
        B = {"x": _table(x, stride), "xs": _table(xs, stride), "base": _table(_base_fill(rng, k, case.values), stride),
             "w": _vector(np.roll(W_CYCLE, -int(rng.integers(5)) if n > 1 else 0)[np.arange(n) % 5]),
             "hot_pos": None, "hot_rows": None, "prev": wire(n) if case.prev else None,
             "last": wire(n) if case.last else None, "cold_wire": None if case.hot == "all_nocold" else wire(n),
             "hot_wire": None, "hot_sum": None}
        if case.hot != "null":
            rows = np.sort(rng.permutation(n)[:n_hot]).astype(np.int64)
            if case.hot in ("some_unsorted", "all", "all_nocold"):
                rows = _unsorted(rng, n, n_hot)
            pos = np.full(n, -1, np.int32)
            pos[rows] = np.arange(n_hot, dtype=np.int32)
            B["hot_pos"] = _vector(pos)
            B["hot_wire"] = wire(max(n_hot, 1))               # hot_pos needs a hot wire even when no row is hot
            if n_hot:
                B["hot_rows"], B["hot_sum"] = _vector(rows), wire(n_hot)
        expect = numpy_run(run_merge, B, NumpyMergeOps(), n_hot)
        if not case.has_two_step() or results_differ(expect, numpy_run(run_merge, B, NumpyMergeOps("contract"), n_hot)):
            return B, expect
    raise AssertionError("%s: no element tells one rounding from two" % case.id)


# ---- n2v_tsum_pack / n2v_tsum_apply, and n2v_merge_pack_rows + n2v_merge_hot_apply as the per-table path
TSUM_COUNTS = ((1,), (5,), (1, 1, 1, 1), (1, 2, 3), (3, 0, 2), (0, 5), (5, 0), (0, 0, 4, 0), (257, 1, 0, 6), (4, 4),
               (8, 3, 1), (), (0,), (0, 0, 0))


class TsumCase(collections.namedtuple("TsumCase", "counts listed stride bf16 values")):
    """counts[t] rows of table t are merged; listed[t]: through a row list that is not ascending, on a table that has
    other rows too (every table another height) — else rows == NULL on a table of counts[t] rows."""

    @property
    def id(self):
        return "%s-s%d-%s-%s" % ("_".join("%d%s" % (c, "L" if l else "N") for c, l in zip(self.counts, self.listed)) or "none",
                                 self.stride, "bf16" if self.bf16 else "f32", self.values)


def tsum_cases():
    out, i = [], 0
    for counts in TSUM_COUNTS:
        for first, step in ((False, 0), (True, 0), (False, 1), (True, 1)):      # all NULL, all listed, mixed both ways
            for bf16 in (False, True):
                listed = tuple(bool((first + step * t) % 2) for t in range(len(counts)))
                out.append(TsumCase(counts, listed, STRIDES[i % len(STRIDES)], bf16, ("randn", "edge")[(i // 2) % 2]))
                i += 1
    for stride in STRIDES:                                    # every stride with table borders inside a block
        for bf16 in (False, True):
            out.append(TsumCase((3, 0, 2), (True, False, True), stride, bf16, "edge"))
            out.append(TsumCase((1, 2, 3), (False, True, False), stride, bf16, "randn"))
    return list(dict.fromkeys(out))


def tsum_tabs(v, n_tabs):
    return [(v["x%d" % t], v["base%d" % t], v["rows%d" % t]) for t in range(n_tabs)]


def run_tsum(ops, v, n_tabs, total, snap):
    tabs = tsum_tabs(v, n_tabs)
    ops.tsum_pack(tabs, v["wire"][:total])
    snap("pack")
    v["wire"][:total] = v["sum"]                              # the all-reduce
    ops.tsum_apply(tabs, v["wire"][:total])
    snap("apply")


def _tsum_buffers(rng, counts, listed, stride, bf16, values, spare=None, repeat=False):
    B = {}
    for t, (c, l) in enumerate(zip(counts, listed)):
        height = c + (1 + t if spare is None else spare) if l else c
        x, base = _pair_fill(rng, height * stride, values)
        B["x%d" % t], B["base%d" % t] = _table(x, stride), _table(base, stride)
        B["rows%d" % t] = _vector(_unsorted(rng, height, c)) if l else None
    if repeat:                                                # for pack only: a row twice
        B["rows0"].v[-1] = B["rows0"].v[0]
    total = sum(counts)
    B["wire"] = _table(_sum_fill(rng, (total + 2) * stride, values, bf16), stride)      # two rows beyond the lists
    B["sum"] = _table(_sum_fill(rng, total * stride, values, bf16), stride)
    return B


@functools.lru_cache(maxsize=None)
def build_tsum(case):
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    B = _tsum_buffers(rng, case.counts, case.listed, case.stride, case.bf16, case.values)
    return B, numpy_run(run_tsum, B, NumpyMergeOps(), len(case.counts), sum(case.counts))


class PackCase(collections.namedtuple("PackCase", "n stride bf16 kind values")):
    """One table and a list of n of its rows, not ascending — kind "perm": a permutation of all n rows; "subset": n of
    n + 1 rows; "repeat": as "subset" with one row twice (pack only: an apply list has no duplicates)."""

    @property
    def id(self):
        return "n%d-s%d-%s-%s-%s" % (self.n, self.stride, "bf16" if self.bf16 else "f32", self.kind, self.values)


def pack_cases():
    out, i = [], 0
    for stride in STRIDES:
        for n in ROWS:
            for bf16 in (False, True):
                out.append(PackCase(n, stride, bf16, ("perm", "subset", "repeat")[i % 3], ("randn", "edge")[(i // 3) % 2]))
                i += 1
    for kind in ("perm", "subset", "repeat"):
        for bf16 in (False, True):
            out.append(PackCase(5, 65, bf16, kind, "edge"))
    return list(dict.fromkeys(out))


def run_per_table(ops, v, n_list, apply, snap):
    """The per-table path of TieredSumMerger: n2v_merge_pack_rows, then n2v_merge_hot_apply with xs aliasing x and a
    weight of one on every row."""
    ops.pack_rows(v["x0"], v["base0"], v["rows0"], v["wire"][:n_list])
    snap("pack")
    if apply:
        v["wire"][:n_list] = v["sum"]
        ops.hot_apply(v["x0"], v["x0"], v["base0"], v["ones"], v["rows0"], v["wire"][:n_list])
        snap("apply")


def run_pack_as_tsum(ops, v, n_list, apply, snap):
    tabs = tsum_tabs(v, 1)
    ops.tsum_pack(tabs, v["wire"][:n_list])
    snap("pack")
    if apply:
        v["wire"][:n_list] = v["sum"]
        ops.tsum_apply(tabs, v["wire"][:n_list])
        snap("apply")


@functools.lru_cache(maxsize=None)
def build_pack(case):
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    B = _tsum_buffers(rng, (case.n,), (True,), case.stride, case.bf16, case.values, spare=0 if case.kind == "perm" else 1,
                      repeat=case.kind == "repeat" and case.n > 1)
    B["ones"] = _vector(np.ones(B["x0"].v.shape[0], F32))
    apply = case.kind != "repeat"
    expect = numpy_run(run_per_table, B, NumpyMergeOps(), case.n, apply)
    return B, expect
