"""Eccentricity statistics on the device: the per-item weights ir / ie / ire / ier of EccenKNN and the per-user ue
(csrc/n2v_eccstats.hip, C-ABI include/n2v_sim.h).

Reference: src/utils.py:53-153 (calculate_ir_from_iu .. calculate_ier_from_iu), which src/main_rec.py:203-301 runs over
the whole ratings file inside fit.  Semantics, quirks included (z(x) = x - (mean / std), the reference's precedence):

    group = distinct (item, timewindow);  unum = its rows;  irg = -log(unum)
    ir  = z(mean of irg over the item's groups)            irz = z(irg) over all groups
    ue  = z(ws / fs),  ws[u] = sum feedback * irz[group],  fs[u] = sum feedback     over the user's rows
    ie  = z(wi / fi),  wi[i] = sum feedback * ue[user],    fi[i] = sum feedback     over the item's rows
    ire = zo(ie * ir)         ier = zo(ie / ir with +-inf -> 0)         zo(x) = (x - min) / (max - min)

Inner indices run in order of first appearance, as eccknn.Trainset's do; duplicate (uid, id) rows count as rows.
Parity: the order of every rounded sum is stated in tests/eccstats_reference.py and the kernels equal that restatement
bit for bit; the restatement is held to output recorded from the reference within a measured bound (pandas sums in
another order).  -log(count) is the host's libm log through a table, i.e. Python's math.log.

The sorts, the unique of the timewindows and the CSR pointers are torch calls; every sum and every statistic is HIP.
There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib

MODES = ("ir", "ie", "ire", "ier")
Z, ZERO_ONE, MUL, DIV, DIV_INF0 = 0, 1, 2, 3, 4      # N2V_ECCSTATS_*
INTERMEDIATES = ("unum", "irg", "irmean", "irz", "ws", "fs", "uer", "wi", "fi", "ier_", "q")


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("n2v_hip.eccstats: no GPU visible (torch.cuda.is_available() is False); no CPU fallback")


def timewindow_utc(timestamps):
    """year * 100 + month of unix timestamps (seconds), int64.

    The reference's mark_timewindow uses time.localtime, i.e. the zone of whatever machine runs it.  UTC is the stated,
    reproducible choice here; a file whose windows were cut in another zone should carry the timewindow column itself."""
    t = np.asarray(timestamps).astype(np.int64).astype("datetime64[s]")
    months = t.astype("datetime64[M]").astype(np.int64)          # months since 1970-01
    return (1970 + months // 12) * 100 + months % 12 + 1


def first_appearance(raw):
    """(inner index of every entry int64, raw ids by inner index as a list): order of first appearance."""
    raw = np.asarray(raw)
    uniq, first, inv = np.unique(raw, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    return rank[inv.reshape(-1)], uniq[order].tolist()


# ---- C-ABI wrappers (device tensors in, device tensors out) -----------------------------------------------------------

def log_table(length):
    """Host fp64 tensor: table[c] = -log(c) by the host's libm, c < length."""
    t = torch.empty(int(length), dtype=torch.float64)
    _lib.check(_lib.load().n2v_eccstats_log_table(int(length), t.data_ptr()))
    return t


def groups(key_sorted, perm, n_tw, n_items):
    """(row_group int32[n] by row, group_begin int64[n_groups + 1], unum int64[n_groups], item_gptr int64[n_items + 1],
    largest unum).  Reads the two counts back, which waits for the stream."""
    lib = _lib.load()
    dev, n = key_sorted.device, key_sorted.numel()
    with torch.cuda.device(dev):
        scratch = torch.empty(int(lib.n2v_eccstats_groups_scratch(n)), dtype=torch.int64, device=dev)
        row_group = torch.empty(n, dtype=torch.int32, device=dev)
        group_begin = torch.empty(n + 1, dtype=torch.int64, device=dev)
        unum = torch.empty(n, dtype=torch.int64, device=dev)
        item_gptr = torch.empty(n_items + 1, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.n2v_eccstats_groups(_lib.ptr(key_sorted), _lib.ptr(perm), n, int(n_tw), int(n_items), _lib.ptr(scratch),
                                           _lib.ptr(row_group), _lib.ptr(group_begin), _lib.ptr(unum), _lib.ptr(item_gptr),
                                           _lib.ptr(counts), _lib.stream_ptr(dev)))
    n_groups, largest = counts.tolist()
    return row_group, group_begin[:n_groups + 1], unum[:n_groups], item_gptr, largest


def irg_of(unum, table):
    """irg fp64[n_groups] = table[unum] for a device copy of log_table(); raises if a count is outside the table."""
    lib = _lib.load()
    dev = unum.device
    with torch.cuda.device(dev):
        irg = torch.empty(unum.numel(), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.n2v_eccstats_irg(_lib.ptr(unum), unum.numel(), _lib.ptr(table), table.numel(), _lib.ptr(irg),
                                        _lib.ptr(status), _lib.stream_ptr(dev)))
    return irg, status


def segsum(seg_ptr, a, perm=None, idx=None, g=None, mean=False):
    """(sum a, sum a * g[idx]) per segment, left to right; the second is None without g."""
    lib = _lib.load()
    dev, n_seg = a.device, seg_ptr.numel() - 1
    with torch.cuda.device(dev):
        scratch = torch.empty(n_seg + 1, dtype=torch.int32, device=dev)
        out = torch.empty(n_seg, dtype=torch.float64, device=dev)
        wout = torch.empty(n_seg, dtype=torch.float64, device=dev) if g is not None else None
        _lib.check(lib.n2v_eccstats_segsum(_lib.ptr(seg_ptr), n_seg, _lib.ptr(perm), _lib.ptr(a), a.numel(), _lib.ptr(idx),
                                           _lib.ptr(g), g.numel() if g is not None else 0, int(bool(mean)), _lib.ptr(scratch),
                                           _lib.ptr(out), _lib.ptr(wout), _lib.stream_ptr(dev)))
    return out, wout


def moments(x):
    """Device fp64[8]: sum, mean, ssd, var, std, min, max, n."""
    lib = _lib.load()
    dev = x.device
    with torch.cuda.device(dev):
        scratch = torch.empty(int(lib.n2v_eccstats_moments_scratch(x.numel())), dtype=torch.float64, device=dev)
        stats = torch.empty(8, dtype=torch.float64, device=dev)
        _lib.check(lib.n2v_eccstats_moments(_lib.ptr(x), x.numel(), _lib.ptr(scratch), _lib.ptr(stats), _lib.stream_ptr(dev)))
    return stats


def finish(op, a, b=None, stats=None):
    lib = _lib.load()
    dev = a.device
    with torch.cuda.device(dev):
        out = torch.empty_like(a)
        _lib.check(lib.n2v_eccstats_finish(op, _lib.ptr(a), _lib.ptr(b), _lib.ptr(stats), a.numel(), _lib.ptr(out),
                                           _lib.stream_ptr(dev)))
    return out


def z_score(x):
    return finish(Z, x, stats=moments(x))


def zero_one(x):
    return finish(ZERO_ONE, x, stats=moments(x))


# ---- the statistics ---------------------------------------------------------------------------------------------------

def _csr_ptr(ids, n):
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=ids.device)
    torch.cumsum(torch.bincount(ids, minlength=n), 0, out=ptr[1:])
    return ptr


def prepare(user, item, timewindow, n_items):
    """The sorts (torch): (key_sorted, perm of the groups, n_tw, perm_u, perm_i).  user / item: int64 device tensors of
    inner ids; timewindow: int64 device tensor."""
    tw_values, tw_rank = torch.unique(timewindow, sorted=True, return_inverse=True)
    n_tw = tw_values.numel()
    if n_items * n_tw >= 2 ** 62:
        raise ValueError("eccstats: %d items x %d timewindows overflow the sort key" % (n_items, n_tw))
    key_sorted, perm_g = torch.sort(item * n_tw + tw_rank, stable=True)
    perm_u = torch.sort(user, stable=True)[1]
    perm_i = torch.sort(item, stable=True)[1]
    return key_sorted, perm_g, n_tw, perm_u, perm_i


def device_statistics(user, item, feedback, prep, n_users, n_items):
    """Every kernel of the chain on device tensors; returns a dict of device tensors (all of INTERMEDIATES, MODES, ue)
    and the status word of the log table."""
    key_sorted, perm_g, n_tw, perm_u, perm_i = prep
    dev = feedback.device
    row_group, _, unum, item_gptr, largest = groups(key_sorted, perm_g, n_tw, n_items)
    irg, status = irg_of(unum, log_table(largest + 1).to(dev))
    irmean, _ = segsum(item_gptr, irg, mean=True)
    ir = z_score(irmean)
    irz = z_score(irg)
    user32 = user.to(torch.int32)
    fs, ws = segsum(_csr_ptr(user, n_users), feedback, perm=perm_u, idx=row_group, g=irz)
    uer = finish(DIV, ws, fs)
    ue = z_score(uer)
    fi, wi = segsum(_csr_ptr(item, n_items), feedback, perm=perm_i, idx=user32, g=ue)
    ier_ = finish(DIV, wi, fi)
    ie = z_score(ier_)
    ire = zero_one(finish(MUL, ie, ir))
    q = finish(DIV_INF0, ie, ir)
    ier = zero_one(q)
    loc = locals()
    return {k: loc[k] for k in INTERMEDIATES + MODES + ("ue",)}, status


class ItemStatistics:
    """ir, ie, ire, ier: fp64 arrays over `items` (raw ids by inner index); ue over `users`.  `intermediates` (when
    asked for): unum, irg, irz per group, irmean, wi, fi, ier_ (= wi / fi), q per item, ws, fs, uer (= ws / fs) per
    user."""

    def __init__(self, users, items, cols, intermediates):
        self.users, self.items = users, items
        self.ir, self.ie, self.ire, self.ier, self.ue = (cols[k] for k in MODES + ("ue",))
        self.intermediates = intermediates

    def weights(self, mode):
        """{raw item id: weight}, the dict EccenKNN.fit accepts."""
        if mode not in MODES:
            raise ValueError("eccstats: mode %r, expected one of %s" % (mode, ", ".join(MODES)))
        return dict(zip(self.items, getattr(self, mode).tolist()))


def item_statistics(uid, id, feedback, timewindow, device="cuda:0", intermediates=False):
    """The statistics of rows (uid[k], id[k], feedback[k], timewindow[k]).  uid / id: sequences of raw ids (any one
    hashable, sortable type per column); feedback: numbers; timewindow: integers (see timewindow_utc)."""
    _require_gpu()
    fb = np.ascontiguousarray(feedback, dtype=np.float64)
    tw = np.ascontiguousarray(timewindow, dtype=np.int64)
    if not (len(uid) == len(id) == len(fb) == len(tw)) or len(fb) == 0:
        raise ValueError("item_statistics: %d uid, %d id, %d feedback, %d timewindow" % (len(uid), len(id), len(fb), len(tw)))
    u, users = first_appearance(uid)
    i, items = first_appearance(id)
    dev = torch.device(device)
    to = lambda a: torch.from_numpy(a).to(dev)
    with torch.cuda.device(dev):
        du, di = to(u), to(i)
        cols, status = device_statistics(du, di, to(fb), prepare(du, di, to(tw), len(items)), len(users), len(items))
        if int(status.item()):
            raise _lib.N2VError("eccstats: a group count outside the log table")
        host = {k: v.cpu().numpy() for k, v in cols.items()}
    return ItemStatistics(users, items, host, {k: host[k] for k in INTERMEDIATES} if intermediates else None)
