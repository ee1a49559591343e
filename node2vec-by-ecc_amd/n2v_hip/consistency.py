"""Eccentricity consistency on the device: how ir / ie / ue septiles move between two periods of a log, and the per-user
"ie profile" with the feature rows built from it (csrc/n2v_ecccons.hip, C-ABI include/n2v_sim.h).

Reference: src/utils.py:163-226 (septile_for_plot, everything before the drawing), :272-279 (mark_septile), :326-379
(calculate_uie_dist, calculate_uvec, make_data, calculate_iu_uvec).

    period      the rows whose timewindow lies in an inclusive (lo, hi) range (None: open), in file order.  The
                reference's ml branch `> 201100 & < 201299` is (201101, 201298); its 30Music branch `<= seg` / `> seg` is
                (None, seg) / (seg + 1, None)
    statistics  eccstats over the period's rows alone, with the period's own inner ids (first appearance inside it)
    support     rows of the item (ir, ie) or user (ue) inside the period, `> min_count` in both periods
    bins        eccsplit's mark kernels over each joined column on its own.  THE ONE DELIBERATE DEFINITION: the reference's
                quicksort leaves ties open; equal values rank by ascending raw id as Python's sorted orders the ids, in
                both columns
    tables      count[a - 1][b - 1], count_sum[a - 1] (row sums), ratio = count * 1.0 / count_sum (NaN in an empty row)
    profile     per user the share of rows (weighted: of feedback, summed in file order) per bin of the item's ie
                among n_bins rank bins of all items; a user without a binned row gets NaN
    features    profile[user] ++ item vector (fp32 widened), rows without a vector dropped; without vectors
                profile[user] ++ [float(int(raw id))]

The sorts, masks and index plumbing are torch calls; joins, tables, profiles and feature rows are HIP.  Integer inputs
are checked by kernels that return a status word: a malformed input is a ValueError.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from . import eccsplit as _eccsplit
from . import eccstats as _eccstats

KINDS = ("ir", "ie", "ue")
MAX_BINS = 256              # N2V_ECCCONS_MAX_BINS
BAD_RANGE, BAD_PTR = 1, 2   # N2V_ECCCONS_BAD_*
LIMIT = 2 ** 31 - 1


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("n2v_hip.consistency: no GPU visible (torch.cuda.is_available() is False); no CPU fallback")


# ---- host checks (every ValueError of the public functions comes before any launch) ------------------------------------

def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def parse_interval(text):
    """'LO:HI' -> (lo, hi), inclusive; an empty side is open: '201101:201298', ':201407', '201408:'."""
    parts = str(text).split(":")
    if len(parts) != 2:
        raise ValueError("consistency: interval %r, expected LO:HI" % (text,))
    try:
        lo, hi = (int(p) if p.strip() else None for p in parts)
    except ValueError:
        raise ValueError("consistency: interval %r, expected integers LO:HI" % (text,))
    return check_interval((lo, hi))


def seg_point_intervals(seg):
    """The reference's 30Music cut: (None, seg), (seg + 1, None)."""
    if not _is_int(seg):
        raise ValueError("consistency: seg point %r is not an integer" % (seg,))
    return (None, int(seg)), (int(seg) + 1, None)


def check_interval(rng):
    try:
        lo, hi = rng
    except (TypeError, ValueError):
        raise ValueError("consistency: period %r, expected (lo, hi)" % (rng,))
    for v in (lo, hi):
        if v is not None and not _is_int(v):
            raise ValueError("consistency: period bound %r is not an integer" % (v,))
    if lo is None and hi is None:
        raise ValueError("consistency: a period needs a bound")
    if lo is not None and hi is not None and lo > hi:
        raise ValueError("consistency: period %r is empty" % (rng,))
    return (None if lo is None else int(lo), None if hi is None else int(hi))


def _check_bins(n, what="n"):
    if not _is_int(n) or not 1 <= int(n) <= MAX_BINS:
        raise ValueError("consistency: %s = %r bins, expected an integer in 1 .. %d" % (what, n, MAX_BINS))
    return int(n)


def _in_period(tw, rng):
    keep = np.ones(len(tw), dtype=bool) if not isinstance(tw, torch.Tensor) else torch.ones_like(tw, dtype=torch.bool)
    if rng[0] is not None:
        keep &= tw >= rng[0]
    if rng[1] is not None:
        keep &= tw <= rng[1]
    return keep


def _rows(uid, id, feedback, timewindow, what):
    fb = np.ascontiguousarray(feedback, dtype=np.float64).reshape(-1)
    tw = np.ascontiguousarray(timewindow, dtype=np.int64).reshape(-1)
    if not len(uid) == len(id) == len(fb) == len(tw) or len(fb) == 0:
        raise ValueError("%s: %d uid, %d id, %d feedback, %d timewindow" % (what, len(uid), len(id), len(fb), len(tw)))
    if len(fb) > LIMIT // 2:
        raise ValueError("%s: %d rows, at most 2^30 - 1" % (what, len(fb)))
    return fb, tw


# ---- C-ABI wrappers (device tensors in, device tensors out) -----------------------------------------------------------

def _status(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _check_i32(a, lo, hi, status):
    _lib.check(_lib.load().n2v_ecccons_check_i32(_lib.ptr(a), a.numel(), int(lo), int(hi), _lib.ptr(status), _lib.stream_ptr(a.device)))


def _check_i64(a, lo, hi, status):
    _lib.check(_lib.load().n2v_ecccons_check_i64(_lib.ptr(a), a.numel(), int(lo), int(hi), _lib.ptr(status), _lib.stream_ptr(a.device)))


def _verdict(status, what):
    s = int(status.item())
    if s & BAD_PTR:
        raise ValueError("consistency: %s: the row pointers do not ascend from 0 to the number of rows" % what)
    if s & BAD_RANGE:
        raise ValueError("consistency: %s: an integer outside its range" % what)


def join(v1, v2, c1, c2, min_count):
    """(ids int64[m] ascending, values 1, values 2) of the entities with c1 > min_count and c2 > min_count; fp64 / int64
    device tensors over one index space.  Reads m back."""
    lib = _lib.load()
    dev, n = v1.device, v1.numel()
    if not (v2.numel() == c1.numel() == c2.numel() == n) or not _is_int(min_count) or min_count < 0:
        raise ValueError("consistency: join of %d, %d values and %d, %d counts, min_count %r" % (n, v2.numel(), c1.numel(), c2.numel(), min_count))
    with torch.cuda.device(dev):
        scratch = torch.empty(int(lib.n2v_eccsplit_scratch(n)), dtype=torch.int64, device=dev)
        ids = torch.empty(n, dtype=torch.int64, device=dev)
        o1, o2 = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.n2v_ecccons_join(_lib.ptr(v1), _lib.ptr(v2), _lib.ptr(c1), _lib.ptr(c2), n, int(min_count), _lib.ptr(scratch),
                                        _lib.ptr(ids), _lib.ptr(o1), _lib.ptr(o2), _lib.ptr(count), _lib.stream_ptr(dev)))
        m = int(count.item())
    return ids[:m], o1[:m], o2[:m]


def crosstab(bins1, bins2, n):
    """(count int64[n][n], count_sum int64[n], ratio fp64[n][n]) of int32 device bins in 1 .. n; ValueError for a bin
    outside."""
    lib = _lib.load()
    n = _check_bins(n)
    dev, m = bins1.device, bins1.numel()
    if bins2.numel() != m or bins1.dtype != torch.int32 or bins2.dtype != torch.int32:
        raise ValueError("consistency: crosstab of %d and %d bins (int32)" % (m, bins2.numel()))
    with torch.cuda.device(dev):
        status = _status(dev)
        _check_i32(bins1, 1, n, status)
        _check_i32(bins2, 1, n, status)
        _verdict(status, "crosstab bins (1 .. %d)" % n)
        count = torch.empty((n, n), dtype=torch.int64, device=dev)
        count_sum = torch.empty(n, dtype=torch.int64, device=dev)
        ratio = torch.empty((n, n), dtype=torch.float64, device=dev)
        _lib.check(lib.n2v_ecccons_crosstab(_lib.ptr(bins1), _lib.ptr(bins2), m, n, _lib.ptr(count), _lib.ptr(count_sum),
                                            _lib.ptr(ratio), _lib.stream_ptr(dev)))
    return count, count_sum, ratio


def profile(user_ptr, perm, item, feedback, item_bin, n_bins, weighted=False):
    """fp64[n_users][n_bins] device.  user_ptr int64[n_users + 1], perm int64[n_rows] (rows grouped by user, file order
    inside), item int64[n_rows], feedback fp64[n_rows], item_bin int32[n_items] in 0 .. n_bins.  ValueError for pointers
    that do not ascend from 0 to n_rows or an integer outside its range."""
    lib = _lib.load()
    n_bins = _check_bins(n_bins, "n_bins")
    dev, n_users, n_rows, n_items = item.device, user_ptr.numel() - 1, item.numel(), item_bin.numel()
    if n_users < 1 or n_items < 1 or perm.numel() != n_rows or feedback.numel() != n_rows or item_bin.dtype != torch.int32:
        raise ValueError("consistency: profile of %d users, %d items, %d rows, %d perm, %d feedback" %
                         (n_users, n_items, n_rows, perm.numel(), feedback.numel()))
    with torch.cuda.device(dev):
        status = _status(dev)
        _lib.check(lib.n2v_ecccons_check_ptr(_lib.ptr(user_ptr), n_users, n_rows, _lib.ptr(status), _lib.stream_ptr(dev)))
        _check_i64(perm, 0, n_rows - 1, status)
        _check_i64(item, 0, n_items - 1, status)
        _check_i32(item_bin, 0, n_bins, status)
        _verdict(status, "profile")
        out = torch.empty((n_users, n_bins), dtype=torch.float64, device=dev)
        _lib.check(lib.n2v_ecccons_profile(_lib.ptr(user_ptr), _lib.ptr(perm), n_users, _lib.ptr(item), _lib.ptr(feedback), n_rows,
                                           _lib.ptr(item_bin), n_items, n_bins, int(bool(weighted)), _lib.ptr(out),
                                           _lib.stream_ptr(dev)))
    return out


def feature_rows(user, item, feedback, prof, vec_slot=None, vec=None, item_value=None):
    """(X fp64[kept][n_bins + d or 1], y fp64[kept], rows int64[kept]) device.  user / item int64[n_rows] inner ids, prof
    fp64[n_users][n_bins]; vec fp32[n_vec][d] with vec_slot int32[n_items] (-1: the item has no vector, its rows are
    dropped), or item_value fp64[n_items].  ValueError for an id or a slot outside its range.  Reads `kept` back."""
    lib = _lib.load()
    dev, n_rows = user.device, user.numel()
    n_users, n_bins = prof.shape
    n_bins = _check_bins(n_bins, "n_bins")
    if (vec is None) == (item_value is None) or (vec is not None and vec_slot is None):
        raise ValueError("consistency: features need item vectors with their slots, or item values")
    n_items = (vec_slot if vec is not None else item_value).numel()
    n_vec, d = (vec.shape[0], vec.shape[1]) if vec is not None else (0, 1)
    if item.numel() != n_rows or feedback.numel() != n_rows or n_rows < 1 or n_items < 1 or n_users < 1 or d < 1:
        raise ValueError("consistency: features of %d user, %d item, %d feedback rows, %d items" % (n_rows, item.numel(), feedback.numel(), n_items))
    with torch.cuda.device(dev):
        status = _status(dev)
        _check_i64(user, 0, n_users - 1, status)
        _check_i64(item, 0, n_items - 1, status)
        if vec is not None:
            _check_i32(vec_slot, -1, n_vec - 1, status)
        _verdict(status, "features")
        scratch = torch.empty(int(lib.n2v_eccsplit_scratch(n_rows)), dtype=torch.int64, device=dev)
        rows = torch.empty(n_rows, dtype=torch.int64, device=dev)
        y = torch.empty(n_rows, dtype=torch.float64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        st = _lib.stream_ptr(dev)
        _lib.check(lib.n2v_ecccons_feature_rows(_lib.ptr(item), _lib.ptr(feedback), n_rows, n_items, _lib.ptr(vec_slot), n_vec,
                                                _lib.ptr(scratch), _lib.ptr(rows), _lib.ptr(y), _lib.ptr(count), st))
        kept = int(count.item())
        X = torch.empty((kept, n_bins + d), dtype=torch.float64, device=dev)
        if kept:
            _lib.check(lib.n2v_ecccons_features(_lib.ptr(rows), kept, _lib.ptr(user), _lib.ptr(item), n_rows, n_users, n_items,
                                                _lib.ptr(prof), n_bins, _lib.ptr(vec_slot), _lib.ptr(vec), n_vec, d,
                                                _lib.ptr(item_value), _lib.ptr(X), st))
    return X, y[:kept], rows[:kept]


# ---- transitions ------------------------------------------------------------------------------------------------------

class Table:
    """One kind's result: count / count_sum / ratio (numpy, index [a - 1][b - 1] = bin a in the first period, bin b in
    the second), ids (raw ids joined, ascending inner id of the file), v1 / v2 (their values), bins1 / bins2."""

    def __init__(self, ids, v1, v2, bins1, bins2, count, count_sum, ratio):
        self.ids, self.v1, self.v2, self.bins1, self.bins2 = ids, v1, v2, bins1, bins2
        self.count, self.count_sum, self.ratio = count, count_sum, ratio

    def frame(self):
        """The reference's long table: rows (bin1, bin2, count, count_sum, ratio) of the non-empty cells, ascending."""
        a, b = np.nonzero(self.count)
        return np.rec.fromarrays([a + 1, b + 1, self.count[a, b], self.count_sum[a], self.ratio[a, b]],
                                 names="bin1,bin2,count,count_sum,ratio")


class Transitions:
    def __init__(self, n, min_count, first, second, tables):
        self.n, self.min_count, self.first, self.second = n, min_count, first, second
        self.ir, self.ie, self.ue = (tables[k] for k in KINDS)

    def frame(self, kind):
        if kind not in KINDS:
            raise ValueError("consistency: kind %r, expected one of %s" % (kind, ", ".join(KINDS)))
        return getattr(self, kind).frame()


def _period(du, di, dfb, dtw, rng, n_users, n_items):
    """The statistics of one period spread over the file's inner ids (NaN where absent) and the supports."""
    lib = _lib.load()
    dev = du.device
    rows = torch.nonzero(_in_period(dtw, rng)).reshape(-1)                # ascending
    pu, pi = du[rows], di[rows]
    first = torch.full((n_users + n_items,), _eccsplit.NONE, dtype=torch.int64, device=dev)
    _lib.check(lib.n2v_eccsplit_first(_lib.ptr(rows), None, rows.numel(), _lib.ptr(du), _lib.ptr(di), du.numel(), n_users, n_items,
                                      _lib.ptr(first), _lib.stream_ptr(dev)))
    present = (first != _eccsplit.NONE)
    nu, ni = int(present[:n_users].sum()), int(present[n_users:].sum())
    local, order = [], []
    for f in (first[:n_users], first[n_users:]):                          # the period's own inner ids: first appearance
        o = torch.sort(f)[1]
        loc = torch.empty_like(o)
        loc[o] = torch.arange(o.numel(), dtype=torch.int64, device=dev)
        local.append(loc)
        order.append(o)
    lu, li = local[0][pu], local[1][pi]
    fb = dfb[rows].contiguous()
    cols, status = _eccstats.device_statistics(lu, li, fb, _eccstats.prepare(lu, li, dtw[rows], ni), nu, ni)
    if int(status.item()):
        raise _lib.N2VError("consistency: a group count outside the log table")
    out = {}
    for kind in KINDS:
        o, n_loc, n_all = (order[0], nu, n_users) if kind == "ue" else (order[1], ni, n_items)
        g = torch.full((n_all,), float("nan"), dtype=torch.float64, device=dev)
        g[o[:n_loc]] = cols[kind]
        out[kind] = g
    return out, torch.bincount(pu, minlength=n_users), torch.bincount(pi, minlength=n_items)


def transitions(uid, id, feedback, timewindow, first, second, n=7, min_count=4, device="cuda:0"):
    """The n x n transition tables of ir, ie and ue between the periods `first` and `second` (inclusive (lo, hi)
    timewindow ranges, None: open) of the rows (uid[k], id[k], feedback[k], timewindow[k]).  An empty period is a
    ValueError; an empty join gives all-zero counts and NaN ratios."""
    fb, tw = _rows(uid, id, feedback, timewindow, "transitions")
    first, second = check_interval(first), check_interval(second)
    n = _check_bins(n)
    if not _is_int(min_count) or min_count < 0:
        raise ValueError("consistency: min_count = %r, expected an integer >= 0" % (min_count,))
    for name, rng in (("first", first), ("second", second)):
        if not _in_period(tw, rng).any():
            raise ValueError("consistency: the %s period %r has no rows" % (name, rng))
    u, users = _eccstats.first_appearance(uid)
    i, items = _eccstats.first_appearance(id)
    _require_gpu()
    dev = torch.device(device)
    to = lambda a: torch.from_numpy(a).to(dev)
    tables = {}
    with torch.cuda.device(dev):
        du, di, dfb, dtw = to(u), to(i), to(fb), to(tw)                   # the rows are uploaded once
        per = [_period(du, di, dfb, dtw, rng, len(users), len(items)) for rng in (first, second)]
        for kind in KINDS:
            names, sup = (users, 1) if kind == "ue" else (items, 2)
            ids, v1, v2 = join(per[0][0][kind], per[1][0][kind], per[0][sup], per[1][sup], int(min_count))
            raw = [names[k] for k in ids.tolist()]
            if raw:
                tr = _eccsplit.tie_rank_of(raw)
                b1 = _eccsplit._mark_device(v1.contiguous(), n, tr)
                b2 = _eccsplit._mark_device(v2.contiguous(), n, tr)
            else:
                b1 = b2 = torch.empty(0, dtype=torch.int32, device=dev)
            count, count_sum, ratio = crosstab(b1, b2, n)
            host = lambda t: t.cpu().numpy()
            tables[kind] = Table(raw, host(v1), host(v2), host(b1), host(b2), host(count), host(count_sum), host(ratio))
    return Transitions(n, int(min_count), first, second, tables)


# ---- profiles and features ----------------------------------------------------------------------------------------------

class ProfileResult:
    """users: raw uids by row of `profile` (fp64 n_users x n_bins); items / item_bin: raw ids and their ie bin; ie."""

    def __init__(self, users, items, ie, item_bin, profile, n_bins, weighted):
        self.users, self.items, self.ie, self.item_bin, self.profile = users, items, ie, item_bin, profile
        self.n_bins, self.weighted = n_bins, weighted


def user_ie_profile(uid, id, feedback, timewindow, n_bins=100, weighted=False, device="cuda:0"):
    """Each user's rows binned by the rank bin (1 .. n_bins) of the rated item's ie and normalised to a distribution."""
    fb, tw = _rows(uid, id, feedback, timewindow, "user_ie_profile")
    n_bins = _check_bins(n_bins, "n_bins")
    u, users = _eccstats.first_appearance(uid)
    i, items = _eccstats.first_appearance(id)
    tr = _eccsplit._check_mark(len(items), n_bins, _eccsplit.tie_rank_of(items))
    _require_gpu()
    dev = torch.device(device)
    to = lambda a: torch.from_numpy(a).to(dev)
    with torch.cuda.device(dev):
        du, di, dfb = to(u), to(i), to(fb)
        prep = _eccstats.prepare(du, di, to(tw), len(items))
        cols, status = _eccstats.device_statistics(du, di, dfb, prep, len(users), len(items))
        if int(status.item()):
            raise _lib.N2VError("consistency: a group count outside the log table")
        item_bin = _eccsplit._mark_device(cols["ie"], n_bins, tr)
        prof = profile(_eccstats._csr_ptr(du, len(users)), prep[3], di, dfb, item_bin, n_bins, weighted)
        return ProfileResult(users, items, cols["ie"].cpu().numpy(), item_bin.cpu().numpy(), prof.cpu().numpy(), n_bins, bool(weighted))


def _vector_of(item_vectors, raw):
    for key in (raw, str(raw)):
        try:
            if key in item_vectors:
                return np.asarray(item_vectors[key], dtype=np.float32).reshape(-1)
        except TypeError:
            pass
    return None


def features(profile_result, uid, id, feedback, item_vectors=None, device="cuda:0"):
    """(X fp64, y fp64, kept row numbers): X[t] = profile[uid of row k] ++ item_vectors[id of row k] for the rows k whose
    item has a vector (a KeyedVectors or {raw id: vector}; a key is looked up as it is, then as str), or, with no
    item_vectors, profile[uid] ++ [float(int(id))] for every row."""
    fb = np.ascontiguousarray(feedback, dtype=np.float64).reshape(-1)
    if not len(uid) == len(id) == len(fb) or len(fb) == 0:
        raise ValueError("features: %d uid, %d id, %d feedback" % (len(uid), len(id), len(fb)))
    prof = np.ascontiguousarray(profile_result.profile, dtype=np.float64)
    pos = {r: k for k, r in enumerate(profile_result.users)}
    u_of, users = _eccstats.first_appearance(uid)
    try:
        u = np.array([pos[r] for r in users], dtype=np.int64)[u_of]
    except KeyError as e:
        raise ValueError("features: uid %r has no profile" % (e.args[0],))
    i, items = _eccstats.first_appearance(id)
    vec = slot = value = None
    if item_vectors is None:
        try:
            value = np.array([float(int(r)) for r in items], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("features: without item vectors every id must be an integer")
        d = 1
    else:
        found = [_vector_of(item_vectors, r) for r in items]
        have = [v for v in found if v is not None]
        d = len(have[0]) if have else int(getattr(item_vectors, "vector_size", 0) or 0)
        if any(len(v) != d for v in have):
            raise ValueError("features: item vectors of different lengths")
        if not have:
            return np.zeros((0, prof.shape[1] + d)), np.zeros(0), np.zeros(0, dtype=np.int64)
        vec = np.ascontiguousarray(np.stack(have), dtype=np.float32)
        slot = np.full(len(items), -1, dtype=np.int32)
        slot[[k for k, v in enumerate(found) if v is not None]] = np.arange(len(have), dtype=np.int32)
    _require_gpu()
    dev = torch.device(device)
    to = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    with torch.cuda.device(dev):
        X, y, rows = feature_rows(to(u), to(i), to(fb), to(prof), to(slot), to(vec), to(value))
        return X.cpu().numpy(), y.cpu().numpy(), rows.cpu().numpy()
