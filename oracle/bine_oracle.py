"""CPU restatement of the reference's BiNE path — TEST INFRASTRUCTURE ONLY (never imported by the product).

Parity status: **unpinned at the bit level, by construction of the reference.**  Its BiNE files do not
import on Python 3 (`from collections import Iterable` src/bine_graph.py:14; `keys.sort()` on dict views
src/bine_graph_utils.py:53-54; modules `graph`, `lsh`, `data_utils`, `graph_utils` that do not exist under
those names src/bine_train.py:9-10, src/bine_graph_utils.py:4,8; datasketch absent), hold no fixtures, and
draw from an unseeded `random.Random()` default argument (src/bine_graph.py:169,224,334).  Two layers:

 (L) *literal* restatements of the reference text (materialised projection rows, `random`-module draws,
     networkx-1.11 `hits` power iteration, numpy skip_gram / KL_divergence / train loop) — what the reference
     computes, in distribution;
 (P) *Philox* restatements of the device algorithm (same counters, same arithmetic) — what the HIP kernels
     must reproduce bit for bit (walks, pools, sampled occurrences, contexts, negatives) or to fp64 rounding
     (training).
tests/ check (P) == HIP exactly and (P) ~ (L) statistically (chi-square on next-vertex and length
distributions), so the chain reference-text -> (L) -> (P) -> HIP is closed without the reference running.

Negatives of a short pool follow the reference's rule: a pool row holds a prefix of `valid` vertices, then -1
(LSH pools of a side smaller than pool_size), and an occurrence draws min(ns, valid) distinct slots of that prefix,
as `random.sample(negs, min(num_negs, len(negs)))` does (src/bine_graph_utils.py:185).  A full row draws exactly
the slots it always did.
"""
import math

import numpy as np

from oracle.n2v_oracle import philox4x32_10

LN10 = math.log(10, math.e)  # src/bine_train.py:300
MAX_TRIALS = 1 << 16
POOL_TRIALS = 16


def _u53(a, b):
    return ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0


def _philox(seed, c0, c1, c2, c3):
    return philox4x32_10((c0 & 0xFFFFFFFF, c1 & 0xFFFFFFFF, c2 & 0xFFFFFFFF, c3 & 0xFFFFFFFF),
                         (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


# ------------------------------------------------------------------------------- (L) HITS, networkx 1.11
def hits_nx111(row_ptr, col, w, max_iter=100, tol=1.0e-8):
    """networkx 1.11 `hits(G)` (third-party, pinned by requirements.txt:networkx==1.11; restated from its
    published source): h = 1/n; repeat {a = M^T h_last; h = M a; h /= max h; a /= max a;
    err = sum |h - h_last|} until err < tol; raises after max_iter.  Returns the un-normalised a
    (the final division by sum(a) cancels in the per-side min-max scaling of
    src/bine_graph_utils.py:76-86)."""
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    h = np.full(n, 1.0 / n)
    for it in range(max_iter):
        hlast = h
        a = np.zeros(n)
        np.add.at(a, col, hlast[rows] * w)          # a[nbr] += hlast[n] * w
        h = np.zeros(n)
        np.add.at(h, rows, a[col] * w)              # h[n] += a[nbr] * w
        h = h * (1.0 / h.max())
        a = a * (1.0 / a.max())
        err = np.abs(h - hlast).sum()
        if err < tol:
            return a, it + 1
    raise RuntimeError("HITS: power iteration failed to converge in %d iterations" % max_iter)


def walk_counts(a, lo, hi, maxT, minT):
    """src/bine_graph_utils.py:62-86 (per-side min-max) + src/bine_graph.py:358 (ceil, floor at minT)."""
    seg = a[lo:hi]
    mx, mn = max(0.0, float(seg.max())), min(100000.0, float(seg.min()))
    span = mx - mn
    auth = (seg - mn) / span if span != 0 else np.zeros(hi - lo)
    return np.maximum(np.ceil(maxT * auth).astype(np.int64), minT), auth


# ------------------------------------------------------------------------------- (L) literal walk
def projection_rows(row_ptr, col, v):
    """Row v of the reference's `matrix` (src/bine_graph_utils.py:223-241): the distinct column indices of
    row v of A*A^T, ascending, v itself included when v has any neighbour."""
    out = set()
    for m in col[row_ptr[v]:row_ptr[v + 1]]:
        out.update(int(x) for x in col[row_ptr[m]:row_ptr[m + 1]])
    return sorted(out)


def literal_walk(matrix_rows, start, percentage, rand, max_tokens=None):
    """random_walk_restart_for_large_bipartite_graph (src/bine_graph.py:263-308) with alpha = 0.
    `matrix_rows(v)` -> list as above; len(G[cur]) is that list without cur (self loops removed,
    src/bine_graph.py:94,128-131).  max_tokens is a harness guard only (the reference has none)."""
    path = [start]
    while len(path) < 1 or rand.random() > percentage:
        if max_tokens is not None and len(path) >= max_tokens:
            break
        cur = path[-1]
        neighbors = matrix_rows(cur)
        if len([x for x in neighbors if x != cur]) > 0:
            if rand.random() >= 0:                      # alpha = 0: always true, consumes a draw
                add_node = rand.choice(neighbors)
                while add_node == cur:
                    add_node = rand.choice(neighbors)
                path.append(add_node)
        else:
            break
    return path


# ------------------------------------------------------------------------------- (P) device walk
def two_hop_prefix(row_ptr, col):
    deg = np.diff(row_ptr)
    return np.concatenate([[0], np.cumsum(deg[col])]).astype(np.int64)


def walk_length(row_ptr, cum2, node, gw, percentage, max_len, seed):
    rb, re = int(row_ptr[node]), int(row_ptr[node + 1])
    paths = int(cum2[re] - cum2[rb])
    length = 1
    if paths - (re - rb) > 0:
        t = 0
        while length < max_len:
            r = _philox(seed, gw, gw >> 32, t, 0)
            if _u53(r[0], r[1]) > percentage:
                length += 1
            else:
                break
            t += 1
    return length


def _intersect(col, a_lo, a_n, b_lo, b_n):
    return len(set(col[a_lo:a_lo + a_n].tolist()) & set(col[b_lo:b_lo + b_n].tolist()))


def _count(stats, key, n=1):
    if stats is not None:
        stats[key] = stats.get(key, 0) + n


def _common_search_stats(col, a_lo, a_n, b_lo, b_n, stats):
    """The branches wave_any_common takes for these two sorted ranges (swap to the shorter range, 64 of its
    elements per round, exit at the first round with a hit)."""
    if a_n > b_n:
        a_lo, a_n, b_lo, b_n = b_lo, b_n, a_lo, a_n
        _count(stats, "swap")
    else:
        _count(stats, "no_swap")
    longer = set(col[b_lo:b_lo + b_n].tolist())
    for i0 in range(0, a_n, 64):
        if i0 == 64:
            _count(stats, "second_round")
        if longer & set(col[a_lo + i0:a_lo + min(i0 + 64, a_n)].tolist()):
            if i0 + 64 < a_n:
                _count(stats, "early_exit")
            return


def device_walk(row_ptr, col, cum2, node, gw, length, seed, stats=None, variant=None):
    """`stats` (optional dict) counts the branches taken: "trials", "retry_self" (the proposal is the current
    vertex), "rejected" (its middle vertex is not the first common neighbour), "steps", "clamp", and the branches of
    the wave-wide search ("swap", "no_swap", "second_round", "early_exit").  `variant` plants an error for
    tests/test_bine_prep_host.py: "keep_all" drops the first-common-neighbour test, "entry_left" searches the CSR
    entry with side="left"."""
    cur = int(node)
    out = [cur]
    for t in range(length - 1):
        rb, re = int(row_ptr[cur]), int(row_ptr[cur + 1])
        base = int(cum2[rb])
        paths = int(cum2[re]) - base
        nxt = cur
        _count(stats, "steps")
        for trial in range(MAX_TRIALS):
            r = _philox(seed, gw, gw >> 32, t, 1 + trial)
            pick = int(math.floor(_u53(r[0], r[1]) * float(paths)))
            if pick >= paths:
                pick = paths - 1
                _count(stats, "clamp")
            e = rb + int(np.searchsorted(cum2[rb + 1:re + 1] - base, pick,
                                         side="left" if variant == "entry_left" else "right"))
            mid = int(col[e])
            k = pick - (int(cum2[e]) - base)
            if variant == "entry_left":                   # the planted search can point one past mid's row
                k = min(k, int(row_ptr[mid + 1] - row_ptr[mid]) - 1)
            w = int(col[int(row_ptr[mid]) + k])
            _count(stats, "trials")
            if w == cur:
                _count(stats, "retry_self")
                continue
            nxt = w
            wb = int(row_ptr[w])
            if variant == "keep_all":
                break
            if stats is not None:
                below = int(np.searchsorted(col[wb:int(row_ptr[w + 1])], mid, side="left"))
                _common_search_stats(col, rb, e - rb, wb, below, stats)
            before = set(col[rb:e].tolist())              # cur's neighbours below mid
            if not (before & set(col[wb:int(row_ptr[w + 1])].tolist())):
                break                                     # mid is the first common neighbour: keep the path
            _count(stats, "rejected")
        cur = nxt
        out.append(cur)
    return out


def neg_pool(row_ptr, col, side_lo, side_hi, v, pool_size, max_jaccard, seed, stats=None, variant=None):
    """One vertex's pool row.  A side of one vertex has nobody to offer: its row is -1, the "no negative" value
    (pool_valid).  `stats` (optional dict) counts "self_draw", "give_up" (the 17th draw kept without the similarity
    test), "fallback" (every draw was v itself), "fallback_wrap", "no_negative", "swap" (v's row longer than the
    candidate's) and "thinned".  `variant`: "no_wrap" takes v + 1 without wrapping to the side's start, "early_give_up"
    gives up one trial early."""
    vb, vn = int(row_ptr[v]), int(row_ptr[v + 1] - row_ptr[v])
    side_n = side_hi - side_lo
    last = POOL_TRIALS - 1 if variant == "early_give_up" else POOL_TRIALS
    out = []
    for s in range(pool_size):
        c = v
        for trial in range(POOL_TRIALS + 1):
            r = _philox(seed, v, s, trial, 0)
            k = min(int(math.floor(_u53(r[0], r[1]) * float(side_n))), side_n - 1)
            c = side_lo + k
            if c == v:
                _count(stats, "self_draw")
                continue
            if trial >= last:
                _count(stats, "give_up")
                break
            cb, cn = int(row_ptr[c]), int(row_ptr[c + 1] - row_ptr[c])
            _count(stats, "swap" if vn > cn else "no_swap")
            mult = _intersect(col, vb, vn, cb, cn)
            if not (float(mult) > max_jaccard * float(vn + cn - mult)):
                break
            _count(stats, "thinned")
        if c == v:
            _count(stats, "fallback")
            if variant == "no_wrap":
                c = v + 1
            else:
                if not v + 1 < side_hi:
                    _count(stats, "fallback_wrap")
                c = v + 1 if v + 1 < side_hi else side_lo
                if c == v:
                    _count(stats, "no_negative")
                    c = -1
        out.append(c)
    return out


def floyd_sample(n, m, words):
    """Floyd's m distinct values of [0, n): value k = floor(words[k] * (j+1) / 2^32), j = n-m+k; j if taken."""
    out = []
    for k in range(m):
        j = n - m + k
        t = (words[k] * (j + 1)) >> 32
        if t in out:
            t = j
        out.append(t)
    return out


def sample_occurrences(c, n_occ, iteration, seed_occ):
    m = min(n_occ, 10)
    words = []
    for blk in range(3):
        words.extend(_philox(seed_occ, c, iteration, blk, 0))
    return floyd_sample(n_occ, m, words)


def pool_valid(pool_row):
    """Number of vertices in a pool row: a prefix of non-negative entries, then -1 up to pool_size."""
    row = [int(x) for x in pool_row]
    valid = sum(1 for x in row if x >= 0)
    if any(x < 0 for x in row[:valid]):
        raise ValueError("pool row is not a valid prefix followed by -1")
    return valid


def occurrence_context(o, c, tokens, tok_walk, walk_off, pool_row, ws, ns, seed_neg, stats=None):
    """Contexts and negatives of the occurrence at token position o of vertex c
    (src/bine_graph_utils.py:169-187: window within the walk, tokens equal to the centre skipped; negatives
    = min(ns, valid) distinct slots of the pool's valid prefix, dropped when inside the window or repeated).
    `stats` (optional dict): counts negatives dropped for being in the window ("neg_in_window")."""
    wk = int(tok_walk[o])
    w0, w1 = int(walk_off[wk]), int(walk_off[wk + 1])
    s, e = max(w0, o - ws), min(w1, o + ws + 1)
    window = [int(x) for x in tokens[s:e]]
    contexts = [z for z in window if z != c]
    words = list(_philox(seed_neg, o, o >> 32, 0, 0)) + list(_philox(seed_neg, o, o >> 32, 1, 0))
    valid = pool_valid(pool_row)
    negs = []
    for slot in floyd_sample(valid, min(ns, valid), words):
        cand = int(pool_row[slot])
        if cand in window:
            if stats is not None:
                stats["neg_in_window"] = stats.get("neg_in_window", 0) + 1
            continue
        if cand in negs or cand == c:
            continue
        negs.append(cand)
    return contexts, negs


# ------------------------------------------------------------------------------- (L) training arithmetic
def skip_gram(center, context, negs, emb, ctx, lam, pa):
    """src/bine_train.py:243-274 on dense tables (emb = 'embedding_vectors', ctx = 'context_vectors')."""
    loss = 0.0
    I_z = {center: 1}
    for node in negs:
        I_z[node] = 0
    V = np.array(emb[context])
    update = np.zeros_like(V)
    for u in I_z.keys():
        Theta = np.array(ctx[u])
        X = float(max(V.dot(Theta), 0))
        sigmod = 1.0 / (1 + (math.exp(-X * 1.0)))
        update += pa * lam * (I_z[u] - sigmod) * Theta
        ctx[u] += pa * lam * (I_z[u] - sigmod) * V
        try:
            loss += pa * (I_z[u] * math.log(sigmod) + (1 - I_z[u]) * math.log(1 - sigmod))
        except ValueError:
            pass
    return update, loss


def kl_divergence(e_ij, u, v, emb, lam, gamma):
    """src/bine_train.py:277-309."""
    U = np.array(emb[u])
    V = np.array(emb[v])
    X = float(max(U.dot(V), 0))
    sigmod = 1.0 / (1 + (math.exp(-X * 1.0)))
    update_u = gamma * lam * ((e_ij * (1 - sigmod)) * 1.0 / LN10) * V
    update_v = gamma * lam * ((e_ij * (1 - sigmod)) * 1.0 / LN10) * U
    loss = gamma * e_ij * math.log(sigmod)
    return update_u, update_v, loss


def train(edge_u, edge_v, edge_w, emb, ctx, occ_ptr, occ_pos, tokens, tok_walk, walk_off, pool, ws, ns, alpha, beta,
          gamma, lam, max_iter, seed_occ, seed_neg, epsilon=1e-3, first=None, stats=None):
    """The loop of src/bine_train.py:452-504 over the rating list, with the device's sampling rule for the
    occurrences / negatives (the reference uses the global `random`).  emb, ctx: float64 [N, d], updated in
    place.  `first` (optional, uint8 per rating: bit 0 user, bit 1 item) replaces the visited dictionaries when
    only a sample of the rating list is passed.  Returns (lam, per-iteration losses).

    `stats` (optional dict) is filled with counts over all iterations: "rows_ref", the rows the reference's
    access pattern moves (2 + 2 * (1 + len(negs)) per skip_gram call, 4 per KL update: what the kernel adds to
    state[5]), and what the data exercised: "blocks", "empty" (blocks of a vertex without occurrences), "capped"
    (blocks of more than 10 occurrences), "occurrences", "max_window" (tokens in the widest window),
    "repeat_context" (context lists holding one vertex twice in a row, a walk z c z), "short_pool" (occurrences
    drawing from a pool with -1 slots), "negs_cut" (occurrences whose pool holds fewer vertices than ns) and
    "neg_in_window"."""
    if stats is not None:
        for k in ("rows_ref", "blocks", "empty", "capped", "occurrences", "max_window", "repeat_context",
                  "short_pool", "negs_cut", "neg_in_window"):
            stats.setdefault(k, 0)
    last_loss = 0.0
    losses = []
    for it in range(max_iter):
        loss = 0.0
        seen = set()
        for e in range(len(edge_u)):
            u, v, w = int(edge_u[e]), int(edge_v[e]), float(edge_w[e])
            for side, (c, pa) in enumerate(((u, alpha), (v, beta))):
                if first is not None:
                    if not (int(first[e]) >> side) & 1:
                        continue
                elif c in seen:
                    continue
                seen.add(c)
                ob = int(occ_ptr[c])
                n_occ = int(occ_ptr[c + 1]) - ob
                if stats is not None:
                    stats["blocks"] += 1
                    stats["empty"] += n_occ == 0
                    stats["capped"] += n_occ > 10
                for idx in sample_occurrences(c, n_occ, it, seed_occ):
                    o = int(occ_pos[ob + idx])
                    contexts, negs = occurrence_context(o, c, tokens, tok_walk, walk_off, pool[c], ws, ns, seed_neg,
                                                        stats)
                    if stats is not None:
                        wk = int(tok_walk[o])
                        valid = pool_valid(pool[c])
                        stats["occurrences"] += 1
                        stats["max_window"] = max(stats["max_window"],
                                                  min(int(walk_off[wk + 1]), o + ws + 1) - max(int(walk_off[wk]), o - ws))
                        stats["repeat_context"] += any(x == y for x, y in zip(contexts[:-1], contexts[1:]))
                        stats["short_pool"] += valid < len(pool[c])
                        stats["negs_cut"] += valid < ns
                        stats["rows_ref"] += len(contexts) * (2 + 2 * (1 + len(negs)))
                    for z in contexts:
                        tmp_z, tmp_loss = skip_gram(c, z, negs, emb, ctx, lam, pa)
                        emb[z] += tmp_z
                        loss += tmp_loss
            if stats is not None:
                stats["rows_ref"] += 4
            update_u, update_v, tmp_loss = kl_divergence(w, u, v, emb, lam, gamma)
            loss += tmp_loss
            emb[u] += update_u
            emb[v] += update_v
        delta_loss = abs(loss - last_loss)
        if last_loss > loss:
            lam *= 1.05
        else:
            lam *= 0.95
        last_loss = loss
        losses.append(loss)
        if delta_loss < epsilon:
            break
    return lam, losses


def init_rows(n, dim, seed):
    """(P) init: U[0,1)^dim rows scaled to unit l2 norm; element c of row r, table t from Philox
    (r lo, r hi, c >> 1, t)."""
    out = np.zeros((2, n, dim))
    for t in range(2):
        for r in range(n):
            for c in range(dim):
                w = _philox(seed, r, r >> 32, c >> 1, t)
                out[t, r, c] = _u53(w[2], w[3]) if c & 1 else _u53(w[0], w[1])
            out[t, r] /= math.sqrt(float((out[t, r] ** 2).sum()))
    return out[0], out[1]
