"""TEST INFRASTRUCTURE — what tests/lsh_cases.py's cases must give, and a second restatement in the kernels' own shape.

`expected(case)`: graph -> signatures, query lists, owners and pool rows from oracle/bine_lsh_oracle.py alone (the
sets, sorted lists and sequential loops of the reference text).  That is what the GPU test compares with.

`shaped_*`: csrc/n2v_lsh.hip restated step for step in plain Python — 64 lanes per chunk, the 512-slot open-addressing
set, ballot ranks, the per-workgroup bitmap that one leader after another reuses, Philox rounds.  It exists for two
things the oracle cannot show: (a) the audits of tests/test_lsh_cases_host.py (how far an insertion probed, which
candidate a lower lane took, how many rounds a row needed, whether a bitmap was reused), and (b) sensitivity — each
`flaw` below is one plausible slip of the kernel, and the host test shows that at least one case's arrays change
under it.  With flaw=None it must equal the oracle on every case.

Flaws:
  "keep_sim_j"    pool epilogue does not clear the bits of sim(j): the next leader on that bitmap loses candidates;
  "rank_le_room"  `rank <= room` in the query chunk and in the pool round: one key too many (it lands in the next row,
                  or in the guard behind the last; the race with that row's own writer is modelled as lost by the
                  owner) and, in the pool, a bit the epilogue does not know of;
  "chunk_to_63"   a chunk scans [base, base + 63): the candidate of lane 63 is never looked at;
  "no_wrap"       the probe sequence lacks `& 511`: slot 512 of a wavefront is slot 0 of the next wavefront of the
                  workgroup (the four sets lie behind one another in LDS; wavefronts that walk the same list in step
                  keep finding their own keys there), and slot 512 of the LAST wavefront is behind the workgroup's LDS,
                  where a read never returns the empty mark: that probe does not end — ProbeRanOff here;
  "popcount_one_trip"  the count of excluded vertices reads bitmap words 0 … 63 only;
  "v_absolute"    the signature of vertex v goes to row v, not v - v_begin."""
import functools

import numpy as np

import lsh_cases as C
from oracle import bine_lsh_oracle as lo
from oracle.n2v_oracle import philox4x32_10

TREES, DEPTH, SLOTS = lo.TREES, lo.DEPTH, C.SET_SLOTS
GUARD = -7


class ProbeRanOff(Exception):
    """A probe sequence left the workgroup's four sets."""


@functools.lru_cache(maxsize=None)
def graph_of(name):
    from n2v_hip import bine
    users, items = C.GRAPHS[name]()
    return bine.BipartiteGraph(users, items, np.ones(len(users)))


def labels_of(g):
    return [str(x) for x in g.user_labels] + [str(x) for x in g.item_labels]


def sides(g):
    from n2v_hip import bine
    return (("u", 0, g.n_u, bine.SEED_POOL_U), ("v", g.n_u, g.n, bine.SEED_POOL_V))


ENGINE_SEED = 77


@functools.lru_cache(maxsize=None)
def signatures_of(name):
    g = graph_of(name)
    hv = np.array([lo.sha1_hash32(s.encode("utf8")) for s in labels_of(g)], dtype=np.uint64)
    return lo.signatures(g.row_ptr, g.col, hv, 0, g.n)


@functools.lru_cache(maxsize=None)
def queries_of(name, k):
    """Per side: (sims, owner) of the oracle."""
    g, sig, out = graph_of(name), signatures_of(name), {}
    for side, a, b, _ in sides(g):
        sims = lo.forest_query_all(sig[a:b], k=k)
        out[side] = (sims, lo.leaders(sims))
    return out


@functools.lru_cache(maxsize=None)
def rows_of(name, k, pool_size):
    """Per side: {leader: pool row (local ids, -1 padded)} of the oracle."""
    from n2v_hip import bine
    g, out = graph_of(name), {}
    for side, a, b, kseed in sides(g):
        sims, owner = queries_of(name, k)[side]
        seed = bine.derive_seed(ENGINE_SEED, kseed)
        out[side] = {int(l): lo.sample_pool(lo.exclusions(sims, int(l)), b - a, pool_size, seed, int(l))
                     for l in np.unique(owner)}
    return out


def expected(case):
    """{side: dict(sig, sims, owner, pool)}; pool int32[n_side][pool_size] in GLOBAL ids as the engine stores it."""
    g, sig, out = graph_of(case.graph), signatures_of(case.graph), {}
    for side, a, b, _ in sides(g):
        sims, owner = queries_of(case.graph, case.k)[side]
        rows = rows_of(case.graph, case.k, case.pool_size)[side]
        pool = np.stack([np.where(rows[int(l)] >= 0, rows[int(l)] + a, -1) for l in owner]).astype(np.int32)
        out[side] = dict(sig=sig[a:b], sims=sims, owner=owner, pool=pool, lo=a, hi=b)
    return out


# ------------------------------------------------------------------------------------------ the forest, as the host lays it out
def forest_ranges(sig):
    """order int[8][n], lo / hi int[n][8][16]: [v][t][r-1] = the sorted positions of tree t whose first r values equal
    v's (BineEngine._forest_side, in numpy)."""
    n = sig.shape[0]
    order, lcp = lo.forest_layout(sig)
    idx = np.arange(n)
    rlo = np.empty((n, TREES, DEPTH), dtype=np.int64)
    rhi = np.empty((n, TREES, DEPTH), dtype=np.int64)
    for t in range(TREES):
        pos = np.empty(n, dtype=np.int64)
        pos[order[t]] = idx
        for r in range(1, DEPTH + 1):
            cut = lcp[t] < r
            start = np.maximum.accumulate(np.where(cut, idx, 0))
            after = np.minimum.accumulate(np.where(cut, idx, n)[::-1])[::-1]
            end = np.concatenate([after[1:], [n]])
            rlo[:, t, r - 1] = start[pos]
            rhi[:, t, r - 1] = end[pos]
    return order, rlo, rhi


def wing_widths(rlo, rhi):
    """Every width of a range that a query scans: the deepest range, then the two wings each level adds."""
    deep = (rhi[:, :, DEPTH - 1] - rlo[:, :, DEPTH - 1]).ravel()
    left = (rlo[:, :, 1:] - rlo[:, :, :-1]).ravel()
    right = (rhi[:, :, :-1] - rhi[:, :, 1:]).ravel()
    return set(deep.tolist()) | set(left.tolist()) | set(right.tolist())


# ------------------------------------------------------------------------------------------ forest_query_kernel
def shaped_queries(order, rlo, rhi, k, flaw=None):
    """-> sim flat int[n*k + 64] (GUARD where nothing was written), sim_n, stats.  Workgroups of 4 wavefronts; the
    wavefronts of a workgroup run one after the other on four sets laid out back to back."""
    n = order.shape[1]
    sim = np.full(n * k + 64, GUARD, dtype=np.int64)
    sim_n = np.zeros(n, dtype=np.int64)
    st = dict(max_probe=0, wrapped=0, hits=0, cut_mid_chunk=0, full_chunks=0, chunk_trips=0)
    mask = (lambda h: h) if flaw == "no_wrap" else (lambda h: h & (SLOTS - 1))
    scan = 63 if flaw == "chunk_to_63" else 64
    stray = []
    for wg in range(0, n, 4):
        lds = np.full(4 * SLOTS, -1, dtype=np.int64)
        for wv in range(min(4, n - wg)):
            v, base_slot = wg + wv, wv * SLOTS

            def contains(key):
                h = C.set_home(key)
                while True:
                    if base_slot + h >= 4 * SLOTS:
                        raise ProbeRanOff(v, key)
                    x = lds[base_slot + h]
                    if x == key:
                        return True
                    if x < 0:
                        return False
                    h = mask(h + 1)

            def insert(key):
                h, probes = C.set_home(key), 1
                while lds[base_slot + h] >= 0:
                    if h == SLOTS - 1:
                        st["wrapped"] += 1
                    h, probes = mask(h + 1), probes + 1
                    if base_slot + h >= 4 * SLOTS:
                        raise ProbeRanOff(v, key)
                lds[base_slot + h] = key
                st["max_probe"] = max(st["max_probe"], probes)

            cnt = 0
            for r in range(DEPTH, 0, -1):
                for t in range(TREES):
                    if cnt >= k:
                        break
                    nlo, nhi = rlo[v, t, r - 1], rhi[v, t, r - 1]
                    wings = ((nlo, nhi), (0, 0)) if r == DEPTH else ((nlo, rlo[v, t, r]), (rhi[v, t, r], nhi))
                    for w_lo, w_hi in wings:
                        base = w_lo
                        while base < w_hi and cnt < k:
                            st["chunk_trips"] += 1
                            keys = [int(order[t, i]) for i in range(base, min(base + scan, w_hi))]
                            st["full_chunks"] += len(keys) == 64
                            fresh = [key for key in keys if not contains(key)]
                            st["hits"] += len(keys) - len(fresh)
                            room = k - cnt
                            take = room + 1 if flaw == "rank_le_room" else room
                            st["cut_mid_chunk"] += len(fresh) > room
                            for rank, key in enumerate(fresh[:take]):
                                if rank < room:
                                    sim[v * k + cnt + rank] = key
                                else:
                                    stray.append((v * k + cnt + rank, key))
                                insert(key)
                            cnt += min(len(fresh), room)
                            base += 64
            sim_n[v] = cnt
    for at, key in stray:                  # a write behind its row races with that row's owner: here it lands last
        sim[at] = key
    return sim, sim_n, st


def rows_of_flat(sim, sim_n, k):
    return [sim[v * k:v * k + int(c)].tolist() for v, c in enumerate(sim_n)]


# ------------------------------------------------------------------------------------------ leader_round_kernel
def shaped_leaders(sims):
    """The sweep in rounds, every round reading the owners of the round before: vertex i walks the earlier vertices
    that list it, ascending; an unresolved one stops it until a later round, a leader owns it, a follower is skipped;
    the end of the list makes it a leader.  -> (owner, rounds)."""
    n = len(sims)
    rev = [[] for _ in range(n)]
    for l, s in enumerate(sims):
        for j in s:
            if j > l:
                rev[j].append(l)
    owner, rounds = np.full(n, -1, dtype=np.int64), 0
    while (owner < 0).any():
        rounds += 1
        before = owner.copy()
        for i in np.nonzero(before < 0)[0]:
            mine = i
            for l in sorted(rev[i]):
                if before[l] < 0:
                    mine = -1
                    break
                if before[l] == l:
                    mine = l
                    break
            owner[i] = mine
    return owner, rounds


# ------------------------------------------------------------------------------------------ lsh_pool_kernel
@functools.lru_cache(maxsize=None)
def _draws(seed, leader, rnd, n_side):
    out = []
    for lane in range(64):
        r = philox4x32_10((leader & 0xFFFFFFFF, rnd & 0xFFFFFFFF, lane, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        out.append(min(int(np.floor(lo._u53(r[0], r[1]) * float(n_side))), n_side - 1))
    return tuple(out)


def shaped_pools(sims, owner, k, n_side, pool_size, seed, groups, flaw=None):
    """-> pool flat int[n_side * pool_size + 64] of LOCAL ids (GUARD where nothing was written; rows of followers
    stay GUARD), stats.  Workgroup b serves leaders b, b + grid, … on one bitmap, one after the other."""
    lead = [int(l) for l in np.nonzero(owner == np.arange(n_side))[0]]
    grid = min(len(lead), groups)
    words = (n_side + 31) // 32
    pool = np.full(n_side * pool_size + 64, GUARD, dtype=np.int64)
    stray = []
    st = dict(served_max=0, rounds_max=0, lower_lane=0, earlier_round=0, counted=0, all_of_it=0, popcount_trips=0,
              stale_words=0, cut_rounds=0, words=words, n_lead=len(lead), complements={})
    for b in range(grid):
        bm = np.zeros(words, dtype=np.uint32)
        mine = lead[b::grid]
        st["served_max"] = max(st["served_max"], len(mine))
        for l in mine:
            st["stale_words"] += int(np.count_nonzero(bm))
            excluded = set(sims[l])
            for j in sims[l]:
                excluded |= set(sims[j])
            for c in excluded:
                bm[c >> 5] |= np.uint32(1 << (c & 31))
            row = l * pool_size
            all_of_it = False
            if n_side <= k * (k + 1) + pool_size:
                st["counted"] += 1
                st["popcount_trips"] = max(st["popcount_trips"], (words + 63) // 64)
                gone = sum(bin(int(w)).count("1") for w in (bm[:64] if flaw == "popcount_one_trip" else bm))
                st["complements"][l] = n_side - gone
                all_of_it = n_side - gone <= pool_size
            cnt = 0
            if all_of_it:
                st["all_of_it"] += 1
                for c in range(n_side):
                    if not (bm[c >> 5] >> np.uint32(c & 31)) & np.uint32(1):
                        pool[row + cnt] = c
                        cnt += 1
                pool[row + cnt:row + pool_size] = -1
            else:
                rnd, proposed = 0, set()
                while cnt < pool_size:
                    cand = _draws(seed, l, rnd, n_side)
                    ok = []
                    for lane, c in enumerate(cand):
                        free = not (bm[c >> 5] >> np.uint32(c & 31)) & np.uint32(1)
                        if free and c in cand[:lane]:
                            st["lower_lane"] += 1
                        elif not free and c in proposed and c not in excluded:
                            st["earlier_round"] += 1
                        if free and c not in cand[:lane]:
                            ok.append(c)
                    room = pool_size - cnt
                    st["cut_rounds"] += len(ok) > room
                    for rank, c in enumerate(ok[:room + 1 if flaw == "rank_le_room" else room]):
                        if rank < room:
                            pool[row + cnt + rank] = c
                        else:
                            stray.append((row + cnt + rank, c))
                        bm[c >> 5] |= np.uint32(1 << (c & 31))
                        proposed.add(c)
                    cnt += min(len(ok), room)
                    rnd += 1
                st["rounds_max"] = max(st["rounds_max"], rnd)
                for c in pool[row:row + pool_size]:
                    bm[int(c) >> 5] = 0
            for c in sims[l]:
                bm[c >> 5] = 0
            if flaw != "keep_sim_j":
                for j in sims[l]:
                    for c in sims[j]:
                        bm[c >> 5] = 0
    for at, c in stray:                    # as in shaped_queries
        pool[at] = c
    return pool, st


# ------------------------------------------------------------------------------------------ minhash_kernel's addressing
def shaped_minhash_rows(sig, v_begin, v_end, rows, flaw=None):
    """What a launch over [v_begin, v_end) leaves in a buffer of `rows` signature rows that held GUARD."""
    out = np.full((rows, lo.NUM_PERM), GUARD, dtype=np.int64)
    for v in range(v_begin, v_end):
        out[v if flaw == "v_absolute" else v - v_begin] = sig[v]
    return out


# ------------------------------------------------------------------------------------------ cached runs of the above
@functools.lru_cache(maxsize=None)
def ranges_of(name, side):
    g = graph_of(name)
    a, b = [(a, b) for s, a, b, _ in sides(g) if s == side][0]
    return forest_ranges(signatures_of(name)[a:b])


@functools.lru_cache(maxsize=None)
def shaped_queries_of(name, side, k, flaw=None):
    return shaped_queries(*ranges_of(name, side), k, flaw=flaw)


def shaped_pools_of(case, side, flaw=None, sims=None):
    from n2v_hip import bine
    g = graph_of(case.graph)
    a, b, kseed = [(a, b, ks) for s, a, b, ks in sides(g) if s == side][0]
    osims, owner = queries_of(case.graph, case.k)[side]
    return shaped_pools(osims if sims is None else sims, owner, case.k, b - a, case.pool_size,
                        bine.derive_seed(ENGINE_SEED, kseed), case.groups, flaw=flaw)
