"""Playlists (listening sessions) from the 30Music event log, on the device: the loop of
src/extract_playlist.py:4-28 as a shifted compare, a cumulative sum and a mask.

On rows in file order: row r+1 continues row r's session iff both have the same uid and
``ts[r+1] < ts[r] + playtime[r] + 300`` (:13); a non-final row of a session contributes its track iff
``playtime > 9`` (:14-15), the final row always does (:21); sessions of <= 1 kept track are dropped (:26).  The
reference reads ``iloc[idx+1]`` on the last row of the file and ends in an IndexError; here the last row simply ends
its session.
"""
import numpy as np
import torch

from .corpus import SentenceCorpus, _device

SESSION_GAP = 300    # seconds after a track's end within which the next event still belongs to the session
MIN_PLAYTIME = 9     # a non-final track counts only when played longer than this


def extract_playlists(uid, timestamp, playtime, tid, as_corpus=False, min_count=5, device=None):
    """uid, tid: sequences of labels (strings or numbers); timestamp, playtime: integers (or strings of integers).
    -> list of sentences of tid labels, or (as_corpus=True) a SentenceCorpus pruned by min_count."""
    n = len(uid)
    if not (len(timestamp) == len(playtime) == len(tid) == n):
        raise ValueError("uid, timestamp, playtime and tid must have one entry per row")
    dev = _device(device)
    if n == 0:
        users, u = np.zeros(0, np.int64), np.zeros(0, np.int64)
        tracks, t = np.zeros(0, np.int64), np.zeros(0, np.int64)
    else:
        users, u = np.unique(np.asarray(uid), return_inverse=True)
        tracks, t = np.unique(np.asarray(tid), return_inverse=True)
    ts = torch.from_numpy(np.asarray(timestamp, dtype=np.int64).reshape(n)).to(dev)
    pt = torch.from_numpy(np.asarray(playtime, dtype=np.int64).reshape(n)).to(dev)
    u = torch.from_numpy(u.astype(np.int64).reshape(n)).to(dev)
    t = torch.from_numpy(t.astype(np.int64).reshape(n)).to(dev)
    cont = torch.zeros(n, dtype=torch.bool, device=dev)            # row r+1 continues row r
    if n > 1:
        cont[:-1] = (u[1:] == u[:-1]) & (ts[1:] < ts[:-1] + pt[:-1] + SESSION_GAP)
    start = torch.ones(n, dtype=torch.bool, device=dev)            # row r opens a session
    if n > 1:
        start[1:] = ~cont[:-1]
    session = torch.cumsum(start.long(), 0) - 1
    gives = ~cont | (pt > MIN_PLAYTIME)
    n_sessions = int(session[-1].item()) + 1 if n else 0
    kept = torch.bincount(session[gives], minlength=n_sessions) if n else torch.zeros(0, dtype=torch.int64, device=dev)
    gives &= (kept > 1)[session] if n else gives
    ids = t[gives]
    lens = kept[kept > 1]
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    if as_corpus:
        return SentenceCorpus.from_ids(tracks, ids, off, min_count)
    lab = tracks[ids.cpu().numpy()].tolist() if n else []
    o = off.cpu().numpy()
    return [lab[o[s]:o[s + 1]] for s in range(len(o) - 1)]
