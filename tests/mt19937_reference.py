"""Restatement of numpy's legacy MT19937 `random_sample` stream for the tests of csrc/n2v_mt19937.hip and
n2v_hip/mt19937.py.  Plain numpy; nothing here imports the product.

The raw (untempered) word sequence x continues a 624-word window `key` = x[0 : 624]:

    x[n] = x[n - 227] ^ twist(x[n - 624], x[n - 623]),   twist(u, v) = (y >> 1) ^ (0x9908b0df if y & 1 else 0),
                                                          y = (u & 0x80000000) | (v & 0x7fffffff)

A word depends only on words at least 227 places back, so 227 words at a time are computed at once.  numpy keeps the
sequence as blocks of 624 words and an index `pos` into the current block; a block twist replaces x[624 b : 624 (b + 1)] by
the next 624 words.  A window that is not block-aligned (which numpy's own state cannot express) is the same thing read
from another start: logical word j of the stream that starts at position `pos` of window `key` is x[pos + j].

    random_sample:  a = temper(x[pos + 2 i]) >> 5,  b = temper(x[pos + 2 i + 1]) >> 6,  (a * 2^26 + b) / 2^53

The tiled layout of n2v_mt19937_fill_tiled (include/n2v_hip.h): the stream is cut into segments of 2 * pairs doubles;
segment s, pair t, component c (double 2 * pairs * s + 2 t + c of the stream) lies at
2 * (((s >> 6) * pairs + t) * 64 + (s & 63)) + c; the buffer holds whole groups of 64 segments.
"""
import functools

import numpy as np

N, M = 624, 397
MATRIX_A, UPPER, LOWER = np.uint32(0x9908b0df), np.uint32(0x80000000), np.uint32(0x7fffffff)


def raw_words(key, n):
    """x[0 : n + 624], the untempered sequence that continues the 624-word window `key`."""
    key = np.asarray(key, dtype=np.uint32)
    assert key.shape == (N,) and n >= 0
    x = np.empty(n + N, dtype=np.uint32)
    x[:N] = key
    for i0 in range(0, n, N - M):
        i1 = min(n, i0 + N - M)
        y = (x[i0:i1] & UPPER) | (x[i0 + 1:i1 + 1] & LOWER)
        x[i0 + N:i1 + N] = x[i0 + M:i1 + M] ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), MATRIX_A, np.uint32(0))
    return x


def temper(y):
    y = np.asarray(y, dtype=np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9d2c5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xefc60000)
    y ^= y >> np.uint32(18)
    return y


def doubles_of_words(w):
    """random_sample's doubles of an even number of raw words."""
    t = temper(w)
    a = (t[0::2] >> np.uint32(5)).astype(np.float64)
    b = (t[1::2] >> np.uint32(6)).astype(np.float64)
    return (a * 67108864.0 + b) / 9007199254740992.0


def doubles(key, pos, n):
    """What RandomState.random_sample(n) returns from state (key, pos), pos = 0 .. 624, for any window `key`."""
    assert 0 <= pos <= N
    x = raw_words(key, max(0, pos + 2 * n - N))
    return doubles_of_words(x[pos:pos + 2 * n])


def window_after(key, words):
    """x[words : words + 624]."""
    return raw_words(key, words)[words:words + N].copy()


def state_after(key, pos, n):
    """(key, pos) numpy holds after random_sample(n) from (key, pos): the block that holds the last word consumed
    (numpy twists only when it needs a word, so pos ends in 1 .. 624 once anything was drawn past the first block)."""
    p = pos + 2 * n
    if p <= N:
        return np.asarray(key, dtype=np.uint32).copy(), p
    blocks = (p - 1) // N
    return window_after(key, N * blocks), p - N * blocks


def apply_positions(x, positions):
    """(g(A) window)[j] = XOR over the set bits p of g of x[p + j], j < 624, for x = raw_words(window, >= max p)."""
    positions = np.asarray(positions, dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(np.asarray(x, dtype=np.uint32), N)
    acc = np.zeros(N, dtype=np.uint32)
    for i0 in range(0, len(positions), 1024):
        acc ^= np.bitwise_xor.reduce(win[positions[i0:i0 + 1024]], axis=0)
    return acc


@functools.lru_cache(maxsize=None)
def tiled_layout(n, pairs):
    """(position of stream double d in the tiled buffer for d < n, doubles the buffer holds) — a literal walk over
    segment s, pair t, component c."""
    where = np.empty(n, dtype=np.int64)
    d = s = 0
    while d < n:
        for t in range(pairs):
            for c in (0, 1):
                if d < n:
                    where[d] = 2 * (((s >> 6) * pairs + t) * 64 + (s & 63)) + c
                    d += 1
        s += 1
    groups = (s + 63) // 64
    where.setflags(write=False)
    return where, groups * 64 * 2 * pairs
