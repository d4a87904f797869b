"""The yardstick of the limiter tests: the look-ahead peak limiter of include/mi355vits.h in numpy, from the rule alone — int64 sums,
np.floor of the double quotient, the same order of double operations for the scale.  It never calls the code under test."""
from __future__ import annotations

import numpy as np

ONE = 1 << 30


def rq_of(x, g, c):
    """rq[t] for the row's samples: ONE where g |x| <= c or x is NaN, else floor((c / a) 2^30)."""
    a = np.float64(g) * np.abs(np.asarray(x, np.float32).astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        over = a > np.float64(c)  # NaN: False
        q = np.floor((np.float64(c) / np.where(over, a, 1.0)) * np.float64(2.0 ** 30))
    return np.where(over, q, float(ONE)).astype(np.int64)


def mq_of(rq, L):
    """mq[i] = min rq[i .. i + L] for i = -L .. n - 1 (index i + L), rq = ONE outside the row."""
    n = len(rq)
    pad = np.concatenate([np.full(L, ONE, np.int64), rq, np.full(L, ONE, np.int64)])  # rq[t] at t + L, t = -L .. n + L - 1
    m = pad.copy()
    w = 1
    while w < L + 1:  # m[j] = min pad[j .. j + w)
        s = min(w, L + 1 - w)
        m = np.minimum(m[: len(m) - s], m[s:])
        w += s
    return m[: n + L]


def mq_direct(rq, L):
    """mq by brute force: the minimum of every window's L + 1 values, one window at a time."""
    n = len(rq)
    at = lambda t: int(rq[t]) if 0 <= t < n else ONE  # noqa: E731
    return np.array([min(at(t) for t in range(i, i + L + 1)) for i in range(-L, n)], np.int64)


def sq_sliding(mq, L):
    """sq[k] = sum mq[k - L .. k] for k = 0 .. n - 1 from a prefix sum (int64: exact)."""
    p = np.concatenate([[0], np.cumsum(mq, dtype=np.int64)])
    n = len(mq) - L
    return p[L + 1: L + 1 + n] - p[:n]


def sq_direct(mq, L):
    n = len(mq) - L
    return np.array([int(mq[k: k + L + 1].sum()) for k in range(n)], np.int64)


def curve(x, g, c, U, L):
    """-> (scale float32 [n], sq int64 [n]) of one row."""
    x = np.asarray(x, np.float32)
    sq = sq_sliding(mq_of(rq_of(x, g, c), L), L) if len(x) else np.zeros(0, np.int64)
    s = sq.astype(np.float64) / (np.float64(L + 1) * np.float64(2.0 ** 30))
    return (np.float64(U) * (np.float64(g) * s)).astype(np.float32), sq


def stats(sq, L):
    """-> (min sq, reduced samples, min s) of a row's sq; an empty row: nothing reduced."""
    full = (L + 1) * ONE
    if len(sq) == 0:
        return full, 0, 1.0
    return int(sq.min()), int((sq < full).sum()), float(np.float64(int(sq.min())) / (np.float64(L + 1) * np.float64(2.0 ** 30)))


def ceiling_linear(ceiling_db):
    """c = 10^(ceiling / 20) from the f32 ceiling the ABI carries, in double."""
    return 10.0 ** (float(np.float32(ceiling_db)) / 20.0)
