"""The yardstick of the true-peak tests: the 4x oversampled peak and its envelope of include/mi355vits.h in numpy, from the rule
alone — ``resample_ref.resample`` (fp64, one rounding per product and per sum, ascending taps) for ``u``, the rule's ``v > m``
comparison for every maximum — and the limiter's curve with ``rq`` made from the envelope (``limiter_ref``'s ``mq_of`` /
``sq_sliding`` behind it).  It never calls the code under test; nothing here is imported by the package."""
from __future__ import annotations

import numpy as np

from tests import limiter_ref as M
from tests import resample_ref as RS

UP = 4


def taps():
    """h[0..80] as numpy makes them (the library's own literal table is compared with this to a relative 2^-50)."""
    return RS.taps(UP, 1)


def oversample(x, h=None):
    """u[0 .. 4 n) of one row: ``resample_ref.resample(x.astype(float64), 4, 1)``, with the taps ``h`` (the library's) when given."""
    x = np.asarray(x, np.float32).astype(np.float64)
    if h is None:
        return RS.resample(x, UP, 1)
    # resample_ref.resample with another table: the same passes, operation for operation
    n = x.shape[0]
    h = np.asarray(h, np.float64)
    half = (h.shape[0] - 1) // 2
    no = UP * n
    idx = np.arange(no, dtype=np.int64) + half
    j_hi, p = idx // UP, idx % UP
    tpp = -(-h.shape[0] // UP)
    hp = np.concatenate([h, np.zeros(tpp * UP - h.shape[0])])
    y = np.zeros(no)
    with np.errstate(invalid="ignore"):
        for i in range(tpp):
            j = j_hi - i
            ok = (j >= 0) & (j < n)
            xv = np.where(ok, x[np.clip(j, 0, max(n - 1, 0))] if n else np.zeros(no), 0.0)
            y = y + hp[p + i * UP] * xv
    return y


def _max_gt(m, v):
    """m = v > m ? v : m, elementwise: a NaN in v is never taken."""
    with np.errstate(invalid="ignore"):
        return np.where(v > m, v, m)


def v_of(x, h=None):
    """v[0 .. 4 n): |x| at phase 0, |u| elsewhere."""
    x = np.asarray(x, np.float32)
    v = np.abs(oversample(x, h))
    v[0::UP] = np.abs(x.astype(np.float64))
    return v


def true_peak(x, h=None):
    """tp of one row (0.0 for an empty one)."""
    v = v_of(x, h)
    v = v[~np.isnan(v)]
    return float(v.max()) if len(v) else 0.0


def envelope(x, h=None):
    """e[0 .. n): the maximum of v over [4 t - 3, 4 t + 3] within the row's outputs."""
    x = np.asarray(x, np.float32)
    n = len(x)
    v = v_of(x, h)
    pad = np.concatenate([np.full(3, np.nan), v, np.full(3, np.nan)])  # v[j] at j + 3; outside [0, 4 n): never taken
    e = np.zeros(n)
    for d in range(7):
        e = _max_gt(e, pad[d: d + UP * n: UP][:n] if n else pad[:0])
    return e


def rq_of_env(e, g, c):
    """limiter_ref.rq_of with a[t] = g * e[t]."""
    a = np.float64(g) * np.asarray(e, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        over = a > np.float64(c)
        q = np.floor((np.float64(c) / np.where(over, a, 1.0)) * np.float64(2.0 ** 30))
    return np.where(over, q, float(M.ONE)).astype(np.int64)


def curve(x, g, c, U, L, h=None):
    """-> (scale float32 [n], sq int64 [n]) of one row in true-peak mode: limiter_ref.curve with rq from the envelope."""
    x = np.asarray(x, np.float32)
    sq = M.sq_sliding(M.mq_of(rq_of_env(envelope(x, h), g, c), L), L) if len(x) else np.zeros(0, np.int64)
    s = sq.astype(np.float64) / (np.float64(L + 1) * np.float64(2.0 ** 30))
    return (np.float64(U) * (np.float64(g) * s)).astype(np.float32), sq


def burst(n, centre, amp=0.53, width=16, noise=0.004, seed=0):
    """A Hann-windowed burst at fs/4 whose crest lies at `centre` — a half-integer: half way between two samples, which sit at 45
    degrees on either side of it — inside quiet noise: the row whose oversampled peak lies well over its sample peak."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * noise
    t = np.arange(n, dtype=np.float64)
    w = np.where(np.abs(t - centre) < width, 0.5 * (1.0 + np.cos(np.pi * (t - centre) / width)), 0.0)
    x += amp * w * np.cos(0.5 * np.pi * (t - centre))
    return x.astype(np.float32)
