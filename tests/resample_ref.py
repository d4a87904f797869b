"""The yardstick of the output-rate tests: ``scipy.signal.resample_poly(x, L, M)``'s default filter and output, restated in
numpy so that a machine without scipy can run it (``tests/test_resample.py`` pins it to scipy where scipy imports).

    h0[m] = fc sinc(fc m) I0(beta sqrt(1 - (m / half)^2)) / I0(beta),  m = -half .. half,  fc = 1 / max(L, M),  beta = 5,
    h     = L h0 / sum(h0),  half = 10 max(L, M)
    y[k]  = sum_j h[k M - j L + half] x[j],  x zero outside [0, n),  k = 0 .. ceil(n L / M) - 1

``resample`` runs it in fp64; ``resample(..., dtype=np.float32)`` is the "plain f32" comparison: taps rounded to f32, f32
products and sums, ascending tap index.  Never the code under test: nothing here is imported by the package.
"""
from __future__ import annotations

from math import gcd

import numpy as np

MAX_RATIO = 640


def ratio(in_hz: int, out_hz: int):
    g = gcd(int(in_hz), int(out_hz))
    return int(out_hz) // g, int(in_hz) // g  # L (up), M (down)


def out_len(n: int, L: int, M: int) -> int:
    return -(-int(n) * L // M)


def taps(L: int, M: int) -> np.ndarray:
    """The 2 * half + 1 taps in fp64."""
    mx = max(L, M)
    half = 10 * mx
    fc = 1.0 / mx
    m = np.arange(-half, half + 1, dtype=np.float64)
    h0 = fc * np.sinc(fc * m) * np.i0(5.0 * np.sqrt(1.0 - (m / half) ** 2)) / np.i0(5.0)
    return L * h0 / h0.sum()


def resample(x, L: int, M: int, dtype=np.float64) -> np.ndarray:
    """One row.  ``taps_per_phase`` vectorised passes, each adding tap index p + i L (ascending i) of every output's phase p."""
    x = np.asarray(x, dtype=dtype).reshape(-1)
    n = x.shape[0]
    h = taps(L, M).astype(dtype)
    half = (h.shape[0] - 1) // 2
    no = out_len(n, L, M)
    k = np.arange(no, dtype=np.int64)
    idx = k * M + half
    j_hi, p = idx // L, idx % L
    tpp = -(-h.shape[0] // L)
    hp = np.concatenate([h, np.zeros(tpp * L - h.shape[0], dtype)])
    y = np.zeros(no, dtype)
    for i in range(tpp):
        j = j_hi - i
        ok = (j >= 0) & (j < n)
        xv = np.where(ok, x[np.clip(j, 0, max(n - 1, 0))] if n else np.zeros(no, dtype), dtype(0))
        y = (y + (hp[p + i * L] * xv).astype(dtype)).astype(dtype)
    return y


def rel_rms(a, ref) -> float:
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    d = float(np.sqrt(np.mean((a - ref) ** 2))) if ref.size else 0.0
    r = float(np.sqrt(np.mean(ref ** 2))) if ref.size else 0.0
    return d / r if r > 0 else d


def errors(y_engine, x_native, L: int, M: int):
    """(engine vs fp64, plain f32 vs fp64) relative RMS for one row."""
    ref = resample(np.asarray(x_native, np.float64), L, M)
    f32 = resample(np.asarray(x_native, np.float32), L, M, np.float32)
    assert len(y_engine) == ref.shape[0], (len(y_engine), ref.shape[0])
    return rel_rms(y_engine, ref), rel_rms(f32, ref)
