"""The yardstick of the loudness tests: ITU-R BS.1770-4 / EBU R128 integrated loudness, the gain rule and the int16 conversion of
the packed streams in numpy, from the definitions of include/mi355vits.h alone.  It never calls the code under test.

The filter is an FFT convolution with the cascade's impulse response, which the plain recurrence generates out to |h| < 1e-18 (a
machine without scipy can run it; tests/test_loudness.py pins it to scipy.signal.lfilter where scipy imports)."""
from __future__ import annotations

import functools
import math

import numpy as np


def k_weighting(fs):
    """((b, a) of the high shelf, (b, a) of the high pass) at ``fs`` Hz, float64."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K]) / a0
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return (b1, a1), (b2, a2)


def _biquad(b, a, x):
    """Direct form I, sample by sample (used for the impulse response only)."""
    y = np.zeros(len(x))
    x1 = x2 = y1 = y2 = 0.0
    for k, v in enumerate(x):
        o = b[0] * v + b[1] * x1 + b[2] * x2 - a[1] * y1 - a[2] * y2
        x2, x1, y2, y1 = x1, v, y1, o
        y[k] = o
    return y


@functools.lru_cache(maxsize=None)
def impulse_response(fs):
    """h of the cascade out to where |h| has stayed below 1e-18 for 2,048 samples."""
    (b1, a1), (b2, a2) = k_weighting(fs)
    n = 4096
    while True:
        x = np.zeros(n)
        x[0] = 1.0
        h = _biquad(b2, a2, _biquad(b1, a1, x))
        big = np.nonzero(np.abs(h) >= 1e-18)[0]
        if big[-1] < n - 2048:
            return h[: big[-1] + 1]
        n *= 2


def k_filter(x, fs):
    """The K-weighted row, float64, zero state at sample 0."""
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return x
    h = impulse_response(fs)
    m = len(x) + len(h) - 1
    nfft = 1 << (m - 1).bit_length()
    y = np.fft.irfft(np.fft.rfft(x, nfft) * np.fft.rfft(h, nfft), nfft)
    return y[: len(x)]


def step(fs):
    return (fs + 5) // 10


def block_energies(x, fs):
    """z_i of every block of the row (one block over a row shorter than 400 ms, none for an empty row)."""
    n, S = len(x), step(fs)
    if n == 0:
        return np.zeros(0)
    y2 = k_filter(x, fs) ** 2
    if n < 4 * S:
        return np.array([y2.sum() / n])
    nb = (n - 4 * S) // S + 1
    E = y2[: (nb + 3) * S].reshape(nb + 3, S).sum(axis=1)  # the step energies: no difference of running sums
    return (E[:-3] + E[1:-2] + E[2:-1] + E[3:]) / (4 * S)


def _lu(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def measure(x, fs):
    """-> (lufs, blocks, gated, margin): margin = the smallest distance in LU of a block's loudness from a gate it is compared with
    (inf when there is none)."""
    z = block_energies(x, fs)
    nb = len(z)
    if nb == 0:
        return -np.inf, 0, 0, np.inf
    l = _lu(z)
    margin = np.min(np.abs(l + 70.0))
    a = l > -70.0
    if not a.any():
        return -np.inf, nb, 0, margin
    rel = _lu(z[a].mean()) - 10.0
    margin = min(margin, np.min(np.abs(l - rel)))
    g = a & (l > rel)
    return float(_lu(z[g].mean())), nb, int(g.sum()), float(margin)


def gain_rule(lufs, peak, target, ceiling):
    """-> (gain, limited) of one row, in float64."""
    g = 1.0 if np.isinf(lufs) else 10.0 ** ((float(target) - float(lufs)) / 20.0)
    p = float(peak)
    if p == 0.0:
        return g, False
    cap = 10.0 ** (float(ceiling) / 20.0) / p
    return (cap, True) if cap < g else (g, False)


def pcm16_quant(x, scale, volume=1.0):
    """The int16 samples of the float32 samples ``x`` under the f32 ``scale`` and the row's ``volume``: one f32 multiply, the clamp
    to +-32767, truncation, then audioop.mul's rule (floor of the double product, clamped) when volume != 1."""
    v = np.asarray(x, np.float32) * np.float32(scale)
    v = np.minimum(np.maximum(v, np.float32(-32767.0)), np.float32(32767.0))
    q = v.astype(np.int32)  # truncates
    if volume != 1.0:
        d = q.astype(np.float64) * float(volume)
        d = np.where(d > 32767.0, 32767.0, np.where(d < -32767.0, -32768.0, d))
        q = np.floor(d).astype(np.int32)
    return q.astype(np.int16)
