"""The yardstick of pitch control (mi355vits_run_pitch): the rule of include/mi355vits.h in int64 and numpy f32, one operation at a
time.  Nothing here is shared with the kernels; every comparison against it is bit for bit (same_bits)."""
import numpy as np

ONE, P, Z = 1 << 20, 128, 12
SAT = 2 ** 31 - 1
F32 = np.float32


def same_bits(a, b):
    """Bitwise equal, except that a NaN equals a NaN (its sign and payload IEEE leaves to the platform)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def table():
    """h[i], i = 0 .. Z P + 1: the closed form in numpy's double, rounded to f32."""
    i = np.arange(Z * P + 2, dtype=np.float64)
    arg = np.maximum(1.0 - (i / (Z * P)) ** 2, 0.0)
    h = (np.sinc(i / P) * np.i0(8.0 * np.sqrt(arg)) / np.i0(8.0)).astype(np.float32)
    h[::P] = 0.0
    h[0] = 1.0
    h[Z * P:] = 0.0
    return h


def inv_of(ratio):
    """(int) rintf(2^20 / p): one f32 division, ties to even."""
    return np.rint(F32(1048576.0) / np.asarray(ratio, np.float32)).astype(np.int64)


def peak(y):
    """The fmaxf chain over |y| from 0.0f: a NaN is never taken."""
    a = np.abs(np.asarray(y, np.float32))
    a = a[~np.isnan(a)]
    return F32(a.max()) if a.size else F32(0.0)


def valid_samples(frames, L, hop):
    return hop * max(1, int(np.asarray(frames, np.int64)[:L].sum()))


def plan(frames, L, ratio, hop):
    """-> Tq [T] int64, wc [T] int64 (saturated), wlen.  At and past L: the row's end."""
    fs = np.asarray(frames, np.int64)
    T = fs.size
    v = np.zeros(T, np.int64)
    inv = np.full(L, ONE, np.int64) if ratio is None else inv_of(np.asarray(ratio, np.float32)[:L])  # behind L: never looked at
    v[:L] = hop * fs[:L] * inv
    tq = np.cumsum(v)
    wc = np.minimum(-((-tq) // ONE), SAT)
    wlen = int(wc[L - 1]) if L > 0 and fs[:L].sum() > 0 else hop
    return tq, wc, wlen


def warp(x, frames, L, ratio, hop, h):
    """y [wlen] of the row x [n], n = hop max(1, sum frames[:L])."""
    x = np.asarray(x, np.float32)
    fs = np.asarray(frames, np.int64)[:L]
    n = valid_samples(fs, L, hop)
    assert x.size == n
    if fs.sum() == 0:  # one pseudo-phoneme of hop samples, inv = ONE
        fs, inv = np.array([1], np.int64), np.array([ONE], np.int64)
    else:
        inv = np.full(L, ONE, np.int64) if ratio is None else inv_of(np.asarray(ratio, np.float32)[:L])
    tq = np.cumsum(hop * fs * inv)
    wc = -((-tq) // ONE)
    wlen = int(wc[-1])
    assert wlen < SAT
    k = np.arange(wlen, dtype=np.int64)
    t = np.searchsorted(wc, k, side="right")  # the smallest t with wc[t] > k, i.e. Tq[t] > k ONE
    tq_prev = np.concatenate([[0], tq[:-1]])[t]
    c_prev = np.concatenate([[0], np.cumsum(fs)[:-1]])[t]
    iv = inv[t]
    q, r = np.divmod(k * ONE - tq_prev, iv)
    i0 = hop * c_prev + q
    D = np.maximum(iv, ONE)
    acc = np.zeros(wlen, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(-2 * Z, 2 * Z + 1):  # j ascending
            j = i0 + d
            N = -d * iv + r
            a = np.abs(N)
            m = a < Z * D
            idx, rem = np.divmod(np.where(m, a, 0) * P, D)
            phi = rem.astype(np.float32) / D.astype(np.float32)
            h0, h1 = h[idx], h[idx + 1]
            coef = h0 + phi * (h1 - h0)
            xj = np.where((j >= 0) & (j < n), x[np.clip(j, 0, n - 1)], F32(0.0)).astype(np.float32)
            acc = np.where(m, acc + coef * xj, acc).astype(np.float32)
        y = np.where(iv >= ONE, acc, (iv.astype(np.float32) * F32(2.0 ** -20)) * acc).astype(np.float32)
    return np.where((iv == ONE) & (r == 0), x[np.clip(i0, 0, n - 1)], y).astype(np.float32)


def position(k, inv):
    """Source position of output k of a row that is one span of constant inv (double; for the tone checks)."""
    return np.asarray(k, np.float64) * ONE / inv
