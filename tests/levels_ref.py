"""The numpy yardstick of level control in one run (mi355vits_run_levels, k_levels), written from the rule of include/mi355vits.h:
qs per sample, a prefix sum in int64, one double division, .astype(float32) and one float32 product.  Never the code under test."""
import numpy as np

ONE = 1 << 20
MAX_RAMP = 4096


def q_of(gain) -> np.ndarray:
    """q[t] = (int32) rintf(gain * 2^20): the float32 product is exact, np.rint rounds ties to even."""
    return np.rint(np.asarray(gain, np.float32) * np.float32(1048576.0)).astype(np.int64)


def valid_samples(cum, L: int, hop: int) -> int:
    """n = hop * max(1, c[L - 1]); hop when L = 0."""
    return int(hop) * max(1, int(cum[L - 1]) if L > 0 else 0)


def qs_of(cum, L: int, gain, hop: int) -> np.ndarray:
    """qs(i), 0 <= i < n: q of the smallest t < L with hop * c[t] > i, ONE when there is none."""
    n = valid_samples(cum, L, hop)
    if L <= 0 or int(cum[L - 1]) <= 0:
        return np.full(n, ONE, np.int64)
    ends = np.asarray(cum[:L], np.int64) * int(hop)
    t = np.searchsorted(ends, np.arange(n, dtype=np.int64), side="right")  # the first t with ends[t] > i
    return q_of(gain[:L])[t]


def scale_cum(cum, L: int, gain, R: int, hop: int) -> np.ndarray:
    """scale[k], 0 <= k < n, float32, from the inclusive scan of the frames."""
    qs = qs_of(cum, L, gain, hop)
    R = int(R)
    ext = np.concatenate([np.full(R, qs[0], np.int64), qs, np.full(R, qs[-1], np.int64)])  # edge values repeat
    P = np.concatenate([np.zeros(1, np.int64), np.cumsum(ext, dtype=np.int64)])
    S = P[2 * R + 1:] - P[: len(qs)]  # sum of qs(i) over k - R <= i <= k + R
    return (S.astype(np.float64) / np.float64((2 * R + 1) * ONE)).astype(np.float32)


def scale(frames, L: int, gain, R: int, hop: int) -> np.ndarray:
    """The same from the frames of every phoneme (what mi355vits_fetch_alignment reports)."""
    return scale_cum(np.cumsum(np.asarray(frames, np.int64)), int(L), gain, R, hop)


def apply(x, s) -> np.ndarray:
    """y[k] = x[k] * scale[k]: one float32 product."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(x, np.float32) * np.asarray(s, np.float32)).astype(np.float32)


def peak(y) -> np.float32:
    """The fmaxf chain over |y| from 0.0f: a NaN is never taken."""
    a = np.abs(np.asarray(y, np.float32))
    a = a[~np.isnan(a)]
    return np.float32(a.max()) if a.size else np.float32(0.0)


def same_bits(got, want) -> bool:
    """Bit for bit — except that a NaN equals a NaN: IEEE leaves the sign and payload of the NaN an invalid product (Inf * 0) makes
    to the platform, and the CPU's differs from the GPU's."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))
