"""The timing rule of include/mi355vits.h (mi355vits_run_timed) restated in numpy: np.float32 products, integer sums in Python
ints / int64, a bisection over uint32 views.  Written from the rule, not from the kernel: one row at a time, no tiles, no waves.

    u[t]    given (the kernel's dur_float tap, or the hook's input)
    c(x)    = x < CAP ? (int) ceil(x) : CAP + 1
    f[t](s) = max(c(fl(u[t] * s)), min_frames[t])
    F(s)    = sum over t < L of f[t](s)
"""
import numpy as np

CAP = 1 << 22  # DURATION_FRAME_CAP
S_MIN = np.float32(2.0 ** -30)
S_MAX = np.float32(2.0 ** 30)
OK, BELOW_FLOOR, UNREACHABLE = 0, 1, 2


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def from_bits(b: int) -> np.float32:
    return np.uint32(b).view(np.float32)


def count(x: np.ndarray) -> np.ndarray:
    """c(x) element-wise, int64.  NaN and +inf are not below CAP: CAP + 1."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        small = x < np.float32(CAP)
    return np.where(small, np.ceil(np.where(small, x, np.float32(0))).astype(np.int64), CAP + 1)


def frames_at(u: np.ndarray, mn: np.ndarray, s) -> np.ndarray:
    """f[t](s) for every t of one row (already cut to t < L), int64."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        prod = (np.asarray(u, np.float32) * np.float32(s)).astype(np.float32)  # ONE f32 multiply per element
    return np.maximum(count(prod), np.asarray(mn, np.int64))


def total(u, mn, s) -> int:
    return int(frames_at(u, mn, s).sum())


def fit_row(u, L, mn=None, target=0):
    """One row: u [T] float32, L phonemes, mn [T] or None, target 0 (none) or 1 .. CAP ->
    (frames [T] int64, factor float32, status)."""
    T = len(u)
    L = int(L)
    uu = np.asarray(u, np.float32)[:L]
    mm = np.zeros(L, np.int64) if mn is None else np.asarray(mn, np.int64)[:L]
    N = int(target)
    out = np.zeros(T, np.int64)
    if N == 0:
        out[:L] = frames_at(uu, mm, np.float32(1.0))
        return out, np.float32(1.0), OK
    if total(uu, mm, S_MIN) > N:  # below the floor: the floor is returned
        out[:L] = frames_at(uu, mm, S_MIN)
        return out, S_MIN, BELOW_FLOOR
    if total(uu, mm, S_MAX) <= N:
        out[:L] = frames_at(uu, mm, S_MAX)
        return out, S_MAX, (OK if total(uu, mm, S_MAX) == N else UNREACHABLE)
    lo, hi = bits(S_MIN), bits(S_MAX)  # F(lo) <= N < F(hi): the largest pattern with F <= N
    steps = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if total(uu, mm, from_bits(mid)) <= N:
            lo = mid
        else:
            hi = mid
        steps += 1
    assert steps <= 30
    s = from_bits(lo)
    s2 = np.nextafter(s, np.float32(np.inf), dtype=np.float32)
    assert bits(s2) == lo + 1
    base, nxt = frames_at(uu, mm, s), frames_at(uu, mm, s2)
    left = N - int(base.sum())
    assert 0 <= left < int(nxt.sum()) - int(base.sum())
    for t in range(L):  # walk t upward
        if left == 0:
            break
        extra = min(int(nxt[t] - base[t]), left)
        base[t] += extra
        left -= extra
    assert left == 0 and int(base.sum()) == N
    out[:L] = base
    return out, s, OK


def fit(u, lens, mn=None, target=None):
    """A batch: u [B, T], lens [B], mn [B, T] or None, target [B] or None ->
    frames [B, T] int32, cum [B, T] int32 (inclusive scan saturated at 2 CAP), ylen [B] int32 = max(1, sum), factor [B] float32,
    status [B] int32."""
    u = np.asarray(u, np.float32)
    B, T = u.shape
    frames = np.zeros((B, T), np.int64)
    factor, status = np.zeros(B, np.float32), np.zeros(B, np.int32)
    for b in range(B):
        frames[b], factor[b], status[b] = fit_row(u[b], lens[b], None if mn is None else mn[b], 0 if target is None else target[b])
    cum = np.minimum(np.cumsum(frames, axis=1), 2 * CAP)
    ylen = np.maximum(1, cum[:, -1])
    return frames.astype(np.int32), cum.astype(np.int32), ylen.astype(np.int32), factor, status


def floor_of(u, L, mn=None) -> int:
    """F(2^-30): the fewest frames a row can be fitted to."""
    L = int(L)
    return total(np.asarray(u, np.float32)[:L], np.zeros(L, np.int64) if mn is None else np.asarray(mn, np.int64)[:L], S_MIN)


def natural(u, L, mn=None) -> int:
    """F(1)."""
    L = int(L)
    return total(np.asarray(u, np.float32)[:L], np.zeros(L, np.int64) if mn is None else np.asarray(mn, np.int64)[:L], np.float32(1.0))
