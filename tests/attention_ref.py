"""Relative-position attention: the fp64 reference, its float32 calibration, the per-element criterion and the case
tables that tests/test_attention.py (CPU model of the kernels) and tests/test_gpu_attention.py (MI355X) share.

The three kernels behind ``test_rel_attention(..., impl=)``: 0 = k_rel_attention (VALU, csrc/kernels_misc.cpp), 1 =
k_rel_attention_mfma4 (T <= 512, five instantiations), 2 = k_rel_attention_stream (any T, five instantiations by head width).

Criterion (check_vs_fp64).  e = norm_err(kernel) and e32 = norm_err(rel_attention_f32), both against rel_attention_fp64 on the
same inputs; the kernel passes when e <= max(3 * e32, 2**-23).  The factor 3 is the project's margin for "f32-grade"
(tests/util.py: f32_grade_vs_fp64); the floor is one rounding of the largest element, needed at T = 1 where the rule is a single
add and the float32 evaluation can be exact.  rel_attention_f32 is the calibration and is never under test."""
import functools

import numpy as np

F32_FACTOR = 3.0
F32_FLOOR = 2.0 ** -23


def rel_attention_fp64(qkv, ek, ev, lengths, n_heads):
    """SURVEY A.4 restated in float64: s = (q / sqrt d) . k + the band term via E_k, keys past the row's length masked,
    softmax, o = P V + the band term via E_v.  Query rows at or past the length are left at zero."""
    qkv = np.asarray(qkv, np.float64)
    ek = np.asarray(ek, np.float64)
    ev = np.asarray(ev, np.float64)
    B, H3, T = qkv.shape
    H = H3 // 3
    d = H // n_heads
    Wn = (ek.shape[0] - 1) // 2
    out = np.zeros((B, H, T))
    for b in range(B):
        L = int(lengths[b])
        if L == 0:
            continue
        idx = np.arange(L)
        rel = idx[None, :] - idx[:, None]
        inwin = np.abs(rel) <= Wn
        relc = np.clip(rel + Wn, 0, 2 * Wn)
        for h in range(n_heads):
            c0 = h * d
            q = qkv[b, c0:c0 + d, :L].T / np.sqrt(d)
            k = qkv[b, H + c0:H + c0 + d, :L].T
            v = qkv[b, 2 * H + c0:2 * H + c0 + d, :L].T
            rl = q @ ek.T
            s = q @ k.T + np.where(inwin, np.take_along_axis(rl, relc, axis=1), 0.0)
            p = np.exp(s - s.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            pw = np.where(inwin, p, 0.0)
            relw = np.zeros((L, 2 * Wn + 1))
            for r in range(2 * Wn + 1):  # inside the window relc == r is the one key j = i + r - Wn
                j = idx + (r - Wn)
                ok = (j >= 0) & (j < L)
                relw[idx[ok], r] = pw[idx[ok], j[ok]]
            out[b, c0:c0 + d, :L] = (p @ v + relw @ ev).T
    return out


def rel_attention_f32(qkv, ek, ev, lengths, n_heads):
    """The same rule evaluated by numpy in float32 throughout: the scaled q, the logits, exp, the sum, both products, and the
    divide last (as the kernels do).  The calibration of check_vs_fp64: what plain float32 arithmetic loses on these inputs."""
    qkv = np.asarray(qkv, np.float32)
    ek = np.asarray(ek, np.float32)
    ev = np.asarray(ev, np.float32)
    B, H3, T = qkv.shape
    H = H3 // 3
    d = H // n_heads
    Wn = (ek.shape[0] - 1) // 2
    scale = np.float32(1.0) / np.sqrt(np.float32(d))
    out = np.zeros((B, H, T), np.float32)
    for b in range(B):
        L = int(lengths[b])
        if L == 0:
            continue
        idx = np.arange(L)
        for h in range(n_heads):
            c0 = h * d
            q = qkv[b, c0:c0 + d, :L].T * scale
            k = qkv[b, H + c0:H + c0 + d, :L].T
            v = qkv[b, 2 * H + c0:2 * H + c0 + d, :L].T
            rl = q @ ek.T
            s = q @ k.T
            for r in range(2 * Wn + 1):
                j = idx + (r - Wn)
                ok = (j >= 0) & (j < L)
                s[idx[ok], j[ok]] += rl[idx[ok], r]
            e = np.exp(s - s.max(axis=1, keepdims=True))
            relw = np.zeros((L, 2 * Wn + 1), np.float32)
            for r in range(2 * Wn + 1):
                j = idx + (r - Wn)
                ok = (j >= 0) & (j < L)
                relw[idx[ok], r] = e[idx[ok], j[ok]]
            o = (e @ v + relw @ ev) / e.sum(axis=1, keepdims=True, dtype=np.float32)
            assert o.dtype == np.float32
            out[b, c0:c0 + d, :L] = o.T
    return out


def attention_case(T, d, lengths, n_heads=2, Wn=4, seed=0, mix_shape=False):
    """Random q/k/v, E_k, E_v for a [len(lengths), 3 * d * n_heads, T] case.  The seed mixes T and d; with mix_shape (the case tables
    below) also n_heads and Wn, away from the shipped two heads and window 4, whose data stay those of a plain call."""
    mix = seed + T + 7 * d
    rng = np.random.default_rng([mix, n_heads, Wn] if mix_shape and (n_heads, Wn) != (2, 4) else mix)
    H = d * n_heads
    qkv = rng.standard_normal((len(lengths), 3 * H, T)).astype(np.float32)
    ek = (0.5 * rng.standard_normal((2 * Wn + 1, d))).astype(np.float32)
    ev = (0.5 * rng.standard_normal((2 * Wn + 1, d))).astype(np.float32)
    return qkv, ek, ev, np.asarray(lengths, np.int32)


def norm_err(got, ref, lens):
    """Worst max|got - ref| / max|ref| over the rows with L > 0, each over its own [:, :L]; inf when a row holds a NaN or an
    infinity on either side (a non-finite element must never pass a comparison)."""
    worst = 0.0
    for b, L in enumerate(lens):
        L = int(L)
        if L:
            r = np.asarray(ref[b][:, :L], np.float64)
            e = float(np.abs(np.asarray(got[b][:, :L], np.float64) - r).max() / np.abs(r).max())
            if not np.isfinite(e):
                return float("inf")
            worst = max(worst, e)
    return worst


def f32_bound(e32):
    return max(F32_FACTOR * e32, F32_FLOOR)


@functools.lru_cache(maxsize=4)
def reference_case(T, d, n_heads, Wn, lengths):
    """(qkv, ek, ev, len, fp64 reference, float32 calibration) of a case: computed once for the checks of one test that share
    it (the last four cases are kept), read-only."""
    qkv, ek, ev, ln = attention_case(T, d, list(lengths), n_heads, Wn, mix_shape=True)
    ref = rel_attention_fp64(qkv, ek, ev, ln, n_heads)
    f32 = rel_attention_f32(qkv, ek, ev, ln, n_heads)
    for a in (qkv, ek, ev, ln, ref, f32):
        a.flags.writeable = False
    return qkv, ek, ev, ln, ref, f32


IMPL_NAMES = {0: "k_rel_attention", 1: "k_rel_attention_mfma4", 2: "k_rel_attention_stream"}


def assert_vs_fp64(got, ref, f32, lens, impl, tag):
    """The criterion on rows that are already computed: got / ref / f32 [B, H, T], lens [B].  Prints e, e32 and their ratio.
    impl 2: query rows at or past L are exact zeros.  impl 0 and 1: every element is written (a padded query row takes the
    reference's -1e4 fill: a finite average of V that never reaches a valid frame and is not compared) and must be finite."""
    for b, L in enumerate(lens):
        assert np.isfinite(got[b][:, :int(L)]).all(), (tag, IMPL_NAMES[impl], b, "a valid element is not finite")
        if impl == 2:
            assert np.all(got[b][:, int(L):] == 0.0), (tag, b, "padded query rows must be zeros")
        else:
            assert np.isfinite(got[b]).all(), (tag, b, "a written element is not finite")
    e, e32 = norm_err(got, ref, lens), norm_err(f32, ref, lens)
    print(f"attention {IMPL_NAMES[impl]} {tag}: e = {e:.3e}  e32 = {e32:.3e}  e/e32 = {e / max(e32, 1e-30):.3f}")
    assert e <= f32_bound(e32), (tag, IMPL_NAMES[impl], e, e32, f32_bound(e32))
    return e, e32


def check_vs_fp64(lib, impl, T, d, n_heads, Wn, lengths):
    """Runs the hook on the case and asserts the criterion of this module's docstring.  Returns the kernel's output."""
    qkv, ek, ev, ln, ref, f32 = reference_case(T, d, n_heads, Wn, tuple(int(n) for n in lengths))
    got = lib.test_rel_attention(qkv, ek, ev, ln, n_heads, impl=impl)
    assert got.shape == ref.shape and got.dtype == np.float32
    assert_vs_fp64(got, ref, f32, ln, impl, f"T={T} d={d} heads={n_heads} W={Wn}")
    return got


def valu_cap(d, n_heads, Wn):
    """The longest T the VALU kernel serves: VitsConfig.attention_cap, the mirror of rel_attention_valu_cap."""
    from mimic3_amd.config import VitsConfig

    cfg = VitsConfig.tiny()
    cfg.hidden_channels, cfg.n_heads, cfg.window_size = d * n_heads, n_heads, Wn
    return cfg.attention_cap


# ---------------------------------------------------------------------------------------------------- the case tables
def case_lengths(T):
    """One batch row each: full, one short, inside the last 32-column tile, a tile and a column short, 17, one id, empty."""
    return sorted(n for n in {T, T - 1, T - 5, T - 33, 17, 1, 0} if 0 <= n <= T)


# (a) the MFMA kernel just before, at and just past a query tile and every NKW boundary (<1,48>, <2,48>, <4>): d = 96, 2 heads, W = 4
MFMA_LENGTH_CLASSES = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512]

# (b) head shapes (d, n_heads, W) on the VALU and the MFMA kernel: widths that are no multiple of 4 or 32, more than three output
# tiles, nrel = 1 and 31, one and four heads
HEAD_SHAPES = [(2, 2, 4), (6, 1, 0), (16, 2, 4), (34, 3, 1), (48, 4, 15), (64, 2, 0), (80, 2, 10), (96, 2, 15), (128, 1, 15)]
HEAD_SHAPE_LENGTHS = [70, 200, 300]

# (c) the streamed kernel at each DP bucket's upper edge and the first width of the next bucket: (d, T, W), W spread over the cases
STREAM_WIDTHS = [2, 16, 18, 32, 34, 64, 66, 96, 98, 128]
STREAM_CASES = [(d, T, (0, 4, 15)[(2 * k + n) % 3]) for k, d in enumerate(STREAM_WIDTHS) for n, T in enumerate((33, 130))]

# (d) shapes of (b) that all three kernels accept: (T, d, n_heads, W)
AGREE_CASES = [(70, 2, 2, 4), (200, 34, 3, 1), (200, 48, 4, 15), (300, 128, 1, 15)]

# (e) the grid-chosen form of the MFMA kernel at d = 96
GRID_FORM_LENGTHS = [100, 230]

# (g) shapes each kernel's hook refuses: (impl, T, d, n_heads, W, message)
REFUSALS = [(1, 513, 96, 2, 4, "MFMA"), (1, 40, 15, 2, 4, "MFMA"), (1, 40, 16, 2, 16, "MFMA"),
            (2, 40, 130, 1, 4, "streamed"), (2, 40, 16, 2, 16, "streamed"),
            (0, "cap + 1", 16, 2, 4, "VALU")]  # "cap + 1": valu_cap(d, n_heads, W) + 1; at the cap itself the kernel must serve

# (h) whole voices: (n_heads, window_size) of VitsConfig.tiny()
VOICE_SHAPES = [(1, 0), (4, 1), (2, 15), (4, 7)]
VOICE_REFUSED = (2, 16)  # above the voice format's window cap of 15: refused when the voice is loaded, never computed


def agree_case(lib, T, d, n_heads, Wn):
    """(d) the three kernels on one input: each within the criterion, and pairwise within twice its bound."""
    lens = case_lengths(T)
    outs = [check_vs_fp64(lib, impl, T, d, n_heads, Wn, lens) for impl in (0, 1, 2)]
    _, _, _, ln, ref, f32 = reference_case(T, d, n_heads, Wn, tuple(lens))
    bound = 2.0 * f32_bound(norm_err(f32, ref, ln))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        e = norm_err(outs[a], outs[b], ln)
        print(f"attention {IMPL_NAMES[a]} vs {IMPL_NAMES[b]} T={T} d={d}: {e:.3e} (bound {bound:.3e})")
        assert e <= bound, (T, d, n_heads, Wn, a, b, e, bound)
    return outs


def grid_form_case(run_small, run_large, T, B_large):
    """(e) four distinct ragged rows as one batch of 4 (run_small) and tiled to B_large rows (run_large): every copy equals its
    small-batch row bit for bit; three rows of the large batch against fp64.  Returns (small, large)."""
    d, n_heads, Wn = 96, 2, 4
    lens = (T, T - 1, T - 33, 17)
    qkv, ek, ev, ln, ref, f32 = reference_case(T, d, n_heads, Wn, lens)
    small = run_small(qkv, ek, ev, ln, n_heads)
    assert_vs_fp64(small, ref, f32, ln, 1, f"T={T} d=96 batch 4")
    assert B_large % 4 == 0
    reps = B_large // 4
    large = run_large(np.tile(qkv, (reps, 1, 1)), ek, ev, np.tile(ln, reps), n_heads)
    for b in range(B_large):
        assert np.array_equal(large[b], small[b % 4]), (T, b, "a row of the large grid differs from its small-batch bits")
    rows = [0, B_large // 2 + 1, B_large - 1]
    assert_vs_fp64(large[rows], ref[[r % 4 for r in rows]], f32[[r % 4 for r in rows]], ln[[r % 4 for r in rows]], 1,
                   f"T={T} d=96 batch {B_large} rows {rows}")
    return small, large


def padding_case(lib, impl):
    """(f) [:, :L] of every row does not depend on what lies past it: the same rows inside T = 333 with 1e3 in every added column
    (the MFMA kernel moves from NKW = 2 to NKW = 4), and T = 200 with 1e3 in every column at or past a row's length."""
    T, d, n_heads, Wn, lens = 200, 96, 2, 4, (200, 150, 70)
    qkv, ek, ev, ln, _, _ = reference_case(T, d, n_heads, Wn, lens)
    plain = check_vs_fp64(lib, impl, T, d, n_heads, Wn, lens)
    wide = np.full((len(lens), qkv.shape[1], 333), 1e3, np.float32)
    wide[:, :, :T] = qkv
    junk = qkv.copy()
    for b, L in enumerate(lens):
        junk[b, :, L:] = 1e3
    for name, x in (("wider batch", wide), ("junk past the length", junk)):
        got = lib.test_rel_attention(x, ek, ev, ln, n_heads, impl=impl)
        for b, L in enumerate(lens):
            assert np.array_equal(got[b, :, :L], plain[b, :, :L]), (IMPL_NAMES[impl], name, b, L)
