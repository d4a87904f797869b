"""The text side's small kernels — k_embed, k_layernorm (both templates), k_dp_det (both math modes) — and the Philox noise
(k_sdp_noise, the keyed branch of k_expand_prior): the fp64 rules, their float32 calibrations and the case tables that
tests/test_small_kernels.py (CPU model of the kernels) and tests/test_gpu_small_kernels.py (MI355X) share.

The rules, per row on its own columns:
  embed      y[c, t] = float32(emb[ids[t], c]) * float32(scale) below len, exact zeros behind it: one float32 product, so bit equality.
  layernorm  v = x (the partial sums added in slice order) + bias; v = 0 at t >= premask_len; v += res; mean over the channels, then
             the biased variance of the centred values (two passes); y = (v - mean) / sqrt(var + eps) * gamma + beta; erf GELU; + add_to;
             0 at t >= out_len.
  dp_det     h1 = LN_1(relu(conv_1((x + cond) * m))); h2 = LN_2(relu(conv_2(h1 * m))); logw = (proj_w . h2 + proj_b) * m — the
             restatement of tests/detdp_util.py (det_logw, which test_small_kernels pins this one to) in numpy.
  noise      Philox4x32-10 from its published definition (Salmon et al., SC'11: multipliers 0xD2511F53 / 0xCD9E8D57, key bumps
             0x9E3779B9 / 0xBB67AE85, ten rounds) under the mapping of csrc/kernels_misc.cpp's philox_normal: counter
             (t, c, low32(utt), tensor ^ high32(utt) * 0x9E3779B9 mod 2^32), key (low32(seed), high32(seed));
             u_i = float32(float32(r_i >> 8) + 0.5f) * 2^-24 IN float32 (from 2^23 on the sum rounds, the last value gives u = 1: that is
             the definition); the cosine's argument is the float32 product 6.2831855f * u_1; then sqrt(-2 ln u_0) * cos(arg) in fp64.
Criterion: the one of tests/attention_ref.py / tests/conv_ref.py (norm_err, f32_bound, assert_vs_fp64: imported, not restated):
e = norm_err(kernel), e32 = norm_err(calibration), both against the fp64 rule; the kernel passes when e <= max(3 e32, 2^-23) and
every valid element is finite.  The calibrations: the same formulas in numpy float32 (log, sqrt, cos for the noise; the kernel's two
passes for LayerNorm; two input channels per float32 addition for k_dp_det's convs, as conv_ref does for the MFMA paths).  They are
never under test."""
import functools

import numpy as np

from tests import conv_ref as CR
from tests.attention_ref import f32_bound, norm_err  # noqa: F401  (re-exported)
from tests.conv_ref import RATIOS, assert_vs_fp64, class_lengths, ratios_into  # noqa: F401  (ratios_into: re-exported)
from tests.sdp_ref import expand_prior_ref, gelu_erf
from tests.wn_ref import JUNK, Twice as _Twice
from mimic3_amd._native import MATH_BF16X3, MATH_F32, NativeError  # noqa: F401

NAN = np.float32(np.nan)  # what the LayerNorm padding tests put where the kernel discards by select
MATHS = [MATH_F32, MATH_BF16X3]
MATH_NAMES = {MATH_F32: "k_dp_det<F32>", MATH_BF16X3: "k_dp_det<split-bf16>"}
DP_OLD_MAX_ABS_TOL = 1e-5  # the engine-level bound on logw of tests/test_det_dp.py (the bite test quotes it)


class Twice(_Twice):
    """wn_ref.Twice over the hooks of this family."""

    def test_embed(self, *a, **k):
        return self._twice(self.lib.test_embed, *a, **k)

    def test_layernorm(self, *a, **k):
        return self._twice(self.lib.test_layernorm, *a, **k)

    def test_dp_det(self, *a, **k):
        return self._twice(self.lib.test_dp_det, *a, **k)

    def test_sdp_noise(self, *a, **k):
        return self._twice(self.lib.test_sdp_noise, *a, **k)

    def test_expand_prior_keyed(self, *a, **k):
        return self._twice(self.lib.test_expand_prior_keyed, *a, **k)


def passes_vs_fp64(got, ref, f32, lens):
    """conv_ref's verdict without asserting (the bite test), [B, T] outputs included."""
    return CR.passes_vs_fp64(*(a[:, None, :] if a.ndim == 2 else a for a in (got, ref, f32)), lens)


def assert_vs_fp64_ill_conditioned(got, ref, f32, lens, who, tag):
    """conv_ref.assert_vs_fp64 without its last clause, the engine-level rel. RMS below 5e-6: for the one case whose INPUT is
    ill-conditioned on purpose (LayerNorm at mean 100, spread 1: v - mean cancels seven bits of any float32 v, so 2^-24 * 100 = 6e-6
    of the spread is the input's own precision, and the calibration shows it).  e <= max(3 e32, 2^-23) and finiteness stay."""
    for b, L in enumerate(lens):
        assert np.isfinite(got[b][:, :int(L)]).all(), (who, tag, b, "a valid element is not finite")
    e, e32 = norm_err(got, ref, lens), norm_err(f32, ref, lens)
    ratio = e / max(e32, 1e-30)
    table = RATIOS.setdefault(CR._ratios_of[0], {})
    table[who] = max(table.get(who, 0.0), ratio if e > 2.0 ** -23 else 0.0)
    print(f"small {who} {tag}: e = {e:.3e}  e32 = {e32:.3e}  e/e32 = {ratio:.3f}")
    assert np.isfinite(e32) and e <= f32_bound(e32), (who, tag, e, e32, ratio, f32_bound(e32), CR.worst_element(got, ref, lens))


def native_of(lib):
    """The NativeLibrary itself (an Engine wants it, not the doubling wrapper)."""
    return lib.lib if isinstance(lib, _Twice) else lib


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


# ---------------------------------------------------------------------------------------------------- Philox
M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KNOWN_ANSWERS = [  # (counter, key, output): the Random123 known-answer vectors of philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32 on arrays of 32-bit words (any broadcastable shapes) -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, np.uint64) & M32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(rounds):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & M32, (k1 + np.uint64(PHILOX_W1)) & M32
    return c0, c1, c2, c3


def draw_words(seed, utt, tensor, c, t, rounds=10, swap_ct=False):
    """(r_0, r_1) of the draw of element (channel c, time t) of tensor `tensor` of utterance `utt` under `seed`: the kernel's mapping.
    rounds / swap_ct: the wrong variants of the bite test."""
    seed, utt = int(seed) & (2 ** 64 - 1), int(utt) & (2 ** 64 - 1)
    c3 = (int(tensor) ^ ((utt >> 32) * PHILOX_W0)) & 0xFFFFFFFF
    a, b = (c, t) if swap_ct else (t, c)
    r = philox4x32(a, b, utt & 0xFFFFFFFF, c3, seed & 0xFFFFFFFF, seed >> 32, rounds)
    return r[0], r[1]


def uniform_of(r):
    """u = float32(float32(r >> 8) + 0.5f) * 2^-24, every step in float32, as the kernel writes it."""
    return ((np.asarray(r, np.uint64) >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def normal_of(r0, r1, dt):
    """Box-Muller on the two words: fp64 (the rule) or float32 with numpy's log, sqrt and cos (the calibration).  The uniforms and
    the cosine's argument are float32 in both: they are part of the definition."""
    u1, u2 = uniform_of(r0), uniform_of(r1)
    arg = np.float32(6.28318530717958647692) * u2
    assert u1.dtype == np.float32 and arg.dtype == np.float32
    with np.errstate(divide="ignore"):
        out = np.sqrt(dt(-2.0) * np.log(u1.astype(dt))) * np.cos(arg.astype(dt))
    assert out.dtype == dt
    return out


def normals(seed, utt, tensor, C, T, dt, **variant):
    """[C, T] draws of one tensor of one utterance."""
    c, t = np.arange(C, dtype=np.uint64)[:, None], np.arange(T, dtype=np.uint64)[None, :]
    r0, r1 = draw_words(seed, utt, tensor, c, t, **variant)
    return normal_of(np.broadcast_to(r0, (C, T)), np.broadcast_to(r1, (C, T)), dt)


def moments(x):
    """(mean, variance - 1, skew, excess kurtosis, lag-one correlation along t, along c) of [C, T] draws, each divided by its standard
    error under N(0, 1) (1 / sqrt N, sqrt(2 / N), sqrt(6 / N), sqrt(24 / N), 1 / sqrt N twice)."""
    x = np.asarray(x, np.float64)
    n = x.size
    m, v = x.mean(), x.var()
    z = (x - m) / np.sqrt(v)
    ct = (z[:, 1:] * z[:, :-1]).mean()
    cc = (z[1:] * z[:-1]).mean()
    return np.asarray([m * np.sqrt(n), (v - 1) / np.sqrt(2 / n), (z ** 3).mean() / np.sqrt(6 / n), ((z ** 4).mean() - 3) / np.sqrt(24 / n),
                       ct * np.sqrt(n), cc * np.sqrt(n)])


SEED = 0x5DEECE66D1234567       # both words non-zero
UTTS = (0, 7, 2 ** 32 + 7, 2 ** 63 + 5)
NOISE_T = [1, 63, 64, 65, 200]
NOISE_W = (0.8, 0.0, 1.0, 0.333)  # a row at 0: exact zeros, no draw


def sdp_noise_rule(T, dt, seed=SEED, utts=UTTS, noise_w=NOISE_W, **variant):
    """z [B, 2, T] = draw(tensor 0) * noise_w[b]."""
    z = np.zeros((len(utts), 2, T), dt)
    for b, (u, w) in enumerate(zip(utts, noise_w)):
        if w != 0:
            z[b] = normals(seed, u, 0, 2, T, dt, **variant) * dt(np.float32(w))
    return z


def check_sdp_noise(lib, T):
    ref, f32 = sdp_noise_rule(T, np.float64), sdp_noise_rule(T, np.float32)
    z = lib.test_sdp_noise(T, SEED, UTTS, NOISE_W)
    assert np.isfinite(z).all() and not np.any(z == JUNK), ("k_sdp_noise", T, "every element is written, and finite")
    lens = [T if w != 0 else 0 for w in NOISE_W]
    assert_vs_fp64(z, ref, f32, lens, "k_sdp_noise", f"T={T}")
    for b, w in enumerate(NOISE_W):
        if w == 0:
            assert np.all(z[b].view(np.uint32) == 0), ("k_sdp_noise", T, "a row at noise_w = 0 is exact +0", b)
    return z


EXPAND_KEYED = [(3, 65), (8, 65), (3, 130), (8, 130)]  # (I, Ty)
EXPAND_NS = (0.667, 0.0, 1.0, 0.5)


@functools.lru_cache(maxsize=4)
def expand_keyed_case(I, Ty):
    """Four rows under the four utterance keys: an empty phoneme in every cum, a row at noise_scale 0, a row with ylen < Ty."""
    rng = np.random.default_rng([11, I, Ty])
    durs = np.asarray([[2, 0, 3, 1, 0, 2, 1], [1, 1, 0, 0, 2, 1, 3], [0, 3, 0, 1, 1, 2, 1], [1, 2, 1, 0, 1, 0, 3]], np.int64)
    scale = np.asarray([Ty // 9 + 1, Ty // 8 + 1, Ty // 8, Ty // 16])
    cum = np.minimum(np.cumsum(durs * scale[:, None], axis=1), Ty).astype(np.int32)
    ylen = cum[:, -1].copy()
    assert ylen[0] == Ty and 0 < ylen[3] < Ty, ylen
    B, Tx = durs.shape
    c = dict(stats=(0.5 * rng.standard_normal((B, 2 * I, Tx))).astype(np.float32), cum=cum, ylen=ylen, ns=np.asarray(EXPAND_NS, np.float32))
    n64 = np.stack([normals(SEED, u, 1, I, Ty, np.float64) for u in UTTS])
    n32 = np.stack([normals(SEED, u, 1, I, Ty, np.float32) for u in UTTS])
    c["ref"] = expand_prior_ref(c["stats"], cum, ylen, Ty, c["ns"], n64, np.float64)
    c["f32"] = expand_prior_ref(c["stats"], cum, ylen, Ty, c["ns"], n32, np.float32)
    return _freeze(c)


def check_expand_keyed(lib, I, Ty):
    c = expand_keyed_case(I, Ty)
    z = lib.test_expand_prior_keyed(c["stats"], c["cum"], c["ylen"], Ty, c["ns"], SEED, UTTS)
    assert np.isfinite(z).all() and not np.any(z == JUNK), ("k_expand_prior keyed", I, Ty, "every element is written, and finite")
    assert_vs_fp64(z, c["ref"], c["f32"], c["ylen"], "k_expand_prior (keyed)", f"I={I} Ty={Ty}")
    for b, n in enumerate(int(v) for v in c["ylen"]):
        assert np.all(z[b][:, n:] == 0.0), ("frames at and past ylen[b] are zero", b, n)
    assert np.array_equal(z[1], c["f32"][1]), "noise_scale 0: the gathered means, bit for bit"
    return z


# ---------------------------------------------------------------------------------------------------- embed
EMBED_H = [1, 3, 4, 5, 192]
EMBED_T = [1, 63, 64, 65, 130]


@functools.lru_cache(maxsize=4)
def embed_case(H, T, S=37):
    """Three rows: full, empty, one that ends inside the last 64-column block.  Ids 0 and S - 1 occur below the lengths; past them
    the ids are negative and over the range."""
    rng = np.random.default_rng([5, H, T])
    start = (T - 1) // 64 * 64
    lens = np.asarray([T, 0, start + (T - start + 1) // 2], np.int32)
    ids = rng.integers(0, S, size=(3, T)).astype(np.int64)
    ids[0, 0], ids[0, -1] = S - 1, 0
    ids[2, 0] = 0 if T > 1 else S - 1
    for b, L in enumerate(lens):
        ids[b, L:] = np.where(np.arange(T - L) % 2 == 0, -1 - np.arange(T - L), S + np.arange(T - L) * 2 ** 33)
    emb = rng.standard_normal((S, H)).astype(np.float32)
    scale = np.float32(np.sqrt(np.float32(H)))
    want = np.zeros((3, H, T), np.float32)
    for b, L in enumerate(lens):
        want[b, :, :L] = (emb[ids[b, :L]] * scale).T
    return _freeze(dict(ids=ids, lens=lens, emb=emb, scale=scale, want=want))


def check_embed(lib, H, T):
    c = embed_case(H, T)
    y = lib.test_embed(c["ids"], c["lens"], c["emb"], c["scale"])
    assert not np.any(y == JUNK), ("k_embed", H, T, "every element of y is written")
    assert np.array_equal(y.view(np.uint32), c["want"].view(np.uint32)), ("k_embed", H, T, "float32(emb) * float32(scale) below the length, +0 behind it")
    return y


# ---------------------------------------------------------------------------------------------------- LayerNorm
LN_C = [1, 5, 16, 17, 192, 255, 256]
LN_T = [1, 15, 16, 17, 33]
LN_C_UNCACHED = [257, 300]
LN_T_UNCACHED = [1, 17, 33]
# (name, options): every option alone, then the engine's four real combinations (alias = the in-place use the engine makes of it)
LN_OPTIONS = [
    ("plain", {}),
    ("in place", dict(alias="x")),
    ("gelu", dict(gelu=True)),
    ("add_to", dict(add_to=True)),
    ("res", dict(res=True)),
    ("bias", dict(bias=True)),
    ("premask_len", dict(premask=True)),
    ("nparts 2", dict(nparts=2)),
    ("nparts 4, strided", dict(nparts=4, stride_pad=5)),
    ("out_len", dict(out_len=True)),
    ("gelu + add_to, y == add_to", dict(gelu=True, add_to=True, alias="add_to")),
    ("nparts 2 + bias + premask + res, y == res", dict(nparts=2, bias=True, premask=True, res=True, alias="res")),
    ("nparts 4 + bias + premask + res, y == res", dict(nparts=4, bias=True, premask=True, res=True, alias="res")),
    ("nparts 2 + bias + premask + res + out_len, y == res", dict(nparts=2, bias=True, premask=True, res=True, out_len=True, alias="res")),
    ("nparts 4 + bias + premask + res + out_len, y == res", dict(nparts=4, bias=True, premask=True, res=True, out_len=True, alias="res", stride_pad=3)),
]
LN_OPTIONS_UNCACHED = [
    ("plain", {}),
    ("in place", dict(alias="x")),
    ("res, y == res", dict(res=True, alias="res")),
    ("gelu + add_to, y == add_to", dict(gelu=True, add_to=True, alias="add_to")),
    ("res + out_len", dict(res=True, out_len=True)),
    ("res + gelu + add_to + out_len, in place", dict(res=True, gelu=True, add_to=True, out_len=True, alias="x")),
]
LN_REFUSED = [dict(nparts=2), dict(bias=True), dict(premask=True)]  # at C = 257


def ln_lengths(T):
    """Rows: full, one short, half, empty — and, below T = 16, further full rows up to 16 full columns in all (the criterion's
    calibration is a maximum over the case's elements: one column is a small sample, as wn_ref.case_lengths says)."""
    return np.asarray([T, max(T - 1, 0), T // 2, 0] + [T] * max(0, -(-16 // T) - 1), np.int32)


def ln_case(C, T, opts=(), kind="random", seed=0):
    """The inputs of a LayerNorm case.  opts: (name, value) pairs over nparts, bias, premask, res, add_to, gelu, out_len, alias,
    stride_pad (extra floats between the slices).  out_len = ln_lengths(T); premask_len = the same less one where positive (the
    engine's two are equal; the kernel must tell them apart).  kind: "random"; "constant" = every column constant over the channels
    (value 1.5 k: the sums are exact, the variance is 0); "offset" = mean 100, spread 1 (what one-pass arithmetic loses)."""
    o = dict(nparts=1, bias=False, premask=False, res=False, add_to=False, gelu=False, out_len=False, alias=None, stride_pad=0)
    o.update(dict(opts))
    rng = np.random.default_rng([seed, C, T, o["nparts"]])
    ol = ln_lengths(T)
    B = len(ol)
    shape = (B, C, T)
    x = rng.standard_normal((o["nparts"],) + shape).astype(np.float32)
    if kind == "constant":
        x = np.broadcast_to((1.5 * (1 + np.arange(B * T) % 7)).astype(np.float32).reshape(B, 1, T), shape)[None].copy()
    elif kind == "offset":
        x = (100.0 + x).astype(np.float32)
    c = dict(x=x if o["nparts"] > 1 else x[0], nparts=o["nparts"], stride_pad=o["stride_pad"],
             bias=(0.3 * rng.standard_normal(C)).astype(np.float32) if o["bias"] else None,
             premask=np.where(ol > 1, ol - 1, ol).astype(np.int32) if o["premask"] else None,
             res=rng.standard_normal(shape).astype(np.float32) if o["res"] else None,
             add_to=rng.standard_normal(shape).astype(np.float32) if o["add_to"] else None,
             gamma=(1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32), beta=(0.2 * rng.standard_normal(C)).astype(np.float32),
             eps=1e-5, gelu=o["gelu"], out_len=ol if o["out_len"] else None, alias=o["alias"])
    c["cmp_len"] = np.full(B, T, np.int32)  # every column t < T is written and counts (zeros under out_len)
    return c


def layernorm_rule(c, dt, one_pass=False, var_count=None):
    """The rule of the module's docstring in dtype dt: [B, C, T], every column.  one_pass: var = E[v^2] - mean^2 (a wrong variant);
    var_count: the variance divided by this instead of C (a wrong variant: the padded channel count)."""
    x = c["x"] if c["nparts"] > 1 else c["x"][None]
    B, C, T = x.shape[1:]
    t = np.arange(T)[None, None, :]
    v = x[0].astype(dt)
    for p in range(1, c["nparts"]):
        v = v + x[p].astype(dt)
    if c["bias"] is not None:
        v = v + c["bias"].astype(dt)[None, :, None]
    if c["premask"] is not None:
        v = np.where(t < c["premask"][:, None, None], v, dt(0))
    if c["res"] is not None:
        v = v + c["res"].astype(dt)
    mean = v.sum(axis=1, keepdims=True, dtype=dt) / dt(C)
    d = v - mean
    if one_pass:
        var = (v * v).sum(axis=1, keepdims=True, dtype=dt) / dt(C) - mean * mean
    else:
        var = (d * d).sum(axis=1, keepdims=True, dtype=dt) / dt(var_count or C)
    with np.errstate(invalid="ignore"):
        y = d * (dt(1) / np.sqrt(var + dt(c["eps"]))) * c["gamma"].astype(dt)[None, :, None] + c["beta"].astype(dt)[None, :, None]
    if c["gelu"]:
        y = gelu_erf(y)
    if c["add_to"] is not None:
        y = y + c["add_to"].astype(dt)
    if c["out_len"] is not None:
        y = np.where(t < c["out_len"][:, None, None], y, dt(0))
    assert y.dtype == dt
    return y


def run_ln(lib, c, alias="case", rows=None, y_prior=None, **replace):
    """The hook call of a case.  alias: "case" = the case's own; rows: a subset of the rows; replace: x / res / add_to replacements."""
    g = lambda k: replace.get(k, c[k])
    sl = (lambda a: a) if rows is None else (lambda a: None if a is None else a[rows])
    x = g("x")
    x = x if rows is None else (x[:, rows] if c["nparts"] > 1 else x[rows])
    n = int(np.prod(x.shape[-3:]))
    return lib.test_layernorm(x, c["gamma"], c["beta"], c["eps"], bias=c["bias"], premask_len=sl(c["premask"]), res=sl(g("res")),
                              add_to=sl(g("add_to")), gelu=c["gelu"], out_len=sl(c["out_len"]), alias=c["alias"] if alias == "case" else alias,
                              part_stride=n + c["stride_pad"],
                              y_prior=y_prior)


def check_ln(lib, c, who, tag, ill_conditioned=False):
    """One case: the aliased run (if any) and the plain one give the same bits; against fp64 by the criterion; every t < T written."""
    got = run_ln(lib, c, alias=None)  # (y starts as JUNK: wrapper default)
    assert not np.any(got == JUNK), (who, tag, "every column t < T is written")
    if c["alias"]:
        assert np.array_equal(run_ln(lib, c).view(np.uint32), got.view(np.uint32)), (who, tag, "in place (y == " + c["alias"] + ") differs from out of place")
    ref, f32 = layernorm_rule(c, np.float64), layernorm_rule(c, np.float32)
    live = [int(n) if np.abs(ref[b]).max() > 0 else 0 for b, n in enumerate(c["cmp_len"])]  # (an all-zero row — out_len 0 — has no scale: checked below)
    (assert_vs_fp64_ill_conditioned if ill_conditioned else assert_vs_fp64)(got, ref, f32, live, who, tag)
    if c["out_len"] is not None:
        for b, L in enumerate(int(n) for n in c["out_len"]):
            assert np.all(got[b, :, L:] == 0.0), (who, tag, "row", b, "exact zeros at and past out_len", L)
    return got


def ln_padding_case(lib, c, who, tag):
    """NaN where the hook's comment says the kernel discards by select — x (every slice) at t >= premask_len, and x, res and add_to at
    t >= out_len — changes no bit anywhere and produces no NaN; a row equals its solo run."""
    plain = run_ln(lib, c, alias=None)
    T = plain.shape[2]
    t = np.arange(T)[None, None, :]
    dead = np.zeros(plain.shape, bool)
    if c["premask"] is not None:
        dead |= t >= c["premask"][:, None, None]
    rep = {}
    if c["out_len"] is not None:
        gone = np.broadcast_to(t >= c["out_len"][:, None, None], plain.shape)
        dead |= gone
        for k in ("res", "add_to"):
            if c[k] is not None:
                rep[k] = np.where(gone, NAN, c[k])
    assert dead.any()
    rep["x"] = np.where(dead[None] if c["nparts"] > 1 else dead, NAN, c["x"])
    got = run_ln(lib, c, alias=None, **rep)
    assert np.isfinite(got).all(), (who, tag, "a NaN past a length came out")
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), (who, tag, "NaN past a length moved an output")
    for b in range(plain.shape[0]):
        one = run_ln(lib, c, alias=None, rows=slice(b, b + 1))
        assert np.array_equal(one[0].view(np.uint32), plain[b].view(np.uint32)), (who, tag, "row", b, "differs from its solo run")


# ---------------------------------------------------------------------------------------------------- k_dp_det
DP_SHAPES = [(32, 32, 1), (64, 32, 3), (192, 64, 3), (192, 256, 3), (32, 256, 5), (96, 160, 5), (256, 256, 7)]  # (H, F, K); the last: the largest LDS request
DP_REFUSED = [(48, 64, 3), (192, 288, 3), (192, 64, 4), (192, 64, 9)]
DP_GROUP = 2  # input channels per float32 addition of the calibration's convs (conv_ref.GROUP for the MFMA paths)


def _ln_rows(h, gamma, beta, dt):
    mean = h.sum(axis=0, dtype=dt) / dt(h.shape[0])
    d = h - mean
    var = (d * d).sum(axis=0, dtype=dt) / dt(h.shape[0])
    return d * (dt(1) / np.sqrt(var + dt(1e-5))) * gamma.astype(dt)[:, None] + beta.astype(dt)[:, None]


def two_term(a):
    """a float32 array with the third term of its three-term bf16 split dropped: hi + mid, exact in float32 (the bite test's variant)."""
    a = np.asarray(a, np.float32)
    hi = CR.bf16_round(a)
    return hi + CR.bf16_round(a - hi)


def dp_det_rule(c, dt, group=0, drop_third=False):
    """logw [B, T] of a case in dtype dt, every row alone.  drop_third: the weights of both convs lose the third term of their bf16
    split (a wrong variant of the split-bf16 kernel: the partial product l_w x h_x gone)."""
    x, lens, w = c["x"], c["lens"], c["w"]
    B, H, T = x.shape
    cut = two_term if drop_third else (lambda a: a)
    out = np.zeros((B, T), dt)
    for b in range(B):
        L = int(lens[b])
        xr = np.zeros((H, T), dt)
        xv = x[b, :, :L].astype(dt)
        if c["cond"] is not None:
            xv = xv + c["cond"][b].astype(dt)[:, None]
        xr[:, :L] = xv
        h = CR._conv_row(xr, cut(w["w1"]), 1, dt, group) + w["b1"].astype(dt)[:, None]
        h = _ln_rows(np.maximum(h, dt(0)), w["g1"], w["be1"], dt)
        h[:, L:] = 0
        h = CR._conv_row(h, cut(w["w2"]), 1, dt, group) + w["b2"].astype(dt)[:, None]
        h = _ln_rows(np.maximum(h, dt(0)), w["g2"], w["be2"], dt)
        v = (w["proj_w"].reshape(-1).astype(dt)[:, None] * h).sum(axis=0, dtype=dt) + dt(w["proj_b"].reshape(-1)[0])
        v[L:] = 0
        assert v.dtype == dt
        out[b] = v
    return out


@functools.lru_cache(maxsize=4)
def dp_case(H, F, K, cols, halo, with_cond, seed=0):
    """T = two work items plus three columns; rows: class_lengths — one short of, on and one past every seam and its halo, 0, 1, T."""
    T = 2 * cols + 3
    lens = class_lengths(T, cols, halo)
    B = len(lens)
    rng = np.random.default_rng([seed, H, F, K])
    r = lambda *s: rng.standard_normal(s)
    w = dict(w1=(r(F, H, K) / np.sqrt(H * K)).astype(np.float32), b1=(0.3 * r(F)).astype(np.float32),
             g1=(1 + 0.2 * r(F)).astype(np.float32), be1=(0.2 * r(F)).astype(np.float32),
             w2=(r(F, F, K) * np.sqrt(2.0 / (F * K))).astype(np.float32), b2=(0.3 * r(F)).astype(np.float32),
             g2=(1 + 0.2 * r(F)).astype(np.float32), be2=(0.2 * r(F)).astype(np.float32),
             proj_w=(0.35 * r(F) / np.sqrt(F)).astype(np.float32), proj_b=np.asarray([0.4], np.float32))
    c = dict(x=r(B, H, T).astype(np.float32), lens=np.asarray(lens, np.int32), cond=(0.5 * r(B, H)).astype(np.float32) if with_cond else None, w=w, T=T)
    c["ref"] = dp_det_rule(c, np.float64)
    c["f32"] = dp_det_rule(c, np.float32, DP_GROUP)
    for v in w.values():
        v.flags.writeable = False
    return _freeze(c)


def check_dp_det(lib, shape, math, with_cond, alone=True):
    """One shape in one math mode: the plan call's seam, the criterion, zeros and every t < T written; alone (the cases with cond,
    which a row carries into its solo run: masking and staging do not depend on it otherwise): JUNK in x at and past len, and every
    row against its solo run."""
    H, F, K = shape
    cols, halo, lds = lib.lab_dp_det_plan(H, F, K, math)
    assert 0 < cols <= 64 and halo == 2 * (K // 2) and 0 < lds <= 160 * 1024, (shape, cols, halo, lds)
    c = dp_case(H, F, K, cols, halo, with_cond)
    T, lens = c["T"], c["lens"]
    tag = f"H={H} F={F} K={K} cond={int(with_cond)} T={T}"
    got = lib.test_dp_det(c["x"], lens, c["w"], c["cond"], math)
    assert not np.any(got == JUNK), (tag, "every t < T is written")
    assert_vs_fp64(got, c["ref"], c["f32"], lens, MATH_NAMES[math], tag)
    for b, L in enumerate(int(n) for n in lens):
        assert np.all(got[b, L:].view(np.uint32) == 0), (tag, "row", b, "logw is exact +0 at and past len", L)
    if alone:
        xj = np.where(np.arange(T)[None, None, :] >= lens[:, None, None], JUNK, c["x"])
        gj = lib.test_dp_det(xj, lens, c["w"], c["cond"], math)
        assert np.array_equal(gj.view(np.uint32), got.view(np.uint32)), (tag, "JUNK in x at and past len moved logw")
    for b in range(len(lens)) if alone else ():
        one = lib.test_dp_det(c["x"][b:b + 1], lens[b:b + 1], c["w"], None if c["cond"] is None else c["cond"][b:b + 1], math)
        assert np.array_equal(one[0].view(np.uint32), got[b].view(np.uint32)), (tag, "row", b, "differs from its solo run")
    return lds


SMALL_KERNELS = ("k_sdp_noise", "k_expand_prior (keyed)", "k_layernorm<cached>", "k_layernorm<uncached>") + tuple(MATH_NAMES.values())


def print_ratios(where, factor=3.0):
    """This family's rows of conv_ref's table (one process may have run the conv modules before)."""
    table = {k: v for k, v in RATIOS.get(where, {}).items() if k in SMALL_KERNELS}
    for who in sorted(table):
        print(f"small kernels worst e / e32 {where}: {who}: {table[who]:.3f}")
    assert all(r <= factor for r in table.values())
