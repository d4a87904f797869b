"""The stochastic duration predictor's kernels alone (csrc/kernels_misc.cpp): the fp64 reference of each
operation, its float32 calibration, the criteria and the case tables that tests/test_sdp_kernels.py (CPU model of the kernels) and
tests/test_gpu_sdp_kernels.py (MI355X) share.

The hooks (include/mi355vits_lab.h): test_dds_stack — impl 0 = one launch per piece, 1 = launch_dds_layer per layer, 2 =
k_dds_stack<6>, 3 = k_dds_stack_b3 (MATH_BF16X3; MATH_BF16W reaches k_dds_stack_b3<true>) —, test_spline_inverse, test_durations,
test_expand_prior.

The rules, written from the operation (HF modeling_vits.py), per row on its own [:, :L] with zero padding:
  pre     x = conv1x1(src) + b (+ cond)        or   x = w[c] * z[zch] + b[c] + src
  layer   x += gelu_erf(LN2(conv1x1(gelu_erf(LN1(dwconv_{K, K^i}(x * mask))))))     LayerNorm over channels, eps 1e-5
  proj    out = conv1x1(x * mask) + b
  spline  the rational-quadratic spline inverse with linear tails: min width / height / derivative 1e-3, the end derivatives from the
          constant log(exp(1 - 1e-3) - 1), the searchsorted with 1e-6 on the last knot, the root 2c / (-b - sqrt(b^2 - 4ac))
  K6      logw = (z - m) * exp(-logs);  w = ceil(exp(logw) * length_scale);  cum = the inclusive scan;  ylen = max(1, sum)
  K7      frame t takes phoneme j = #{j : cum_j <= t}:  z = m_p[j] + noise * exp(logs_p[j]) * noise_scale
tests/test_sdp_kernels.py pins these to oracle/vits_oracle.py's modules in double.

Criterion for float outputs, the one of tests/wn_ref.py (norm_err and f32_bound come from tests/attention_ref.py, unchanged): e =
norm_err(kernel), e32 = norm_err(the float32 model), both against fp64 on the same inputs, per row over its own columns; a kernel
passes when e <= max(3 * e32, 2**-23).  The float32 model is the SAME numpy code run in float32 with every channel sum taken in
ascending channel order, one addition per channel: it follows no kernel's order and is never under test.  For MATH_BF16W both the
reference and the model take the dense weights rounded to the nearest bf16 (pack_conv_weights_bf16x3_mode's leading term).

Integer outputs (w_ceil, cum, ylen): an element is DECIDED when |w64 - round(w64)| > w64 * 2**-18 (w64 = exp(lw) * m * ls in fp64):
float32 arithmetic on |logw| <= 4 — (z - m) * es, expf and two multiplies — stays below 2**-19 relative.  Decided elements equal
ceil(w64); undecided ones lie within 1 of it; at most 0.5 % of a case's valid elements may be undecided (DURATION_CASES' seeds are
chosen from the fp64 reference alone so that every case holds that; the expected share is about 2 w 2**-18)."""
import functools
import math
import types

import numpy as np
import torch

from tests.attention_ref import f32_bound, norm_err

IMPL_NAMES = {0: "one launch per piece", 1: "launch_dds_layer", 2: "k_dds_stack<6>", 3: "k_dds_stack_b3<false>", "3w": "k_dds_stack_b3<true>"}
MATH_F32, MATH_BF16X3, MATH_BF16W = 0, 1, 2
JUNK = np.float32(-7.5e29)  # prior contents of the output buffers: large, finite, an unmistakable bit pattern
HUGE = np.float32(3.0e38)
FRAME_CAP = 1 << 22         # csrc/kernels.h DURATION_FRAME_CAP
EPS = 1e-5


# ------------------------------------------------------------------------------------------------ the operations, any dtype
def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def gelu_erf(x):
    dt = x.dtype.type
    return dt(0.5) * x * (dt(1.0) + _erf(x * dt(math.sqrt(0.5))))


def chan_sum(x):
    """sum over axis 0 in ascending order, one addition per channel, in x's dtype"""
    s = np.zeros(x.shape[1:], x.dtype)
    for c in range(x.shape[0]):
        s = s + x[c]
    return s


def layernorm(x, gamma, beta):
    """x [C, L]: over channels, eps 1e-5"""
    dt = x.dtype.type
    C = x.shape[0]
    mean = chan_sum(x) / dt(C)
    d = x - mean[None, :]
    var = chan_sum(d * d) / dt(C)
    return d * (dt(1.0) / np.sqrt(var + dt(EPS)))[None, :] * gamma.astype(dt)[:, None] + beta.astype(dt)[:, None]


def conv1x1(x, w, bias):
    """x [Cin, L], w [Cout, Cin, 1]: the channels summed in ascending order, then the bias"""
    dt = x.dtype.type
    w = w.astype(dt)
    acc = np.zeros((w.shape[0], x.shape[1]), dt)
    for c in range(x.shape[0]):
        acc = acc + w[:, c, 0][:, None] * x[c][None, :]
    return acc + bias.astype(dt)[:, None]


def dwconv(x, w, bias, dil):
    """depthwise 'same' conv of one row x [C, L] (zero padding): w [C, 1, K]"""
    dt = x.dtype.type
    C, L = x.shape
    K = w.shape[2]
    pad = (K - 1) // 2 * dil
    xp = np.zeros((C, L + 2 * pad), dt)
    xp[:, pad:pad + L] = x
    acc = np.repeat(bias.astype(dt)[:, None], L, axis=1)
    for k in range(K):
        acc = acc + w[:, 0, k].astype(dt)[:, None] * xp[:, k * dil:k * dil + L]
    return acc


def dds_layer(x, lay, dil):
    y = gelu_erf(layernorm(dwconv(x, lay["dw_w"], lay["dw_b"], dil), lay["g1"], lay["b1"]))
    y = gelu_erf(layernorm(conv1x1(y, lay["w1x1"], lay["bias1x1"]), lay["g2"], lay["b2"]))
    return x + y


def softplus(x):
    """log(1 + exp(x)), x itself above 20 (torch.nn.functional.softplus's default threshold)"""
    with np.errstate(over="ignore"):
        return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, x.dtype.type(30)))))


def spline_inverse(x1, theta, nb, tail, inv_sqrt_fc):
    """x1 [n], theta [3 nb - 1, n] -> [n], in theta's dtype.  HF modeling_vits.py:93-302, reverse."""
    dt = theta.dtype.type
    x1 = x1.astype(dt)
    tb, mn = dt(tail), dt(1e-3)
    isf = dt(np.float32(inv_sqrt_fc))
    n = x1.shape[0]

    def knots(u):
        e = np.exp(u - u.max(axis=0, keepdims=True))
        p = mn + (dt(1.0) - mn * dt(nb)) * (e / chan_sum(e)[None, :])
        c = np.zeros((nb + 1, n), dt)
        run = np.zeros(n, dt)
        for i in range(nb):
            run = run + p[i]
            c[i + 1] = run
        c = dt(2.0) * tb * c - tb
        c[0] = -tb
        c[nb] = tb
        return c

    cw, ch = knots(theta[:nb] * isf), knots(theta[nb:2 * nb] * isf)
    const = dt(math.log(math.exp(1 - 1e-3) - 1))
    ud = np.concatenate([np.full((1, n), const, dt), theta[2 * nb:], np.full((1, n), const, dt)], axis=0)
    dv = mn + softplus(ud)
    locs = ch.copy()
    locs[nb] = locs[nb] + dt(1e-6)
    inside = (x1 >= -tb) & (x1 <= tb)
    xin = np.clip(np.where(np.isfinite(x1), x1, dt(0.0)), -tb, tb)
    bin_ = np.clip((xin[None, :] >= locs).sum(axis=0) - 1, 0, nb - 1)
    g = lambda a, o=0: np.take_along_axis(a, (bin_ + o)[None, :], axis=0)[0]
    in_cw, in_w = g(cw), g(cw, 1) - g(cw)
    in_ch, in_h = g(ch), g(ch, 1) - g(ch)
    delta = in_h / in_w
    d0, d1 = g(dv), g(dv, 1)
    t1 = d0 + d1 - dt(2.0) * delta
    u = xin - in_ch
    t3 = u * t1
    a = in_h * (delta - d0) + t3
    b = in_h * d0 - t3
    c = -delta * u
    # the discriminant is >= 0 inside the bin ((in_h d1)^2 at its upper knot): the max is the identity in exact arithmetic and in the
    # fp64 run (the oracle pin holds to 1e-12 with it); in float32 the two terms cancel to either sign next to a flat knot
    root = (dt(2.0) * c) / (-b - np.sqrt(np.maximum(b * b - dt(4.0) * a * c, dt(0.0))))
    out = root * in_w + in_cw
    assert out.dtype == theta.dtype
    return np.where(inside, out, x1)


def bf16_round(w):
    """float32 -> the nearest bf16 (ties to even), as float32"""
    b = np.ascontiguousarray(w, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(w))


class Twice:
    """A library with every kernel-hook call repeated: the two results must be the same bits (a race between a kernel's phases is
    invisible to the CPU model; the device tests wrap their library in this)."""

    def __init__(self, lib):
        self.lib = lib

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("test_"):
            return fn

        def twice(*a, **k):
            r1, r2 = fn(*a, **k), fn(*a, **k)
            for u, v in zip(r1 if isinstance(r1, tuple) else (r1,), r2 if isinstance(r2, tuple) else (r2,)):
                assert (u is None and v is None) or np.array_equal(u, v, equal_nan=True), (name, "two runs of one case differ")
            return r1
        return twice


# ------------------------------------------------------------------------------------------------ the stack
def stack_ref(c, dt, bf16w=False):
    """(x_out [B, C, T], out [B, Cp, T] or None, z [B, 2, T] or None) of stack case c in dtype dt; zero at and past a row's length
    (x_out is compared below it only).  Every row alone on its own columns."""
    rw = bf16_round if bf16w else (lambda w: w)
    B, C, T = c["src"].shape
    affine = c["pre_w"].ndim == 1
    pw = c["proj_w"]
    x_out = np.zeros((B, C, T), dt)
    out = None if pw is None else np.zeros((B, pw.shape[0], T), dt)
    z = None if c["z"] is None else c["z"].astype(dt)
    for b, L in enumerate(int(n) for n in c["lens"]):
        if z is not None and c["spline"]:
            z[b, :, L:] = 0
        if L == 0:
            continue
        src = c["src"][b, :, :L].astype(dt)
        if affine:
            x = c["pre_w"].astype(dt)[:, None] * c["z"][b, c["zch"], :L].astype(dt)[None, :] + c["pre_b"].astype(dt)[:, None] + src
        else:
            x = conv1x1(src, rw(c["pre_w"]), c["pre_b"])
            if c["cond"] is not None:
                x = x + c["cond"][b].astype(dt)[:, None]
        K = c["layers"][0]["dw_w"].shape[2]
        for i, lay in enumerate(c["layers"]):
            x = dds_layer(x, dict(lay, w1x1=rw(lay["w1x1"])), K ** i)
        assert x.dtype == dt
        x_out[b, :, :L] = x
        if pw is not None:
            th = conv1x1(x, rw(pw), c["proj_b"])
            out[b, :, :L] = th
            if c["spline"]:
                z[b, 1 - c["zch"], :L] = spline_inverse(c["z"][b, 1 - c["zch"], :L], th, c["nb"], c["tail"], c["isf"])
    return x_out, out, z


TAIL = 5.0


@functools.lru_cache(maxsize=16)
def stack_case(C, T, lens, affine, with_cond, zch, n_layers, proj, K=3, seed=0):
    """The inputs of a stack case and its fp64 result, computed once and read-only.  proj: 0 = none, 29 / 47 = ConvFlow's theta for 10 / 16
    bins with the spline (affine pre), anything else = a plain proj of that many rows."""
    rng = np.random.default_rng([seed, C, T, int(affine), int(with_cond), zch, n_layers, proj, K])
    B = len(lens)
    f = lambda a: np.asarray(a, np.float32)
    spline = bool(affine and proj in (29, 47))
    c = dict(
        src=f(rng.standard_normal((B, C, T))), lens=np.asarray(lens, np.int32),
        pre_w=f(rng.standard_normal(C)) if affine else f(rng.standard_normal((C, C, 1)) / np.sqrt(C)),
        pre_b=f(0.3 * rng.standard_normal(C)),
        cond=f(0.5 * rng.standard_normal((B, C))) if with_cond and not affine else None,
        z=f(1.5 * rng.standard_normal((B, 2, T))) if affine else None, zch=zch,
        layers=[dict(dw_w=f(rng.standard_normal((C, 1, K)) / np.sqrt(K)), dw_b=f(0.3 * rng.standard_normal(C)),
                     g1=f(1 + 0.2 * rng.standard_normal(C)), b1=f(0.2 * rng.standard_normal(C)),
                     w1x1=f(rng.standard_normal((C, C, 1)) / np.sqrt(C)), bias1x1=f(0.3 * rng.standard_normal(C)),
                     g2=f(1 + 0.2 * rng.standard_normal(C)), b2=f(0.2 * rng.standard_normal(C))) for _ in range(n_layers)],
        # theta's width / height rows at scale sqrt(C): after the spline's 1 / sqrt(C) the logits spread over a few units, as a trained
        # flow's do; the derivative rows (not scaled by the spline) at scale 1
        proj_w=f(rng.standard_normal((proj, C, 1)) * np.where(np.arange(proj) < (2 * (proj + 1) // 3 if spline else 0), 1.0, 1 / np.sqrt(C))[:, None, None]) if proj else None,
        proj_b=f(0.3 * rng.standard_normal(proj)) if proj else None,
        spline=spline, nb=(proj + 1) // 3 if spline else 0, tail=TAIL, isf=np.float32(1.0 / np.sqrt(C)))
    c["key"] = (C, T, tuple(lens), affine, with_cond, zch, n_layers, proj, K, seed)
    c["ref"] = {False: stack_ref(c, np.float64)}
    c["f32"] = {}
    _freeze(c)
    return c


def _freeze(c):
    """every array of a case (its layers' and its references' too) read-only"""
    todo = list(c.values())
    while todo:
        v = todo.pop()
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
        elif isinstance(v, dict):
            todo += list(v.values())
        elif isinstance(v, (list, tuple)):
            todo += list(v)


def stack_refs(c, bf16w):
    """(fp64, float32 model) of a case; the MATH_BF16W pair takes the dense weights rounded to bf16"""
    if bf16w not in c["ref"]:
        c["ref"][bf16w] = stack_ref(c, np.float64, bf16w)
    if bf16w not in c["f32"]:
        c["f32"][bf16w] = stack_ref(c, np.float32, bf16w)
    return c["ref"][bf16w], c["f32"][bf16w]


def run_stack(lib, impl, c, math=None, src=None, z=None, out_prior=None, x_out_prior=None):
    pc = 0 if c["proj_w"] is None else c["proj_w"].shape[0]
    B, C, T = c["src"].shape
    return lib.test_dds_stack(
        c["src"] if src is None else src, c["pre_w"], c["pre_b"], c["layers"], c["lens"], impl=impl, math=math, cond=c["cond"],
        z=c["z"] if z is None else z, zch=c["zch"], proj_w=c["proj_w"], proj_b=c["proj_b"], spline=c["spline"], nb=c["nb"], tail=c["tail"],
        inv_sqrt_fc=c["isf"], out_prior=np.full((B, pc, T), JUNK) if out_prior is None and pc else out_prior,
        x_out_prior=np.full((B, C, T), JUNK) if x_out_prior is None else x_out_prior)


RATIOS = {}   # worst e / e32 per impl (and kernel) seen in this process: printed by the tests' last one, DESIGN.md quotes them


def criterion(got, ref, f32, lens, who, tag, name):
    """e <= max(3 e32, 2**-23) on one output; every valid element finite.  Collects e / e32 under `who`."""
    assert got.shape == ref.shape and got.dtype == np.float32, (tag, name, got.shape, ref.shape)
    e, e32 = norm_err(got, ref, lens), norm_err(f32, ref, lens)
    ratio = e / max(e32, 1e-30)
    RATIOS[who] = max(RATIOS.get(who, 0.0), ratio if e > 2.0 ** -23 else 0.0)
    print(f"sdp {IMPL_NAMES.get(who, who)} {tag} {name}: e = {e:.3e}  e32 = {e32:.3e}  e/e32 = {ratio:.3f}")
    assert e <= f32_bound(e32), (tag, IMPL_NAMES.get(who, who), name, e, e32, f32_bound(e32), worst_element(got, ref, lens))


def worst_element(got, ref, lens):
    best = (0.0, None)
    for b, L in enumerate(int(n) for n in lens):
        if L:
            d = np.abs(np.asarray(got[b][:, :L], np.float64) - ref[b][:, :L])
            d = np.where(np.isfinite(d), d, np.inf)
            i = np.unravel_index(int(np.argmax(d)), d.shape)
            if d[i] >= best[0]:
                best = (float(d[i]), (b, int(i[0]), int(i[1]), float(got[b][i]), float(ref[b][i])))
    return best[1]


def assert_stack(got, c, impl, tag, math=None):
    """The float criterion on x_out, out and z below every row's length, and the hook's contract at and past it: out is zero up to T, z
    (with the spline) zero in both channels, x_out written everywhere; without the spline z is returned as it came."""
    bf16w = math == MATH_BF16W
    who = "3w" if bf16w else impl
    ref, f32 = stack_refs(c, bf16w)
    lens = c["lens"]
    T = c["src"].shape[2]
    for name, g, r, m in zip(("x_out", "out", "z"), got, ref, f32):
        if r is None:
            assert g is None, (tag, name)
            continue
        if name == "z" and not c["spline"]:
            assert np.array_equal(g, c["z"]), (tag, "no path writes z without the spline")
            continue
        criterion(g, r, m, lens, who, tag, name)
        for b, L in enumerate(int(n) for n in lens):
            if name == "x_out":
                assert not np.any(g[b] == JUNK), (tag, IMPL_NAMES[impl], "x_out is written at every column", b)
            else:
                assert np.all(g[b][:, L:] == 0.0), (tag, IMPL_NAMES[impl], name, "exact zeros from len[b] to T", b, L, T)
            if name == "z":
                assert np.array_equal(g[b, c["zch"], :L], c["z"][b, c["zch"], :L]), (tag, "z[zch] keeps its contents below len[b]", b)


def check_stack(lib, impl, c, tag, math=None):
    got = run_stack(lib, impl, c, math=math)
    assert_stack(got, c, impl, tag, math)
    return got


def assert_same_bits_below_len(a, b, lens, tag):
    for name, u, v in zip(("x_out", "out", "z"), a, b):
        if u is None:
            continue
        for r, L in enumerate(int(n) for n in lens):
            assert np.array_equal(u[r][:, :L], v[r][:, :L]), (tag, name, "row", r, L)


# ------------------------------------------------------------------------------------------------ the stack's case tables
LENGTH_CLASSES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 97]  # around the 32-column tiles, their 16-column halo, odd T
IMPL0_LENGTH_CLASSES = [1, 17, 33, 64, 97]
STACK_IMPLS = [1, 2, 3]
MAX_ROWS = 6


def row_lengths(T):
    """0, 1, T and around every 32-column seam s <= T + 16: s - 16, s - 13 (the taps' reach), s - 1, s, s + 1, s + 13, s + 16"""
    s = {0, 1, T}
    for m in range(32, T + 17, 32):
        s |= {m - 16, m - 13, m - 1, m, m + 1, m + 13, m + 16}
    return sorted(n for n in s if 0 <= n <= T)


def row_batches(T):
    """row_lengths(T) in ragged batches of up to MAX_ROWS rows, long and short rows mixed in each"""
    r = row_lengths(T)
    nb = -(-len(r) // MAX_ROWS)
    return [tuple(r[i::nb]) for i in range(nb)]


# (affine pre, cond given, zch, n_layers, proj rows): dp.proj behind the conv pre + cond; ConvFlow's theta for 10 and 16 bins with the
# spline behind the affine pre on either channel; one output row; no proj (x_out only); every depth
OPTION_CASES = [(False, True, 0, 3, 192), (True, False, 0, 3, 29), (True, False, 1, 3, 47), (False, False, 0, 2, 1), (True, False, 1, 1, 0),
                (True, False, 1, 2, 29), (False, True, 0, 1, 47), (True, False, 0, 2, 192), (False, False, 0, 3, 0)]


def length_class_cases(T, C=192):
    """One case per ragged batch of row_lengths(T); the options rotate with T and the batch."""
    n0 = LENGTH_CLASSES.index(T) if T in LENGTH_CLASSES else T
    return [stack_case(C, T, lens, *OPTION_CASES[(n0 + i) % len(OPTION_CASES)]) for i, lens in enumerate(row_batches(T))]


OPTIONS_T = 49
OPTIONS_LENS = (49, 48, 33, 19, 1, 0)


def option_cases(C=192):
    return [stack_case(C, OPTIONS_T, OPTIONS_LENS, *o) for o in OPTION_CASES]


def independence_cases():
    """a ConvFlow stack with the spline, and the dp stack: rows ending on, inside the halo of and past the seams"""
    lens = (65, 64, 51, 33, 16, 1)
    return [stack_case(192, 65, lens, True, False, 1, 3, 29), stack_case(192, 65, lens, False, True, 0, 3, 192)]


def single_row(c, b):
    """row b of case c alone, as a case of its own (reference not needed)"""
    d = dict(c, src=c["src"][b:b + 1], lens=c["lens"][b:b + 1], cond=None if c["cond"] is None else c["cond"][b:b + 1],
             z=None if c["z"] is None else c["z"][b:b + 1])
    return d


def widened(c, extra, fill):
    """case c with T enlarged by `extra` columns of `fill` in src and z"""
    B, C, T = c["src"].shape
    src = np.full((B, C, T + extra), fill, np.float32)
    src[:, :, :T] = c["src"]
    z = None
    if c["z"] is not None:
        z = np.full((B, 2, T + extra), fill, np.float32)
        z[:, :, :T] = c["z"]
    return dict(c, src=src, z=z)


def poisoned(c, pattern):
    """case c with `pattern` (cycled) in src and z at and past every row's length"""
    B, C, T = c["src"].shape
    past = np.arange(T)[None, None, :] >= c["lens"][:, None, None]
    pat = np.resize(np.asarray(pattern, np.float32), T)[None, None, :]
    src = np.where(past, pat, c["src"]).astype(np.float32)
    z = None if c["z"] is None else np.where(past, pat, c["z"]).astype(np.float32)
    return dict(c, src=src, z=z)


POISON = [np.float32(np.nan), HUGE, -HUGE, np.float32(np.inf), JUNK]


# ------------------------------------------------------------------------------------------------ the spline alone
def _ulp(x, n):
    """x moved by n float32 ulps"""
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return x


@functools.lru_cache(maxsize=8)
def spline_case(nb, kind, ch_x0, seed=0):
    """theta [B, 3 nb - 1, T], z [B, 2, T], ragged len; x1 = z[:, 1 - ch_x0] sits on the tails, one ulp inside and outside each, on every
    knot of the cumulative heights (computed in fp64) and one float32 ulp either side, at 0, and on random values up to 1.3 tail.
    kind: "s1" / "s8" = random theta at scale 1 / 8 sqrt(C); "h40" / "w40" = one height / width logit at +40 (after the scale), so every
    other bin sits at its 1e-3 floor; "d30" = the interior derivative parameters at -30 and +30 alternately."""
    rng = np.random.default_rng([seed, nb, ch_x0, sum(map(ord, kind))])
    B, isf = 4, np.float32(1.0 / np.sqrt(192.0))
    nth = 3 * nb - 1
    scale = 8.0 if kind == "s8" else 1.0
    T = 6 + 3 * (nb + 1) + 1 + 12
    lens = np.asarray([T, T - 5, 7, 0], np.int32)
    theta = (rng.standard_normal((B, nth, T)) * scale / isf).astype(np.float32)
    theta[:, 2 * nb:] = rng.standard_normal((B, nb - 1, T)) * 2
    if kind in ("h40", "w40"):
        o = nb if kind == "h40" else 0
        hot = rng.integers(0, nb, size=(B, T))
        for b in range(B):
            theta[b, o + hot[b], np.arange(T)] = np.float32(40.0 / isf)
    if kind == "d30":
        theta[:, 2 * nb::2] = -30.0
        theta[:, 2 * nb + 1::2] = 30.0
    # the knots of the heights per column, in fp64, from the reference's own pieces
    x1 = np.zeros((B, T), np.float32)
    for b in range(B):
        u = theta[b, nb:2 * nb].astype(np.float64) * np.float64(isf)
        e = np.exp(u - u.max(axis=0, keepdims=True))
        p = 1e-3 + (1 - 1e-3 * nb) * e / e.sum(axis=0, keepdims=True)
        kn = 2 * TAIL * np.concatenate([np.zeros((1, T)), np.cumsum(p, axis=0)]) - TAIL
        kn[0], kn[nb] = -TAIL, TAIL
        vals = [_ulp(-TAIL, d) for d in (0, 1, -1)] + [_ulp(TAIL, d) for d in (0, 1, -1)]
        col = 0
        for v in vals:
            x1[b, col] = v
            col += 1
        for i in range(nb + 1):
            for d in (0, 1, -1):
                x1[b, col] = _ulp(np.float32(kn[i, col]), d)
                col += 1
        x1[b, col] = 0.0
        col += 1
        x1[b, col:] = rng.uniform(-1.3 * TAIL, 1.3 * TAIL, T - col)
    z = np.zeros((B, 2, T), np.float32)
    z[:, 1 - ch_x0] = x1
    z[:, ch_x0] = rng.standard_normal((B, T))
    c = dict(theta=theta, z=z, lens=lens, nb=nb, ch_x0=ch_x0, isf=isf, kind=kind)
    c["ref"] = spline_ref(c, np.float64)
    c["f32"] = spline_ref(c, np.float32)
    _freeze(c)
    return c


def spline_ref(c, dt):
    z = c["z"].astype(dt)
    for b, L in enumerate(int(n) for n in c["lens"]):
        z[b, :, L:] = 0
        if L:
            z[b, 1 - c["ch_x0"], :L] = spline_inverse(c["z"][b, 1 - c["ch_x0"], :L], c["theta"][b, :, :L].astype(dt), c["nb"], TAIL, c["isf"])
    return z


SPLINE_KINDS = ["s1", "s8", "h40", "w40", "d30"]
SPLINE_CASES = [(nb, kind, (i + j) % 2) for i, nb in enumerate((10, 16)) for j, kind in enumerate(SPLINE_KINDS)]


def check_spline(lib, nb, kind, ch_x0):
    c = spline_case(nb, kind, ch_x0)
    lens = c["lens"]
    past = np.arange(c["z"].shape[2])[None, None, :] >= lens[:, None, None]
    outs = []
    for fill in (None, np.float32(np.nan), HUGE):  # what lies at and past len[b] in theta and z changes nothing
        th = c["theta"] if fill is None else np.where(past, fill, c["theta"]).astype(np.float32)
        z = c["z"] if fill is None else np.where(past, fill, c["z"]).astype(np.float32)
        got = lib.test_spline_inverse(th, z, lens, nb, ch_x0=ch_x0, tail=TAIL, inv_sqrt_fc=c["isf"])
        outs.append(got)
        for b, L in enumerate(int(n) for n in lens):
            assert np.all(got[b][:, L:] == 0.0), ("columns at and past len[b] read zero in both channels", kind, b)
            assert np.array_equal(got[b, ch_x0, :L], c["z"][b, ch_x0, :L]), ("z[ch_x0] keeps its contents", kind, b)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), (kind, "the padding reached a valid column")
    criterion(outs[0], c["ref"], c["f32"], lens, "spline", f"nb={nb} {kind} ch_x0={ch_x0}", "z")
    return outs[0]


# ------------------------------------------------------------------------------------------------ durations
EA_M, EA_LOGS = np.float32(0.25), np.float32(-0.2)  # |logw| <= 3.25 * exp(0.2) = 3.97
# (T, rows' lengths, rows' length scales, seed): T around the kernel's 256-thread stride; the seeds were picked on the CPU from
# durations_ref alone (the first for which the case's undecided share is under the cap: tests/test_sdp_kernels.py asserts it)
DURATION_CASES = [(1, (1, 0), (1.0, 1.0), 0), (255, (255, 254, 1), (1.0, 1.3, 0.7), 0), (256, (256, 255, 100), (1.0, 0.55, 2.0), 0),
                  (257, (257, 256, 0), (1.0, 1.15, 1.0), 0), (600, (600, 599, 300, 257), (1.0, 0.8, 1.25, 3.0), 0)]
UNDECIDED_CAP = 0.005


def durations_ref(z, ch, lens, ls, ea_m=EA_M, ea_logs=EA_LOGS, dt=np.float64):
    """(logw [B, 1, T], w [B, T]) in dtype dt: zero at and past a row's length"""
    B, _, T = z.shape
    m = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    lw = (z[:, ch].astype(dt) - dt(ea_m)) * np.exp(-dt(ea_logs)) * m
    w = np.exp(lw) * m * np.asarray(ls, np.float32).astype(dt)[:, None]
    assert lw.dtype == dt
    return lw[:, None, :], w


@functools.lru_cache(maxsize=8)
def durations_case(T, lens, ls, seed):
    rng = np.random.default_rng([seed, T, len(lens)])
    z = rng.uniform(-3, 3, (len(lens), 2, T)).astype(np.float32)
    z[:, :, :] *= (np.arange(T)[None, None, :] < np.asarray(lens)[:, None, None])  # the engine's z is zero past a row (the spline)
    ch = T % 2
    lw, w = durations_ref(z, ch, lens, ls)
    valid = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    decided = (np.abs(w - np.round(w)) > w * 2.0 ** -18) | ~valid
    c = dict(z=z, ch=ch, lens=np.asarray(lens, np.int32), ls=np.asarray(ls, np.float32), lw=lw, w=w, decided=decided,
             share=float((~decided).sum() / max(1, valid.sum())), lw32=durations_ref(z, ch, lens, ls, dt=np.float32)[0])
    _freeze(c)
    return c


def scan(w_ceil):
    """the inclusive scan, saturating at 2 cap, and ylen = max(1, sum)"""
    cum = np.minimum(np.cumsum(w_ceil.astype(np.int64), axis=1), 2 * FRAME_CAP).astype(np.int32)
    return cum, np.maximum(cum[:, -1], 1)


def check_durations(lib, T, lens, ls, seed):
    c = durations_case(T, lens, ls, seed)
    print(f"sdp durations T={T} rows={lens}: undecided share {c['share']:.5f} (cap {UNDECIDED_CAP})")
    assert c["share"] <= UNDECIDED_CAP, ("too many undecided elements in this case: pick another seed", c["share"])
    logw, w_ceil, cum, ylen = lib.test_durations(c["z"], c["lens"], EA_M, EA_LOGS, ch=c["ch"], length_scale=c["ls"])
    criterion(logw[:, None, :], c["lw"], c["lw32"], c["lens"], "durations", f"T={T}", "logw")
    want = np.ceil(c["w"]).astype(np.int64)
    d = c["decided"]
    assert np.array_equal(w_ceil[d], want[d]), ("a decided duration moved", np.argwhere(d & (w_ceil != want))[:4])
    assert np.all(np.abs(w_ceil[~d] - want[~d]) <= 1)
    for b, L in enumerate(int(n) for n in c["lens"]):
        assert np.all(logw[b, L:] == 0.0) and np.all(w_ceil[b, L:] == 0), ("zero at and past len[b]", b)
    own_cum, own_ylen = scan(w_ceil)
    assert np.array_equal(cum, own_cum) and np.array_equal(ylen, own_ylen), "cum / ylen are not the scan of the kernel's own w_ceil"
    full = d.all(axis=1)
    ref_cum, ref_ylen = scan(want)
    assert np.array_equal(cum[full], ref_cum[full]) and np.array_equal(ylen[full], ref_ylen[full])
    return w_ceil


def forced_duration_cases(lib):
    """Exact expectations: z = ea_m at length_scale 1 gives one frame each; length_scale 0 gives none and ylen 1; +inf, NaN and
    w >= 2**22 give cap + 1; forced counts of -1 and cap + 1 give cap + 1; 600 phonemes forced at the cap saturate cum at 2 cap; len 0."""
    cap = FRAME_CAP
    z = np.zeros((3, 2, 5), np.float32)
    z[:, 1] = EA_M
    lens = [5, 3, 0]
    logw, w, cum, ylen = lib.test_durations(z, lens, EA_M, EA_LOGS, ch=1, length_scale=1.0)
    assert np.all(logw == 0.0)
    assert w.tolist() == [[1] * 5, [1, 1, 1, 0, 0], [0] * 5] and cum.tolist() == [[1, 2, 3, 4, 5], [1, 2, 3, 3, 3], [0] * 5] and ylen.tolist() == [5, 3, 1]
    z[:, 1] = np.float32([[1.0, -2.0, 3.0, 0.5, 0.0]])
    logw, w, cum, ylen = lib.test_durations(z, [5, 5, 5], EA_M, EA_LOGS, ch=1, length_scale=0.0)
    assert np.all(w == 0) and np.all(cum == 0) and ylen.tolist() == [1, 1, 1]
    # +inf, NaN and w >= 2**22: one over the cap; just below the cap: the cap itself
    z = np.zeros((1, 2, 6), np.float32)
    z[0, 0] = [np.inf, np.nan, 200.0, np.log(np.float32(cap)) + np.float32(0.001), np.log(np.float32(cap)) * np.float32(0.9999), -np.inf]
    logw, w, cum, ylen = lib.test_durations(z, [6], 0.0, 0.0, ch=0, length_scale=1.0)
    w64 = np.exp(np.float64(z[0, 0, 4]))
    assert w[0, :4].tolist() == [cap + 1] * 4 and w[0, 5] == 0 and abs(int(w[0, 4]) - int(np.ceil(w64))) <= 1 + int(w64 * 2.0 ** -18)
    assert cum[0].tolist() == np.minimum(np.cumsum(w[0].astype(np.int64)), 2 * cap).tolist() and ylen[0] == 2 * cap
    forced = np.asarray([[3, -1, cap + 1, cap, 0, 7]], np.int32)
    logw, w, cum, ylen = lib.test_durations(z, [5], 0.0, 0.0, ch=0, length_scale=1.0, forced=forced)
    assert w[0].tolist() == [3, cap + 1, cap + 1, cap, 0, 0]
    # 600 phonemes forced at the cap: cum saturates at 2 cap, no overflow
    z = np.zeros((2, 2, 600), np.float32)
    forced = np.full((2, 600), cap, np.int32)
    logw, w, cum, ylen = lib.test_durations(z, [600, 1], 0.0, 0.0, ch=0, length_scale=1.0, forced=forced)
    assert cum[0, 0] == cap and np.all(cum[0, 1:] == 2 * cap) and ylen.tolist() == [2 * cap, cap] and np.all(w[1, 1:] == 0) and np.all(cum[1] == cap)


# ------------------------------------------------------------------------------------------------ the length regulator
def expand_prior_ref(stats, cum, ylen, Ty, ns, inj, dt):
    B, I2, Tx = stats.shape
    I = I2 // 2
    z = np.zeros((B, I, Ty), dt)
    for b in range(B):
        n = min(int(ylen[b]), Ty)
        j = np.searchsorted(cum[b], np.arange(n), side="right")
        ok = j < Tx
        jj = np.minimum(j, Tx - 1)
        v = stats[b, :I][:, jj].astype(dt)
        if ns[b] != 0:
            v = v + inj[b, :, :n].astype(dt) * np.exp(stats[b, I:][:, jj].astype(dt)) * dt(ns[b])
        z[b, :, :n] = np.where(ok[None, :], v, 0)
    return z


# (I, Ty, injected frames): Ty around the kernel's 64-frame blocks; frames > Ty = the row stride of the injected noise
EXPAND_CASES = [(5, 1, 1), (5, 63, 63), (192, 64, 70), (5, 65, 65), (192, 65, 97)]


@functools.lru_cache(maxsize=8)
def expand_case(I, Ty, frames, seed=0):
    """Rows: zero-duration phonemes at the start, in the middle and at the end (repeated cum entries); noise_scale 0; a row that sums to
    0 with ylen 1; a row shorter than Ty; a row whose cum ends below its ylen (frames with no phoneme: zeros)."""
    rng = np.random.default_rng([seed, I, Ty, frames])
    Tx = 9
    durs = np.asarray([[0, 0, 3, 0, 0, 2, 1, 0, 0], [2, 0, 0, 0, 1, 1, 1, 1, 0], [1, 2, 0, 3, 0, 1, 0, 0, 0], [0] * 9, [1, 0, 1, 0, 1, 0, 1, 0, 0],
                       [0, 1, 0, 0, 0, 0, 0, 0, 0]], np.int64)
    B = durs.shape[0]
    scale = np.asarray([max(1, Ty // 7), max(1, Ty // 6), max(1, Ty // 9), 1, max(1, Ty // 10), 1])
    cum = np.cumsum(durs * scale[:, None], axis=1)
    cum = np.minimum(cum, Ty).astype(np.int32)
    ylen = np.maximum(cum[:, -1], 1).astype(np.int32)
    ylen[5] = min(Ty, 3)  # past the row's last phoneme
    ns = np.asarray([0.667, 0.0, 1.0, 0.8, 0.333, 0.5], np.float32)
    c = dict(stats=rng.standard_normal((B, 2 * I, Tx)).astype(np.float32), cum=cum, ylen=ylen, ns=ns, Ty=Ty,
             inj=rng.standard_normal((B, I, frames)).astype(np.float32))
    c["ref"] = expand_prior_ref(c["stats"], cum, ylen, Ty, ns, c["inj"], np.float64)
    c["f32"] = expand_prior_ref(c["stats"], cum, ylen, Ty, ns, c["inj"], np.float32)
    _freeze(c)
    return c


def check_expand(lib, I, Ty, frames):
    c = expand_case(I, Ty, frames)
    inj = c["inj"].copy()
    inj[1] = np.nan  # a row at noise_scale 0 never reads its noise
    for b in range(inj.shape[0]):
        inj[b, :, int(c["ylen"][b]):] = np.nan  # nor does a frame at or past ylen[b]
    z = lib.test_expand_prior(c["stats"], c["cum"], c["ylen"], Ty, noise_scale=c["ns"], injected=inj)
    live = np.where(np.abs(c["ref"]).max(axis=(1, 2)) > 0, c["ylen"], 0)  # (a row of zeros has no scale to normalise by: checked below)
    criterion(z, c["ref"], c["f32"], live, "expand_prior", f"I={I} Ty={Ty} frames={frames}", "z")
    for b, n in enumerate(int(v) for v in c["ylen"]):
        assert np.all(z[b][:, n:] == 0.0), ("frames at and past ylen[b] are zero", b, n)
    assert np.array_equal(z[1], c["f32"][1]), "noise_scale 0: the gathered means, bit for bit"
    assert np.all(z[3] == 0.0) and c["ylen"][3] == 1, "a row that sums to 0: ylen 1, all zeros"
    z0 = lib.test_expand_prior(c["stats"], c["cum"], c["ylen"], Ty, noise_scale=0.0, injected=None)
    assert np.array_equal(z0, expand_prior_ref(c["stats"], c["cum"], c["ylen"], Ty, np.zeros_like(c["ns"]), None, np.float32))
    return z


# ------------------------------------------------------------------------------------------------ the oracle's modules in double
def oracle_for(c):
    """oracle/vits_oracle.py's VitsOracle in double over the weights of stack case c, named as a ConvFlow (dp.flows.3) and as the
    predictor's own stack (dp.convs)"""
    w = {}
    for p in ("dp.flows.3.convs", "dp.convs"):
        for i, lay in enumerate(c["layers"]):
            w[f"{p}.convs_sep.{i}.weight"], w[f"{p}.convs_sep.{i}.bias"] = lay["dw_w"], lay["dw_b"]
            w[f"{p}.convs_1x1.{i}.weight"], w[f"{p}.convs_1x1.{i}.bias"] = lay["w1x1"], lay["bias1x1"]
            w[f"{p}.norms_1.{i}.gamma"], w[f"{p}.norms_1.{i}.beta"] = lay["g1"], lay["b1"]
            w[f"{p}.norms_2.{i}.gamma"], w[f"{p}.norms_2.{i}.beta"] = lay["g2"], lay["b2"]
    if c["pre_w"].ndim == 1:
        w["dp.flows.3.pre.weight"], w["dp.flows.3.pre.bias"] = c["pre_w"].reshape(-1, 1, 1), c["pre_b"]
        if c["proj_w"] is not None:
            w["dp.flows.3.proj.weight"], w["dp.flows.3.proj.bias"] = c["proj_w"], c["proj_b"]
    else:
        w["dp.pre.weight"], w["dp.pre.bias"] = c["pre_w"], c["pre_b"]
        if c["proj_w"] is not None:
            w["dp.proj.weight"], w["dp.proj.bias"] = c["proj_w"], c["proj_b"]
    return oracle(c["nb"], c["src"].shape[1], c["layers"][0]["dw_w"].shape[2], len(c["layers"]), w)


def oracle(nb, C, K, n_layers, weights):
    from oracle.vits_oracle import VitsOracle
    cfg = types.SimpleNamespace(validate=lambda: None, dp_kernel_size=K, dp_dds_layers=n_layers, dp_tail_bound=TAIL, dp_num_bins=nb, hidden_channels=C)
    return VitsOracle(cfg, weights, dtype=torch.float64)


def oracle_stack(c):
    """(x_out * mask, out, z) of stack case c by the oracle's modules, every row alone at its own length (rows with L = 0 stay zero)"""
    o = oracle_for(c)
    ref = c["ref"][False]
    outs = [np.zeros_like(r) if r is not None else None for r in ref]
    if outs[2] is not None:
        outs[2][:] = ref[2]  # (what no module computes: rows of length 0, and z without the spline)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)
    for b, L in enumerate(int(n) for n in c["lens"]):
        if L == 0:
            continue
        mask = torch.ones(1, 1, L, dtype=torch.float64)
        src = t(c["src"][b:b + 1, :, :L])
        if c["pre_w"].ndim == 1:
            z = t(c["z"][b:b + 1, :, :L])
            if c["zch"] == 1:
                z = torch.flip(z, [1])
            x0 = z[:, :1]
            x = o._dds("dp.flows.3.convs", o._conv("dp.flows.3.pre", x0), mask, g=src)
            outs[0][b, :, :L] = x[0].numpy()
            if c["proj_w"] is not None:
                outs[1][b, :, :L] = (o._conv("dp.flows.3.proj", x) * mask)[0].numpy()
            if c["spline"]:
                z2 = o._convflow_reverse(3, z, mask, src)
                if c["zch"] == 1:
                    z2 = torch.flip(z2, [1])
                outs[2][b, :, :L] = z2[0].numpy()
        else:
            h = o._conv("dp.pre", src)
            if c["cond"] is not None:
                h = h + t(c["cond"][b])[None, :, None]
            x = o._dds("dp.convs", h, mask)
            outs[0][b, :, :L] = x[0].numpy()
            if c["proj_w"] is not None:
                outs[1][b, :, :L] = (o._conv("dp.proj", x) * mask)[0].numpy()
    return outs
