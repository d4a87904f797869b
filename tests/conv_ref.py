"""The convolution family (csrc/kernels_conv.cpp, csrc/kernels_rbc.cpp) and the decoder's tail: the fp64 references, their float32
calibrations, the per-element criterion and the case tables that tests/test_conv_kernels.py (CPU model of the kernels) and
tests/test_gpu_conv_kernels.py (MI355X) share.

The rule of a Conv1d hook call (``test_conv1d``), per row on its own columns, straight from epi_std's order:
    v = conv(lrelu_slope(x * [t < in_len]));  v += bias;  v += cond;  relu;  (mask_before_res: v = 0 at t >= out_len);
    v = res + v  (res_sub: res - v);  v *= out_scale;  (else: v = 0 at t >= out_len);  accumulating: v += y.
Transposed convs come from the definition (y[co, i s - p + k] += x[ci, i] w[ci, co, k]), never through convt_to_polyphase, which is
under test.  enc_o_ln: LN_c(res + conv1x1(x * mask_in) + bias) * mask_ln.  conv_post: tanh(conv(lrelu_0.01(x * mask))), no bias.
MATH_BF16W: reference and calibration take the weights rounded to the nearest bf16 (the packed weights' leading term), as
tests/sdp_ref.py does.

Criterion (assert_vs_fp64): the one of tests/attention_ref.py and tests/wn_ref.py (norm_err, f32_bound and TIGHT_REL_RMS_TOL are
imported, not restated): e = norm_err(kernel) and e32 = norm_err(calibration), both against the fp64 rule on the same inputs, per
row over its own columns; the kernel passes when e <= max(3 * e32, 2**-23), every valid element is finite, and its rel. RMS per
row stays below the engine-level tests' 5e-6.  The calibration is the rule in numpy float32 with the products summed tap by tap,
GROUP input channels per float32 addition: 2 for the MFMA paths (v_mfma_f32_32x32x2_f32 takes two channels per rounding of an
accumulator; the split-bf16 instruction takes 16 channels in six instructions: 2.7), 1 for the fmaf chains of the generic kernels
and of conv_post.  It is never under test."""
import functools

import numpy as np

from tests.attention_ref import f32_bound, norm_err
from tests.sdp_ref import bf16_round
from tests.util import TIGHT_REL_RMS_TOL, rel_rms
from tests.wn_ref import JUNK, Env, Twice, worst_element  # noqa: F401  (re-exported to the two test modules)
from mimic3_amd._native import (CONVK_B3_PC, CONVK_B3_STAGED32, CONVK_B3_STAGED64, CONVK_CONVT_GENERIC, CONVK_ENC_B3, CONVK_ENC_B3W6,  # noqa: F401
                                CONVK_ENC_B3W8, CONVK_F32_DIRECT, CONVK_F32_SPLITK, CONVK_F32_STAGED, CONVK_GENERIC, CONVK_RB_CONV,
                                CONVK_RB_CONV_PW, CONVK_UPS64, CONVK_UPS_PL, MATH_BF16W, MATH_BF16X3, MATH_F32, NativeError)

IMPL_NAMES = {0: "k_conv1d_generic", 1: "launch_conv1d_mfma f32", 2: "k_conv1d_b3", 3: "launch_enc_conv_b3", 4: "launch_rb_conv"}
CONVT_NAMES = {0: "k_conv_transpose1d", 1: "polyphase f32 MFMA", 2: "polyphase split-bf16", 3: "launch_ups_pl"}
GROUP = {0: 1, 1: 2, 2: 2, 3: 2, 4: 2}        # Conv1d impl -> input channels per float32 addition of the calibration
CONVT_GROUP = {0: 1, 1: 2, 2: 2, 3: 2}
OLD_MAX_ABS_TOL = 5e-5  # the threshold of the conv tests in tests/test_gpu_parity.py / tests/test_emu_engine.py (the bite test quotes it)


# ---------------------------------------------------------------------------------------------------- the rules
def _lrelu(x, slope, dt):
    return x if slope == 1.0 else np.where(x >= 0, x, x * dt(slope))


def _conv_row(x, w, dil, dt, group):
    """'same' Conv1d of one row x [Cin, T] (zero outside) without a bias, in dtype dt: the products summed tap by tap, `group` input
    channels per addition (0: a whole tap's).  y[co, t] = sum w[co, ci, k] x[ci, t - pad + k dil], pad = (K - 1) dil // 2."""
    Cout, Cin, K = w.shape
    T = x.shape[1]
    pad = (K * dil - dil) // 2
    xp = np.zeros((Cin, T + (K - 1) * dil), dt)
    xp[:, pad:pad + T] = x
    acc = np.zeros((Cout, T), dt)
    g = group or Cin
    for k in range(K):
        for c0 in range(0, Cin, g):
            acc = acc + w[:, c0:c0 + g, k].astype(dt) @ xp[c0:c0 + g, k * dil:k * dil + T]
    assert acc.dtype == dt
    return acc


def conv1d_rule(c, dt, group=0, bf16w=False):
    """The rule of the module's docstring for a case dict, every row alone, in dtype dt.  Returns [B, Cout, T]: every column t < T of
    every row, as impl 0 - 3 write them (zeros under out_len as the epilogue gives them)."""
    x, w = c["x"], (bf16_round(c["w"]) if bf16w else c["w"])
    B, Cin, T = x.shape
    Cout = w.shape[0]
    y = np.zeros((B, Cout, T), dt)
    t = np.arange(T)
    for b in range(B):
        Li = T if c["in_len"] is None else int(c["in_len"][b])
        Lo = T if c["out_len"] is None else int(c["out_len"][b])
        xr = np.zeros((Cin, T), dt)
        xr[:, :Li] = _lrelu(x[b, :, :Li].astype(dt), c["in_slope"], dt)
        v = _conv_row(xr, w, c["dil"], dt, group)
        if c["bias"] is not None:
            v = v + c["bias"].astype(dt)[:, None]
        if c["cond"] is not None:
            v = v + c["cond"][b].astype(dt)[:, None]
        if c["relu"]:
            v = np.maximum(v, dt(0))
        live = (t < Lo)[None, :]
        if c["mask_before_res"]:
            v = np.where(live, v, dt(0))
        if c["res"] is not None:
            r = c["res"][b].astype(dt)
            v = r - v if c["res_sub"] else r + v
        v = v * dt(c["out_scale"])
        if not c["mask_before_res"]:
            v = np.where(live, v, dt(0))
        if c["y0"] is not None:
            v = v + c["y0"][b].astype(dt)
        assert v.dtype == dt
        y[b] = v
    return y


def convt_rule(x, w, bias, stride, in_slope, lens, dt, group=0):
    """ConvTranspose1d (padding (K - stride) / 2) of lrelu(x[b, :, :len_b]) from the definition, in dtype dt: y [B, Cout, Tin * stride];
    a row's positions at or past len_b * stride hold what the zero-extended row gives."""
    B, Cin, Tin = x.shape
    Cout, K = w.shape[1], w.shape[2]
    p = (K - stride) // 2
    Tout = Tin * stride
    y = np.zeros((B, Cout, Tout), dt)
    g = group or Cin
    for b in range(B):
        L = Tin if lens is None else int(lens[b])
        xr = np.zeros((Cin, Tin), dt)
        xr[:, :L] = _lrelu(x[b, :, :L].astype(dt), in_slope, dt)
        acc = np.zeros((Cout, Tout + 2 * K), dt)  # position n sits at n + K
        # an output takes its taps from the later input first (k = r, then r + s of the input before it), as the polyphase filter does
        for k in range(K):
            for c0 in range(0, Cin, g):
                contrib = w[c0:c0 + g, :, k].astype(dt).T @ xr[c0:c0 + g]  # [Cout, Tin], lands at n = i * stride - p + k
                sl = slice(K - p + k, K - p + k + Tin * stride, stride)
                acc[:, sl] = acc[:, sl] + contrib
        v = acc[:, K:K + Tout]
        if bias is not None:
            v = v + bias.astype(dt)[:, None]
        assert v.dtype == dt
        y[b] = v
    return y


def enc_o_ln_rule(c, dt, group=0, bf16w=False):
    x, w = c["x"], (bf16_round(c["w"]) if bf16w else c["w"])
    B, C, T = x.shape
    y = np.zeros((B, C, T), dt)
    for b in range(B):
        Li = T if c["in_len"] is None else int(c["in_len"][b])
        Lo = T if c["out_len"] is None else int(c["out_len"][b])
        xr = np.zeros((C, T), dt)
        xr[:, :Li] = x[b, :, :Li]
        v = c["res"][b].astype(dt) + (_conv_row(xr, w, 1, dt, group) + c["bias"].astype(dt)[:, None])
        mean = v.sum(axis=0, dtype=dt) / dt(C)
        d = v - mean
        var = (d * d).sum(axis=0, dtype=dt) / dt(C)
        o = d * (dt(1) / np.sqrt(var + dt(c["eps"]))) * c["gamma"].astype(dt)[:, None] + c["beta"].astype(dt)[:, None]
        o[:, Lo:] = 0
        assert o.dtype == dt
        y[b] = o
    return y


def conv_post_rule(x, w, valid_len, dt):
    """tanh(conv(lrelu_0.01(x * mask))), Cout = 1, no bias: [B, L]; the calibration (float32) sums channel by channel, tap by tap."""
    B, Cin, L = x.shape
    y = np.zeros((B, L), dt)
    for b in range(B):
        vl = int(valid_len[b])
        xr = np.zeros((Cin, L), dt)
        xr[:, :vl] = _lrelu(x[b, :, :vl].astype(dt), 0.01, dt)
        y[b] = np.tanh(_conv_row(xr, w, 1, dt, 1)[0])
    return y


def pcm16_rule(audio, peaks, valid_len, volumes=None):
    """audio_float_to_int16 (scale 32767 / max(0.01, peak), clip, truncate) and audioop.mul (double product, clip, floor) in numpy on the
    kernel's own float32 audio and peaks: exact integers."""
    B, L = audio.shape
    out = np.zeros((B, L), np.int16)
    for b in range(B):
        vl = int(valid_len[b])
        scale = np.float32(32767.0) / np.maximum(np.float32(0.01), np.float32(peaks[b]))
        v = np.clip(audio[b, :vl].astype(np.float32) * scale, np.float32(-32767.0), np.float32(32767.0))
        q = np.trunc(v).astype(np.int32)
        if volumes is not None and volumes[b] != 1.0:
            d = np.clip(q.astype(np.float64) * float(volumes[b]), -32768.0, 32767.0)
            q = np.floor(d).astype(np.int32)
        out[b, :vl] = q.astype(np.int16)
    return out


# ---------------------------------------------------------------------------------------------------- the criterion
RATIOS = {}  # library ("CPU model", "MI355X") -> kernel family -> worst e / e32 seen in this process (printed by the closing tests; DESIGN.md quotes them)
_ratios_of = ["?"]


def ratios_into(where):
    """Names the library whose calls the criterion sees from here on (each test module's `lib` fixture): one process runs the CPU
    model's module before the device's, and each closing test prints its own library's figures."""
    _ratios_of[0] = where


def assert_vs_fp64(got, ref, f32, lens, who, tag):
    """The criterion of the module's docstring on rows that are already computed: got / ref / f32 [B, C, T] (or [B, T]), lens [B] = the
    columns of each row that count.  Prints e, e32 and their ratio; returns e / e32."""
    got, ref, f32 = (a[:, None, :] if a.ndim == 2 else a for a in (got, ref, f32))
    assert got.shape == ref.shape == f32.shape and got.dtype == np.float32, (who, tag, got.shape, ref.shape, got.dtype)
    for b, L in enumerate(lens):
        assert np.isfinite(got[b][:, :int(L)]).all(), (who, tag, b, "a valid element is not finite")
    e, e32 = norm_err(got, ref, lens), norm_err(f32, ref, lens)
    assert np.isfinite(e32), (who, tag, "the calibration is not finite: a row's reference is all zero")
    rms = max([rel_rms(got[b][:, :int(L)], ref[b][:, :int(L)]) for b, L in enumerate(lens) if L] or [0.0])
    ratio = e / max(e32, 1e-30)
    table = RATIOS.setdefault(_ratios_of[0], {})
    table[who] = max(table.get(who, 0.0), ratio if e > 2.0 ** -23 else 0.0)
    print(f"conv {who} {tag}: e = {e:.3e}  e32 = {e32:.3e}  e/e32 = {ratio:.3f}  rel rms = {rms:.3e}")
    assert e <= f32_bound(e32), (who, tag, e, e32, ratio, f32_bound(e32), worst_element(got, ref, lens))
    assert rms < TIGHT_REL_RMS_TOL, (who, tag, rms)
    return ratio


def passes_vs_fp64(got, ref, f32, lens):
    """The criterion's verdict without asserting (the bite test)."""
    return norm_err(got, ref, lens) <= f32_bound(norm_err(f32, ref, lens))


# ---------------------------------------------------------------------------------------------------- Conv1d cases
OPT_DEFAULTS = dict(bias=True, res=False, res_sub=False, relu=False, cond=False, mask_before_res=False, out_scale=1.0, accumulate=False,
                    in_slope=1.0, out_lt_in=False, lens=True, out_len=True)


@functools.lru_cache(maxsize=8)
def conv_case(Cin, Cout, K, dil, T, lens, opts=(), seed=0):
    """The inputs of a Conv1d case and its fp64 results, computed once and read-only.  lens: the rows' in_len (= out_len; with the
    option out_lt_in, out_len = in_len - 3 where that is positive; with out_len off there is none, and every column t < T counts).
    opts: a tuple of (name, value) over OPT_DEFAULTS."""
    o = dict(OPT_DEFAULTS, **dict(opts))
    rng = np.random.default_rng([seed, Cin, Cout, K, dil, T, len(lens)])
    B = len(lens)
    ln = np.asarray(lens, np.int32)
    c = dict(
        x=rng.standard_normal((B, Cin, T)).astype(np.float32),
        w=(rng.standard_normal((Cout, Cin, K)) / np.sqrt(Cin * K)).astype(np.float32),
        bias=(0.3 * rng.standard_normal(Cout)).astype(np.float32) if o["bias"] else None,
        res=rng.standard_normal((B, Cout, T)).astype(np.float32) if o["res"] else None,
        cond=(0.5 * rng.standard_normal((B, Cout))).astype(np.float32) if o["cond"] else None,
        y0=rng.standard_normal((B, Cout, T)).astype(np.float32) if o["accumulate"] else None,
        in_len=ln if o["lens"] else None,
        out_len=(np.where(ln > 3, ln - 3, ln).astype(np.int32) if o["out_lt_in"] else ln) if o["lens"] and o["out_len"] else None,
        dil=dil, in_slope=o["in_slope"], relu=o["relu"], res_sub=o["res_sub"], mask_before_res=o["mask_before_res"],
        out_scale=o["out_scale"])
    c["cmp_len"] = c["out_len"] if c["out_len"] is not None else np.full(B, T, np.int32)
    c["ref"], c["f32"] = {}, {}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def refs(c, group, bf16w=False):
    """(fp64 rule, float32 calibration) of a case, each computed once per (group, weight rounding)."""
    if bf16w not in c["ref"]:
        c["ref"][bf16w] = conv1d_rule(c, np.float64, 0, bf16w)
    if (group, bf16w) not in c["f32"]:
        c["f32"][(group, bf16w)] = conv1d_rule(c, np.float32, group, bf16w)
    return c["ref"][bf16w], c["f32"][(group, bf16w)]


def run_conv(lib, impl, c, math=None, fixed_rule=False, x=None, res=None, y_prior=None):
    """The hook call of a case.  x / res: replacements (the padding tests); y_prior: what y holds before the launch."""
    acc = c["y0"] is not None
    return lib.test_conv1d(c["x"] if x is None else x, c["w"], c["bias"], c["res"] if res is None else res, dilation=c["dil"], impl=impl,
                           in_len=c["in_len"], out_len=c["out_len"], in_slope=c["in_slope"], relu=c["relu"], out_scale=c["out_scale"],
                           res_sub=c["res_sub"], accumulate_into=(c["y0"] if y_prior is None else y_prior) if acc else None,
                           y_prior=None if acc else y_prior, math=math, cond=c["cond"], mask_before_res=c["mask_before_res"],
                           fixed_rule=fixed_rule)


def plan_of(lib, impl, c, math=None, fixed_rule=False):
    B, Cin, T = c["x"].shape
    Cout, _, K = c["w"].shape
    return lib.lab_conv_plan(impl, B, Cin, Cout, T, K, c["dil"], 0, math, fixed_rule, c["res"] is not None, c["cond"] is not None, c["in_len"])


def check_conv(lib, impl, c, tag, math=None, fixed_rule=False, who=None):
    """One hook call of a case against fp64 by the criterion; returns the output."""
    got = run_conv(lib, impl, c, math, fixed_rule)
    ref, f32 = refs(c, GROUP[impl], math == MATH_BF16W)
    assert_vs_fp64(got, ref, f32, c["cmp_len"], who or IMPL_NAMES[impl], tag + (" bf16w" if math == MATH_BF16W else ""))
    return got


def same_valid_bits(a, b, lens, what):
    for r, L in enumerate(lens):
        L = int(L)
        assert np.array_equal(a[r][..., :L], b[r][..., :L]), (what, "row", r, "differs below its length", L)


def ragged_lengths(T, cols, halo=1):
    """One batch row each: full, empty, one column, and around EVERY seam of `cols`-column work items up to T (cols: one width, or the
    widths of all the forms that run the case) — one short of it, on it, one past it, and `halo` columns to either side (the row's
    end inside the halo of the next / of its own last item)."""
    s = {T, 0, 1}
    for width in ((cols,) if isinstance(cols, int) else cols):
        for m in range(width, T + 1, width):
            s |= {m - 1, m, m + 1, m - halo, m + halo}
    return tuple(sorted(n for n in s if 0 <= n <= T))


def length_classes(cols):
    """T of a kernel form with `cols`-column items: 1, an item -1 / 0 / +1, two items + 1 (odd: the scalar staging and epilogue
    branches), one odd T and one T % 4 == 0 (vec / ovec)."""
    return sorted({1, cols - 1, cols, cols + 1, 2 * cols + 1, 37, 2 * cols + 4} - {0})


def class_lengths(T, cols, halo):
    """Rows of a length-class case: every ragged end of ragged_lengths (five a seam: some twenty rows at the widest case, the
    tensors stay below a million floats), the full row first."""
    return (T,) + tuple(n for n in ragged_lengths(T, cols, halo) if n != T)


def last_seam_lengths(T, cols):
    """Rows of a deep-C_in case (few rows, to keep x small): full, empty, one column, and one short of / on / one past the last seam
    below T; the earlier seams are the whole-tensor T of the case's other lengths."""
    m = T // cols * cols
    return tuple(dict.fromkeys(n for n in (T, 0, 1, m - 1, m, m + 1) if 0 <= n <= T))


def derived(c, **changes):
    """A case with some fields replaced and results of its own: the cached case's `ref` / `f32` tables are not shared."""
    return dict(c, **changes, ref={}, f32={})


# ---- f32 MFMA conv (impl 1): (Cin, Cout, K, dil) per kernel, and the tiles MI355VITS_CONV_CFG can force for a row-tile count
F32_TILES_4 = [(2, 2, 2, 2), (1, 2, 2, 2), (1, 1, 2, 2)]  # four row tiles and more
F32_TILES_2 = [(1, 2, 2, 2), (1, 1, 2, 2)]                # two or three
F32_TILES_1 = [(1, 2, 1, 4), (1, 1, 1, 4)]                # one


def f32_tiles(Cout):
    n = (Cout + 31) // 32
    return F32_TILES_4 if n >= 4 else F32_TILES_2 if n >= 2 else F32_TILES_1


def tile_cols(tile):
    return 32 * tile[1] * tile[3]


STAGED_SHAPES = [(32, 128, 7, 3), (32, 29, 7, 3), (32, 70, 5, 1), (32, 64, 7, 3)]  # n_tiles 4, 1, 3 (Cout % 32 != 0 twice), 2
DIRECT_SHAPES = [(64, 128, 1, 1), (16, 32, 3, 1), (512, 64, 1, 1)]  # (the last: 256 k-steps, below split-k's 512)
SPLITK_SHAPES = [(768, 192, 3, 1), (1024, 64, 1, 1)]
# Cin -> (chunk, ring) of the staged kernel at K = 5: 64-channel chunks unrolled, the ring pipeline, the plain loop twice
CHUNK_RING = {64: (64, 32), 48: (48, 0), 6: (6, -1), 70: (14, -1)}
FORCED_CHUNKS = {32: (32, 0), 8: (8, -1)}  # MI355VITS_CONV_CHUNK on Cin = 128 -> (chunk, ring)

# a small orthogonal table over the epilogue's options (every option on and off, every pair of neighbours in epi_std's order together once)
OPTION_CASES = [
    (),
    (("bias", False),),
    (("res", True),),
    (("res", True), ("res_sub", True), ("out_scale", 0.5)),
    (("relu", True), ("cond", True)),
    (("res", True), ("mask_before_res", True), ("relu", True)),
    (("accumulate", True), ("in_slope", 0.1)),
    (("res", True), ("accumulate", True), ("cond", True), ("out_scale", 1.5), ("in_slope", 0.1)),
    (("out_lt_in", True), ("res", True), ("mask_before_res", True), ("cond", True)),
    (("lens", False), ("bias", False), ("in_slope", 0.1)),
]
# options (on top of res) under which the hook's comment names values other than zeros at and past a row's end (conv_whole_range_case)
WHOLE_RANGE_OPTS = [
    ("mask_before_res, out_len < in_len", (("mask_before_res", True), ("out_lt_in", True), ("out_scale", 0.5))),
    ("mask_before_res, res_sub, accumulating", (("mask_before_res", True), ("res_sub", True), ("accumulate", True))),
    ("no out_len", (("out_len", False),)),
]
RBC_OPTION_CASES = [(("res", True),), (("res", True), ("bias", False), ("out_scale", 0.5)), (("res", True), ("accumulate", True), ("in_slope", 0.1))]
RBC_KD = [(3, 1), (3, 2), (5, 2), (5, 6), (7, 3), (7, 12)]
RBC_T = 300
RBC_LENS = (300, 258, 257, 256, 255, 129, 128, 127, 97, 96, 65, 33, 32, 31, 1, 0)  # on, before and past 32- and 128-column items

ENC_T = [1, 63, 64, 65, 127, 128, 129]
ENC_ROWLOOPS = [1, 2, 3, 4, 6]
# (Cin, Cout, K, MI355VITS_ENC_WIDE) -> the kernel the plan call must report
ENC_WIDE_FORMS = [((192, 768, 3, 1), CONVK_ENC_B3W8), ((192, 256, 1, 1), CONVK_ENC_B3W8), ((192, 192, 3, 1), CONVK_ENC_B3W6),
                  ((192, 576, 1, 1), CONVK_ENC_B3W6), ((96, 96, 3, 2), CONVK_ENC_B3W8), ((96, 192, 1, 1), CONVK_ENC_B3W6)]
ENC_SLICES = [(96, 192, 3), (192, 192, 1), (384, 192, 3), (768, 192, 1), (768, 192, 3)]  # the slices' raw sums from 384 on


def enc_lengths(T):
    return tuple(sorted({T, T - 1, max(T - 33, 0), min(T, 65), min(T, 63), 1, 0}, reverse=True))


# ---------------------------------------------------------------------------------------------------- transposed conv cases
CONVT_SHAPES = [(6, 3, 4, 2), (16, 8, 16, 8), (64, 32, 8, 4)]  # (Cin, Cout, K, stride)
UPS_SHAPES = {(256, 128, 16, 8): (32, 64), (128, 64, 16, 8): (32, 128), (64, 32, 8, 4): (31, 127)}  # -> item positions (narrow, wide)


@functools.lru_cache(maxsize=6)
def convt_case(Cin, Cout, K, stride, Tin, lens=None, seed=0, B=2):
    rng = np.random.default_rng([seed, Cin, Cout, K, stride, Tin])
    B = B if lens is None else len(lens)
    c = dict(x=rng.standard_normal((B, Cin, Tin)).astype(np.float32),
             w=(rng.standard_normal((Cin, Cout, K)) / np.sqrt(Cin * K / stride)).astype(np.float32),
             bias=(0.3 * rng.standard_normal(Cout)).astype(np.float32), stride=stride, in_slope=0.1,
             lens=None if lens is None else np.asarray(lens, np.int32))
    c["cmp_len"] = np.full(B, Tin * stride, np.int32) if lens is None else c["lens"] * stride
    c["ref"] = convt_rule(c["x"], c["w"], c["bias"], stride, 0.1, c["lens"], np.float64)
    c["f32"] = {}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def convt_position(c, b, n):
    """Output position n of row b of a transposed-conv case, every channel, in fp64: bias + the taps k with i stride - p + k = n over
    the inputs i below the row's length."""
    w, s = c["w"].astype(np.float64), c["stride"]
    K = w.shape[2]
    L = c["x"].shape[2] if c["lens"] is None else int(c["lens"][b])
    v = c["bias"].astype(np.float64)
    for k in range(K):
        i, r = divmod(n + (K - s) // 2 - k, s)
        if r == 0 and 0 <= i < L:
            v = v + w[:, :, k].T @ _lrelu(c["x"][b, :, i].astype(np.float64), c["in_slope"], np.float64)
    return v


def check_convt(lib, impl, c, tag, y_prior=None):
    got = lib.test_conv_transpose1d(c["x"], c["w"], c["bias"], c["stride"], in_slope=c["in_slope"], impl=impl, in_len=c["lens"], y_prior=y_prior)
    g = CONVT_GROUP[impl]
    if g not in c["f32"]:
        c["f32"][g] = convt_rule(c["x"], c["w"], c["bias"], c["stride"], c["in_slope"], c["lens"], np.float32, g)
    assert_vs_fp64(got, c["ref"], c["f32"][g], c["cmp_len"], CONVT_NAMES[impl], tag)
    # the first and the last output position of every row with any, each summed on its own from the definition (not read out of
    # convt_rule's scatter, whose edges this also checks)
    bound = f32_bound(norm_err(c["f32"][g], c["ref"], c["cmp_len"]))
    for b, n in enumerate(int(v) for v in c["cmp_len"]):
        for pos in {0, n - 1} if n else ():
            d = np.abs(got[b][:, pos] - convt_position(c, b, pos)).max() / np.abs(c["ref"][b][:, :n]).max()
            assert d <= bound, (CONVT_NAMES[impl], tag, "row", b, "output position", pos, d, bound)
    return got


# ---------------------------------------------------------------------------------------------------- enc_o_ln and conv_post cases
ENC_O_LN_T = [1, 31, 32, 33, 65]


@functools.lru_cache(maxsize=6)
def enc_o_ln_case(T, seed=0):
    rng = np.random.default_rng([seed, T, 192])
    lens = sorted({T, T - 1, max(T - 32, 0), min(T, 33), min(T, 31), 1, 0}, reverse=True)
    B, C = len(lens), 192
    ln = np.asarray(lens, np.int32)
    c = dict(x=rng.standard_normal((B, C, T)).astype(np.float32), w=(rng.standard_normal((C, C, 1)) / np.sqrt(C)).astype(np.float32),
             bias=(0.3 * rng.standard_normal(C)).astype(np.float32), res=rng.standard_normal((B, C, T)).astype(np.float32),
             gamma=(1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32), beta=(0.2 * rng.standard_normal(C)).astype(np.float32),
             eps=1e-5, in_len=ln, out_len=np.where(ln > 2, ln - 2, ln).astype(np.int32))  # in_len != ln_out_len
    c["ref"] = {w: enc_o_ln_rule(c, np.float64, 0, w) for w in (False, True)}
    c["f32"] = {w: enc_o_ln_rule(c, np.float32, 2, w) for w in (False, True)}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


CPD_TW, CPD_T, CPV_T, CP_T = 248, 1984, 2048, 1024  # csrc/kernels_conv.cpp: the dpp kernel's tile and workgroup, the vec / staged kernels' workgroups
CONV_POST_DPP_L = [1, 247, 248, 249, 1983, 1984, 1985, 2 * 1984 + 3]
VOLUMES = (1.0, 0.5, 2.5)


@functools.lru_cache(maxsize=8)
def conv_post_case(Cin, K, L, pitch4=True, seed=0):
    """x [B, Cin, P] with P = L rounded up to a multiple of four (the vector kernels need an aligned pitch; valid_len carries L) or L
    itself; rows: full, L - 1, around half, a quiet one (peak below 0.01), an empty one."""
    P = (L + 3) // 4 * 4 if pitch4 else L
    rng = np.random.default_rng([seed, Cin, K, L])
    lens = [L, max(L - 1, 0), (L + 1) // 2, L, 0]
    B = len(lens)
    x = rng.standard_normal((B, Cin, P)).astype(np.float32)
    x[3] *= np.float32(1e-3)  # the quiet row: |audio| ~ 1e-3, below the 0.01 floor of the scale
    w = (rng.standard_normal((1, Cin, K)) * (1.5 / np.sqrt(Cin * K))).astype(np.float32)
    c = dict(x=x, w=w, lens=np.asarray(lens, np.int32))
    c["ref"] = conv_post_rule(x, w, c["lens"], np.float64)
    c["f32"] = conv_post_rule(x, w, c["lens"], np.float32)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def check_conv_post(lib, c, want_kernel, tag, volumes=None):
    """One hook call: the audio against fp64, the peaks and the PCM exact from the kernel's own audio.  Returns (audio, peaks, pcm)."""
    B, _, P = c["x"].shape
    lens = c["lens"]
    audio, peaks, pcm, kernel = lib.test_conv_post(c["x"], c["w"], lens, volumes, audio_prior=np.full((B, P), JUNK, np.float32),
                                                  pcm_prior=np.full((B, P), 12345, np.int16))
    assert kernel == want_kernel, (tag, "launch_conv_post_tanh picked kernel", kernel, "not", want_kernel)
    assert_vs_fp64(audio, c["ref"], c["f32"], lens, ("k_conv_post_tanh_dpp", "k_conv_post_tanh_vec", "k_conv_post_tanh")[kernel], tag)
    assert np.isfinite(audio).all() and np.all(np.abs(audio) <= 1.0), (tag, "every sample t < L is written")
    pad = (c["w"].shape[2] - 1) // 2
    for b, n in enumerate(int(v) for v in lens):
        assert np.all(audio[b, n + pad:] == 0.0), (tag, "zeros behind the taps' reach past valid_len", b)
        want = np.abs(audio[b, :n]).max() if n else np.float32(0.0)
        assert peaks[b].view(np.uint32) == np.float32(want).view(np.uint32), (tag, "peak of row", b, float(peaks[b]), float(want))
    assert peaks[3] < 0.01 and (lens[3] == 0 or peaks[3] > 0.0), (tag, "the quiet row's peak sits below the scale's floor", float(peaks[3]))
    assert np.array_equal(pcm, pcm16_rule(audio, peaks, lens, volumes)), (tag, "pcm differs from the rule on the kernel's own audio")
    return audio, peaks, pcm


# ---------------------------------------------------------------------------------------------------- shared test bodies
def cfg_env(tile):
    return Env(MI355VITS_CONV_CFG=",".join(str(v) for v in tile))


def run_rows(lib, impl, c, rows, math=None, fixed_rule=False):
    """The hook call of a case on a subset of its rows (a smaller grid over the same data)."""
    sl = lambda a: None if a is None else a[rows]
    return lib.test_conv1d(c["x"][rows], c["w"], c["bias"], sl(c["res"]), dilation=c["dil"], impl=impl, in_len=sl(c["in_len"]),
                           out_len=sl(c["out_len"]), in_slope=c["in_slope"], relu=c["relu"], out_scale=c["out_scale"], res_sub=c["res_sub"],
                           accumulate_into=sl(c["y0"]), math=math, cond=sl(c["cond"]), mask_before_res=c["mask_before_res"], fixed_rule=fixed_rule)


def f32_tiles_case(lib, shape, T, opts=()):
    """impl 1 on one shape at one T under every tile MI355VITS_CONV_CFG can force for it: the plan call reports the forced tile (and the
    kernel the shape takes), every tile meets the criterion, and all tiles give the same bits below each row's length (launch_cfg:
    the chunk, hence the summation order, is fixed by C_in alone).  Returns {tile: plan}."""
    Cin, Cout, K, dil = shape
    halo = (K - 1) // 2 * dil
    tiles = f32_tiles(Cout)
    c = conv_case(Cin, Cout, K, dil, T, class_lengths(T, sorted({tile_cols(t) for t in tiles}), max(halo, 1)), opts)
    outs, plans = [], {}
    for tile in tiles:
        with cfg_env(tile):
            p = plan_of(lib, 1, c)
            assert p.tile == tile and p.cols == tile_cols(tile) and p.rows == 32 * tile[0] * tile[2], (shape, T, tile, p.tile, p.cols, p.rows)
            outs.append(check_conv(lib, 1, c, f"{shape} T={T} tile {tile}", who=("", "k_conv1d_mfma", "k_conv_direct_mfma", "k_conv_direct_splitk")[p.kernel]))
        plans[tile] = p
    assert len({p.kernel for p in plans.values()}) == 1 and len({(p.chunk, p.ring) for p in plans.values()}) == 1, (shape, T, "the tile must not move the kernel or the chunk")
    for tile, o in zip(tiles[1:], outs[1:]):
        same_valid_bits(outs[0], o, c["cmp_len"], (shape, T, "tile", tile, "against tile", tiles[0]))
    return plans


def b3_tiles_case(lib, math, T=200):
    """impl 2 (fixed_rule, T <= 512) on 32 -> 128 channels, K = 3: the three EPI_STD tile shapes, each reached by its grid (48, 24
    and 2 rows), the plan call reporting it; each against fp64 and the common rows bit for bit."""
    lens = tuple([T, T - 1, 193, 192, 191, 97, 1, 0] + [T - (5 * b) % 64 for b in range(40)])
    c = conv_case(32, 128, 3, 1, T, lens, (("res", True),))
    outs = {}
    for B, tile in ((48, (2, 3, 2, 2)), (24, (1, 3, 2, 2)), (2, (1, 2, 1, 4))):
        p = lib.lab_conv_plan(2, B, 32, 128, T, 3, 1, 0, math, True, True, False, c["in_len"][:B])
        assert p.kernel == CONVK_B3_STAGED32 and p.tile == tile and p.chunk == 32, (B, p.kernel, p.tile, p.chunk)
        got = run_rows(lib, 2, c, slice(0, B), math, True)
        ref, f32 = refs(c, GROUP[2], math == MATH_BF16W)
        assert_vs_fp64(got, ref[:B], f32[:B], c["cmp_len"][:B], "k_conv1d_b3", f"tile {tile}" + (" bf16w" if math == MATH_BF16W else ""))
        outs[B] = got
    same_valid_bits(outs[48][:24], outs[24], c["cmp_len"][:24], "k_conv1d_b3 (2,3,2,2) against (1,3,2,2)")
    same_valid_bits(outs[48][:2], outs[2], c["cmp_len"][:2], "k_conv1d_b3 (2,3,2,2) against (1,2,1,4)")


def enc_forms_case(lib, math, shape, T, forms):
    """impl 3 on one (Cin, Cout, K) at one T under a list of (env, wanted kernel, wanted rb_loop or None): each form reported by the
    plan call and against fp64, all forms bit for bit the first one below the rows' lengths.  Split convs (Cin > 192) carry no
    epilogue: raw sums."""
    Cin, Cout, K = shape
    split = Cin > 192
    c = conv_case(Cin, Cout, K, 1, T, enc_lengths(T), (("bias", False), ("lens", True)) if split else (("res", True),))
    if split:  # (a split conv has no out_len: the columns past in_len hold the zero-extended row's taps; the rows' own columns count)
        c = derived(c, out_len=None, cmp_len=c["in_len"])
    outs = []
    for env, kernel, rb in forms:
        with Env(**env):
            p = plan_of(lib, 3, c, math)
            assert p.kernel == kernel and (rb is None or p.rb_loop == rb), (shape, T, env, p.kernel, p.rb_loop, kernel, rb)
            assert p.cols == (64 if kernel == CONVK_ENC_B3 else 128), (shape, env, p.cols)
            outs.append(check_conv(lib, 3, c, f"{shape} T={T} {env}", math, who=("k_enc_b3", "k_enc_b3w<8>", "k_enc_b3w<6>")[kernel - CONVK_ENC_B3]))
    for (env, _, _), o in zip(forms[1:], outs[1:]):
        same_valid_bits(outs[0], o, c["cmp_len"], (shape, T, env, "against", forms[0][0]))


def rbc_case(lib, kd, opts):
    """impl 4 at T = 300 on ragged rows: both widths and both item orders, the plan call reporting the width, each against fp64, all
    four bit for bit below the rows' lengths."""
    K, dil = kd
    c = conv_case(128, 128, K, dil, RBC_T, RBC_LENS, opts)
    c = derived(c, out_len=None, cmp_len=c["in_len"])  # (the kernel has no out_len: it writes what the items hold)
    outs = []
    for wide in (0, 1):
        for order in (0, 1):
            with Env(MI355VITS_RBC_WIDE=wide, MI355VITS_RBC_ITEM_ORDER=order):
                p = plan_of(lib, 4, c)
                assert p.kernel == (CONVK_RB_CONV_PW if wide else CONVK_RB_CONV) and p.cols == (128 if wide else 32), (kd, wide, p.kernel, p.cols)
                items = sum(-(-int(n) // p.cols) for n in RBC_LENS)
                assert 0 < p.grid[0] <= items
                outs.append(check_conv(lib, 4, c, f"K={K} d={dil} wide={wide} order={order} {opts}", who="k_rb_conv_pw" if wide else "k_rb_conv"))
    for o in outs[1:]:
        same_valid_bits(outs[0], o, c["cmp_len"], ("launch_rb_conv", kd, "forms differ"))


def past(lens, T):
    return np.arange(T)[None, None, :] >= np.asarray(lens)[:, None, None]


def conv_padding_case(lib, impl, c, math=None, fixed_rule=False, accumulate=False):
    """Everything at and past each row's length that the hook's comment calls unused — x at t >= in_len, res at t >= out_len, the prior
    y — replaced by JUNK: valid columns keep their bits; impl 0 - 3 write exact zeros at out_len <= t < T (accumulating: the prior
    y + 0, i.e. JUNK again).  (mask_before_res and a case without out_len, where other values stand there: conv_whole_range_case.)"""
    assert impl != 4 and not c["mask_before_res"] and c["out_len"] is not None
    B, Cin, T = c["x"].shape
    plain = run_conv(lib, impl, c, math, fixed_rule)
    x = np.where(past(c["in_len"], T), JUNK, c["x"])
    res = None if c["res"] is None else np.where(past(c["out_len"], T), JUNK, c["res"])
    prior = np.full(plain.shape, JUNK, np.float32) if not accumulate else np.where(past(c["out_len"], T), JUNK, c["y0"])
    got = run_conv(lib, impl, c, math, fixed_rule, x=x, res=res, y_prior=prior)
    same_valid_bits(plain, got, c["cmp_len"], (IMPL_NAMES[impl], "JUNK past the lengths reached a valid column"))
    for b, L in enumerate(int(n) for n in c["out_len"]):
        assert np.all(got[b, :, L:] == (JUNK if accumulate else 0.0)), (IMPL_NAMES[impl], "row", b, "past out_len", L)
    return got


def conv_whole_range_case(lib, impl, c, tag, math=None, fixed_rule=False):
    """What the hook's comment says impl 0 - 3 write at and past a row's length where that is not zeros: with mask_before_res,
    res * out_scale at t >= out_len (res is READ there and keeps its values; accumulating, so does the prior y); without out_len,
    the conv of the zero-extended row at t >= in_len.  Every column t < T of every row against the rule, which computes them, by the
    criterion; then JUNK in x at t >= in_len (never used: select) and, not accumulating, all over the prior y moves no bit."""
    assert impl != 4 and c["in_len"] is not None and (c["mask_before_res"] or c["out_len"] is None)
    B, _, T = c["x"].shape
    whole = derived(c, cmp_len=np.full(B, T, np.int32))
    plain = check_conv(lib, impl, whole, f"{tag}: every column t < T", math, fixed_rule)
    x = np.where(past(c["in_len"], T), JUNK, c["x"])
    prior = None if c["y0"] is not None else np.full(plain.shape, JUNK, np.float32)
    got = run_conv(lib, impl, c, math, fixed_rule, x=x, y_prior=prior)
    assert np.array_equal(plain, got), (IMPL_NAMES[impl], tag, "JUNK in x past in_len or in the prior y moved an output")


def rbc_padding_case(lib, kd, wide, accumulate):
    """impl 4: inside the item that holds column in_len - 1 the columns at and past in_len hold the epilogue on the zero-extended row
    (res and, accumulating, the prior y READ there): the rule's values, by the criterion, up to that item's end.  Then x, res and
    the prior y hold JUNK at and past in_len (res and an accumulating conv's prior y are read there and reach padded columns only:
    finite JUNK, as the hook's comment asks).  Valid columns keep their bits; past the item that holds column in_len - 1 nothing is
    written; an empty row is not touched."""
    K, dil = kd
    c = derived(conv_case(128, 128, K, dil, RBC_T, RBC_LENS, (("res", True), ("accumulate", accumulate))), out_len=None)
    lens = c["in_len"]
    with Env(MI355VITS_RBC_WIDE=wide):
        cols = plan_of(lib, 4, c).cols
        plain = run_conv(lib, 4, c)
        ends = np.asarray([min(RBC_T, -(-int(L) // cols) * cols) for L in lens], np.int32)
        ref, f32 = refs(c, GROUP[4])  # (no out_len: the rule gives every column of the zero-extended row)
        assert_vs_fp64(plain, ref, f32, ends, "k_rb_conv_pw" if wide else "k_rb_conv", f"K={K} d={dil} acc={accumulate}: up to each row's last item's end")
        p = past(lens, RBC_T)
        prior = np.where(p, JUNK, c["y0"]) if accumulate else np.full(plain.shape, JUNK, np.float32)
        got = run_conv(lib, 4, c, x=np.where(p, JUNK, c["x"]), res=np.where(p, JUNK, c["res"]), y_prior=prior)
    same_valid_bits(plain, got, lens, ("launch_rb_conv", kd, wide, "JUNK past in_len reached a valid column"))
    for b, L in enumerate(int(n) for n in lens):
        end = min(RBC_T, -(-L // cols) * cols)
        assert np.all(got[b, :, end:] == JUNK), ("launch_rb_conv", kd, wide, "row", b, "written past its last item", L, end)
        assert np.isfinite(got[b]).all()


def enc_o_ln_check(lib, T, math):
    """k_enc_o_ln at one T: against fp64, in place == out of place, JUNK past the lengths, zeros under ln_out_len."""
    c = enc_o_ln_case(T)
    w = math == MATH_BF16W
    args = (c["w"], c["bias"])
    y = lib.test_enc_o_ln(c["x"], *args, c["res"], c["gamma"], c["beta"], c["in_len"], c["out_len"], math=math)
    assert_vs_fp64(y, c["ref"][w], c["f32"][w], c["out_len"], "k_enc_o_ln", f"T={T}" + (" bf16w" if w else ""))
    y_in = lib.test_enc_o_ln(c["x"], *args, c["res"], c["gamma"], c["beta"], c["in_len"], c["out_len"], math=math, in_place=True)
    assert np.array_equal(y, y_in), ("k_enc_o_ln", T, "in place differs from out of place")
    x = np.where(past(c["in_len"], T), JUNK, c["x"])
    res = np.where(past(c["out_len"], T), JUNK, c["res"])
    y_j = lib.test_enc_o_ln(x, *args, res, c["gamma"], c["beta"], c["in_len"], c["out_len"], math=math, y_prior=np.full_like(c["x"], JUNK))
    same_valid_bits(y, y_j, c["out_len"], ("k_enc_o_ln", T, "JUNK past the lengths reached a valid column"))
    for b, L in enumerate(int(n) for n in c["out_len"]):
        assert np.all(y_j[b, :, L:] == 0.0), ("k_enc_o_ln", T, "row", b, "past ln_out_len")


def grid_rule_case(lib, impl, shape, T, want_kernel, want_tile=None, want_cols=None, transposed=False, max_batch=600):
    """The product's own grid rule (no lab switch): the smallest batch of T-column rows for which the plan call reports the wanted
    kernel (and tile, or item width) on this device — three rows against fp64, every row bit for bit its single-row run.  Returns the batch."""
    if transposed:
        Cin, Cout, K, stride = shape
        plan = lambda B: lib.lab_conv_plan(impl, B, Cin, Cout, T, K, 1, stride)
    else:
        Cin, Cout, K, dil = shape
        plan = lambda B: lib.lab_conv_plan(impl, B, Cin, Cout, T, K, dil, 0, None, False, impl == 4, False, np.full(B, T, np.int32))
    ok = lambda p: p.kernel == want_kernel and (want_tile is None or p.tile == want_tile) and (want_cols is None or p.cols == want_cols)
    assert not ok(plan(1)), (shape, "a single row already takes the wide form")
    for B in range(2, max_batch + 1):
        if ok(plan(B)):
            break
    else:
        raise AssertionError(f"no batch of up to {max_batch} rows x {T} columns reaches kernel {want_kernel} {want_tile} on this device")
    lens = tuple(max(T - (3 * b) % max(T // 2, 1), 1) for b in range(B))
    some = [0, B // 2, B - 1]
    if transposed:
        c = convt_case(Cin, Cout, K, stride, T, lens)
        assert ok(lib.lab_conv_plan(impl, B, Cin, Cout, T, K, 1, stride, lengths=c["lens"])), (shape, B, "the ragged batch left the form")
        got = lib.test_conv_transpose1d(c["x"], c["w"], c["bias"], stride, in_slope=0.1, impl=impl, in_len=c["lens"])
        f32 = convt_rule(c["x"][some], c["w"], c["bias"], stride, 0.1, c["lens"][some], np.float32, CONVT_GROUP[impl])
        assert_vs_fp64(got[some], c["ref"][some], f32, c["cmp_len"][some], CONVT_NAMES[impl], f"grid rule: {B} rows x {T}")
        for b in range(B):
            one = lib.test_conv_transpose1d(c["x"][b:b + 1], c["w"], c["bias"], stride, in_slope=0.1, impl=impl, in_len=c["lens"][b:b + 1])
            n = int(c["cmp_len"][b])
            assert np.array_equal(one[0, :, :n], got[b, :, :n]), (CONVT_NAMES[impl], B, "row", b, "differs from its single-row bits")
        return B
    c = conv_case(Cin, Cout, K, dil, T, lens, (("res", True),) if impl == 4 else ())
    if impl == 4:
        c = dict(c, out_len=None, cmp_len=c["in_len"])
    assert ok(plan_of(lib, impl, c)), (shape, B, "the ragged batch left the form")
    got = run_conv(lib, impl, c)
    sub = dict(c, x=c["x"][some], res=None if c["res"] is None else c["res"][some], in_len=c["in_len"][some],
               out_len=None if c["out_len"] is None else c["out_len"][some], cmp_len=c["cmp_len"][some], ref={}, f32={})
    ref, f32 = refs(sub, GROUP[impl])
    assert_vs_fp64(got[some], ref, f32, sub["cmp_len"], IMPL_NAMES[impl], f"grid rule: {B} rows x {T}")
    for b in range(B):
        one = run_rows(lib, impl, c, slice(b, b + 1))
        n = int(c["cmp_len"][b])
        assert np.array_equal(one[0, :, :n], got[b, :, :n]), (IMPL_NAMES[impl], B, "row", b, "differs from its single-row bits")
    return B


def print_ratios(where):
    table = RATIOS.get(where, {})
    for who in sorted(table):
        print(f"conv worst e / e32 {where}: {who}: {table[who]:.3f}")
    assert all(r <= 3.0 for r in table.values())


def convt_pc_case(lib, B, Tin, cu_count=None, cus_list=(None,)):
    """Impl 2 of the transposed hook on 64 -> 32, s = 4: k_conv1d_b3_pc against the one-tile-per-workgroup k_conv1d_b3
    (MI355VITS_NO_B3_PC; lab build and CPU model), the plan call reporting the form and the persistent grid; cu_count (CPU model
    only) sets the CUs the grid is sized by."""
    c = convt_case(64, 32, 8, 4, Tin, seed=3, B=B)
    prior = np.full((B, 32, Tin * 4), JUNK, np.float32)
    with Env(MI355VITS_NO_B3_PC=1):
        p = lib.lab_conv_plan(2, B, 64, 32, Tin, 8, 1, 4)
        assert p.kernel == CONVK_B3_STAGED64 and p.chunk == 64 and p.grid[2] == B, (p.kernel, p.chunk, list(p.grid))
        base = check_convt(lib, 2, c, f"{B} x {Tin}: one tile per workgroup", y_prior=prior)
        items = p.grid[0] * p.grid[1] * p.grid[2]
    for cus in cus_list:
        if cus is not None:
            cu_count(cus)
        p = lib.lab_conv_plan(2, B, 64, 32, Tin, 8, 1, 4)
        assert p.kernel == CONVK_B3_PC and list(p.grid)[1:] == [1, 1] and 0 < p.grid[0] <= items, (cus, p.kernel, list(p.grid), items)
        assert cus is None or p.grid[0] == min(cus, items)
        got = check_convt(lib, 2, c, f"{B} x {Tin}: persistent, grid {p.grid[0]} for {items} items", y_prior=prior)
        assert np.array_equal(got, base), (cus, "the persistent form differs from the staged kernel")
    return items
