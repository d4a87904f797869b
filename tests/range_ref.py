"""Value-range edges: the kernel forms of the other *_ref.py modules on data OFF the unit Gaussian their case tables draw — the
profiles, their checks and the numpy models of the bite proofs that tests/test_value_ranges.py (CPU model of the kernels) and
tests/test_gpu_value_ranges.py (MI355X) share.  The fp64 rules, the float32 calibrations, norm_err / f32_bound / assert_vs_fp64 and
the Twice wrapper are those of tests/conv_ref.py, wn_ref.py, attention_ref.py, mrf_ref.py, small_ref.py and sdp_ref.py: imported,
not restated.  A profile takes a case of those modules' builders and replaces some of its arrays (the builders stay as they are).

  1 homogeneity    conv / transposed conv / MRF forms: x, bias and res times 2^k (k = +20, -20) must scale the output bit for bit: a
                   power of two commutes with every float32 and bf16 rounding while nothing overflows or goes subnormal.
  2 DC offset      the same conv forms on x = mu + N(0, 1), mu in {32, 1024}, with weights that sum to zero over C_in for each tap
                   and output channel: every product is O(mu), the reference O(1).  e <= max(3 e32, 2^-23) as everywhere; the
                   float32 calibration runs on the same inputs with the same accumulation group.  (The engine-level rel. RMS
                   clause of conv_ref.assert_vs_fp64 is left out as in small_ref.assert_vs_fp64_ill_conditioned: the INPUT cancels
                   log2(mu) bits of any float32 evaluation.)  One MRF table on x = 8 + N(0, 1).
  3 gate           WaveNet layer forms with w_in * 2^-10 and b_in + cond = a grid of pre-activations around wn_gate_f's clamps
                   (tanh +-15, sigmoid +-30), beyond them, and around 0.
  4 softmax        attention forms on peaked rows (q, k * 6), on a running maximum that rises / falls by 8 per 32 keys, and on one key
                   lifted by 60 in each row's last key tile.
  5 LayerNorm      k_layernorm by column: mean 1000 . std 1, mean -1000 . std 1e-2, constant 0.1, std 1e-3, std 1e4, zeros, and
                   gamma * 6 into GELU's tails; the LayerNorms inside k_enc_o_ln, the DDS stack forms and k_dp_det on "mean 32 . std 1"
                   and "std 1e-3" at their first LayerNorm.
  6 decoder tail   conv_post / pcm16 on a saturated row (x * 64) and on a row of zeros with a non-empty length.

GATE pairing.  The tanh half takes TANH_GRID[c % 15], the sigmoid half SIG_GRID[c % 11] at channel c: 15 and 11 are coprime, so the
165 first channels of H = 192 hold every (tanh, sigmoid) pair once.  At H = 32 the same rule gives 32 distinct pairs: every tanh
value meets two or three sigmoid values, every sigmoid value two or three tanh values (channel c pairs c % 15 with c % 11)."""
import numpy as np

from tests import attention_ref as A
from tests import conv_ref as CR
from tests import mrf_ref as M
from tests import sdp_ref as SD
from tests import small_ref as SM
from tests import wn_ref as Wn
from tests.attention_ref import f32_bound, norm_err
from tests.sdp_ref import Twice, bf16_round  # noqa: F401  (Twice: the device module wraps its libraries in it)
from tests.wn_ref import Env
from mimic3_amd._native import (CONVK_B3_PC, CONVK_B3_STAGED32, CONVK_B3_STAGED64, CONVK_CONVT_GENERIC, CONVK_ENC_B3, CONVK_ENC_B3W8,
                                CONVK_F32_DIRECT, CONVK_F32_SPLITK, CONVK_F32_STAGED, CONVK_GENERIC, CONVK_RB_CONV, CONVK_RB_CONV_PW,
                                CONVK_UPS64, CONVK_UPS_PL, MATH_BF16W, MATH_BF16X3, MATH_F32)

F32 = np.float32
MATH_NAMES = {None: "f32", MATH_F32: "f32", MATH_BF16X3: "bf16x3", MATH_BF16W: "bf16w"}

RAN = {}         # library -> (form, profile) pairs run on it: the closing tests compare them with the table of test_value_ranges' docstring
FIGURES = {}     # library -> (profile, form) -> worst e / e32 seen (printed by the closing tests; DESIGN.md quotes them)


class Libs:
    """The libraries of a test module: `plain` runs what the product's rules pick, `lab` reads the lab switches (Env) at every
    launch.  On the CPU model both are the one library; on the device the hooks library and the lab build."""

    def __init__(self, plain, lab, where):
        self.plain, self.lab, self.where = plain, lab, where

    def pick(self, env):
        return self.lab if env else self.plain


def note(libs, profile, form, e=None, e32=None):
    RAN.setdefault(libs.where, set()).add((form, profile))
    if e is not None:
        t = FIGURES.setdefault(libs.where, {})
        t[(profile, form)] = max(t.get((profile, form), 0.0), e / max(e32, 1e-30) if e > 2.0 ** -23 else 0.0)


def rows(T):
    """The rows of every case here: full, one short, 17, one column, empty."""
    return tuple(dict.fromkeys(n for n in (T, T - 1, 17, 1, 0) if 0 <= n <= T))


def criterion(got, ref, f32, lens, who, tag):
    """e <= max(3 e32, 2^-23) per row over its own columns, every valid element finite, the calibration finite: conv_ref's criterion
    without the engine-level rel. RMS clause (small_ref.assert_vs_fp64_ill_conditioned), returning (e, e32)."""
    got, ref, f32 = (a[:, None, :] if a.ndim == 2 else a for a in (got, ref, f32))
    for b, L in enumerate(lens):
        assert np.isfinite(ref[b][:, :int(L)]).all() and np.isfinite(f32[b][:, :int(L)]).all(), (who, tag, b, "reference or calibration not finite")
    SM.assert_vs_fp64_ill_conditioned(got, ref, f32, lens, who, tag)
    return norm_err(got, ref, lens), norm_err(f32, ref, lens)


# ---------------------------------------------------------------------------------------------------- the conv forms
NARROW = dict(MI355VITS_ENC_WIDE=0, MI355VITS_ENC_ROWLOOP=1)
B3 = (MATH_BF16X3, MATH_BF16W)
# name -> (hook impl, (Cin, Cout, K, dil), T, math modes, lab switches, fixed_rule, the kernel the plan call must report)
CONV_FORMS = {
    "k_conv1d_generic":      (0, (32, 70, 5, 1), 33, (None,), {}, False, CONVK_GENERIC),
    "k_conv1d_mfma":         (1, (32, 70, 5, 1), 33, (None,), {}, False, CONVK_F32_STAGED),
    "k_conv_direct_mfma":    (1, (64, 70, 1, 1), 33, (None,), {}, False, CONVK_F32_DIRECT),
    "k_conv_direct_splitk":  (1, (1024, 40, 1, 1), 33, (None,), {}, False, CONVK_F32_SPLITK),
    "k_conv1d_b3":           (2, (32, 128, 3, 1), 33, B3, {}, True, CONVK_B3_STAGED32),
    "k_conv1d_b3 chunk-64":  (2, (64, 64, 2, 1), 33, B3, {}, True, CONVK_B3_STAGED64),
    "k_enc_b3":              (3, (192, 96, 3, 1), 141, B3, NARROW, False, CONVK_ENC_B3),
    "k_enc_b3w":             (3, (192, 96, 3, 1), 141, B3, dict(MI355VITS_ENC_WIDE=2), False, CONVK_ENC_B3W8),
    "k_rb_conv":             (4, (128, 128, 7, 3), 33, (None,), dict(MI355VITS_RBC_WIDE=0), False, CONVK_RB_CONV),
    "k_rb_conv_pw":          (4, (128, 128, 7, 3), 141, (None,), dict(MI355VITS_RBC_WIDE=1), False, CONVK_RB_CONV_PW),
}
# name -> (hook impl, (Cin, Cout, K, stride), Tin, rows (None: two full rows, the hooks of impl 0 - 2 take no lengths), lab switches, kernel)
CONVT_FORMS = {
    "k_conv_transpose1d":       (0, (64, 32, 8, 4), 17, None, {}, CONVK_CONVT_GENERIC),
    "polyphase f32 direct":     (1, (64, 32, 8, 4), 33, None, {}, CONVK_F32_DIRECT),
    "polyphase f32 staged":     (1, (128, 64, 16, 8), 17, None, {}, CONVK_F32_STAGED),
    "polyphase k_conv1d_b3":    (2, (64, 32, 8, 4), 33, None, {}, CONVK_B3_STAGED64),
    "k_conv1d_b3_pc":           (2, (64, 32, 8, 4), 2000, (2000,) * 5, {}, CONVK_B3_PC),
    "k_ups_pl":                 (3, (128, 64, 16, 8), 33, rows(33), dict(MI355VITS_RBC_WIDE=0), CONVK_UPS_PL),
    "k_ups64":                  (3, (64, 32, 8, 4), 33, rows(33), dict(MI355VITS_RBC_WIDE=0), CONVK_UPS64),
}
# name -> (hook impl, math, C, T, seg): the smallest C of mrf_ref's tables per kernel, T = one work item + 5 columns (k_mrf_fused<32>: the
# item is 512 columns wide, 97 columns stay inside one)
MRF_FORMS = {
    "k_mrf_fused f32":     (0, MATH_F32, 64, 197, 0),
    "k_mrf_fused bf16x3":  (0, MATH_BF16X3, 64, 197, 0),
    "k_mrf_fused<32>":     (0, MATH_BF16X3, 32, 97, 0),
    "k_mrf_p<32>":         (1, None, 32, 325, 0),
    "k_mrf_p<64>":         (1, None, 64, 101, 0),
    "k_mrf_s<64>":         (2, None, 64, 101, 48),
}
CONV_OPTS = (("res", True), ("in_slope", 0.1))


def conv_form_case(name):
    impl, (Cin, Cout, K, dil), T = CONV_FORMS[name][:3]
    c = CR.conv_case(Cin, Cout, K, dil, T, rows(T), CONV_OPTS)
    return CR.derived(c, out_len=None, cmp_len=c["in_len"]) if impl == 4 else c  # (k_rb_conv has no out_len: conv_ref.rbc_case)


def convt_form_case(name):
    _, (Cin, Cout, K, s), Tin, lens = CONVT_FORMS[name][:4]
    if lens is not None and len(set(lens)) == 1:  # full rows as a batch of their own
        return CR.convt_case(Cin, Cout, K, s, Tin, seed=3, B=len(lens))
    return CR.convt_case(Cin, Cout, K, s, Tin, lens)


def run_convt(lib, impl, c):
    return lib.test_conv_transpose1d(c["x"], c["w"], c["bias"], c["stride"], in_slope=c["in_slope"], impl=impl, in_len=c["lens"])


def plan_is(lib, name):
    """The plan call reports the kernel the form's name stands for (no kernel runs)."""
    if name in CONV_FORMS:
        impl, _, _, maths, _, fixed, kernel = CONV_FORMS[name]
        got = CR.plan_of(lib, impl, conv_form_case(name), maths[0], fixed).kernel
    else:
        impl, (Cin, Cout, K, s), Tin, lens, _, kernel = CONVT_FORMS[name]
        got = lib.lab_conv_plan(impl, 2 if lens is None else len(lens), Cin, Cout, Tin, K, 1, s, lengths=lens if impl == 3 else None).kernel
    assert got == kernel, (name, "the plan call reports kernel", got, "not", kernel)


# ---------------------------------------------------------------------------------------------------- 1: homogeneity
POWERS = (20, -20)


def within_2_60(*arrays):
    """Every non-zero element lies within 2^+-60: no product of the case overflows float32 or goes subnormal."""
    for a in arrays:
        if a is not None:
            v = np.abs(np.asarray(a, np.float64))
            v = v[v != 0]
            assert np.isfinite(v).all() and (v.size == 0 or (v.min() >= 2.0 ** -60 and v.max() <= 2.0 ** 60)), (float(v.min()), float(v.max()))


def same_scaled_bits(plain, scaled, k, lens, what):
    want = plain * F32(2.0 ** k)
    for b, L in enumerate(int(n) for n in lens):
        assert np.array_equal(scaled[b][..., :L].view(np.uint32), want[b][..., :L].view(np.uint32)), (what, f"2^{k}", "row", b, "is not the plain run times 2^k bit for bit")


def scale(a, k):
    return None if a is None else (a * F32(2.0 ** k)).astype(F32)


def homogeneity_conv(libs, name):
    impl, _, _, maths, env, fixed, _ = CONV_FORMS[name]
    lib = libs.pick(env)
    c = conv_form_case(name)
    with Env(**env):
        plan_is(lib, name)
        for math in maths:
            plain = CR.run_conv(lib, impl, c, math, fixed)
            ref, _ = CR.refs(c, CR.GROUP[impl], math == MATH_BF16W)
            for k in POWERS:
                s = CR.derived(c, x=scale(c["x"], k), bias=scale(c["bias"], k), res=scale(c["res"], k))
                within_2_60(s["x"], s["bias"], s["res"], s["w"], ref * 2.0 ** k)
                same_scaled_bits(plain, CR.run_conv(lib, impl, s, math, fixed), k, c["cmp_len"], (name, MATH_NAMES[math]))
    note(libs, 1, name)


def homogeneity_convt(libs, name):
    impl, _, _, _, env, _ = CONVT_FORMS[name]
    lib = libs.pick(env)
    c = convt_form_case(name)
    with Env(**env):
        plan_is(lib, name)
        plain = run_convt(lib, impl, c)
        for k in POWERS:
            s = dict(c, x=scale(c["x"], k), bias=scale(c["bias"], k))
            within_2_60(s["x"], s["bias"], s["w"], c["ref"] * 2.0 ** k)
            same_scaled_bits(plain, run_convt(lib, impl, s), k, c["cmp_len"], name)
    note(libs, 1, name)


def mrf_form_case(name, offset=0.0):
    impl, math, C, T, seg = MRF_FORMS[name]
    c = M.reference_case(C, T, M.LOW_KS, M.LOW_DILS, rows(T))
    if offset:
        x = (c["x"] + F32(offset)).astype(F32)
        c = dict(c, x=x, ref=M.mrf_stage_fp64(x, c["ks"], c["dils"], c["w"], c["b"], c["lens"], c["out_scale"]), f32={})
    return c


def homogeneity_mrf(libs, name):
    impl, math, C, T, seg = MRF_FORMS[name]
    lib = libs.plain
    c = mrf_form_case(name)
    plain = M.run_case(lib, impl, c, math=math, seg=seg)
    for k in POWERS:
        s = dict(c, x=scale(c["x"], k), b=[[scale(v, k) for v in p] for p in c["b"]])
        within_2_60(s["x"], *[v for p in s["b"] + s["w"] for v in p], c["ref"] * 2.0 ** k)
        same_scaled_bits(plain, M.run_case(lib, impl, s, math=math, seg=seg), k, c["lens"], name)
    note(libs, 1, name)


# ---------------------------------------------------------------------------------------------------- 2: DC offset
MUS = (32.0, 1024.0)


def zero_sum(w, axis):
    """w with its mean over C_in (axis) taken out in fp64: each tap of each output channel sums to zero up to one float32 rounding a weight."""
    w = w.astype(np.float64)
    return (w - w.mean(axis=axis, keepdims=True)).astype(F32)


def dc_conv_case(name, mu):
    c = conv_form_case(name)
    return CR.derived(c, x=(c["x"] + F32(mu)).astype(F32), w=zero_sum(c["w"], 1))


def dc_conv(libs, name, mu, math):
    impl, _, _, _, env, fixed, _ = CONV_FORMS[name]
    lib = libs.pick(env)
    c = dc_conv_case(name, mu)
    with Env(**env):
        got = CR.run_conv(lib, impl, c, math, fixed)
    ref, f32 = CR.refs(c, CR.GROUP[impl], math == MATH_BF16W)
    assert np.abs(ref).max() < 64.0, (name, mu, "the reference stays O(1)")
    note(libs, 2, name, norm_err(got, ref, c["cmp_len"]), norm_err(f32, ref, c["cmp_len"]))  # (before the verdict: a case over the bound is in the tables too)
    return criterion(got, ref, f32, c["cmp_len"], name, f"mu={mu:g} {MATH_NAMES[math]}")


def dc_convt_case(name, mu):
    c = convt_form_case(name)
    c = dict(c, x=(c["x"] + F32(mu)).astype(F32), w=zero_sum(c["w"], 0))
    c["ref"] = CR.convt_rule(c["x"], c["w"], c["bias"], c["stride"], c["in_slope"], c["lens"], np.float64)
    return c


def dc_convt(libs, name, mu):
    impl, _, _, _, env, _ = CONVT_FORMS[name]
    lib = libs.pick(env)
    c = dc_convt_case(name, mu)
    with Env(**env):
        got = run_convt(lib, impl, c)
    f32 = CR.convt_rule(c["x"], c["w"], c["bias"], c["stride"], c["in_slope"], c["lens"], F32, CR.CONVT_GROUP[impl])
    assert np.abs(c["ref"]).max() < 64.0, (name, mu, "the reference stays O(1)")
    e, e32 = criterion(got, c["ref"], f32, c["cmp_len"], name, f"mu={mu:g}")
    note(libs, 2, name, e, e32)
    return e, e32


def dc_mrf(libs, name):
    impl, math, C, T, seg = MRF_FORMS[name]
    c = mrf_form_case(name, 8.0)
    assert np.isfinite(c["ref"]).all() and np.isfinite(M.calibration(c, impl, math)).all()
    got = M.run_case(libs.plain, impl, c, math=math, seg=seg)
    M.assert_vs_fp64(got, c, impl, f"{name} x = 8 + N(0, 1)", math=math)
    note(libs, 2, name, norm_err(got, c["ref"], c["lens"]), norm_err(M.calibration(c, impl, math), c["ref"], c["lens"]))


# ---------------------------------------------------------------------------------------------------- 3: gate saturation
TANH_GRID = (0.0, 1e-4, -1e-4, 0.5, -0.5, 3.0, -3.0, 14.9, -14.9, 15.1, -15.1, 40.0, -40.0, 100.0, -100.0)
SIG_GRID = (0.0, 1.0, -1.0, 29.9, -29.9, 30.1, -30.1, 60.0, -60.0, 100.0, -100.0)
B3_NT = [dict(MI355VITS_WN_B3_NT=1), dict(MI355VITS_WN_B3_NT=3, MI355VITS_WN_EPI=0), dict(MI355VITS_WN_B3_NT=3, MI355VITS_WN_EPI=1), dict(MI355VITS_WN_B3_NT=4)]
# name -> (hook impl, H, T, lab switches): T = 33 for the 32-column forms, wn_ref.KD_T = 141 for the 96- and 128-column ones
GATE_FORMS = {
    "gate conv + res/skip conv":                (0, 192, Wn.KD_T, {}),
    "EPI_GATE conv tile (2,2,2,2)":             (0, 192, Wn.KD_T, dict(MI355VITS_CONV_CFG="2,2,2,2")),
    "EPI_GATE conv tile (2,1,2,2)":             (0, 192, Wn.KD_T, dict(MI355VITS_CONV_CFG="2,1,2,2")),
    "launch_wn_layer H=192":                    (1, 192, 33, {}),
    "launch_wn_layer H=192 geometry 0":         (1, 192, 33, dict(MI355VITS_WN_SIX_WAVES=0)),
    "launch_wn_layer H=192 geometry 1":         (1, 192, 33, dict(MI355VITS_WN_SIX_WAVES=1)),
    "launch_wn_layer H=192 geometry 2":         (1, 192, 33, dict(MI355VITS_WN_SIX_WAVES=2)),
    "launch_wn_layer H=32":                     (1, 32, 33, {}),
    "k_wn_layer_b3":                            (2, 192, 33, {}),
    "k_wn_layer_b3 32 columns":                 (2, 192, 33, B3_NT[0]),
    "k_wn_layer_b3 96 columns, epilogue 0":     (2, 192, Wn.KD_T, B3_NT[1]),
    "k_wn_layer_b3 96 columns, epilogue 1":     (2, 192, Wn.KD_T, B3_NT[2]),
    "k_wn_layer_b3 128 columns":                (2, 192, Wn.KD_T, B3_NT[3]),
    "k_wn_layer_b3 32x32x16, 32 columns":       (2, 192, 33, dict(B3_NT[0], MI355VITS_WN_SHAPE=32)),
    "k_wn_layer_b3 32x32x16, 128 columns":      (2, 192, Wn.KD_T, dict(B3_NT[3], MI355VITS_WN_SHAPE=32)),
}
_gate_cases = {}


def gate_grid(H):
    c = np.arange(H)
    return np.concatenate([np.asarray(TANH_GRID, np.float64)[c % len(TANH_GRID)], np.asarray(SIG_GRID, np.float64)[c % len(SIG_GRID)]])


def gate_case(H, T, saturate=True):
    """wn_ref.reference_case(H, T, 5, 1, 2 H, rows(T)) with w_in * 2^-10, b_in = 3/4 of the grid and cond = 1/4 of it in every row
    (saturate=False: the case as drawn, the Gaussian table's).  The fp64 rule and the float32 calibration are computed here and
    asserted finite (numpy's exp overflows to inf at -100: 1 / (1 + inf) = 0, harmless)."""
    key = (H, T, saturate)
    if key not in _gate_cases:
        c = Wn.reference_case(H, T, 5, 1, 2 * H, rows(T))
        if saturate:
            g = gate_grid(H)
            c = dict(c, w_in=(c["w_in"] * F32(2.0 ** -10)).astype(F32), b_in=(0.75 * g).astype(F32),
                     cond=np.tile((0.25 * g).astype(F32), (len(c["lens"]), 1)), f32={})
            with np.errstate(over="ignore"):
                c["ref"] = Wn.wn_layer_fp64(c["h"], c["skip"], c["w_in"], c["b_in"], c["w_rs"], c["b_rs"], c["lens"], 1, c["cond"], False)
        with np.errstate(over="ignore"):
            f32 = Wn.calibration(c, 1)
        assert all(np.isfinite(a).all() for a in c["ref"] + f32), (H, T, "the rule or the calibration is not finite")
        _gate_cases[key] = c
    return _gate_cases[key]


def gate_saturation(libs, name):
    impl, H, T, env = GATE_FORMS[name]
    lib = libs.pick(env)
    c = gate_case(H, T)
    with Env(**env):
        if impl == 2 and "MI355VITS_WN_B3_NT" in env:
            assert lib.lab_wn_plan(len(c["lens"]), T)[0] == {1: 32, 3: 96, 4: 128}[env["MI355VITS_WN_B3_NT"]], (name, "the plan call reports another tile")
        got = Wn.run_case(lib, impl, c)
    Wn.assert_vs_fp64(got, c, impl, f"gate saturation, {name}")
    cal = Wn.calibration(c, impl)
    for g, r, m in zip(got, c["ref"], cal):
        note(libs, 3, name, norm_err(g, r, c["lens"]), norm_err(m, r, c["lens"]))


def wn_layer_with_gate(c, gate):
    """(h', skip') of a case in numpy float32 as wn_ref's calibration computes them (two channels per addition), with `gate(a_t, a_s)`
    in place of tanh(a_t) * sigmoid(a_s): the bite proof's model, never a kernel."""
    H = c["h"].shape[1]
    h2, s2 = np.zeros_like(c["h"]), np.zeros_like(c["h"])
    for b, L in enumerate(int(n) for n in c["lens"]):
        if L:
            a = Wn._conv(c["h"][b, :, :L], c["w_in"], c["b_in"] + c["cond"][b], 1, F32, 2)
            rs = Wn._conv(gate(a[:H], a[H:]).astype(F32), c["w_rs"], c["b_rs"], 1, F32, 2)
            h2[b, :, :L] = c["h"][b, :, :L] + rs[:H]
            s2[b, :, :L] = c["skip"][b, :, :L] + rs[H:]
    return h2, s2


def gate_clamped(limit):
    def gate(at, as_):
        with np.errstate(over="ignore"):
            return np.tanh(np.clip(at, F32(-limit), F32(limit))) * (F32(1) / (F32(1) + np.exp(-as_)))
    return gate


def gate_passes(c, got):
    cal = Wn.calibration(c, 1)
    return all(norm_err(g, r, c["lens"]) <= f32_bound(norm_err(m, r, c["lens"])) for g, r, m in zip(got, c["ref"], cal))


# ---------------------------------------------------------------------------------------------------- 4: softmax maxima
# name -> (hook impl, T, d, heads, W): the smallest T of attention_ref's length classes at which the form walks three key tiles —
# k_rel_attention_stream's four waves take every fourth 32-key tile, so a wave meets three from T = 257 on (tiles 0, 4, 8);
# k_rel_attention_mfma4 holds a row's five tiles at T = 129 (NKW = 2); the VALU kernel walks T = 70 key by key.
ATTN_FORMS = {
    "k_rel_attention":        (0, 70, 16, 2, 4),
    "k_rel_attention_mfma4":  (1, 129, 96, 2, 4),
    "k_rel_attention_stream": (2, 257, 96, 2, 4),
}
ATTN_KINDS = ("peaked", "rising", "falling", "lifted")
_attn_cases = {}


def attn_case(T, d, n_heads, Wn_, kind):
    """attention_ref.attention_case on rows(T), then by kind —
    peaked: q, k * 6 (logit std 36, near one-hot rows);
    rising / falling: channel 0 of every head holds 4 sqrt(d) in q and +- j / 16 in k: the content logit moves by 8 per 32 keys;
    lifted: the same constant in q, and in every row the key two short of the row's end carries 15 there: that key's logit is 60
            above the others', inside the relative window of the row's last queries, more than W keys away (and in the last key
            tile) for every other query;
    gauss: the case as drawn (the bite proof's Gaussian table)."""
    key = (T, d, n_heads, Wn_, kind)
    if key not in _attn_cases:
        lens = rows(T)
        qkv, ek, ev, ln = A.attention_case(T, d, list(lens), n_heads, Wn_)
        qkv = qkv.copy()
        H = d * n_heads
        ch = np.arange(n_heads) * d
        if kind == "peaked":
            qkv[:, :2 * H] *= F32(6.0)
        elif kind in ("rising", "falling", "lifted"):
            qkv[:, ch, :] = F32(4.0 * np.sqrt(d))
            if kind == "lifted":
                for b, L in enumerate(lens):
                    qkv[b, H + ch, max(L - 2, 0)] = F32(15.0)
            else:
                qkv[:, H + ch, :] = (np.arange(T, dtype=F32) / F32(16.0 if kind == "rising" else -16.0))[None, None, :]
        else:
            assert kind == "gauss"
        ref, f32 = A.rel_attention_fp64(qkv, ek, ev, ln, n_heads), A.rel_attention_f32(qkv, ek, ev, ln, n_heads)
        assert np.isfinite(ref).all() and np.isfinite(f32).all()
        _attn_cases[key] = (qkv, ek, ev, ln, ref, f32)
    return _attn_cases[key]


def softmax_maxima(libs, name, kind):
    impl, T, d, n_heads, Wn_ = ATTN_FORMS[name]
    qkv, ek, ev, ln, ref, f32 = attn_case(T, d, n_heads, Wn_, kind)
    got = libs.plain.test_rel_attention(qkv, ek, ev, ln, n_heads, impl=impl)
    e, e32 = A.assert_vs_fp64(got, ref, f32, ln, impl, f"{kind} T={T} d={d}")
    note(libs, 4, name, e, e32)


def online_softmax(qkv, ek, ev, lens, n_heads, tile=32, skip_rescale_at=None):
    """The rule of attention_ref.rel_attention_f32 with the keys taken `tile` at a time under a running maximum, in numpy float32: at
    every tile alpha = exp(mx - mnew) rescales the sum and the accumulated numerators (content and relative-value).
    skip_rescale_at: the tile at which the broken variant leaves the content numerator as it is.  The bite proof's model."""
    qkv, ek, ev = (np.asarray(a, F32) for a in (qkv, ek, ev))
    B, H3, T = qkv.shape
    H = H3 // 3
    d = H // n_heads
    W = (ek.shape[0] - 1) // 2
    sc = F32(1.0) / np.sqrt(F32(d))
    out = np.zeros((B, H, T), F32)
    for b, L in enumerate(int(n) for n in lens):
        idx = np.arange(L)
        for h in range(n_heads if L else 0):
            c0 = h * d
            q, k, v = qkv[b, c0:c0 + d, :L].T * sc, qkv[b, H + c0:H + c0 + d, :L].T, qkv[b, 2 * H + c0:2 * H + c0 + d, :L].T
            rel = idx[None, :] - idx[:, None]
            inwin = np.abs(rel) <= W
            s = q @ k.T + np.where(inwin, np.take_along_axis(q @ ek.T, np.clip(rel + W, 0, 2 * W), axis=1), F32(0))
            mx, den = np.full(L, F32(-3e38)), np.zeros(L, F32)
            num = np.zeros((L, d), F32)
            for n, j0 in enumerate(range(0, L, tile)):
                st = s[:, j0:j0 + tile]
                mnew = np.maximum(mx, st.max(axis=1))
                alpha = np.exp(mx - mnew)
                p = np.exp(st - mnew[:, None])
                band = np.zeros((L, d), F32)
                for r in range(2 * W + 1):
                    j = idx + (r - W)
                    ok = (j >= j0) & (j < min(j0 + tile, L))
                    band[idx[ok]] += p[idx[ok], j[ok] - j0][:, None] * ev[r][None, :]
                den = den * alpha + p.sum(axis=1, dtype=F32)
                num = (num if n == skip_rescale_at else num * alpha[:, None]) + p @ v[j0:j0 + tile] + band
                mx = mnew
            o = num / den[:, None]
            assert o.dtype == F32
            out[b, c0:c0 + d, :L] = o.T
    return out


# ---------------------------------------------------------------------------------------------------- 5: LayerNorm conditioning
LN_COLUMNS = ("mean 1000, std 1", "mean -1000, std 1e-2", "constant 0.1", "std 1e-3", "std 1e4", "zeros", "unit")  # column t holds LN_COLUMNS[t % 7]
LN_T = 35
# name -> (C, options of small_ref.ln_case, gamma factor): each of res / bias / nparts / gelu / add_to on once; the uncached template
# takes no bias and no partial sums (small_ref.LN_REFUSED)
LN_FORMS = {
    "k_layernorm<cached>": (192, [("plain", {}, 1.0), ("res", dict(res=True), 1.0), ("bias", dict(bias=True), 1.0), ("nparts 2", dict(nparts=2), 1.0),
                                  ("gelu", dict(gelu=True), 1.0), ("add_to", dict(add_to=True), 1.0), ("gelu, gamma * 6", dict(gelu=True), 6.0)]),
    "k_layernorm<uncached>": (300, [("plain", {}, 1.0), ("res", dict(res=True), 1.0), ("gelu", dict(gelu=True), 1.0), ("add_to", dict(add_to=True), 1.0),
                                    ("gelu, gamma * 6", dict(gelu=True), 6.0)]),
}
SMALL = F32(2.0 ** -16)  # what the other addends of v (res, bias, the second partial sum) are scaled by: present, and far below every column's spread but the constant ones'


def ln_profile_case(C, opts, gamma_factor=1.0):
    """small_ref.ln_case(C, LN_T, opts) with the first addend of v replaced column by column (LN_COLUMNS) and the other addends of v
    (res, bias, further partial sums) times 2^-16, so that v keeps each column's conditioning; add_to, gamma (times the factor) and
    beta as drawn."""
    c = SM.ln_case(C, LN_T, tuple(opts.items()))
    x = c["x"] if c["nparts"] > 1 else c["x"][None]
    n = x[0].copy()  # N(0, 1) [B, C, T]
    t = np.arange(LN_T)
    first = np.select([t % 7 == k for k in range(7)],
                      [1000.0 + n, -1000.0 + 1e-2 * n, np.full_like(n, 0.1), 1e-3 * n, 1e4 * n, np.zeros_like(n), n]).astype(F32)
    x = np.concatenate([first[None], x[1:] * SMALL])
    c.update(x=x if c["nparts"] > 1 else x[0], gamma=(c["gamma"] * F32(gamma_factor)).astype(F32))
    for k in ("res", "bias"):
        if c[k] is not None:
            c[k] = c[k] * SMALL
    return c


def ln_conditioning(libs, name, which):
    """One option case of a k_layernorm template: the criterion per column profile (a column's own scale: the cancelling columns must
    not hide the others behind their float32 error), every element of every column in exactly one group."""
    C, cases = LN_FORMS[name]
    tag0, opts, gf = cases[which]
    c = ln_profile_case(C, opts, gf)
    got = SM.run_ln(libs.plain, c, alias=None)
    assert not np.any(got == SM.JUNK), (name, tag0, "every column t < T is written")
    with np.errstate(invalid="ignore"):
        ref, f32 = SM.layernorm_rule(c, np.float64), SM.layernorm_rule(c, F32)
    assert np.isfinite(ref).all() and np.isfinite(f32).all(), (name, tag0, "the rule or the calibration is not finite")
    t = np.arange(LN_T)
    for k, col in enumerate(LN_COLUMNS):
        sel = t % 7 == k
        lens = np.full(got.shape[0], int(sel.sum()), np.int32)
        e, e32 = criterion(got[:, :, sel], ref[:, :, sel], f32[:, :, sel], lens, name, f"{tag0}: {col}")
        note(libs, 5, name, e, e32)
    return got


def one_pass_passes(c, columns=True):
    """The verdict on the one-pass variance E[v^2] - mean^2 in float32 (small_ref.layernorm_rule's wrong variant): per column profile
    (columns=True, this module's cases) or over whole rows (the Gaussian table's cases)."""
    with np.errstate(invalid="ignore"):
        ref, f32, bad = SM.layernorm_rule(c, np.float64), SM.layernorm_rule(c, F32), SM.layernorm_rule(c, F32, one_pass=True)
    if not columns:
        return SM.passes_vs_fp64(bad, ref, f32, c["cmp_len"])
    t = np.arange(ref.shape[2])
    return {col: SM.passes_vs_fp64(bad[:, :, t % 7 == k], ref[:, :, t % 7 == k], f32[:, :, t % 7 == k], np.full(ref.shape[0], int((t % 7 == k).sum())))
            for k, col in enumerate(LN_COLUMNS)}


LN_INNER = ("mean 32, std 1", "std 1e-3")  # what the first LayerNorm of a composite kernel sees


def enc_o_ln_conditioning(libs, kind, math):
    """k_enc_o_ln: LN_c(res + conv1x1(x) + bias).  "mean 32, std 1": res + 32; "std 1e-3": x, bias and res times 1e-3."""
    c = dict(CR.enc_o_ln_case(33))
    if kind == LN_INNER[0]:
        c["res"] = (c["res"] + F32(32.0)).astype(F32)
    else:
        for k in ("x", "bias", "res"):
            c[k] = (c[k] * F32(1e-3)).astype(F32)
    w = math == MATH_BF16W
    ref, f32 = CR.enc_o_ln_rule(c, np.float64, 0, w), CR.enc_o_ln_rule(c, F32, 2, w)
    assert np.isfinite(ref).all() and np.isfinite(f32).all()
    y = libs.plain.test_enc_o_ln(c["x"], c["w"], c["bias"], c["res"], c["gamma"], c["beta"], c["in_len"], c["out_len"], math=math)
    tag = f"{kind} {MATH_NAMES[math]}"
    CR.assert_vs_fp64(y, ref, f32, c["out_len"], "k_enc_o_ln", tag)
    note(libs, 5, "k_enc_o_ln", norm_err(y, ref, c["out_len"]), norm_err(f32, ref, c["out_len"]))


# test_dds_stack's impl (and math) per form
STACK_FORMS = {"one launch per piece": (0, None), "launch_dds_layer": (1, None), "k_dds_stack<6>": (2, None), "k_dds_stack_b3<false>": (3, None),
               "k_dds_stack_b3<true>": (3, MATH_BF16W)}
_stack_cases = {}


def stack_profile_case(kind):
    """sdp_ref.stack_case (192 channels, conv pre with cond, three layers, a 192-row proj) on rows(33).  The first LayerNorm reads
    dwconv(pre(src) + cond) + dw_b.  "mean 32, std 1": the first layer's dw_b + 32; "std 1e-3": src, pre_b, cond and the first
    layer's dw_b times 1e-3."""
    if kind not in _stack_cases:
        base = SD.stack_case(192, 33, rows(33), False, True, 0, 3, 192)
        c = dict(base)
        lay0 = dict(base["layers"][0])
        if kind == LN_INNER[0]:
            lay0["dw_b"] = (lay0["dw_b"] + F32(32.0)).astype(F32)
        else:
            lay0["dw_b"] = (lay0["dw_b"] * F32(1e-3)).astype(F32)
            for k in ("src", "pre_b", "cond"):
                c[k] = (c[k] * F32(1e-3)).astype(F32)
        c["layers"] = [lay0] + list(base["layers"][1:])
        c["key"] = base["key"] + (kind,)
        c["ref"] = {False: SD.stack_ref(c, np.float64)}
        c["f32"] = {}
        _stack_cases[kind] = c
    return _stack_cases[kind]


def stack_conditioning(libs, kind):
    """Every stack form on one case: each against fp64 by sdp_ref's criterion, launch_dds_layer and k_dds_stack<6> with equal bits
    (test_stack_forms_give_the_same_bits_on_every_option's rule)."""
    c = stack_profile_case(kind)
    outs = {}
    for name, (impl, math) in STACK_FORMS.items():
        ref, f32 = SD.stack_refs(c, math == MATH_BF16W)
        assert all(np.isfinite(a).all() for a in ref + f32 if a is not None), (name, kind, "the rule or the model is not finite")
        outs[name] = SD.check_stack(libs.plain, impl, c, f"{kind}: {name}", math=math)
        for g, r, m in zip(outs[name][:2], ref[:2], f32[:2]):
            note(libs, 5, name, norm_err(g, r, c["lens"]), norm_err(m, r, c["lens"]))
    SD.assert_same_bits_below_len(outs["launch_dds_layer"], outs["k_dds_stack<6>"], c["lens"], f"{kind}: launch_dds_layer vs k_dds_stack<6>")


DP_SHAPE = (64, 32, 3)


def dp_det_conditioning(libs, kind, math):
    """k_dp_det, whose first LayerNorm reads relu(conv_1(x + cond) + b1).  "mean 32, std 1": b1 + 32; "std 1e-3": x, cond and b1 times 1e-3."""
    lib = libs.plain
    cols, halo, _ = lib.lab_dp_det_plan(*DP_SHAPE, math)
    base = SM.dp_case(*DP_SHAPE, cols, halo, True)
    c, w = dict(base), dict(base["w"])
    if kind == LN_INNER[0]:
        w["b1"] = (w["b1"] + F32(32.0)).astype(F32)
    else:
        w["b1"] = (w["b1"] * F32(1e-3)).astype(F32)
        c["x"], c["cond"] = (c["x"] * F32(1e-3)).astype(F32), (c["cond"] * F32(1e-3)).astype(F32)
    c["w"] = w
    ref, f32 = SM.dp_det_rule(c, np.float64), SM.dp_det_rule(c, F32, SM.DP_GROUP)
    assert np.isfinite(ref).all() and np.isfinite(f32).all()
    got = lib.test_dp_det(c["x"], c["lens"], c["w"], c["cond"], math)
    SM.assert_vs_fp64(got, ref, f32, c["lens"], SM.MATH_NAMES[math], kind)
    note(libs, 5, SM.MATH_NAMES[math], norm_err(got[:, None], ref[:, None], c["lens"]), norm_err(f32[:, None], ref[:, None], c["lens"]))


# ---------------------------------------------------------------------------------------------------- 6: decoder tail
TAIL_FORMS = {"k_conv_post_tanh_dpp": ({}, 0), "k_conv_post_tanh_vec": (dict(MI355VITS_CONV_POST_V1=1), 1), "k_conv_post_tanh": (dict(MI355VITS_CONV_POST_STAGED=1), 2)}
TAIL_L = 2 * 248 + 3  # three tiles of the dpp kernel, the last one ragged; one workgroup of the other two
_tail_case = []


def tail_case():
    """conv_ref.conv_post_case(8, 7, TAIL_L) with row 0 times 64 (|acc| up to some 100: saturated) and row 2 all zeros over its
    length of about L / 2; row 1 as drawn, row 3 the quiet one, row 4 empty.  `pre0` = row 0's fp64 pre-activation."""
    if not _tail_case:
        base = CR.conv_post_case(8, 7, TAIL_L)
        x = base["x"].copy()
        x[0] *= F32(64.0)
        x[2] = 0
        c = dict(x=x, w=base["w"], lens=base["lens"])
        assert c["lens"][2] > 0 and c["lens"][4] == 0
        c["ref"], c["f32"] = CR.conv_post_rule(x, c["w"], c["lens"], np.float64), CR.conv_post_rule(x, c["w"], c["lens"], F32)
        xr = np.where(x[0] >= 0, x[0], x[0] * 0.01).astype(np.float64) * (np.arange(x.shape[2]) < c["lens"][0])[None, :]
        c["pre0"] = CR._conv_row(xr, c["w"], 1, np.float64, 0)[0]
        assert np.isfinite(c["ref"]).all() and np.isfinite(c["f32"]).all() and (np.abs(c["pre0"]) > 20).any()
        _tail_case.append(c)
    return _tail_case[0]


def decoder_tail(libs, name):
    """One conv_post kernel on tail_case: the criterion on every row with a non-zero reference, exact values on the saturated and on
    the zero row, peaks and PCM by conv_ref's rules.  Returns (audio, peaks, pcm)."""
    env, kernel = TAIL_FORMS[name]
    c = tail_case()
    lens = c["lens"]
    B, _, P = c["x"].shape
    with Env(**env):
        audio, peaks, pcm, ran = libs.pick(env).test_conv_post(c["x"], c["w"], lens, None, audio_prior=np.full((B, P), CR.JUNK, F32),
                                                               pcm_prior=np.full((B, P), 12345, np.int16))
    assert ran == kernel, (name, "launch_conv_post_tanh picked kernel", ran)
    live = [int(n) if b != 2 else 0 for b, n in enumerate(lens)]  # (row 2's reference is all zero: no scale; its values are exact, below)
    CR.assert_vs_fp64(audio, c["ref"], c["f32"], live, name, "decoder tail")
    note(libs, 6, name, norm_err(audio[:, None], c["ref"][:, None], live), norm_err(c["f32"][:, None], c["ref"][:, None], live))
    assert np.isfinite(audio).all() and np.all(np.abs(audio) <= 1.0)
    for b, n in enumerate(int(v) for v in lens):
        want = np.abs(audio[b, :n]).max() if n else F32(0.0)
        assert peaks[b].view(np.uint32) == F32(want).view(np.uint32), (name, "peak of row", b, float(peaks[b]), float(want))
    assert np.array_equal(pcm, CR.pcm16_rule(audio, peaks, lens, None)), (name, "pcm differs from the rule on the kernel's own audio")
    # the saturated row: +-1.0f exactly wherever the fp64 pre-activation exceeds 10 (1 - tanh(10) = 4e-9, below half an ulp of 1.0f)
    L0 = int(lens[0])
    sat = np.abs(c["pre0"][:L0]) > 10.0
    assert sat.sum() > L0 // 2, (name, "the saturated row saturates", int(sat.sum()))
    assert np.array_equal(audio[0, :L0][sat].view(np.uint32), np.sign(c["pre0"][:L0][sat]).astype(F32).view(np.uint32)), (name, "tanh is exactly +-1.0f beyond |10|")
    assert peaks[0].view(np.uint32) == F32(1.0).view(np.uint32), (name, "the saturated row's peak is 1.0f", float(peaks[0]))
    assert np.array_equal(pcm[0, :L0][sat], (32767 * np.sign(c["pre0"][:L0][sat])).astype(np.int16)), (name, "pcm is +-32767 where the audio is +-1")
    # the row of zeros: peak +0, audio and pcm all zero
    L2 = int(lens[2])
    assert peaks[2].view(np.uint32) == 0 and np.all(audio[2].view(np.uint32) << 1 == 0) and np.all(pcm[2, :L2] == 0), (name, "the zero row", float(peaks[2]))
    return audio, peaks, pcm


# ---------------------------------------------------------------------------------------------------- bite proof: a split product
def split3(a):
    """The three-term bf16 split of a float32 array: (hi, mid, lo), each a bf16 value as float32."""
    a = np.asarray(a, F32)
    hi = bf16_round(a)
    mid = bf16_round(a - hi)
    return hi, mid, bf16_round(a - hi - mid)


def split_conv(c, keep):
    """conv1d_rule's sum in fp64 over the partial products (i, j) of `keep` — term i of the weights' split times term j of the split
    of the staged input lrelu(x) in float32 — with the rule's epilogue: the kernels' six products are (0,0) (0,1) (1,0) (0,2) (1,1)
    (2,0).  Never a kernel."""
    ws, xs = split3(c["w"]), split3(CR._lrelu(c["x"], c["in_slope"], F32))
    out = None
    for i, j in keep:
        first = out is None
        part = CR.conv1d_rule(CR.derived(c, w=ws[i], x=xs[j], in_slope=1.0, bias=c["bias"] if first else None, res=c["res"] if first else None), np.float64)
        out = part if first else out + part
    return out.astype(F32)


SIX_OF_NINE = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))
FOUR_OF_NINE = SIX_OF_NINE[:4]
