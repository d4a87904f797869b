"""The stochastic duration predictor's kernels alone, on the CPU model of the kernels, against fp64 per element: the case tables of
tests/sdp_ref.py (tests/test_gpu_sdp_kernels.py runs them on the MI355X).  k_dds_stack<6>, k_dds_stack_b3 in both math modes,
k_dds_layer and the one-launch-per-piece path around every 32-column seam and its 16-column halo, on ragged rows, with junk past
every row's end; k_spline_inverse on and around every knot; k_durations' integers; k_expand_prior.  The fp64 reference itself is
pinned to oracle/vits_oracle.py's modules in double, and the float32 model is calibrated, here only."""
import numpy as np
import pytest

from mimic3_amd._native import NativeError
from tests import sdp_ref as S


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("n", range(len(S.OPTION_CASES)))
def test_fp64_reference_is_the_oracles_modules_in_double(n):
    """A transcription slip in tests/sdp_ref.py must not become the standard: oracle/vits_oracle.py's _dds, _convflow_reverse and
    _spline_inverse in double on the same weights agree to 1e-12 relative (C = 64: 1 / sqrt(C) is the same number in both)."""
    c = S.stack_case(64, S.OPTIONS_T, S.OPTIONS_LENS, *S.OPTION_CASES[n])
    for name, mine, theirs in zip(("x_out", "out", "z"), c["ref"][False], S.oracle_stack(c)):
        if mine is not None:
            err = float(np.abs(mine - theirs).max() / np.abs(theirs).max())
            print(f"sdp reference vs oracle, options {S.OPTION_CASES[n]} {name}: {err:.3e}")
            assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("nb,kind,ch_x0", S.SPLINE_CASES)
def test_fp64_spline_is_the_oracles_in_double(nb, kind, ch_x0):
    import torch
    c = S.spline_case(nb, kind, ch_x0)
    o = S.oracle(nb, 192, 3, 1, {})
    t = torch.from_numpy(c["theta"].astype(np.float64)).permute(0, 2, 1)
    isf = float(c["isf"])
    x1 = torch.from_numpy(c["z"][:, 1 - ch_x0].astype(np.float64))
    theirs = o._spline_inverse(x1, t[..., :nb] * isf, t[..., nb:2 * nb] * isf, t[..., 2 * nb:].clone()).numpy()
    for b, L in enumerate(int(v) for v in c["lens"]):
        if L:
            err = float(np.abs(c["ref"][b, 1 - ch_x0, :L] - theirs[b, :L]).max() / np.abs(theirs[b, :L]).max())
            assert err <= 1e-12, (kind, b, err)


def test_float32_model_is_a_calibration():
    """The float32 model's own error against fp64 lies where float32 arithmetic puts it: a few 2**-24 for the stack, below 1e-4 for
    the spline's worst case (bins at their 1e-3 floor: the root cancels)."""
    c = S.stack_case(192, S.OPTIONS_T, S.OPTIONS_LENS, *S.OPTION_CASES[0])
    ref, f32 = S.stack_refs(c, False)
    for r, m in zip(ref[:2], f32[:2]):
        e32 = S.norm_err(m, r, c["lens"])
        assert 2.0 ** -26 < e32 < 2.0 ** -18, e32
    for nb, kind, ch in S.SPLINE_CASES:
        sc = S.spline_case(nb, kind, ch)
        e32 = S.norm_err(sc["f32"], sc["ref"], sc["lens"])
        print(f"sdp spline float32 model nb={nb} {kind}: e32 = {e32:.3e}")
        # (d30: at a derivative on its 1e-3 floor the inverse has slope 1000: a float32 ulp of a knot, 2**-22 of the range, times 1000)
        assert e32 < (1000 * 2.0 ** -20 if kind == "d30" else 1e-4), (nb, kind, e32)
    assert np.array_equal(S.bf16_round(np.float32([1.0, 1.00390625, 1.01171875, -1.005])), np.float32([1.0, 1.0, 1.015625, -1.0078125]))


# ---------------------------------------------------------------------------------------------------- the stack
@pytest.mark.parametrize("T", S.LENGTH_CLASSES)
def test_stack_length_classes_vs_fp64(emu_lib, T):
    """T around every 32-column tile and its halo; rows ending at 0, 1, T and 16, 13, 1, 0 columns to either side of every seam, in
    ragged batches; k_dds_layer, k_dds_stack<6> and k_dds_stack_b3 each against fp64, the first two with equal bits."""
    for c in S.length_class_cases(T):
        outs = {impl: S.check_stack(emu_lib, impl, c, f"T={T} rows={tuple(c['lens'])}") for impl in S.STACK_IMPLS}
        S.assert_same_bits_below_len(outs[1], outs[2], c["lens"], f"T={T}: launch_dds_layer vs k_dds_stack<6>")


@pytest.mark.parametrize("T", S.IMPL0_LENGTH_CLASSES)
def test_one_launch_per_piece_length_classes_vs_fp64(emu_lib, T):
    for c in S.length_class_cases(T):
        S.check_stack(emu_lib, 0, c, f"T={T} rows={tuple(c['lens'])}")


@pytest.mark.parametrize("impl", [0] + S.STACK_IMPLS)
def test_stack_options_vs_fp64(emu_lib, impl):
    """Both pre forms, cond NULL and given, zch 0 and 1, 1 / 2 / 3 layers, proj of 192, 29, 47 and 1 rows and none: all nine."""
    for c in S.option_cases():
        S.check_stack(emu_lib, impl, c, f"options {c['key'][3:8]}")


def test_stack_forms_give_the_same_bits_on_every_option(emu_lib):
    for c in S.option_cases():
        a, b = S.run_stack(emu_lib, 1, c), S.run_stack(emu_lib, 2, c)
        S.assert_same_bits_below_len(a, b, c["lens"], f"options {c['key'][3:8]}")


def test_bf16w_form_vs_fp64_with_bf16_weights(emu_lib):
    """k_dds_stack_b3<true>, which only the hook reaches: against fp64 over the dense weights rounded to bf16, same criterion."""
    for c in S.option_cases()[:3] + S.length_class_cases(33):
        S.check_stack(emu_lib, 3, c, f"bf16w {c['key'][1:8]}", math=S.MATH_BF16W)


@pytest.mark.parametrize("C", [70, 6])
def test_one_launch_per_piece_other_channel_counts(emu_lib, C):
    """C = 70 (even: the f32-MFMA conv kernel, channels past two 32-row tiles) and C = 6 through the generic pieces."""
    for o in S.OPTION_CASES[:5]:
        proj = min(o[4], C) if o[4] == 192 else o[4]
        c = S.stack_case(C, 33, (33, 32, 19, 1, 0), o[0], o[1], o[2], o[3], proj)
        S.check_stack(emu_lib, 0, c, f"C={C} options {c['key'][3:8]}")


def test_stack_refusals(emu_lib):
    """MI355VITS_ERR_INVALID before any launch: four layers (reach 40 > 16), K = 5 and C = 96 for the stack kernels, 17 bins, a
    parameter count that is not 3 nb - 1, a length out of range, a math mode the path does not run."""
    lens = (20, 7)
    c4 = S.stack_case(192, 20, lens, False, False, 0, 4, 192)
    for impl in (2, 3):
        with pytest.raises(NativeError, match="not supported"):
            S.run_stack(emu_lib, impl, c4)
    S.check_stack(emu_lib, 1, c4, "four layers: launch_dds_layer serves them")
    c5 = S.stack_case(192, 20, lens, False, False, 0, 2, 192, 5)
    c96 = S.stack_case(96, 20, lens, False, False, 0, 2, 96)
    for impl in (2, 3):
        for c in (c5, c96):
            with pytest.raises(NativeError, match="not supported"):
                S.run_stack(emu_lib, impl, c)
    with pytest.raises(NativeError, match="not supported"):
        S.run_stack(emu_lib, 1, c96)
    S.check_stack(emu_lib, 0, c5, "K = 5: the pieces serve it")
    S.check_stack(emu_lib, 0, c96, "C = 96: the pieces serve it")
    c = S.stack_case(192, 20, lens, True, False, 0, 2, 29)
    for impl in (0, 1, 2, 3):
        with pytest.raises(NativeError, match="nb"):
            S.run_stack(emu_lib, impl, dict(c, nb=17))
        with pytest.raises(NativeError, match="3 nb - 1"):
            S.run_stack(emu_lib, impl, dict(c, nb=9))
        with pytest.raises(NativeError, match="len out of range"):
            S.run_stack(emu_lib, impl, dict(c, lens=np.asarray([21, 0], np.int32)))
        with pytest.raises(NativeError, match="len out of range"):
            S.run_stack(emu_lib, impl, dict(c, lens=np.asarray([20, -1], np.int32)))
    for impl, math in ((0, S.MATH_BF16X3), (1, S.MATH_BF16W), (2, S.MATH_BF16X3), (3, S.MATH_F32), (3, 3), (4, S.MATH_F32)):
        with pytest.raises(NativeError):
            S.run_stack(emu_lib, impl, c, math=math)


@pytest.mark.parametrize("impl", [0] + S.STACK_IMPLS)
def test_stack_rows_do_not_depend_on_neighbours(emu_lib, impl):
    """Bit for bit below len[b]: a row alone equals the row inside its ragged batch; T enlarged by 1, 31 and 40 columns changes
    nothing; NaN, infinities and huge finite values in src and z at and past len[b] change nothing, and out / z stay exact zeros there."""
    for c in S.independence_cases():
        base = S.check_stack(emu_lib, impl, c, f"independence {c['key'][3:8]}")
        for b in (1, 3, 5):
            one = S.run_stack(emu_lib, impl, S.single_row(c, b))
            S.assert_same_bits_below_len(one, tuple(None if o is None else o[b:b + 1] for o in base), c["lens"][b:b + 1], f"row {b} alone")
        for extra, fill in ((1, 0.0), (31, S.HUGE), (40, np.nan)):
            wide = S.run_stack(emu_lib, impl, S.widened(c, extra, np.float32(fill)))
            S.assert_same_bits_below_len(wide, base, c["lens"], f"T + {extra}")
        got = S.run_stack(emu_lib, impl, S.poisoned(c, S.POISON))
        S.assert_same_bits_below_len(got, base, c["lens"], "NaN / inf / huge past len[b]")
        for name, g in zip(("out", "z"), got[1:]):
            if g is not None and (name == "out" or c["spline"]):
                for b, L in enumerate(int(n) for n in c["lens"]):
                    assert np.all(g[b][:, L:] == 0.0), (name, "exact zeros at and past len[b]", b)


# ---------------------------------------------------------------------------------------------------- the spline alone
@pytest.mark.parametrize("nb,kind,ch_x0", S.SPLINE_CASES)
def test_spline_on_and_around_every_knot(emu_lib, nb, kind, ch_x0):
    S.check_spline(emu_lib, nb, kind, ch_x0)


def test_spline_refusals(emu_lib):
    c = S.spline_case(16, "s1", 0)
    for nb in (17, 1):
        with pytest.raises(NativeError, match="nb"):
            emu_lib.test_spline_inverse(c["theta"], c["z"], c["lens"], nb)
    with pytest.raises(NativeError, match="len out of range"):
        emu_lib.test_spline_inverse(c["theta"], c["z"], c["lens"] + 1, 16)


# ---------------------------------------------------------------------------------------------------- durations
@pytest.mark.parametrize("T,lens,ls,seed", S.DURATION_CASES)
def test_durations_random(emu_lib, T, lens, ls, seed):
    S.check_durations(emu_lib, T, lens, ls, seed)


def test_durations_forced_cases(emu_lib):
    S.forced_duration_cases(emu_lib)
    with pytest.raises(NativeError, match="len out of range"):
        emu_lib.test_durations(np.zeros((2, 2, 600), np.float32), [601, 1])


# ---------------------------------------------------------------------------------------------------- the length regulator
@pytest.mark.parametrize("I,Ty,frames", S.EXPAND_CASES)
def test_expand_prior(emu_lib, I, Ty, frames):
    S.check_expand(emu_lib, I, Ty, frames)


def test_expand_prior_refusals(emu_lib):
    c = S.expand_case(5, 63, 63)
    with pytest.raises(NativeError, match="injected"):
        emu_lib.test_expand_prior(c["stats"], c["cum"], c["ylen"], 63, noise_scale=c["ns"], injected=None)
    with pytest.raises(NativeError, match="injected_frames"):
        emu_lib.test_expand_prior(c["stats"], c["cum"], c["ylen"], 63, noise_scale=c["ns"], injected=c["inj"][:, :, :62])
    with pytest.raises(NativeError, match="ylen out of range"):
        emu_lib.test_expand_prior(c["stats"], c["cum"], c["ylen"] + 63, 63, noise_scale=c["ns"], injected=c["inj"])


def test_zz_worst_ratios_of_this_run():
    """The worst e / e32 of every stack form over the cases this process ran (DESIGN.md 4.7b quotes them): printed, and within the
    factor.  The spline's, durations' and the length regulator's figures are printed with them; each of their cases asserts its own."""
    print("worst e / e32 per path on the CPU model:", {S.IMPL_NAMES.get(k, k): round(v, 3) for k, v in S.RATIOS.items()})
    forms = {k: v for k, v in S.RATIOS.items() if k in S.IMPL_NAMES}
    assert forms and all(v <= 3.0 for v in forms.values()), forms
