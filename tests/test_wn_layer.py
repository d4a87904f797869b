"""One WaveNet layer of the coupling flow alone, on the CPU model of the kernels, against fp64 per element: the case tables of
tests/wn_ref.py (tests/test_gpu_wn_layer.py runs them on the MI355X).  The two-launch path, launch_wn_layer's four kernels and
k_wn_layer_b3 in its 32-, 96- and 128-column forms with both epilogues, around every tile seam, on ragged rows, and with junk past
every row's end."""
import numpy as np
import pytest

from mimic3_amd._native import MATH_BF16X3, MATH_F32, NativeError
from tests import wn_ref as Wn

PATHS = Wn.PATHS


@pytest.mark.parametrize("T", Wn.LENGTH_CLASSES)
@pytest.mark.parametrize("impl,H", PATHS)
def test_length_classes_vs_fp64(emu_lib, impl, H, T):
    """T around every tile width; rows ending at column 1, a column short of, on and past every seam, and an empty row."""
    Wn.check_vs_fp64(emu_lib, impl, H, T, 5, 1, 2 * H, Wn.case_lengths(T))


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("n,kd", list(enumerate(Wn.KD_CASES)))
def test_kernel_sizes_and_dilations_vs_fp64(emu_lib, impl, n, kd):
    """Every (K, dilation) up to both halo limits; rows ending inside the halo of the next tile.  The options alternate with the case."""
    K, dil = kd
    si, two, cd = Wn.OPTION_CASES[n % len(Wn.OPTION_CASES)]
    Wn.check_vs_fp64(emu_lib, impl, 192, Wn.KD_T, K, dil, 384 if two else 192, Wn.kd_lengths(K, dil), with_cond=cd, skip_init=si)


@pytest.mark.parametrize("impl,H", [(0, 192)] + PATHS)
def test_options_vs_fp64(emu_lib, impl, H):
    """skip_init 0 / 1, Crs = H / 2H, cond NULL / given: all eight."""
    for si, two, cd in Wn.OPTION_CASES:
        Wn.check_vs_fp64(emu_lib, impl, H, 97, 5, 1, 2 * H if two else H, (97, 96, 65, 33, 1, 0), with_cond=cd, skip_init=si)


def test_refusals(emu_lib):
    """One past each halo limit, a channel count or a math mode the path does not serve: MI355VITS_ERR_INVALID before any launch."""
    for K, dil in Wn.KD_REFUSED:
        c = Wn.reference_case(192, 40, K, dil, 384, (40, 7))
        assert np.isfinite(c["ref"][0]).all()
        for impl in (1, 2):
            with pytest.raises(NativeError, match="not supported"):
                Wn.run_case(emu_lib, impl, c)
        Wn.assert_vs_fp64(Wn.run_case(emu_lib, 0, c), c, 0, f"K={K} d={dil}: the two-launch path serves it")
        with pytest.raises(NativeError):
            emu_lib.lab_wn_plan(2, 40, K, dil)
    c = Wn.reference_case(32, 40, 5, 1, 64, (40, 7))
    with pytest.raises(NativeError, match="not supported"):
        Wn.run_case(emu_lib, 2, c)
    c = Wn.reference_case(64, 40, 5, 1, 128, (40, 7))
    with pytest.raises(NativeError, match="not supported"):
        Wn.run_case(emu_lib, 1, c)
    c = Wn.reference_case(192, 40, 5, 1, 384, (40, 7))
    args = (c["h"], c["skip"], c["w_in"], c["b_in"], c["w_rs"], c["b_rs"], c["lens"])
    for impl, math in ((1, MATH_BF16X3), (2, MATH_F32), (2, 2), (2, 3), (0, MATH_BF16X3), (3, MATH_F32)):
        with pytest.raises(NativeError):
            emu_lib.test_wn_layer(*args, impl=impl, math=math)
    with pytest.raises(NativeError, match="len out of range"):
        emu_lib.test_wn_layer(*args[:-1], [41, 0], impl=1)


@pytest.mark.parametrize("impl", [1, 2])
def test_every_form_through_the_lab_switches(emu_lib, impl):
    """k_wn_layer_b3 with 32- / 96- / 128-column tiles and both epilogues of the 96-column form; launch_wn_layer's three geometries."""
    Wn.forms_case(emu_lib, impl)


@pytest.mark.parametrize("T", Wn.FORM_LENGTH_CLASSES)
@pytest.mark.parametrize("impl", [1, 2])
def test_every_form_at_the_small_lengths(emu_lib, impl, T):
    """The wide tiles on tensors narrower than a tile and one column past it, every geometry on rows that are not 16-byte aligned."""
    Wn.forms_at_length(emu_lib, impl, T)


def test_two_launch_path_with_an_odd_channel_count(emu_lib):
    """H = 7: neither conv fits the MFMA kernel (it needs an even Cin), both run the generic one."""
    for two in (True, False):
        Wn.check_vs_fp64(emu_lib, 0, 7, 45, 3, 2, 14 if two else 7, (45, 44, 33, 1, 0), with_cond=two, skip_init=not two)


@pytest.mark.parametrize("K,dil", [(3, 4)] + Wn.KD_PAST_128)
def test_128_column_form_and_its_halo_limit(emu_lib, K, dil):
    """(3, 4) is the widest layer the 128-column form takes; one past it the launcher serves the 96-column form (forms_case asserts
    what the plan call reports for each forced width)."""
    Wn.forms_case(emu_lib, 2, K, dil)


def test_the_three_paths_agree(emu_lib):
    Wn.agree_case(emu_lib)


@pytest.mark.parametrize("two,skip_init", [(True, False), (True, True), (False, False)])
@pytest.mark.parametrize("impl", [0, 1, 2])
def test_rows_do_not_depend_on_padding(emu_lib, impl, two, skip_init):
    tiles = []
    for env in (Wn.B3_FORMS if impl == 2 else Wn.F32_FORMS[:1]):
        with Wn.Env(**env):
            tiles.append(Wn.padding_case(emu_lib, impl, two=two, skip_init=skip_init))
    assert impl != 2 or tiles == Wn.B3_FORM_TILES


def test_zz_worst_ratios_of_this_run():
    """The worst e / e32 of every path over the cases this process ran (DESIGN.md 4.7a quotes them): printed, and within the factor."""
    print("worst e / e32 per impl on the CPU model:", {k: round(v, 3) for k, v in sorted(Wn.RATIOS.items())})
    assert all(v <= 3.0 for v in Wn.RATIOS.values()), Wn.RATIOS
