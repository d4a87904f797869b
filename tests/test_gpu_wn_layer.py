"""One WaveNet layer of the coupling flow alone on the MI355X (pytest -m gpu), against fp64 per element: the case tables of
tests/wn_ref.py that tests/test_wn_layer.py runs on the CPU model.  Every hook call here is made TWICE and must return equal bits:
the kernels reuse LDS across barriers (the h tile becomes the u tile), and only the device can show a race.  The product's own
kernels run through the hooks library (the forms its grid rule picks); every form is forced through the lab library's switches."""
import numpy as np
import pytest

from mimic3_amd._native import MATH_BF16X3, MATH_F32, NativeError
from tests import wn_ref as Wn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twice(gpu_hooks):
    return Wn.Twice(gpu_hooks)


@pytest.fixture(scope="module")
def twice_lab(lab_lib):
    return Wn.Twice(lab_lib)


@pytest.mark.parametrize("T", Wn.LENGTH_CLASSES)
@pytest.mark.parametrize("impl,H", Wn.PATHS)
def test_length_classes_vs_fp64(twice, impl, H, T):
    Wn.check_vs_fp64(twice, impl, H, T, 5, 1, 2 * H, Wn.case_lengths(T))


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("n,kd", list(enumerate(Wn.KD_CASES)))
def test_kernel_sizes_and_dilations_vs_fp64(twice, impl, n, kd):
    K, dil = kd
    si, two, cd = Wn.OPTION_CASES[n % len(Wn.OPTION_CASES)]
    Wn.check_vs_fp64(twice, impl, 192, Wn.KD_T, K, dil, 384 if two else 192, Wn.kd_lengths(K, dil), with_cond=cd, skip_init=si)


@pytest.mark.parametrize("impl,H", [(0, 192)] + Wn.PATHS)
def test_options_vs_fp64(twice, impl, H):
    for si, two, cd in Wn.OPTION_CASES:
        Wn.check_vs_fp64(twice, impl, H, 97, 5, 1, 2 * H if two else H, (97, 96, 65, 33, 1, 0), with_cond=cd, skip_init=si)


def test_refusals(gpu_hooks):
    for K, dil in Wn.KD_REFUSED:
        c = Wn.reference_case(192, 40, K, dil, 384, (40, 7))
        for impl in (1, 2):
            with pytest.raises(NativeError, match="not supported"):
                Wn.run_case(gpu_hooks, impl, c)
    c = Wn.reference_case(192, 40, 5, 1, 384, (40, 7))
    args = (c["h"], c["skip"], c["w_in"], c["b_in"], c["w_rs"], c["b_rs"], c["lens"])
    for impl, math in ((1, MATH_BF16X3), (2, MATH_F32), (2, 2), (2, 3)):
        with pytest.raises(NativeError):
            gpu_hooks.test_wn_layer(*args, impl=impl, math=math)


@pytest.mark.parametrize("impl", [1, 2])
def test_every_form_through_the_lab_switches(twice_lab, impl):
    Wn.forms_case(twice_lab, impl)


@pytest.mark.parametrize("T", Wn.FORM_LENGTH_CLASSES)
@pytest.mark.parametrize("impl", [1, 2])
def test_every_form_at_the_small_lengths(twice_lab, impl, T):
    Wn.forms_at_length(twice_lab, impl, T)


def test_two_launch_path_with_an_odd_channel_count(twice):
    for two in (True, False):
        Wn.check_vs_fp64(twice, 0, 7, 45, 3, 2, 14 if two else 7, (45, 44, 33, 1, 0), with_cond=two, skip_init=not two)


@pytest.mark.parametrize("K,dil", [(3, 4)] + Wn.KD_PAST_128)
def test_128_column_form_and_its_halo_limit(twice_lab, K, dil):
    Wn.forms_case(twice_lab, 2, K, dil)


@pytest.mark.parametrize("want", [96, 128])
def test_product_grid_reaches_the_wide_tiles(twice, want):
    """The hooks library runs the product's launcher: a few rows x 3,200 columns reach the 96- and the 128-column form of
    k_wn_layer_b3 by its grid rule (the plan call says at which batch), with the bits of the 32-column form."""
    Wn.grid_case(twice, 2, want)


@pytest.mark.parametrize("want", [1, 0])
def test_product_grid_reaches_every_f32_geometry(twice, want):
    Wn.grid_case(twice, 1, want)


def test_the_three_paths_agree(twice):
    Wn.agree_case(twice)


@pytest.mark.parametrize("two,skip_init", [(True, False), (True, True), (False, False)])
@pytest.mark.parametrize("impl", [0, 1, 2])
def test_rows_do_not_depend_on_padding(twice_lab, twice, impl, two, skip_init):
    assert Wn.padding_case(twice, impl, two=two, skip_init=skip_init) == 32  # the product's small-grid form
    tiles = []
    for env in (Wn.B3_FORMS if impl == 2 else Wn.F32_FORMS if impl == 1 else []):
        with Wn.Env(**env):
            tiles.append(Wn.padding_case(twice_lab, impl, two=two, skip_init=skip_init))
    assert impl != 2 or tiles == Wn.B3_FORM_TILES


def test_zz_worst_ratios_of_this_run():
    print("worst e / e32 per impl on the device:", {k: round(v, 3) for k, v in sorted(Wn.RATIOS.items())})
    assert all(v <= 3.0 for v in Wn.RATIOS.values()), Wn.RATIOS
