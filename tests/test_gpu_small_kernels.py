"""The text side's small kernels and the Philox noise on the MI355X: the case tables of tests/test_small_kernels.py
(tests/small_ref.py) on the device, every hook call made twice with equal bits demanded (small_ref.Twice).

Two libraries: the tests of tests/test_small_kernels.py themselves run on the LAB build (`lab_lib`), collected here with this
module's `lib`; the PRODUCT's own objects (`gpu_hooks`) run one pass over every kernel of the family — none of them reads a lab
switch, so the two builds must give the same bits.

form -> test: the table of tests/test_small_kernels.py, with
  every kernel of the family in the product's objects, bit for bit the lab build     test_product_objects_give_the_lab_builds_bits
  k_dp_det's largest LDS request (256, 256, 7) on the product's objects              test_product_objects_give_the_lab_builds_bits"""
import numpy as np
import pytest

from tests import small_ref as S
from tests import test_small_kernels as C

pytestmark = pytest.mark.gpu
C_WHERE = "MI355X"


@pytest.fixture(scope="module")
def lib(lab_lib):
    """The lab build with every hook call doubled: what the tests taken from tests/test_small_kernels.py run on."""
    S.ratios_into(C_WHERE)
    return S.Twice(lab_lib)


@pytest.fixture(scope="module")
def hooks(gpu_hooks):
    """The product's objects with every hook call doubled."""
    S.ratios_into(C_WHERE)
    return S.Twice(gpu_hooks)


# ---- the CPU-model module's tests on the device (its tables, its assertions)
test_embed = C.test_embed
test_layernorm_cached = C.test_layernorm_cached
test_layernorm_constant_and_offset_columns = C.test_layernorm_constant_and_offset_columns
test_layernorm_padding = C.test_layernorm_padding
test_layernorm_uncached = C.test_layernorm_uncached
test_layernorm_refusals = C.test_layernorm_refusals
test_dp_det = C.test_dp_det
test_dp_det_plan_and_refusals = C.test_dp_det_plan_and_refusals
test_sdp_noise = C.test_sdp_noise
test_expand_prior_keyed = C.test_expand_prior_keyed
test_engine_draws_are_the_reference_tensors = C.test_engine_draws_are_the_reference_tensors


def test_product_objects_give_the_lab_builds_bits(hooks, lib):
    """One case per kernel on the product's objects: the criterion (the check_* bodies), and the same bits as the lab build."""
    same = lambda a, b, what: np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)
    same(S.check_embed(hooks, 192, 130), S.check_embed(lib, 192, 130), "k_embed")
    for C_, T, opts, who in ((192, 33, S.LN_OPTIONS[-1][1], "k_layernorm<cached>"), (17, 17, S.LN_OPTIONS[10][1], "k_layernorm<cached>"),
                             (300, 33, S.LN_OPTIONS_UNCACHED[-1][1], "k_layernorm<uncached>")):
        c = S.ln_case(C_, T, tuple(opts.items()))
        same(S.check_ln(hooks, c, who, f"product C={C_} T={T}"), S.run_ln(lib, c), who)
    for shape in ((192, 64, 3), (256, 256, 7)):
        for math in S.MATHS:
            S.check_dp_det(hooks, shape, math, True)
            c = S.dp_case(*shape, *hooks.lab_dp_det_plan(*shape, math)[:2], True)
            same(hooks.test_dp_det(c["x"], c["lens"], c["w"], c["cond"], math), lib.test_dp_det(c["x"], c["lens"], c["w"], c["cond"], math), S.MATH_NAMES[math])
    same(S.check_sdp_noise(hooks, 200), S.check_sdp_noise(lib, 200), "k_sdp_noise")
    same(S.check_expand_keyed(hooks, 8, 130), S.check_expand_keyed(lib, 8, 130), "k_expand_prior (keyed)")


def test_zz_worst_ratios_of_this_run(lib):
    """Prints the worst e / e32 per kernel over the tests of this module that ran before it (DESIGN.md quotes the figures)."""
    S.print_ratios(C_WHERE)
