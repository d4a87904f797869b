"""Value-range edges on the MI355X (pytest -m gpu): the profiles and tables of tests/test_value_ranges.py (tests/range_ref.py) on the
device, every hook call made TWICE with equal bits demanded (sdp_ref.Twice, over every hook).  On the CPU model exp, the reciprocal
and tanh are libm's; only here do wn_gate_f's v_exp_f32 / v_rcp_f32, the device's expf in the online softmax, its rsqrt in the
LayerNorms and its tanhf at saturation meet these values.

The forms that a shape, a math mode or `impl=` selects run on the product's objects (`gpu_hooks`, which reads no switch); the forms
behind an MI355VITS_* switch run on the lab build, as in tests/test_gpu_conv_kernels.py and tests/test_gpu_wn_layer.py.  The table
of tests/test_value_ranges.py's docstring is the table of this module: test_zz_every_form_ran_its_profiles compares it with what ran
here.  The bite proofs run on numpy models and stay in the CPU module."""
import pytest

from tests import range_ref as R
from tests import test_value_ranges as C

pytestmark = pytest.mark.gpu
WHERE = "MI355X"


@pytest.fixture(scope="module")
def libs(gpu_hooks, lab_lib):
    return R.Libs(R.Twice(gpu_hooks), R.Twice(lab_lib), WHERE)


test_homogeneity_conv = C.test_homogeneity_conv
test_homogeneity_transposed_conv = C.test_homogeneity_transposed_conv
test_homogeneity_mrf_stage = C.test_homogeneity_mrf_stage


# DESIGN.md 4.7e, "A limit of the resblock conv on the device": measured e / e32 of the four cases on the MI355X (e, e32):
#   k_rb_conv     mu = 32: 3.83 (9.81e-6, 2.56e-6)    mu = 1024: 6.67 (5.18e-4, 7.76e-5)
#   k_rb_conv_pw  mu = 32: 3.29 (1.05e-5, 3.18e-6)    mu = 1024: 4.50 (3.79e-4, 8.42e-5)
# (on the CPU model, which sums an instruction's 32 products in float and rounds once, they pass at 2.2 - 2.9)
RB_CONV_LIMIT = pytest.mark.xfail(strict=True, reason="DESIGN.md 4.7e: v_mfma_f32_16x16x32_bf16 sums its 32 products below float32; on a DC offset "
                                                     "k_rb_conv's one accumulator chain exceeds 3 x the float32 calibration")


@pytest.mark.parametrize("mu", R.MUS)
@pytest.mark.parametrize("name", [pytest.param(n, marks=RB_CONV_LIMIT) if n in ("k_rb_conv", "k_rb_conv_pw") else n for n in R.CONV_FORMS])
def test_dc_offset_conv(libs, name, mu):
    C.test_dc_offset_conv(libs, name, mu)


test_dc_offset_transposed_conv = C.test_dc_offset_transposed_conv
test_dc_offset_mrf_stage = C.test_dc_offset_mrf_stage
test_gate_saturation = C.test_gate_saturation
test_softmax_maxima = C.test_softmax_maxima
test_layernorm_conditioning = C.test_layernorm_conditioning
test_enc_o_ln_conditioning = C.test_enc_o_ln_conditioning
test_stack_conditioning = C.test_stack_conditioning
test_dp_det_conditioning = C.test_dp_det_conditioning
test_decoder_tail = C.test_decoder_tail


def test_zz_every_form_ran_its_profiles(libs):
    for (profile, form), ratio in sorted(R.FIGURES.get(WHERE, {}).items()):
        print(f"value ranges worst e / e32 {WHERE}: profile {profile} {form}: {ratio:.3f}")
    want = C.docstring_table(C.__doc__)
    ran = R.RAN.get(WHERE, set())
    assert ran == want, (sorted(ran - want), sorted(want - ran))
