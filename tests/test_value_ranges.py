"""Value-range edges on the CPU model of the kernels: every kernel form of the per-family modules on data off the unit Gaussian that
their case tables draw (tests/range_ref.py holds the profiles, the checks and the numpy models of the bite proofs; the same tables
run on the MI355X in tests/test_gpu_value_ranges.py).  Profiles: 1 power-of-two homogeneity (bit-exact), 2 DC offset with
cancelling weights, 3 gate saturation, 4 peaked and moving softmax maxima, 5 LayerNorm conditioning, 6 the decoder's tail.

form -> profiles (test_zz_every_form_ran_its_profiles compares this table with what ran)
  k_conv1d_generic                              1 2
  k_conv1d_mfma                                 1 2
  k_conv_direct_mfma                            1 2
  k_conv_direct_splitk                          1 2
  k_conv1d_b3                                   1 2
  k_conv1d_b3 chunk-64                          1 2
  k_enc_b3                                      1 2
  k_enc_b3w                                     1 2
  k_rb_conv                                     1 2
  k_rb_conv_pw                                  1 2
  k_conv_transpose1d                            1 2
  polyphase f32 direct                          1 2
  polyphase f32 staged                          1 2
  polyphase k_conv1d_b3                         1 2
  k_conv1d_b3_pc                                1 2
  k_ups_pl                                      1 2
  k_ups64                                       1 2
  k_mrf_fused f32                               1 2
  k_mrf_fused bf16x3                            1 2
  k_mrf_fused<32>                               1 2
  k_mrf_p<32>                                   1 2
  k_mrf_p<64>                                   1 2
  k_mrf_s<64>                                   1 2
  gate conv + res/skip conv                     3
  EPI_GATE conv tile (2,2,2,2)                  3
  EPI_GATE conv tile (2,1,2,2)                  3
  launch_wn_layer H=192                         3
  launch_wn_layer H=192 geometry 0              3
  launch_wn_layer H=192 geometry 1              3
  launch_wn_layer H=192 geometry 2              3
  launch_wn_layer H=32                          3
  k_wn_layer_b3                                 3
  k_wn_layer_b3 32 columns                      3
  k_wn_layer_b3 96 columns, epilogue 0          3
  k_wn_layer_b3 96 columns, epilogue 1          3
  k_wn_layer_b3 128 columns                     3
  k_wn_layer_b3 32x32x16, 32 columns            3
  k_wn_layer_b3 32x32x16, 128 columns           3
  k_rel_attention                               4
  k_rel_attention_mfma4                         4
  k_rel_attention_stream                        4
  k_layernorm<cached>                           5
  k_layernorm<uncached>                         5
  k_enc_o_ln                                    5
  one launch per piece                          5
  launch_dds_layer                              5
  k_dds_stack<6>                                5
  k_dds_stack_b3<false>                         5
  k_dds_stack_b3<true>                          5
  k_dp_det<F32>                                 5
  k_dp_det<split-bf16>                          5
  k_conv_post_tanh_dpp                          6
  k_conv_post_tanh_vec                          6
  k_conv_post_tanh                              6
(k_pcm16 runs behind each conv_post kernel in the one hook call.)

The proofs that the profiles bite, on numpy models and never on a kernel: test_tanh_clamp_at_6_fails_the_gate_profile (with what a
clamp at 8 gives), test_one_pass_variance_fails_the_layernorm_profile, test_skipped_rescale_fails_the_rising_maximum,
test_four_of_nine_partial_products_fail_the_dc_offset."""
import re

import numpy as np
import pytest

from tests import range_ref as R

WHERE = "CPU model"


@pytest.fixture(scope="module")
def libs(emu_lib):
    return R.Libs(emu_lib, emu_lib, WHERE)


# ------------------------------------------------------------------------------------------------ 1: homogeneity
@pytest.mark.parametrize("name", list(R.CONV_FORMS))
def test_homogeneity_conv(libs, name):
    """x, bias and res times 2^20 and 2^-20: the plain run's output times 2^k, bit for bit, in every math mode of the form."""
    R.homogeneity_conv(libs, name)


@pytest.mark.parametrize("name", list(R.CONVT_FORMS))
def test_homogeneity_transposed_conv(libs, name):
    R.homogeneity_convt(libs, name)


@pytest.mark.parametrize("name", list(R.MRF_FORMS))
def test_homogeneity_mrf_stage(libs, name):
    R.homogeneity_mrf(libs, name)


# ------------------------------------------------------------------------------------------------ 2: DC offset
@pytest.mark.parametrize("mu", R.MUS)
@pytest.mark.parametrize("name", list(R.CONV_FORMS))
def test_dc_offset_conv(libs, name, mu):
    """x = mu + N(0, 1) on weights that sum to zero over C_in: products of O(mu), a reference of O(1)."""
    for math in R.CONV_FORMS[name][3]:
        R.dc_conv(libs, name, mu, math)


@pytest.mark.parametrize("mu", R.MUS)
@pytest.mark.parametrize("name", list(R.CONVT_FORMS))
def test_dc_offset_transposed_conv(libs, name, mu):
    R.dc_convt(libs, name, mu)


@pytest.mark.parametrize("name", list(R.MRF_FORMS))
def test_dc_offset_mrf_stage(libs, name):
    """x = 8 + N(0, 1): what leaky ReLU leaves on a decoder activation."""
    R.dc_mrf(libs, name)


# ------------------------------------------------------------------------------------------------ 3: gate saturation
@pytest.mark.parametrize("name", list(R.GATE_FORMS))
def test_gate_saturation(libs, name):
    """Pre-activations on, beside and far beyond wn_gate_f's clamps and around 0, every (tanh, sigmoid) pair of the grid."""
    R.gate_saturation(libs, name)


def test_gate_grid_pairs_every_tanh_value_with_every_sigmoid_value():
    g = R.gate_grid(192)
    assert len({(a, s) for a, s in zip(g[:192], g[192:])}) == len(R.TANH_GRID) * len(R.SIG_GRID) == 165
    g = R.gate_grid(32)
    assert len({(a, s) for a, s in zip(g[:32], g[32:])}) == 32 and set(g[:32]) == set(R.TANH_GRID) and set(g[32:]) == set(R.SIG_GRID)


# ------------------------------------------------------------------------------------------------ 4: softmax maxima
@pytest.mark.parametrize("kind", R.ATTN_KINDS)
@pytest.mark.parametrize("name", list(R.ATTN_FORMS))
def test_softmax_maxima(libs, name, kind):
    R.softmax_maxima(libs, name, kind)


# ------------------------------------------------------------------------------------------------ 5: LayerNorm conditioning
@pytest.mark.parametrize("name", list(R.LN_FORMS))
def test_layernorm_conditioning(libs, name):
    """Every option case of the template, the criterion per column profile."""
    for which in range(len(R.LN_FORMS[name][1])):
        R.ln_conditioning(libs, name, which)


@pytest.mark.parametrize("math", R.B3)
@pytest.mark.parametrize("kind", R.LN_INNER)
def test_enc_o_ln_conditioning(libs, kind, math):
    R.enc_o_ln_conditioning(libs, kind, math)


@pytest.mark.parametrize("kind", R.LN_INNER)
def test_stack_conditioning(libs, kind):
    R.stack_conditioning(libs, kind)


@pytest.mark.parametrize("math", R.SM.MATHS)
@pytest.mark.parametrize("kind", R.LN_INNER)
def test_dp_det_conditioning(libs, kind, math):
    R.dp_det_conditioning(libs, kind, math)


# ------------------------------------------------------------------------------------------------ 6: decoder tail
def test_decoder_tail(libs):
    """A saturated row and a row of zeros through the three conv_post kernels and k_pcm16: exact values, and the three agree bitwise."""
    outs = [R.decoder_tail(libs, name) for name in R.TAIL_FORMS]
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ the proofs that the profiles bite
def test_tanh_clamp_at_6_fails_the_gate_profile():
    """A numpy gate whose tanh argument is clamped at +-6 (1 - tanh(6) = 1.2e-5) fails profile 3 and passes the Gaussian table, where
    no pre-activation reaches 6.  A clamp at +-8 moves a saturated tanh by 1 - tanh(8) = 2.3e-7, two ulps of 1.0f: h' and skip then
    differ from fp64 by 2.8e-7 of their size where the calibration itself differs by 2.5e-7, so no float32-grade criterion on the
    layer's outputs can tell it from tanhf — measured and asserted here, with the clamp at 15 (the kernels') equal to no clamp."""
    for H, T in ((192, 33), (32, 33)):
        sat, gauss = R.gate_case(H, T), R.gate_case(H, T, saturate=False)
        assert not R.gate_passes(sat, R.wn_layer_with_gate(sat, R.gate_clamped(6.0))), (H, "a clamp at 6 passes the saturated grid")
        assert R.gate_passes(gauss, R.wn_layer_with_gate(gauss, R.gate_clamped(6.0))), (H, "a clamp at 6 fails the Gaussian table")
        at8, free = R.wn_layer_with_gate(sat, R.gate_clamped(8.0)), R.wn_layer_with_gate(sat, R.gate_clamped(1e30))
        for name, a, f, r in zip(("h'", "skip"), at8, free, sat["ref"]):
            print(f"gate clamp at 8, H={H} {name}: e = {R.norm_err(a, r, sat['lens']):.3e}  unclamped e32 = {R.norm_err(f, r, sat['lens']):.3e}")
        assert R.gate_passes(sat, at8), (H, "a clamp at 8 is within float32 of tanh: the criterion cannot see it")
        for a, b in zip(R.wn_layer_with_gate(sat, R.gate_clamped(15.0)), free):
            assert np.array_equal(a, b), (H, "tanhf is +-1.0f from 15 on: the kernels' clamp moves no float32 value")


def test_one_pass_variance_fails_the_layernorm_profile():
    """var = E[v^2] - mean^2 in float32 fails the columns of mean +-1000 and passes every whole-row case of the Gaussian table."""
    for C in (192, 300):
        verdict = R.one_pass_passes(R.ln_profile_case(C, {}))
        assert not verdict["mean 1000, std 1"] and not verdict["mean -1000, std 1e-2"], verdict
        assert R.one_pass_passes(R.SM.ln_case(C, 33), columns=False), (C, "one pass fails the Gaussian table")


def test_skipped_rescale_fails_the_rising_maximum():
    """An online softmax over 32-key tiles that leaves its accumulated numerator as it is at a row's last tile — alpha applied to the
    sum only — fails profile 4 "rising", and the intact one passes.  It fails the Gaussian table too (the running maximum of unit
    logits still moves at a late tile in some of a batch's rows: e = 0.2), so only this half of the proof stands; what the profile
    adds is that EVERY row rescales at EVERY tile, by e^-8."""
    impl, T, d, heads, W = R.ATTN_FORMS["k_rel_attention_stream"]
    qkv, ek, ev, ln, ref, f32 = R.attn_case(T, d, heads, W, "rising")
    bound = R.f32_bound(R.norm_err(f32, ref, ln))
    last = (T - 1) // 32
    assert R.norm_err(R.online_softmax(qkv, ek, ev, ln, heads), ref, ln) <= bound
    e = R.norm_err(R.online_softmax(qkv, ek, ev, ln, heads, skip_rescale_at=last), ref, ln)
    print(f"online softmax without the numerator's rescale at tile {last}: e = {e:.3e}  bound = {bound:.3e}")
    assert e > bound


def test_four_of_nine_partial_products_fail_the_dc_offset():
    """A split product that keeps four of the nine partial products (the leading one, both first-order ones and h_w x l_x) fails
    profile 2 at mu = 1024; the six the kernels keep pass."""
    for name in ("k_conv1d_b3", "k_enc_b3"):
        c = R.dc_conv_case(name, 1024.0)
        ref, f32 = R.CR.refs(c, R.CR.GROUP[R.CONV_FORMS[name][0]])
        assert R.CR.passes_vs_fp64(R.split_conv(c, R.SIX_OF_NINE), ref, f32, c["cmp_len"]), name
        assert not R.CR.passes_vs_fp64(R.split_conv(c, R.FOUR_OF_NINE), ref, f32, c["cmp_len"]), name


# ------------------------------------------------------------------------------------------------ the table
def docstring_table(doc):
    """{(form, profile)} of a module docstring's "form -> profiles" table."""
    pairs = set()
    for line in doc.split("form -> profiles", 1)[1].splitlines()[1:]:
        m = re.fullmatch(r"  (\S.*?)\s{2,}((?:\d ?)+)", line.rstrip())
        if not m:
            break
        pairs |= {(m.group(1), int(p)) for p in m.group(2).split()}
    return pairs


def test_zz_every_form_ran_its_profiles(libs):
    """The (form, profile) pairs the tests above ran are the docstring's table, pair for pair; prints the worst e / e32 per profile
    and form (DESIGN.md quotes them)."""
    for (profile, form), ratio in sorted(R.FIGURES.get(libs.where, {}).items()):
        print(f"value ranges worst e / e32 {libs.where}: profile {profile} {form}: {ratio:.3f}")
    want = docstring_table(__doc__)
    assert len(want) == 77, len(want)
    ran = R.RAN.get(libs.where, set())
    assert ran == want, (sorted(ran - want), sorted(want - ran))
