"""The convolution family and the decoder's tail on the MI355X: the case tables of tests/test_conv_kernels.py (tests/conv_ref.py) on
the device, every hook call made twice with equal bits demanded (conv_ref.Twice).

Two libraries: the LAB build (`lab_lib`), where the launchers read the lab switches at every launch, walks every form — those are
the tests of tests/test_conv_kernels.py themselves, collected here with this module's `lib`; the PRODUCT's own objects
(`gpu_hooks`, no switch is read) run what the product's rules pick: the forms the shapes alone select, and — test_grid_rule_* —
the forms only a full grid selects, found through the plan call at the smallest batch that reaches them.

form -> test: the table of tests/test_conv_kernels.py, with
  (2,2,2,2) staged tile by the product's fill rule     test_grid_rule_staged_tile
  k_enc_b3w by the product's grid rule                 test_grid_rule_enc_wide
  k_rb_conv_pw by the product's grid rule              test_grid_rule_rb_conv_pw
  wide k_ups_pl by the product's grid rule             test_grid_rule_ups_wide
  k_conv1d_b3_pc on fewer items than CUs and on more   test_convt_split_bf16_pc_on_the_device"""
import pytest

from tests import conv_ref as R
from tests import test_conv_kernels as C
from tests.conv_ref import CONVK_ENC_B3, CONVK_F32_DIRECT, CONVK_F32_SPLITK, CONVK_F32_STAGED, MATH_BF16W, MATH_BF16X3

pytestmark = pytest.mark.gpu
C_WHERE = "MI355X"
MATHS = C.MATHS
VOL = C.VOL


@pytest.fixture(scope="module")
def lib(lab_lib):
    """The lab build with every hook call doubled: what the tests taken from tests/test_conv_kernels.py run on."""
    R.ratios_into(C_WHERE)
    return R.Twice(lab_lib)


@pytest.fixture(scope="module")
def hooks(gpu_hooks):
    """The product's objects with every hook call doubled."""
    R.ratios_into(C_WHERE)
    return R.Twice(gpu_hooks)


# ---- the lab build walks every form: the CPU-model module's tests on the device (its tables, its assertions)
test_plan_reports_the_kernel_of_every_family = C.test_plan_reports_the_kernel_of_every_family
test_refusals = C.test_refusals
test_f32_staged_tiles = C.test_f32_staged_tiles
test_f32_direct = C.test_f32_direct
test_f32_splitk = C.test_f32_splitk
test_f32_chunk_and_ring_variants = C.test_f32_chunk_and_ring_variants
test_f32_forced_chunk = C.test_f32_forced_chunk
test_f32_vec_and_ovec_branches = C.test_f32_vec_and_ovec_branches
test_options_on_every_impl = C.test_options_on_every_impl
test_b3_tiles = C.test_b3_tiles
test_b3_chunk64 = C.test_b3_chunk64
test_enc_rowloop_forms = C.test_enc_rowloop_forms
test_enc_wide_forms = C.test_enc_wide_forms
test_enc_slices_and_lengths = C.test_enc_slices_and_lengths
test_rbc_forms = C.test_rbc_forms
test_padding_rbc = C.test_padding_rbc
test_padding_conv1d = C.test_padding_conv1d
test_convt_generic_and_f32 = C.test_convt_generic_and_f32
test_convt_f32_staged_direct_lds = C.test_convt_f32_staged_direct_lds
test_ups_forms = C.test_ups_forms
test_enc_o_ln = C.test_enc_o_ln
test_conv_post_dpp = C.test_conv_post_dpp
test_conv_post_vec = C.test_conv_post_vec
test_conv_post_staged = C.test_conv_post_staged
test_conv_post_kernels_agree = C.test_conv_post_kernels_agree
test_wn_two_launch_path_under_forced_tiles = C.test_wn_two_launch_path_under_forced_tiles


def test_convt_split_bf16_pc_on_the_device(lib):
    """k_conv1d_b3_pc against the one-tile-per-workgroup kernel on 110 items (fewer than the CUs) and on 264 (several items per
    workgroup on a 256-CU device): the same bits, the plan call reporting the persistent grid.
    The second case is the one tensor of this module well past a million floats, and cannot be smaller: the persistent grid is one
    workgroup per CU, so a workgroup takes a second item only past 256 items, and from 96 items on the launcher's tile is 128 output
    rows x 192 columns: 257 items are 6.3M outputs at any split into rows and columns (24 rows x 2,000 positions: 264 items, 6.1M)."""
    assert R.convt_pc_case(lib, 5, 2000) == 110
    assert R.convt_pc_case(lib, 24, 2000) == 264


# ---- the product's objects: what its own rules pick
@pytest.mark.parametrize("opts", R.OPTION_CASES, ids=lambda o: "+".join(k for k, _ in o) or "plain")
def test_product_options_on_every_impl(hooks, opts):
    """test_options_on_every_impl without its lab switch: generic, staged / direct / split-k f32, split-bf16 staged, k_enc_b3."""
    T = 133
    lens = R.class_lengths(T, 64, 2)
    c = R.conv_case(32, 70, 5, 1, T, lens, opts)
    R.check_conv(hooks, 0, c, f"product {opts}")
    assert R.plan_of(hooks, 1, c).kernel == CONVK_F32_STAGED
    R.check_conv(hooks, 1, c, f"product staged {opts}", who="k_conv1d_mfma")
    for math in MATHS:
        R.check_conv(hooks, 2, c, f"product {opts}", math, fixed_rule=True)
    c = R.conv_case(64, 70, 1, 1, T, lens, opts)
    assert R.plan_of(hooks, 1, c).kernel == CONVK_F32_DIRECT
    R.check_conv(hooks, 1, c, f"product direct {opts}", who="k_conv_direct_mfma")
    c = R.conv_case(1024, 40, 1, 1, 37, (37, 36, 0), opts)
    assert R.plan_of(hooks, 1, c).kernel == CONVK_F32_SPLITK
    R.check_conv(hooks, 1, c, f"product split-k {opts}", who="k_conv_direct_splitk")
    c = R.conv_case(192, 96, 3, 1, 70, R.enc_lengths(70), opts)
    for math in MATHS:
        assert R.plan_of(hooks, 3, c, math).kernel == CONVK_ENC_B3
        R.check_conv(hooks, 3, c, f"product {opts}", math, who="k_enc_b3")


@pytest.mark.parametrize("math", MATHS)
def test_product_b3_tiles(hooks, math):
    """The three EPI_STD tiles of the split-bf16 staged kernel are picked by the grid alone: the product's objects reach them."""
    R.b3_tiles_case(hooks, math)


def test_product_padding_and_tail(hooks):
    """The padding contract, k_enc_o_ln and the three conv_post kernels (each picked by the shape: K = 7 aligned, K = 5 aligned, an
    odd pitch) on the product's objects."""
    opts = (("res", True), ("in_slope", 0.1))
    c = R.conv_case(32, 70, 5, 1, 133, R.class_lengths(133, 64, 2), opts)
    for impl, kw in ((0, {}), (1, {}), (2, dict(math=MATH_BF16X3, fixed_rule=True)), (2, dict(math=MATH_BF16W, fixed_rule=True))):
        R.conv_padding_case(hooks, impl, c, **kw)
        for name, more in R.WHOLE_RANGE_OPTS:
            R.conv_whole_range_case(hooks, impl, R.conv_case(32, 70, 5, 1, 133, R.class_lengths(133, 64, 2), opts + more), "product " + name, **kw)
    ce = R.conv_case(192, 96, 3, 1, 130, R.enc_lengths(130), opts)
    for math in MATHS:
        R.conv_padding_case(hooks, 3, ce, math=math)
        for name, more in R.WHOLE_RANGE_OPTS:
            R.conv_whole_range_case(hooks, 3, R.conv_case(192, 96, 3, 1, 130, R.enc_lengths(130), opts + more), "product " + name, math=math)
        R.enc_o_ln_check(hooks, 33, math)
    for kd in ((7, 12), (3, 1)):
        R.rbc_padding_case(hooks, kd, 0, True)
    R.check_conv_post(hooks, R.conv_post_case(32, 7, 1985), 0, "product dpp", VOL)
    R.check_conv_post(hooks, R.conv_post_case(4, 5, 2049), 1, "product vec", VOL)
    R.check_conv_post(hooks, R.conv_post_case(4, 7, 1025, pitch4=False), 2, "product staged", VOL)


def test_grid_rule_staged_tile(hooks):
    """The (2,2,2,2) tile of the staged f32 kernel by the product's fill rule, at C_in = 32 (the smallest tensors that reach it).
    y passes a million floats here and cannot be smaller: the rule takes the tile once its 128 x 128 workgroups fill most of the
    256 CUs, which is some 3M outputs however they are split into rows and columns (x, at C_in = 32, is a quarter of that)."""
    B = R.grid_rule_case(hooks, 1, (32, 128, 7, 3), 512, CONVK_F32_STAGED, (2, 2, 2, 2))
    print("(2,2,2,2) staged tile from", B, "rows x 512")


def test_grid_rule_enc_wide(hooks):
    B = R.grid_rule_case(hooks, 3, (192, 192, 3, 1), 9, R.CONVK_ENC_B3W6)
    print("k_enc_b3w from", B, "rows x 9")


def test_grid_rule_rb_conv_pw(hooks):
    B = R.grid_rule_case(hooks, 4, (128, 128, 7, 3), 9, R.CONVK_RB_CONV_PW)
    print("k_rb_conv_pw from", B, "rows x 9")


def test_grid_rule_ups_wide(hooks):
    """The 128-position items of k_ups_pl<128> by the product's grid rule."""
    B = R.grid_rule_case(hooks, 3, (128, 64, 16, 8), 5, R.CONVK_UPS_PL, want_cols=128, transposed=True)
    print("wide k_ups_pl items from", B, "rows x 5")


def test_zz_worst_ratios_of_this_run(lib):
    """Prints the worst e / e32 per kernel over the tests of this module that ran before it (DESIGN.md quotes the figures)."""
    R.print_ratios(C_WHERE)
