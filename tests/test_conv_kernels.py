"""The convolution family and the decoder's tail on the CPU model of the kernels: every kernel form the launchers can pick, run alone
through the lab hooks, against fp64 per element (tests/conv_ref.py holds the rules, the criterion and the case tables; the same
tables run on the MI355X in tests/test_gpu_conv_kernels.py).

form -> test
  k_conv1d_generic                                   test_options_on_every_impl, test_padding_conv1d
  k_conv1d_mfma, five tiles, staged                  test_f32_staged_tiles
  k_conv1d_mfma chunk 64 / ring / plain loop         test_f32_chunk_and_ring_variants, test_f32_forced_chunk
  k_conv1d_mfma vec / yvec / ovec                    test_f32_vec_and_ovec_branches
  k_conv_direct_mfma                                 test_f32_direct
  k_conv_direct_splitk                               test_f32_splitk
  k_conv1d_b3, three tiles, BF16X3 / BF16W           test_b3_tiles
  k_conv1d_b3 64-channel chunks, k_conv1d_b3_pc      test_b3_chunk64, test_convt_split_bf16_pc_and_staged
  k_enc_b3 rb_loop 1 / 2 / 3 / 4 / 6                 test_enc_rowloop_forms
  k_enc_b3w eight / six row tiles                    test_enc_wide_forms, test_enc_slices_and_lengths
  k_rb_conv / k_rb_conv_pw                           test_rbc_forms, test_padding_rbc
  k_conv_transpose1d                                 test_convt_generic_and_f32
  polyphase on the f32 kernels (staged / direct)     test_convt_generic_and_f32, test_convt_f32_staged_direct_lds
  k_ups_pl / k_ups64                                 test_ups_forms
  k_enc_o_ln                                         test_enc_o_ln
  k_conv_post_tanh_dpp / _vec / k_conv_post_tanh,
  the row peak, k_pcm16                              test_conv_post_dpp, test_conv_post_vec, test_conv_post_staged, test_conv_post_kernels_agree
  two-launch WaveNet path under forced tiles         test_wn_two_launch_path_under_forced_tiles
and test_dropped_partial_product_fails_the_criterion_and_passes_the_old_threshold is the proof that the criterion bites."""
import numpy as np
import pytest

from tests import conv_ref as R
from tests import wn_ref
from tests.conv_ref import (CONVK_B3_PC, CONVK_B3_STAGED32, CONVK_B3_STAGED64, CONVK_CONVT_GENERIC, CONVK_ENC_B3, CONVK_F32_DIRECT,
                            CONVK_F32_SPLITK, CONVK_F32_STAGED, CONVK_GENERIC, CONVK_UPS64, CONVK_UPS_PL, MATH_BF16W, MATH_BF16X3, MATH_F32,
                            Env, NativeError)

WHERE = "CPU model"


@pytest.fixture(scope="module")
def lib(emu_lib):
    R.ratios_into(WHERE)
    return emu_lib


@pytest.fixture
def cu_count(emu_lib):
    """Sets the compute units the CPU model reports; restores the default afterwards."""
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(0)


MATHS = [MATH_BF16X3, MATH_BF16W]
NARROW = dict(MI355VITS_ENC_WIDE=0, MI355VITS_ENC_ROWLOOP=1)  # k_enc_b3, one row block per workgroup (the CPU model's eight CUs would loop)


# ------------------------------------------------------------------------------------------------ the plan call
def test_plan_reports_the_kernel_of_every_family(lib):
    """One shape per kernel of mi355vits_lab_conv_plan's list, no kernel runs: the kernel, the work item, the chunk."""
    P = lib.lab_conv_plan
    p = P(0, 2, 7, 5, 100, 3)
    assert (p.kernel, p.cols, p.rows) == (CONVK_GENERIC, 64, 32) and list(p.grid) == [2, 1, 2]
    assert P(1, 2, 32, 128, 600, 7, 3).kernel == CONVK_F32_STAGED
    assert P(1, 2, 64, 128, 600, 1).kernel == CONVK_F32_DIRECT
    assert P(1, 2, 768, 192, 512, 3).kernel == CONVK_F32_SPLITK and P(1, 2, 768, 192, 513, 3).kernel == CONVK_F32_STAGED
    assert P(1, 2, 512, 64, 100, 1).kernel == CONVK_F32_DIRECT  # 256 k-steps: below split-k's 512
    assert P(1, 2, 16, 32, 512, 3).kernel == CONVK_F32_DIRECT and P(1, 2, 16, 32, 513, 3).kernel == CONVK_F32_STAGED
    assert P(1, 2, 16, 32, 512, 3, fixed_rule=True).kernel == CONVK_F32_STAGED
    p = P(2, 2, 64, 128, 600, 3)
    assert (p.kernel, p.chunk, p.tile) == (CONVK_B3_STAGED32, 32, (1, 2, 1, 4))
    assert P(2, 2, 64, 128, 600, 2).kernel == CONVK_B3_STAGED64 and P(2, 2, 64, 128, 600, 2).chunk == 64
    assert P(2, 2, 96, 128, 600, 2).kernel == CONVK_B3_STAGED32
    p = P(3, 2, 192, 192, 100, 3)
    assert (p.kernel, p.cols, p.rows, p.rb_loop, p.chunk) == (CONVK_ENC_B3, 64, 64, 1, 192)
    assert P(3, 2, 96, 192, 100, 1).chunk == 96
    p = P(4, 2, 128, 128, 100, 7, 3, has_res=True, lengths=[100, 0])
    assert (p.kernel, p.cols, p.rows) == (R.CONVK_RB_CONV, 32, 128) and p.grid[0] == 4
    p = P(0, 2, 6, 3, 50, 4, stride=2)
    assert (p.kernel, p.cols) == (CONVK_CONVT_GENERIC, 64) and list(p.grid) == [2, 1, 2]
    assert P(1, 2, 64, 32, 50, 8, stride=4).kernel == CONVK_F32_DIRECT
    assert P(1, 2, 128, 64, 50, 16, stride=8).kernel == CONVK_F32_STAGED
    assert P(2, 3, 64, 32, 2000, 8, stride=4).kernel == CONVK_B3_STAGED64  # (a 256-column tile's two staging buffers do not fit: small grids stay one tile per workgroup)
    p = P(2, 5, 64, 32, 2000, 8, stride=4)
    assert p.kernel == CONVK_B3_PC and p.chunk == 64 and list(p.grid)[1:] == [1, 1]
    assert P(3, 2, 128, 64, 50, 16, stride=8, lengths=[50, 50]).kernel == CONVK_UPS_PL
    p = P(3, 2, 64, 32, 50, 8, stride=4, lengths=[50, 0])
    assert (p.kernel, p.cols, p.grid[0]) == (CONVK_UPS64, 31, 2)


def test_case_tables_hold_every_seam():
    """The rows of a length-class case end one short of, on and one past EACH seam of every tile width that runs it, and within the
    halo to either side of each; the full row comes first, and no tensor of the widest case passes a million floats."""
    for T, cols, halo in ((257, 128, 9), (260, (64, 128), 9), (133, 64, 2), (129, 64, 2), (513, (128, 256), 9)):
        lens = R.class_lengths(T, cols, halo)
        assert lens[0] == T and len(set(lens)) == len(lens) and {0, 1} <= set(lens)
        for width in ((cols,) if isinstance(cols, int) else cols):
            for m in range(width, T + 1, width):
                assert {n for n in (m - 1, m, m + 1, m - halo, m + halo) if n <= T} <= set(lens), (T, width, m, lens)
    assert {255, 256, 247} <= set(R.class_lengths(257, 128, 9))  # T = 2 cols + 1: one short of and on the second seam, and in its halo
    for shape in R.STAGED_SHAPES:
        Cin, Cout, K, dil = shape
        widths = sorted({R.tile_cols(t) for t in R.f32_tiles(Cout)})
        rows = len(R.class_lengths(2 * 128 + 4, widths, (K - 1) // 2 * dil))
        assert rows * max(Cin, Cout) * (2 * 128 + 4) < 1 << 20, (shape, rows)
    assert R.last_seam_lengths(100, 32) == (100, 0, 1, 95, 96, 97) and R.last_seam_lengths(32, 32) == (32, 0, 1, 31)


def test_refusals(lib):
    """A shape, math mode or option the chosen kernel does not serve: NativeError before any launch (hook and plan call alike)."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 32, 40)).astype(np.float32)
    w = rng.standard_normal((32, 32, 3)).astype(np.float32)
    bad = [dict(impl=5), dict(impl=-1), dict(impl=0, math=MATH_BF16X3), dict(impl=1, math=MATH_BF16W), dict(impl=2, math=MATH_F32, fixed_rule=True),
           dict(impl=2), dict(impl=3, math=MATH_F32), dict(impl=3), dict(impl=4), dict(impl=4, math=MATH_BF16W), dict(impl=0, fixed_rule=True),
           dict(impl=3, fixed_rule=True), dict(impl=1, in_len=[41]), dict(impl=1, out_len=[-1])]
    for kw in bad:
        with pytest.raises(NativeError):
            lib.test_conv1d(x, w, **kw)
    lib.test_conv1d(x, w, impl=2, fixed_rule=True)  # (the flow's rule serves T <= 512)
    with pytest.raises(NativeError):
        lib.test_conv1d(x[:, :31], w[:, :31], impl=1)  # odd Cin
    x4 = rng.standard_normal((1, 128, 40)).astype(np.float32)
    w4 = rng.standard_normal((128, 128, 3)).astype(np.float32)
    ok = dict(impl=4, res=x4, in_len=[40])
    lib.test_conv1d(x4, w4, **ok)
    for kw in (dict(relu=True), dict(res_sub=True), dict(mask_before_res=True), dict(out_len=[40]), dict(cond=np.zeros((1, 128), np.float32)), dict(dilation=3)):
        with pytest.raises(NativeError):
            lib.test_conv1d(x4, w4, **dict(ok, **kw))
    xs = rng.standard_normal((1, 384, 20)).astype(np.float32)
    ws = rng.standard_normal((64, 384, 1)).astype(np.float32)
    lib.test_conv1d(xs, ws, impl=3)
    for kw in (dict(bias=np.zeros(64, np.float32)), dict(out_scale=0.5), dict(cond=np.zeros((1, 64), np.float32)), dict(out_len=[20]), dict(relu=True)):
        with pytest.raises(NativeError):
            lib.test_conv1d(xs, ws, impl=3, **kw)
    with pytest.raises(NativeError):
        lib.test_conv1d(xs, rng.standard_normal((64, 384, 5)).astype(np.float32), impl=3)
    xt = rng.standard_normal((1, 6, 9)).astype(np.float32)
    wt = rng.standard_normal((6, 3, 4)).astype(np.float32)
    for kw in (dict(impl=4), dict(impl=3), dict(impl=2), dict(impl=0, in_len=[9])):
        with pytest.raises(NativeError):
            lib.test_conv_transpose1d(xt, wt, None, 2, **kw)
    with pytest.raises(NativeError):
        lib.test_conv_transpose1d(xt, wt[:, :, :3], None, 2)  # K - stride odd
    with pytest.raises(NativeError):
        lib.lab_conv_plan(2, 1, 32, 32, 40, 3)
    with pytest.raises(NativeError):
        lib.lab_conv_plan(3, 1, 100, 32, 40, 3)
    c = R.enc_o_ln_case(1)
    with pytest.raises(NativeError):
        lib.test_enc_o_ln(c["x"], c["w"], c["bias"], c["res"], c["gamma"], c["beta"], math=MATH_F32)
    cp = R.conv_post_case(4, 7, 1)
    with pytest.raises(NativeError):
        lib.test_conv_post(cp["x"], cp["w"][:, :, :6], cp["lens"])  # even K
    with pytest.raises(NativeError):
        lib.test_conv_post(cp["x"], cp["w"], cp["lens"] + 5)


# ------------------------------------------------------------------------------------------------ f32 MFMA conv (impl 1)
@pytest.mark.parametrize("shape", R.STAGED_SHAPES)
def test_f32_staged_tiles(lib, shape):
    """Every tile MI355VITS_CONV_CFG can force, at every length class of the tiles' widths (32 - 128 columns)."""
    for T in sorted(set(R.length_classes(64) + R.length_classes(128) + [31, 32, 33])):
        plans = R.f32_tiles_case(lib, shape, T)
        assert all(p.kernel == CONVK_F32_STAGED and p.chunk == 32 and p.ring == 0 for p in plans.values()), (shape, T)


@pytest.mark.parametrize("shape", R.DIRECT_SHAPES)
def test_f32_direct(lib, shape):
    for T in (1, 31, 32, 33, 37, 65, 132) + ((257,) if shape[0] <= 64 else ()):  # (C_in = 512: x stays below a million floats)
        plans = R.f32_tiles_case(lib, shape, T, (("res", True), ("in_slope", 0.1)))
        assert all(p.kernel == CONVK_F32_DIRECT for p in plans.values()), (shape, T)


@pytest.mark.parametrize("shape", R.SPLITK_SHAPES)
def test_f32_splitk(lib, shape):
    Cin, Cout, K, dil = shape
    for T in (1, 31, 32, 33, 65, 100):
        c = R.conv_case(Cin, Cout, K, dil, T, R.last_seam_lengths(T, 32), (("res", True),))
        p = R.plan_of(lib, 1, c)
        assert (p.kernel, p.cols, p.rows) == (CONVK_F32_SPLITK, 32, 32), (shape, T, p.kernel)
        R.check_conv(lib, 1, c, f"{shape} T={T}", who="k_conv_direct_splitk")


@pytest.mark.parametrize("Cin", sorted(R.CHUNK_RING))
def test_f32_chunk_and_ring_variants(lib, Cin):
    """The three instantiations of the staged kernel's weight ring, picked by the chunk that C_in gives."""
    for T in (37, 132):
        plans = R.f32_tiles_case(lib, (Cin, 64, 5, 1), T)
        assert all(p.kernel == CONVK_F32_STAGED and (p.chunk, p.ring) == R.CHUNK_RING[Cin] for p in plans.values()), (Cin, [(p.chunk, p.ring) for p in plans.values()])


@pytest.mark.parametrize("chunk", sorted(R.FORCED_CHUNKS))
def test_f32_forced_chunk(lib, chunk):
    """MI355VITS_CONV_CHUNK on C_in = 128 (four / sixteen chunks per tile instead of two); MI355VITS_CONV_LDS_KB shrinks it likewise."""
    with Env(MI355VITS_CONV_CHUNK=chunk):
        plans = R.f32_tiles_case(lib, (128, 64, 5, 1), 133)
    assert all((p.chunk, p.ring) == R.FORCED_CHUNKS[chunk] for p in plans.values())
    with Env(MI355VITS_CONV_LDS_KB=8):  # 128-column tile: LD = 136 floats, 8 KiB hold 14 rows -> the largest even divisor of 128 that fits: 8
        c = R.conv_case(128, 64, 5, 1, 133, R.class_lengths(133, 128, 2))
        with R.cfg_env((1, 2, 2, 2)):
            assert R.plan_of(lib, 1, c).chunk == 8
            R.check_conv(lib, 1, c, "LDS cap 8 KiB", who="k_conv1d_mfma")


def test_f32_vec_and_ovec_branches(lib):
    """T % 4 == 0: 16-byte staging and the row-major epilogue through LDS; MI355VITS_CONV_NO_OVEC: the register epilogue; odd T: the
    scalar branches.  The two epilogues give the same bits, with every option of the epilogue."""
    for opts in R.OPTION_CASES:
        c = R.conv_case(32, 70, 5, 1, 132, R.class_lengths(132, 64, 2), opts)
        p = R.plan_of(lib, 1, c)
        assert (p.kernel, p.vec, p.yvec, p.ovec) == (CONVK_F32_STAGED, 1, 1, 1), (opts, p.vec, p.yvec, p.ovec)
        a = R.check_conv(lib, 1, c, f"ovec {opts}", who="k_conv1d_mfma")
        with Env(MI355VITS_CONV_NO_OVEC=1):
            p = R.plan_of(lib, 1, c)
            assert (p.vec, p.yvec, p.ovec) == (1, 1, 0)
            b = R.check_conv(lib, 1, c, f"no ovec {opts}", who="k_conv1d_mfma")
        assert np.array_equal(a, b), (opts, "the two epilogues differ")
    c = R.conv_case(32, 70, 5, 1, 133, R.class_lengths(133, 64, 2))
    p = R.plan_of(lib, 1, c)
    assert (p.vec, p.yvec, p.ovec) == (0, 0, 0)


# ------------------------------------------------------------------------------------------------ options on every impl
@pytest.mark.parametrize("opts", R.OPTION_CASES, ids=lambda o: "+".join(k for k, _ in o) or "plain")
def test_options_on_every_impl(lib, opts):
    """bias, res, res_sub, relu, cond, mask_before_res, out_scale, accumulate, in_slope, out_len < in_len: on and off, on the generic
    kernel, the staged / direct / split-k f32 kernels, the split-bf16 staged kernel and the encoder's slice kernel."""
    T = 133
    lens = R.class_lengths(T, 64, 2)
    c = R.conv_case(32, 70, 5, 1, T, lens, opts)
    R.check_conv(lib, 0, c, f"{opts}")
    R.check_conv(lib, 1, c, f"staged {opts}", who="k_conv1d_mfma")
    for math in MATHS:
        R.check_conv(lib, 2, c, f"{opts}", math, fixed_rule=True)
    c = R.conv_case(64, 70, 1, 1, T, lens, opts)
    assert R.plan_of(lib, 1, c).kernel == CONVK_F32_DIRECT
    R.check_conv(lib, 1, c, f"direct {opts}", who="k_conv_direct_mfma")
    c = R.conv_case(1024, 40, 1, 1, 37, (37, 36, 0), opts)
    assert R.plan_of(lib, 1, c).kernel == CONVK_F32_SPLITK
    R.check_conv(lib, 1, c, f"split-k {opts}", who="k_conv_direct_splitk")
    c = R.conv_case(192, 96, 3, 1, 70, R.enc_lengths(70), opts)
    for math in MATHS:
        R.check_conv(lib, 3, c, f"{opts}", math, who="k_enc_b3")
        if not dict(opts).get("cond"):
            with Env(MI355VITS_ENC_WIDE=2):
                assert R.plan_of(lib, 3, c, math).kernel == R.CONVK_ENC_B3W8
                R.check_conv(lib, 3, c, f"wide {opts}", math, who="k_enc_b3w<8>")


# ------------------------------------------------------------------------------------------------ split-bf16 staged conv (impl 2)
@pytest.mark.parametrize("math", MATHS)
def test_b3_tiles(lib, math):
    R.b3_tiles_case(lib, math)


@pytest.mark.parametrize("math", MATHS)
def test_b3_chunk64(lib, math):
    """The 64-channel-chunk form (K <= 2, C_in % 64 == 0) next to the 32-channel one on the same taps; T > 512 without fixed_rule, and
    fixed_rule on a T <= 512 tensor against refusal without it."""
    for Cin, K, kernel in ((64, 2, CONVK_B3_STAGED64), (128, 1, CONVK_B3_STAGED64), (96, 2, CONVK_B3_STAGED32)):
        c = R.conv_case(Cin, 64, K, 1, 517, (517, 516, 257, 1, 0), (("res", True),))
        p = R.plan_of(lib, 2, c, math)
        assert p.kernel == kernel and p.chunk == (64 if kernel == CONVK_B3_STAGED64 else 32), (Cin, K, p.kernel, p.chunk)
        R.check_conv(lib, 2, c, f"Cin={Cin} K={K} T=517", math)
    c = R.conv_case(64, 64, 2, 1, 133, R.class_lengths(133, 64, 1))
    with pytest.raises(NativeError):
        R.run_conv(lib, 2, c, math)
    assert R.plan_of(lib, 2, c, math, fixed_rule=True).kernel == CONVK_B3_STAGED64
    R.check_conv(lib, 2, c, "fixed_rule T=133", math, fixed_rule=True)


# ------------------------------------------------------------------------------------------------ encoder slice (impl 3)
@pytest.mark.parametrize("math", MATHS)
def test_enc_rowloop_forms(lib, math):
    """k_enc_b3 with 1, 2, 3, 4 and 6 row blocks per workgroup, and k_enc_b3w, on 192 -> 768: the same bits."""
    forms = [(dict(MI355VITS_ENC_ROWLOOP=r, MI355VITS_ENC_WIDE=0), CONVK_ENC_B3, r) for r in R.ENC_ROWLOOPS]
    forms.append((dict(MI355VITS_ENC_WIDE=1), R.CONVK_ENC_B3W8, 3))
    for T in (129, 65):
        R.enc_forms_case(lib, math, (192, 768, 3), T, forms)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("form", R.ENC_WIDE_FORMS, ids=lambda f: "x".join(str(v) for v in f[0]))
def test_enc_wide_forms(lib, math, form):
    """k_enc_b3w with eight and six row tiles (MI355VITS_ENC_WIDE = 1; 2 below six row tiles) is bit for bit the 64-column form."""
    (Cin, Cout, K, wide), kernel = form
    for T in (129, 127, 1):
        R.enc_forms_case(lib, math, (Cin, Cout, K), T, [(NARROW, CONVK_ENC_B3, 1), (dict(MI355VITS_ENC_WIDE=wide), kernel, None)])


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("shape", R.ENC_SLICES, ids=lambda s: "x".join(str(v) for v in s))
def test_enc_slices_and_lengths(lib, math, shape):
    """C_in = 96, 192, 384, 768 (from 384 on: the slices' raw sums), K in {1, 3}, every T around the 64- and 128-column items."""
    for T in R.ENC_T:
        R.enc_forms_case(lib, math, shape, T, [(NARROW, CONVK_ENC_B3, 1), (dict(MI355VITS_ENC_WIDE=1), R.CONVK_ENC_B3W6, 1)])


# ------------------------------------------------------------------------------------------------ resident-input resblock conv (impl 4)
@pytest.mark.parametrize("kd", R.RBC_KD, ids=lambda kd: f"k{kd[0]}d{kd[1]}")
def test_rbc_forms(lib, kd):
    """Writing and accumulating at every (K, dilation); the scaled form without a bias at (7, 3)."""
    for opts in R.RBC_OPTION_CASES if kd == (7, 3) else (R.RBC_OPTION_CASES[0], R.RBC_OPTION_CASES[2]):
        R.rbc_case(lib, kd, opts)


@pytest.mark.parametrize("wide", [0, 1])
def test_padding_rbc(lib, wide):
    for kd in ((7, 12), (3, 1)):
        for acc in (False, True):
            R.rbc_padding_case(lib, kd, wide, acc)


# ------------------------------------------------------------------------------------------------ padding (impl 0 - 3)
def test_padding_conv1d(lib):
    """JUNK in x at t >= in_len, in res at t >= out_len and all over the prior y: valid columns keep their bits, zeros under out_len.
    Where the hook's comment names other values past a row's end — res * out_scale with mask_before_res (out_len < in_len, and
    accumulating), the zero-extended row's conv without out_len — every column t < T is compared with the rule."""
    opts = (("res", True), ("in_slope", 0.1))
    lens = R.class_lengths(133, 64, 2)
    c = R.conv_case(32, 70, 5, 1, 133, lens, opts)
    c4 = R.conv_case(32, 70, 5, 1, 132, R.class_lengths(132, 64, 2), opts)
    ca = R.conv_case(32, 70, 5, 1, 133, lens, opts + (("accumulate", True),))
    co = R.conv_case(32, 70, 5, 1, 133, lens, opts + (("out_lt_in", True),))
    for impl, kw in ((0, {}), (1, {}), (2, dict(math=MATH_BF16X3, fixed_rule=True)), (2, dict(math=MATH_BF16W, fixed_rule=True))):
        for case in (c, c4, co):
            R.conv_padding_case(lib, impl, case, **kw)
        R.conv_padding_case(lib, impl, ca, accumulate=True, **kw)
        for name, more in R.WHOLE_RANGE_OPTS:
            R.conv_whole_range_case(lib, impl, R.conv_case(32, 70, 5, 1, 133, lens, opts + more), name, **kw)
            R.conv_whole_range_case(lib, impl, R.conv_case(32, 70, 5, 1, 132, R.class_lengths(132, 64, 2), opts + more), name + ", T % 4 == 0", **kw)
    for shape in ((64, 70, 1, 1), (1024, 40, 1, 1)):  # direct, split-k
        cd = R.conv_case(*shape, 37, (37, 36, 33, 32, 31, 1, 0), opts)
        R.conv_padding_case(lib, 1, cd)
        for name, more in R.WHOLE_RANGE_OPTS:
            R.conv_whole_range_case(lib, 1, R.conv_case(*shape, 37, (37, 36, 33, 32, 31, 1, 0), opts + more), name)
    ce = R.conv_case(192, 96, 3, 1, 130, R.enc_lengths(130), opts)
    for math in MATHS:
        for wide in (0, 2):
            with Env(MI355VITS_ENC_WIDE=wide):
                R.conv_padding_case(lib, 3, ce, math=math)
                for name, more in R.WHOLE_RANGE_OPTS:
                    R.conv_whole_range_case(lib, 3, R.conv_case(192, 96, 3, 1, 130, R.enc_lengths(130), opts + more), name, math=math)


# ------------------------------------------------------------------------------------------------ transposed conv
@pytest.mark.parametrize("shape", R.CONVT_SHAPES + [(6, 3, 6, 2), (8, 4, 3, 1)], ids=lambda s: "x".join(str(v) for v in s))
def test_convt_generic_and_f32(lib, shape):
    """Impl 0 and 1 from the definition, K = 2 s and not; every output position is written (the prior y holds JUNK)."""
    Cin, Cout, K, s = shape
    for Tin in (1, 2, 15, 16, 17, 37, 70):
        c = R.convt_case(Cin, Cout, K, s, Tin)
        prior = np.full((2, Cout, Tin * s), R.JUNK, np.float32)
        p = lib.lab_conv_plan(0, 2, Cin, Cout, Tin, K, 1, s)
        assert p.kernel == CONVK_CONVT_GENERIC
        R.check_convt(lib, 0, c, f"{shape} Tin={Tin}", y_prior=prior)
        R.check_convt(lib, 1, c, f"{shape} Tin={Tin}", y_prior=prior)


def test_convt_f32_staged_direct_lds(lib):
    """64 -> 32, s = 4 on the f32 kernels: direct by default, staged with MI355VITS_POLY_DIRECT_CIN = 0, and the staged kernel's
    epilogue through LDS with MI355VITS_CONV_POLY_LDS — the same polyphase sums in three stores."""
    outs = []
    for Tin in (129, 132, 31):
        c = R.convt_case(64, 32, 8, 4, Tin)
        for env, kernel, ovec in ((dict(), CONVK_F32_DIRECT, 0), (dict(MI355VITS_POLY_DIRECT_CIN=0), CONVK_F32_STAGED, 0),
                                  (dict(MI355VITS_POLY_DIRECT_CIN=0, MI355VITS_CONV_POLY_LDS=1), CONVK_F32_STAGED, 1)):
            with Env(**env):
                p = lib.lab_conv_plan(1, 2, 64, 32, Tin, 8, 1, 4)
                assert (p.kernel, p.ovec) == (kernel, ovec), (Tin, env, p.kernel, p.ovec)
                outs.append(R.check_convt(lib, 1, c, f"Tin={Tin} {env}", y_prior=np.full((2, 32, Tin * 4), R.JUNK, np.float32)))
        assert np.array_equal(outs[-1], outs[-2]), (Tin, "the LDS epilogue differs from the register scatter")


def test_convt_split_bf16_pc_and_staged(lib, cu_count):
    """Impl 2 on 64 -> 32, s = 4 at 5 rows x 2,000 positions (110 tiles of 192 x 64: the grid at which the launcher leaves the
    256-column tile, whose two staging buffers would not fit): the persistent producer / consumer form on fewer items than CUs and
    on several items per workgroup, and the one-tile-per-workgroup kernel (MI355VITS_NO_B3_PC): the same bits, the plan call
    reporting the persistent grid."""
    R.convt_pc_case(lib, 5, 2000, cu_count, (3, 8, 64, 256))


@pytest.mark.parametrize("shape", list(R.UPS_SHAPES), ids=lambda s: "x".join(str(v) for v in s))
def test_ups_forms(lib, shape):
    """Impl 3, all three upsamplers, narrow and wide items, Tin around the items, ragged in_len with 0; JUNK in x past in_len and all
    over the prior y: an empty row is not touched."""
    Cin, Cout, K, s = shape
    for wide, item in zip((0, 1), R.UPS_SHAPES[shape]):
        for Tin in sorted({1, item - 1, item, item + 1, 2 * item + 1}):
            lens = tuple(sorted({Tin, Tin - 1, max(Tin - item, 0), min(Tin, item - 1), 1, 0}, reverse=True))
            c = R.convt_case(Cin, Cout, K, s, Tin, lens)
            with Env(MI355VITS_RBC_WIDE=wide):
                p = lib.lab_conv_plan(3, len(lens), Cin, Cout, Tin, K, 1, s, lengths=lens)
                assert p.kernel == (CONVK_UPS64 if Cin == 64 else CONVK_UPS_PL) and p.cols == item, (shape, wide, p.kernel, p.cols)
                plain = R.check_convt(lib, 3, c, f"{shape} wide={wide} Tin={Tin}")
                x = np.where(R.past(lens, Tin), R.JUNK, c["x"])
                got = lib.test_conv_transpose1d(x, c["w"], c["bias"], s, in_slope=0.1, impl=3, in_len=c["lens"],
                                                y_prior=np.full(plain.shape, R.JUNK, np.float32))
            R.same_valid_bits(plain, got, c["cmp_len"], (shape, wide, Tin, "JUNK past in_len reached a valid position"))
            for b, n in enumerate(lens):
                if n == 0:
                    assert np.all(got[b] == R.JUNK), (shape, wide, Tin, "an empty row was written")


# ------------------------------------------------------------------------------------------------ enc_o_ln, conv_post
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("T", R.ENC_O_LN_T)
def test_enc_o_ln(lib, T, math):
    R.enc_o_ln_check(lib, T, math)


VOL = np.array([1.0, 0.5, 2.5, 2.5, 0.5])


@pytest.mark.parametrize("Cin", [32, 4])
def test_conv_post_dpp(lib, Cin):
    """k_conv_post_tanh_dpp around its 248-sample tile and its 1,984-sample workgroup; volumes 1, 0.5 and 2.5 (clipping), a quiet row
    and an empty one; the pitch rounded up to four, valid_len carrying the odd lengths."""
    for L in R.CONV_POST_DPP_L:
        c = R.conv_post_case(Cin, 7, L)
        R.check_conv_post(lib, c, 0, f"Cin={Cin} L={L}", VOL)
    _, _, pcm = R.check_conv_post(lib, R.conv_post_case(Cin, 7, 1985), 0, "no volumes", None)
    assert np.abs(pcm.astype(np.int32)).max() == 32767


@pytest.mark.parametrize("K", [3, 5, 9, 7])
def test_conv_post_vec(lib, K):
    """k_conv_post_tanh_vec around CPV_T = 2048 (K = 7 through MI355VITS_CONV_POST_V1)."""
    with Env(MI355VITS_CONV_POST_V1=1):
        for L in (1, 7, 8, 9, 2047, 2048, 2049, 2 * 2048 + 3):
            R.check_conv_post(lib, R.conv_post_case(4, K, L), 1, f"K={K} L={L}", VOL)


def test_conv_post_staged(lib):
    """k_conv_post_tanh around CP_T = 1024: an odd pitch, K = 11, and MI355VITS_CONV_POST_STAGED on an aligned K = 7 tensor."""
    for L in (1, 1023, 1025, 2 * 1024 + 3):
        R.check_conv_post(lib, R.conv_post_case(4, 7, L, pitch4=False), 2, f"odd pitch L={L}", VOL)
    for L in (1024, 1027):
        R.check_conv_post(lib, R.conv_post_case(6, 11, L, pitch4=L % 4 != 0), 2, f"K=11 L={L}", VOL)
    with Env(MI355VITS_CONV_POST_STAGED=1):
        R.check_conv_post(lib, R.conv_post_case(4, 7, 1024), 2, "forced", VOL)


def test_conv_post_kernels_agree(lib):
    """The three kernels give the same audio bits, peaks and PCM on a shape all three serve (K = 7), and JUNK in x past valid_len
    reaches nothing."""
    c = R.conv_post_case(8, 7, 2 * 1984 + 3)
    outs = [R.check_conv_post(lib, c, 0, "dpp", VOL)]
    with Env(MI355VITS_CONV_POST_V1=1):
        outs.append(R.check_conv_post(lib, c, 1, "vec", VOL))
    with Env(MI355VITS_CONV_POST_STAGED=1):
        outs.append(R.check_conv_post(lib, c, 2, "staged", VOL))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)
    x = np.where(np.arange(c["x"].shape[2])[None, None, :] >= c["lens"][:, None, None], R.JUNK, c["x"])
    for env in (dict(), dict(MI355VITS_CONV_POST_V1=1), dict(MI355VITS_CONV_POST_STAGED=1)):
        with Env(**env):
            audio, peaks, pcm, _ = lib.test_conv_post(x, c["w"], c["lens"], VOL)
        for a, b in zip(outs[0], (audio, peaks, pcm)):
            assert np.array_equal(a, b), (env, "JUNK past valid_len moved the output")


# ------------------------------------------------------------------------------------------------ the WaveNet two-launch path
@pytest.mark.parametrize("tile", [(2, 2, 2, 2), (2, 1, 2, 2), (1, 2, 2, 2), (1, 1, 2, 2)])
def test_wn_two_launch_path_under_forced_tiles(lib, tile):
    """The gate conv (EPI_GATE: (2,2,2,2), (2,1,2,2)) and the res / skip conv (EPI_RESSKIP: (2,2,2,2), (1,2,2,2), (1,1,2,2)) of
    mi355vits_test_wn_layer's impl 0 under each tile their candidate lists hold (a tile a list lacks leaves that conv on its rule)."""
    with R.cfg_env(tile):
        wn_ref.check_vs_fp64(lib, 0, 192, 141, 5, 1, 384, wn_ref.kd_lengths(5, 1))


# ------------------------------------------------------------------------------------------------ the proof that the tests bite
@pytest.mark.parametrize("drop", [1, 2, 3])
def test_dropped_partial_product_fails_the_criterion_and_passes_the_old_threshold(emu_lib, drop, monkeypatch):
    """MI355VITS_EMU_DROP leaves one of the three smallest of the six partial products out of the CPU model's b3 loops (1: l_w x h_x,
    2: h_w x l_x, 3: m_w x m_x).  The per-element criterion fails for the split-bf16 staged kernel and for the encoder's slice kernel on
    one small case each, and the same outputs pass `max |y - ref| < 5e-5`, the threshold of test_conv1d_kernels /
    test_encoder_slice_kernel_vs_fp64: the gap these tests close."""
    cases = [(2, R.conv_case(64, 64, 3, 1, 133, R.class_lengths(133, 64, 1)), dict(fixed_rule=True)),
             (3, R.conv_case(192, 192, 3, 1, 70, R.enc_lengths(70)), {})]
    for impl, c, kw in cases:
        ref, f32 = R.refs(c, R.GROUP[impl])
        intact = R.run_conv(emu_lib, impl, c, MATH_BF16X3, **kw)
        assert R.passes_vs_fp64(intact, ref, f32, c["cmp_len"])
        monkeypatch.setenv("MI355VITS_EMU_DROP", str(drop))
        broken = R.run_conv(emu_lib, impl, c, MATH_BF16X3, **kw)
        monkeypatch.delenv("MI355VITS_EMU_DROP")
        e, e32 = R.norm_err(broken, ref, c["cmp_len"]), R.norm_err(f32, ref, c["cmp_len"])
        old = max(float(np.abs(broken[b, :, :n].astype(np.float64) - ref[b, :, :n]).max()) for b, n in enumerate(c["cmp_len"]) if n)
        print(f"drop {drop} impl {impl}: e = {e:.3e}  e32 = {e32:.3e}  e/e32 = {e / e32:.1f}  max abs = {old:.3e} (old threshold {R.OLD_MAX_ABS_TOL})")
        assert not R.passes_vs_fp64(broken, ref, f32, c["cmp_len"]), (drop, impl, e, e32)
        assert old < R.OLD_MAX_ABS_TOL, (drop, impl, old)


def test_zz_worst_ratios_of_this_run(lib):
    """Prints the worst e / e32 per kernel over the tests of this module that ran before it (DESIGN.md quotes the figures)."""
    R.print_ratios(WHERE)
