"""The multi-receptive-field stage kernels alone, on the CPU model of the kernels, against fp64 per element: the case tables of
tests/mrf_ref.py (tests/test_gpu_mrf_stage.py runs them on the MI355X).  k_mrf_fused in both math modes, k_mrf_p<32> / <64> and the
row sweep k_mrf_s<64>, at the seams of their work items, with several items per persistent workgroup, on ragged rows, and with
junk past every row's end."""
import numpy as np
import pytest

from mimic3_amd._native import MATH_BF16X3, MATH_F32, NativeError
from tests import mrf_ref as M


@pytest.fixture
def two_cus(emu_lib):
    """Two compute units: every persistent workgroup of k_mrf_p / k_mrf_s walks several items."""
    emu_lib.emu_set_cu_count(2)
    yield emu_lib
    emu_lib.emu_set_cu_count(0)


def test_plan_call_reports_the_kernels_geometry(emu_lib):
    assert M.plan(emu_lib, 0, 32) == (512, 45, 0, 0) and M.plan(emu_lib, 0, 64) == (192, 45, 0, 0)
    assert M.plan(emu_lib, 1, 32) == (320, 45, 0, 0) and M.plan(emu_lib, 1, 64) == (96, 45, 0, 0)
    assert M.plan(emu_lib, 2, 64) == (48, 45, 128, 176)
    assert M.plan(emu_lib, 0, 128, (3, 5), ((1, 2), (2, 6))) == (96, 16, 0, 0)
    for impl, C, ks, dils in [(0, 128, M.LOW_KS, M.LOW_DILS), (1, 128, M.LOW_KS, M.LOW_DILS), (2, 32, M.LOW_KS, M.LOW_DILS),
                              (1, 64, (3, 5), M.LOW_DILS[:2]), (1, 32, (3, 5, 9), M.LOW_DILS), (0, 48, M.LOW_KS, M.LOW_DILS)]:
        with pytest.raises(NativeError, match="not supported"):
            M.plan(emu_lib, impl, C, ks, dils)


@pytest.mark.parametrize("dils", [M.LOW_DILS] + M.OTHER_DILS)
@pytest.mark.parametrize("C", [32, 64])
def test_block_kernel_at_its_item_seams(two_cus, C, dils):
    """k_mrf_p: rows ending 1, 2, R, R + 1, W - 1, W, W + 1, W + R, W + R + 1, 2 W + 1 columns in, an empty row; two compute units,
    so every workgroup walks several (row, block) items (C = 32: the next item's x is staged under the running one) — and the same bits
    with one item per workgroup."""
    c, got = M.block_case(two_cus, C, dils)
    two_cus.emu_set_cu_count(64)
    assert np.array_equal(M.run_case(two_cus, 1, c), got), "the bits depend on the items a workgroup walks"


@pytest.mark.parametrize("C", [32, 64])
def test_rows_of_a_full_grid_are_their_single_row_bits(emu_lib, C):
    """More items than compute units, several rows: every row bit for bit what it is alone (the device test's case at a small size)."""
    emu_lib.emu_set_cu_count(4)
    try:
        M.many_items_case(emu_lib, C, 4, items_per_row=3)
    finally:
        emu_lib.emu_set_cu_count(0)


@pytest.mark.parametrize("C", [32, 64])
def test_block_kernel_at_every_tensor_width(emu_lib, C):
    W, R, _, _ = M.plan(emu_lib, 1, C)
    for T in M.edge_lengths(W, R):
        M.width_case(emu_lib, C, T)


def test_row_sweep_is_the_block_kernel_bit_for_bit(emu_lib):
    """k_mrf_s with the planner's shortest segment (24 steps), a longer one and one that holds the whole row, over rows on which both
    rings wrap more than six times; rows end in the first and in the last step of a segment, on a seam, inside the pipeline fill."""
    M.sweep_case(emu_lib, [1152, 1200, 1248], padding_segs=[1152])  # (12 items on the model's 8 compute units)


@pytest.mark.parametrize("dils", [M.LOW_DILS] + M.OTHER_DILS)
def test_row_sweep_with_segments_shorter_than_the_planner_returns(emu_lib, dils):
    """Segments of 1, 2, 3 and 5 steps (mrf_s_segment never returns fewer than 24): every segment is an independent work item with
    its own pipeline fill, so launch_mrf_s serves any positive multiple of the step — and the hook says so.  The ragged batch of the
    block kernel's seams: rows shorter than the fill, ending in a segment's first and last step."""
    W, R, _, _ = M.plan(emu_lib, 1, 64, M.LOW_KS, dils)
    T = 2 * W + 1
    M.sweep_case(emu_lib, [48, 96, 144, 240], dils, T=T, rows=M.ragged_batch(W, R), padding_segs=[48, 144])


@pytest.mark.parametrize("C,math", [(64, MATH_F32), (32, MATH_BF16X3)])
def test_fused_kernel_at_every_tensor_width(emu_lib, C, math):
    """T = 1, 2, R, R + 1, W - 1, W, W + 1, W + R, W + R + 1, 2 W + 1 for k_mrf_fused, one channel count per math mode."""
    W, R, _, _ = M.plan(emu_lib, 0, C)
    for T in M.edge_lengths(W, R):
        M.fused_width_case(emu_lib, C, math, T)


@pytest.mark.parametrize("C,ks,dils,math,out_scale", M.FUSED_CASES)
def test_fused_kernel_vs_fp64(emu_lib, C, ks, dils, math, out_scale):
    M.fused_case(emu_lib, C, ks, dils, math, out_scale)


def test_the_three_kernels_agree(emu_lib):
    """One input through k_mrf_fused (both modes) and k_mrf_p (k_mrf_s is bit for bit k_mrf_p: the sweep tests): pairwise within the
    sum of their bounds."""
    c, p = M.block_case(emu_lib, 64)
    outs = {(1, 1): p, (0, 0): M.run_case(emu_lib, 0, c, math=MATH_F32), (0, 1): M.run_case(emu_lib, 0, c, math=MATH_BF16X3)}
    keys = list(outs)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            bound = sum(M.f32_bound(M.norm_err(M.calibration(c, *k), c["ref"], c["lens"])) for k in (a, b))
            e = M.norm_err(outs[a], outs[b], c["lens"])
            print(f"mrf {a} vs {b}: {e:.3e} (bound {bound:.3e})")
            assert e <= bound, (a, b, e, bound)


def test_hook_refuses_what_a_kernel_does_not_serve(emu_lib):
    c = M.reference_case(64, 100, M.LOW_KS, M.LOW_DILS, (100, 7))
    for kw in (dict(impl=2, seg=0), dict(impl=2, seg=47), dict(impl=2, seg=100), dict(impl=2, seg=-48), dict(impl=1, math=MATH_F32),
               dict(impl=0, math=2), dict(impl=3)):
        with pytest.raises(NativeError):
            M.run_case(emu_lib, kw.pop("impl"), c, **kw)
    c32 = M.reference_case(32, 100, M.LOW_KS, M.LOW_DILS, (100, 7))
    with pytest.raises(NativeError, match="not supported"):
        M.run_case(emu_lib, 2, c32, seg=48)


def test_zz_worst_ratios_of_this_run():
    print("worst e / e32 per (impl, math) on the CPU model:", {k: round(v, 3) for k, v in sorted(M.RATIOS.items())})
    assert all(v <= 3.0 for v in M.RATIOS.values()), M.RATIOS
