"""The multi-receptive-field stage kernels alone on the MI355X (pytest -m gpu), against fp64 per element: the case tables of
tests/mrf_ref.py that tests/test_mrf_stage.py runs on the CPU model.  Every hook call here is made TWICE and must return equal
bits: k_mrf_p stages the next item under the running one and k_mrf_s hands columns from wave to wave through LDS rings — a
producer / consumer race shows only on the device."""
import numpy as np
import pytest
import torch

from mimic3_amd._native import MATH_BF16X3, MATH_F32, NativeError
from tests import mrf_ref as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twice(gpu_hooks):
    return M.Twice(gpu_hooks)


def test_plan_call_reports_the_kernels_geometry(gpu_hooks):
    assert M.plan(gpu_hooks, 0, 32) == (512, 45, 0, 0) and M.plan(gpu_hooks, 0, 64) == (192, 45, 0, 0)
    assert M.plan(gpu_hooks, 1, 32) == (320, 45, 0, 0) and M.plan(gpu_hooks, 1, 64) == (96, 45, 0, 0)
    assert M.plan(gpu_hooks, 2, 64) == (48, 45, 128, 176)
    for impl, C, dils in [(1, 128, M.LOW_DILS), (2, 32, M.LOW_DILS)] + [(i, 64, d) for i in (1, 2) for d in M.OTHER_DILS]:
        with pytest.raises(NativeError, match="not supported"):  # the device libraries hold the "_low" dilations only
            M.plan(gpu_hooks, impl, C, M.LOW_KS, dils)


@pytest.mark.parametrize("C", [32, 64])
def test_block_kernel_at_its_item_seams(twice, C):
    M.block_case(twice, C)


@pytest.mark.parametrize("C", [32, 64])
def test_block_kernel_at_every_tensor_width(twice, C):
    W, R, _, _ = M.plan(twice, 1, C)
    for T in M.edge_lengths(W, R):
        M.width_case(twice, C, T)


@pytest.mark.parametrize("C", [32, 64])
def test_several_items_per_persistent_workgroup(twice, C):
    """Just over one item per compute unit (9 rows x 30 items on 256 units: under 100k columns)."""
    M.many_items_case(twice, C, torch.cuda.get_device_properties(0).multi_processor_count)


def test_row_sweep_is_the_block_kernel_bit_for_bit(twice):
    M.sweep_case(twice, [1152, 1200, 1248], padding_segs=[1152])


def test_row_sweep_with_segments_shorter_than_the_planner_returns(twice):
    W, R, _, _ = M.plan(twice, 1, 64)
    M.sweep_case(twice, [48, 96, 144, 240], T=2 * W + 1, rows=M.ragged_batch(W, R), padding_segs=[48, 144])


@pytest.mark.parametrize("C,math", [(64, MATH_F32), (32, MATH_BF16X3)])
def test_fused_kernel_at_every_tensor_width(twice, C, math):
    """T = 1, 2, R, R + 1, W - 1, W, W + 1, W + R, W + R + 1, 2 W + 1 for k_mrf_fused, one channel count per math mode."""
    W, R, _, _ = M.plan(twice, 0, C)
    for T in M.edge_lengths(W, R):
        M.fused_width_case(twice, C, math, T)


@pytest.mark.parametrize("C,ks,dils,math,out_scale", M.FUSED_CASES)
def test_fused_kernel_vs_fp64(twice, C, ks, dils, math, out_scale):
    M.fused_case(twice, C, ks, dils, math, out_scale)


def test_the_three_kernels_agree(twice):
    c, p = M.block_case(twice, 64)
    outs = {(1, 1): p, (0, 0): M.run_case(twice, 0, c, math=MATH_F32), (0, 1): M.run_case(twice, 0, c, math=MATH_BF16X3)}
    keys = list(outs)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            bound = sum(M.f32_bound(M.norm_err(M.calibration(c, *k), c["ref"], c["lens"])) for k in (a, b))
            e = M.norm_err(outs[a], outs[b], c["lens"])
            print(f"mrf {a} vs {b}: {e:.3e} (bound {bound:.3e})")
            assert e <= bound, (a, b, e, bound)


def test_hook_refuses_what_a_kernel_does_not_serve(gpu_hooks):
    c = M.reference_case(64, 100, M.LOW_KS, M.LOW_DILS, (100, 7))
    for kw in (dict(impl=2, seg=0), dict(impl=2, seg=47), dict(impl=2, seg=100), dict(impl=1, math=MATH_F32), dict(impl=0, math=2)):
        with pytest.raises(NativeError):
            M.run_case(gpu_hooks, kw.pop("impl"), c, **kw)


def test_zz_worst_ratios_of_this_run():
    print("worst e / e32 per (impl, math) on the device:", {k: round(v, 3) for k, v in sorted(M.RATIOS.items())})
    assert all(v <= 3.0 for v in M.RATIOS.values()), M.RATIOS
