"""Device twin of tests/test_grid_geometry_and_poison.py: the resident-input kernels on ragged rows at their edges with poisoned
inputs, at sizes where the item count exceeds the MI355X's 256 compute units and is no multiple of it (workgroups walk several
items with their forward-only cursors), plus one small grid (one item per workgroup); and the headline voice on a NaN-filled
workspace."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from tests.test_grid_geometry_and_poison import _check_rows, _poison
from tests.util import check_parity

pytestmark = pytest.mark.gpu
CUS = 256


def _lens(T, N, halo, min_items, extra=0):
    """Row lengths at the kernel's edges (empty, one column, shorter than the halo, item width - 1 / exact / + 1, T - 1, T, two
    items), then full rows until there are at least `min_items` items of N positions and their count is no multiple of 256."""
    lens = [0, 1, min(5, max(1, halo - 1)), N - 1, N, N + 1, T - 1, T, 2 * N]
    items = lambda: sum((n + extra + N - 1) // N for n in lens if n > 0)  # noqa: E731
    while items() < min_items or items() % CUS == 0:
        lens.append(T)
    return np.array(lens, np.int32)


def _errors(y, ref, lens, stride):
    d = [y[b, :, :n * stride].astype(np.float64) - ref[b, :, :n * stride] for b, n in enumerate(lens) if n]
    return float(np.sqrt(sum(float(np.sum(e * e)) for e in d) / sum(e.size for e in d))), max(float(np.abs(e).max()) for e in d)


# (T, item width the count is taken in, least item count): 128-column items, more than 256 of them (k_rb_conv_pw on 256
# workgroups); fewer than 256 items of 128 columns but more than 256 of 32 (k_rb_conv on 256 workgroups); a small grid
RBC_GRIDS = {"wide": (3800, 128, CUS + 1), "narrow": (1000, 32, CUS + 1), "small": (260, 32, 27)}


@pytest.mark.parametrize("kd", [(7, 12), (3, 1), (5, 6)])
@pytest.mark.parametrize("grid", list(RBC_GRIDS))
def test_resident_input_resblock_conv_ragged_rows_vs_fp64(gpu_hooks, kd, grid):
    """k_rb_conv_pw / k_rb_conv (impl 4) on ragged rows whose inputs past their ends are qNaN (one row +Inf): per row against the
    fp64 conv of that row alone, at the bound of test_gpu_parity.py's fp64 test plus a per-row largest error."""
    K, dil = kd
    T, N, min_items = RBC_GRIDS[grid]
    lens = _lens(T, N, (K - 1) // 2 * dil, min_items)
    assert (sum((n + 127) // 128 for n in lens) >= CUS) == (grid == "wide")
    B, C = len(lens), 128
    rng = np.random.default_rng(1000 * K + dil + T)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    w = (rng.standard_normal((C, C, K)) / np.sqrt(C * K)).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    res = rng.standard_normal((B, C, T)).astype(np.float32)
    x0 = np.where(np.arange(T)[None, None, :] < lens[:, None, None], x, 0).astype(np.float32)
    conv = F.conv1d(F.leaky_relu(torch.from_numpy(x0).double(), 0.1), torch.from_numpy(w).double(), torch.from_numpy(bias).double(),
                    dilation=dil, padding=(K * dil - dil) // 2)
    ref = ((conv + torch.from_numpy(res).double()) * 0.5).numpy()
    err1, maxabs1 = _errors(gpu_hooks.test_conv1d(x0, w, bias, res, dilation=dil, impl=1, in_len=lens, in_slope=0.1, out_scale=0.5), ref, lens, 1)
    y = gpu_hooks.test_conv1d(_poison(x, lens, inf_row=3), w, bias, res, dilation=dil, impl=4, in_len=lens, in_slope=0.1, out_scale=0.5)
    _check_rows(y, ref, lens, 1, err1, maxabs1)


# (Cin, Cout, stride, K) -> positions per item of the large-grid form (k_ups_pl 64 / 128 positions, k_ups64 127)
UPS_ITEMS = {(256, 128, 8, 16): 64, (128, 64, 8, 16): 128, (64, 32, 4, 8): 127}


@pytest.mark.parametrize("case", list(UPS_ITEMS))
@pytest.mark.parametrize("grid", ["large", "small"])
def test_resident_input_upsamplers_ragged_rows_vs_fp64(gpu_hooks, case, grid):
    """k_ups_pl / k_ups64 (conv-transpose impl 3) with per-row input lengths, the inputs past every row's end poisoned: per row
    against ConvTranspose1d(leaky(x[b, :, :len_b])) in fp64 on [0, len_b x stride)."""
    Cin, Cout, stride, K = case
    N = UPS_ITEMS[case]
    Tin = 20 * N + 17 if grid == "large" else 300
    lens = _lens(Tin, N, 1, CUS + 1 if grid == "large" else 27, extra=1)
    B = len(lens)
    rng = np.random.default_rng(Cin + Tin)
    x = rng.standard_normal((B, Cin, Tin)).astype(np.float32)
    w = (rng.standard_normal((Cin, Cout, K)) / np.sqrt(Cin * K / stride)).astype(np.float32)
    bias = rng.standard_normal(Cout).astype(np.float32)
    x0 = np.where(np.arange(Tin)[None, None, :] < lens[:, None, None], x, 0).astype(np.float32)
    ref = F.conv_transpose1d(F.leaky_relu(torch.from_numpy(x0).double(), 0.1), torch.from_numpy(w).double(), torch.from_numpy(bias).double(),
                             stride=stride, padding=(K - stride) // 2).numpy()
    err1, maxabs1 = _errors(gpu_hooks.test_conv_transpose1d(x0, w, bias, stride, in_slope=0.1, impl=1), ref, lens, stride)
    y = gpu_hooks.test_conv_transpose1d(_poison(x, lens, inf_row=4), w, bias, stride, in_slope=0.1, impl=3, in_len=lens)
    _check_rows(y, ref, lens, stride, err1, maxabs1)


def test_headline_voice_on_a_nan_filled_workspace(gpu_hooks):
    """apope_low (synthetic weights), 24 ragged rows with natural durations at deterministic scales, on a handle whose workspace a
    larger batch sized first and a quiet NaN then filled: every row bitwise its solo run on a fresh handle, and two rows of a
    ragged pair on the refilled workspace within check_parity's tight bound."""
    cfg = VitsConfig.apope_low()
    w = W.synthetic_weights(cfg, seed=131, frames_per_id=3.0)
    blob = W.pack(cfg, w)
    rng = np.random.default_rng(131)
    B, Tx = 24, 64
    lengths = rng.integers(1, Tx + 1, B)
    lengths[0], lengths[5] = Tx, 1
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    scales = [0.0, 1.0, 0.0]
    fresh = Engine(blob, device=0, library=gpu_hooks)
    solo = [fresh.run(ids[b:b + 1, :n], [n], scales, want_pcm16=True) for b, n in enumerate(lengths)]
    fresh.close()
    eng = Engine(blob, device=0, library=gpu_hooks)
    eng.run(rng.integers(1, cfg.num_symbols, (B + 4, Tx)), np.full(B + 4, Tx), scales,
            forced_durations=np.full((B + 4, Tx), 8, np.int32))  # sizes the workspace past what the ragged batch needs
    eng.fill_workspace(0x7FC00000)
    out = eng.run(ids, lengths, scales, want_pcm16=True)
    assert np.isfinite(out["audio"]).all()
    for b in range(B):
        L = int(solo[b]["lengths"][0])
        assert L == int(out["lengths"][b]), b
        assert np.array_equal(solo[b]["audio"][0, :L], out["audio"][b, :L]), b
        assert np.array_equal(solo[b]["pcm"][0, :L], out["pcm"][b, :L]), b
    eng.fill_workspace(0x7FC00000)
    pair = [0, 5]
    check_parity(gpu_hooks, cfg, ids=ids[pair], lengths=lengths[pair], weights=w, engine=eng)
    eng.close()
