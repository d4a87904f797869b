"""Device twin of tests/test_wn_shape.py (pytest -m gpu): k_wn_layer_b3 on v_mfma_f32_16x16x32_bf16 against fp64 per element at the
lengths around its 16-column tiles, its forms bit for bit among themselves, the 32x32x16 form behind MI355VITS_WN_SHAPE=32 under the
same criterion, MATH_BF16W through the engine, and a batch on a NaN-filled workspace against its rows' solo runs.  Every hook call is
made twice and must return equal bits (tests/wn_ref.py, Twice)."""
import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from tests import wn_ref as Wn
from tests.test_wn_shape import (SHAPE_LENGTHS, SHAPE_OPTIONS, bf16w_forms_case, bf16w_shapes_case, bf16w_voice,  # noqa: F401 (fixture)
                                 shape_case, shape_lengths)
from tests.util import TIGHT_REL_RMS_TOL, rel_rms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twice(gpu_hooks):
    return Wn.Twice(gpu_hooks)


@pytest.fixture(scope="module")
def twice_lab(lab_lib):
    return Wn.Twice(lab_lib)


@pytest.mark.parametrize("two,cond", SHAPE_OPTIONS)
@pytest.mark.parametrize("T", SHAPE_LENGTHS)
def test_layer_vs_fp64_around_the_16_column_tiles(twice, T, two, cond):
    shape_case(twice, T, two, cond)


@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("T", [33, 129])
def test_forms_agree_bitwise_and_meet_the_criterion(twice_lab, T, two):
    outs = []
    for env in Wn.B3_FORMS:
        with Wn.Env(**env):
            outs.append(shape_case(twice_lab, T, two, True))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            for r, L in enumerate(shape_lengths(T)):
                assert np.array_equal(a[r, :, :L], b[r, :, :L])


@pytest.mark.parametrize("two,cond", SHAPE_OPTIONS)
def test_the_32x32x16_form_behind_the_lab_switch(twice_lab, two, cond):
    """Against fp64 under the same criterion, not bit for bit against the default: the sums inside an MFMA run over other channels."""
    for T in (17, 129):
        new = shape_case(twice_lab, T, two, cond)
        with Wn.Env(MI355VITS_WN_SHAPE=32):
            old = shape_case(twice_lab, T, two, cond)
        assert not np.array_equal(new[1], old[1])


def _voice(seed):
    cfg = VitsConfig.apope_low()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=seed, frames_per_id=3.0))


def test_bf16w_through_the_engine_on_both_shapes(lab_lib):
    """MATH_BF16W (the weights' leading bf16 term only): the two shapes form the same exact products and differ in the order of the f32
    sums alone, so each is within the engine tests' tight bound of the exactly summed result and the two within twice that."""
    cfg, blob = _voice(77)
    rng = np.random.default_rng(77)
    ids, lengths = rng.integers(1, cfg.num_symbols, (2, 20)), np.array([20, 13])
    out = {}
    for shape in (16, 32):
        with Wn.Env(MI355VITS_WN_SHAPE=shape):
            eng = Engine(blob, device=0, library=lab_lib)
            eng.set_math("bf16w")
            out[shape] = eng.run(ids, lengths, [0.0, 1.0, 0.0])
            eng.close()
    assert np.array_equal(out[16]["lengths"], out[32]["lengths"])
    for b, L in enumerate(int(n) for n in out[16]["lengths"]):
        e = rel_rms(out[16]["audio"][b, :L], out[32]["audio"][b, :L])
        print(f"bf16w row {b}: 16x16x32 vs 32x32x16 rel rms {e:.3e}")
        assert e < 2 * TIGHT_REL_RMS_TOL, (b, e)
        assert not np.array_equal(out[16]["audio"][b, :L], out[32]["audio"][b, :L])


def test_bf16w_forms_agree_bitwise_on_the_device(lab_lib, bf16w_voice):  # noqa: F811
    """k_wn_layer_b3<16, true, 1 / 3 / 4> forced through the lab switches (two short rows alone would only ever take the 32-column
    form; a large MATH_BF16W batch runs the wide ones): the same bits at the flow's output and in the waveform."""
    bf16w_forms_case(lab_lib, bf16w_voice, device=0)


def test_bf16w_the_two_shapes_agree_at_the_f32_level_on_the_device(lab_lib, bf16w_voice):  # noqa: F811
    for env in (dict(MI355VITS_WN_B3_NT=3), dict(MI355VITS_WN_B3_NT=4)):
        with Wn.Env(**env):
            bf16w_shapes_case(lab_lib, bf16w_voice, device=0)


def test_batched_equals_solo_on_a_nan_filled_workspace(gpu_hooks):
    """Six ragged rows on a handle whose workspace a larger batch sized first and a quiet NaN then filled: every row bit for bit its
    solo run on a fresh handle (the flow's WaveNet layers run on 16x16x32 tiles, 32 columns wide solo and batched alike here)."""
    cfg, blob = _voice(78)
    rng = np.random.default_rng(78)
    B, Tx = 6, 24
    lengths = np.array([24, 1, 17, 9, 24, 5])
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    scales = [0.0, 1.0, 0.0]
    fresh = Engine(blob, device=0, library=gpu_hooks)
    solo = [fresh.run(ids[b:b + 1, :n], [n], scales) for b, n in enumerate(lengths)]
    fresh.close()
    eng = Engine(blob, device=0, library=gpu_hooks)
    eng.run(rng.integers(1, cfg.num_symbols, (B + 2, Tx)), np.full(B + 2, Tx), scales, forced_durations=np.full((B + 2, Tx), 6, np.int32))
    eng.fill_workspace(0x7FC00000)
    out = eng.run(ids, lengths, scales)
    eng.close()
    assert np.isfinite(out["audio"]).all()
    for b in range(B):
        L = int(solo[b]["lengths"][0])
        assert L == int(out["lengths"][b]), b
        assert np.array_equal(solo[b]["audio"][0, :L], out["audio"][b, :L]), b
