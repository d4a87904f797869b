"""Relative-position attention on the MI355X (pytest -m gpu): every kernel form against fp64 per element, over the case tables
of tests/attention_ref.py that tests/test_attention.py runs on the CPU model.  Every hook call here is made TWICE and must return
equal bits: the MFMA kernel reuses its LDS tables (tab, red, ored) across five barriers, and only the device can show a race."""
import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError
from tests import attention_ref as A
from tests.test_attention import voice
from tests.util import check_parity

pytestmark = pytest.mark.gpu


class Twice:
    """The hooks library with every attention call repeated: the two results must be the same bits."""

    def __init__(self, lib):
        self.lib = lib

    def test_rel_attention(self, qkv, ek, ev, ln, n_heads, impl):
        a = self.lib.test_rel_attention(qkv, ek, ev, ln, n_heads, impl=impl)
        b = self.lib.test_rel_attention(qkv, ek, ev, ln, n_heads, impl=impl)
        assert np.array_equal(a, b), (A.IMPL_NAMES[impl], qkv.shape, "two runs of one case differ")
        return a


@pytest.fixture(scope="module")
def twice(gpu_hooks):
    return Twice(gpu_hooks)


@pytest.mark.parametrize("T", A.MFMA_LENGTH_CLASSES)
def test_mfma_length_classes_vs_fp64(twice, T):
    """(a) k_rel_attention_mfma4<1,48>, <2,48> and <4> at d = 96 (at most 7 rows: far below four workgroups per compute unit)."""
    A.check_vs_fp64(twice, 1, T, 96, 2, 4, A.case_lengths(T))


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("T", A.HEAD_SHAPE_LENGTHS)
@pytest.mark.parametrize("d,n_heads,Wn", A.HEAD_SHAPES)
def test_head_shapes_vs_fp64(twice, impl, T, d, n_heads, Wn):
    """(b) the VALU kernel and the MFMA kernel's <1>, <2>, <4> forms."""
    A.check_vs_fp64(twice, impl, T, d, n_heads, Wn, A.case_lengths(T))


@pytest.mark.parametrize("d,T,Wn", A.STREAM_CASES)
def test_stream_instantiations_vs_fp64(twice, d, T, Wn):
    """(c) k_rel_attention_stream<8 | 16 | 32 | 48 | 64>."""
    A.check_vs_fp64(twice, 2, T, d, 2, Wn, A.case_lengths(T))


@pytest.mark.parametrize("T,d,n_heads,Wn", A.AGREE_CASES)
def test_the_three_kernels_agree(twice, T, d, n_heads, Wn):
    """(d)"""
    A.agree_case(twice, T, d, n_heads, Wn)


@pytest.mark.parametrize("T", A.GRID_FORM_LENGTHS)
def test_grid_chosen_form_is_the_same_function(twice, T):
    """(e) launch_rel_attention_mfma takes the prefetched form <NKW, 48> at d = 96 unless ceil(T / 32) * n_heads * B >= 4 x the
    compute units, where the 76-register trips form <NKW> runs (the form that serves batch 256).  Batch 4 is prefetched; the large
    batch has >= 8 * 256 workgroups — twice the threshold of a 256-unit part, so it holds on any partition of it.  The hook cannot
    report which form ran; tests/test_gpu_lab_ab.py forces the form by its lab switch."""
    B = 4
    while -(-T // 32) * 2 * B < 8 * 256:
        B *= 2
    run = lambda qkv, ek, ev, ln, n_heads: twice.test_rel_attention(qkv, ek, ev, ln, n_heads, impl=1)
    A.grid_form_case(run, run, T, B)


@pytest.mark.parametrize("impl", [0, 1, 2])
def test_rows_do_not_depend_on_padding(twice, impl):
    """(f)"""
    A.padding_case(twice, impl)


@pytest.mark.parametrize("n_heads,window_size", A.VOICE_SHAPES)
def test_voices_with_other_attention_shapes(gpu_lib, n_heads, window_size):
    """(h) the tiny voice with one and four heads and windows 0 .. 15, every tap against the oracle."""
    out, _ = check_parity(gpu_lib, voice(n_heads, window_size), B=3, Tx=70, noise=True, frames_per_id=1.1)
    print("tap errors", n_heads, window_size, out["tap_errors"])


def test_voice_with_window_16_is_refused(gpu_lib):
    """(h) window 16 is above the voice format's cap: loading fails, nothing is computed (see tests/test_attention.py)."""
    cfg = voice(*A.VOICE_REFUSED)
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=100, frames_per_id=1.1))
    with pytest.raises(NativeError, match="invalid voice config"):
        Engine(blob, library=gpu_lib)
