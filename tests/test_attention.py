"""Relative-position attention, every kernel form against fp64 per element, on the CPU model of the kernels (tests/emu).
tests/test_gpu_attention.py runs the same case tables (tests/attention_ref.py) on the MI355X.

The model runs a workgroup's threads in order between barriers, so it checks indexing, masks, band ends and tile edges — not a
missing barrier: the device file repeats every case and demands equal bits for that."""
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError
from mimic3_amd.config import VitsConfig
from tests import attention_ref as A
from tests.util import check_parity

DEFAULT_CUS = 8  # what the CPU model reports unless a test sets another count


@pytest.fixture
def cu_count(emu_lib):
    """Sets the compute units the CPU model reports; restores the default afterwards."""
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(DEFAULT_CUS)


@pytest.mark.parametrize("T", A.MFMA_LENGTH_CLASSES)
def test_mfma_length_classes_vs_fp64(emu_lib, cu_count, T):
    """(a) k_rel_attention_mfma4<1,48>, <2,48> and <4> at d = 96.  The model reports 256 compute units here so that the grid
    (ceil(T / 32) * heads * rows workgroups) stays below four per unit and T <= 256 takes the prefetched forms, as on the device."""
    cu_count(256)
    A.check_vs_fp64(emu_lib, 1, T, 96, 2, 4, A.case_lengths(T))


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("T", A.HEAD_SHAPE_LENGTHS)
@pytest.mark.parametrize("d,n_heads,Wn", A.HEAD_SHAPES)
def test_head_shapes_vs_fp64(emu_lib, cu_count, impl, T, d, n_heads, Wn):
    """(b) the VALU kernel and the MFMA kernel's <1>, <2>, <4> forms.  d = 96 on the MFMA kernel runs twice: at the model's 8 units
    the grid takes the trips form, at 256 units (as on the device) the prefetched <1,48> / <2,48> with their nrel = 31 handling."""
    A.check_vs_fp64(emu_lib, impl, T, d, n_heads, Wn, A.case_lengths(T))
    if impl == 1 and d == 96:
        cu_count(256)
        A.check_vs_fp64(emu_lib, impl, T, d, n_heads, Wn, A.case_lengths(T))


@pytest.mark.parametrize("d,T,Wn", A.STREAM_CASES)
def test_stream_instantiations_vs_fp64(emu_lib, d, T, Wn):
    """(c) k_rel_attention_stream<8 | 16 | 32 | 48 | 64>."""
    A.check_vs_fp64(emu_lib, 2, T, d, 2, Wn, A.case_lengths(T))


@pytest.mark.parametrize("T,d,n_heads,Wn", A.AGREE_CASES)
def test_the_three_kernels_agree(emu_lib, T, d, n_heads, Wn):
    """(d)"""
    A.agree_case(emu_lib, T, d, n_heads, Wn)


@pytest.mark.parametrize("T", A.GRID_FORM_LENGTHS)
def test_grid_chosen_form_is_the_same_function(emu_lib, cu_count, T):
    """(e) launch_rel_attention_mfma takes the prefetched form <NKW, 48> at d = 96 unless ceil(T / 32) * n_heads * B >= 4 x the
    compute units, where the 76-register trips form <NKW> runs.  Batch 4 at 256 units: prefetched; batch 16 at 8 units: trips.
    The hook cannot report which form ran; tests/test_emu_engine.py forces the form by its lab switch."""
    def run(cus):
        def f(qkv, ek, ev, ln, n_heads):
            cu_count(cus)
            return emu_lib.test_rel_attention(qkv, ek, ev, ln, n_heads, impl=1)
        return f
    A.grid_form_case(run(256), run(8), T, 16)


@pytest.mark.parametrize("impl", [0, 1, 2])
def test_rows_do_not_depend_on_padding(emu_lib, cu_count, impl):
    """(f)"""
    cu_count(256)
    A.padding_case(emu_lib, impl)


@pytest.mark.parametrize("impl,T,d,n_heads,Wn,message", A.REFUSALS)
def test_hook_refuses_unsupported_shapes(emu_lib, impl, T, d, n_heads, Wn, message):
    """(g) refused before any launch."""
    if T == "cap + 1":
        T = A.valu_cap(d, n_heads, Wn) + 1
    qkv, ek, ev, ln = A.attention_case(T, d, [T], n_heads, Wn)
    with pytest.raises(NativeError, match=message):
        emu_lib.test_rel_attention(qkv, ek, ev, ln, n_heads, impl=impl)


def test_valu_kernel_serves_its_cap(emu_lib):
    """(g) the other side of the VALU refusal: T = cap is served (rows far shorter than T, so the fp64 reference stays small)."""
    d, n_heads, Wn = 16, 2, 4
    cap = A.valu_cap(d, n_heads, Wn)
    assert cap == 4096 - d - (2 * Wn + 1)
    A.check_vs_fp64(emu_lib, 0, cap, d, n_heads, Wn, [33, 17])


def voice(n_heads, window_size):
    cfg = VitsConfig.tiny()
    cfg.n_heads, cfg.window_size = n_heads, window_size
    return cfg


@pytest.mark.parametrize("n_heads,window_size", A.VOICE_SHAPES)
def test_voices_with_other_attention_shapes(emu_lib, n_heads, window_size):
    """(h) the tiny voice with one and four heads and windows 0 .. 15, every tap against the oracle."""
    out, _ = check_parity(emu_lib, voice(n_heads, window_size), B=3, Tx=70, noise=True, frames_per_id=1.1)
    print("tap errors", n_heads, window_size, out["tap_errors"])


def test_voice_with_window_16_is_refused(emu_lib):
    """(h) window 16: the MFMA and the streamed kernel refuse it, and so does the voice format (validate_config caps the window
    at 15), so no voice reaches the VALU fallback with it: loading fails, nothing is computed."""
    cfg = voice(*A.VOICE_REFUSED)
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=100, frames_per_id=1.1))
    with pytest.raises(NativeError, match="invalid voice config"):
        Engine(blob, library=emu_lib)
