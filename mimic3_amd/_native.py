"""ctypes binding of ``libmi355vits.so`` (C ABI: ``include/mi355vits.h``).

The product path loads exactly one file — ``mimic3_amd/csrc/libmi355vits.so`` built by hipcc for
gfx950 — and raises if it is missing or if no HIP device is visible.  There is no CPU fallback.
(``NativeLibrary(path)`` accepts an explicit path only so the test-suite can point the same
binding at its CPU model of the kernels, ``tests/emu/libmi355vits_emu.so``.)
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import threading
from typing import Dict, List, Optional, Tuple

import numpy as np

from .config import CVitsConfig, VitsConfig

WANT_FLOAT = 1
WANT_PCM16 = 2
DEVICE_ONLY = 4
DEBUG_TAPS = 8

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIBRARY = os.path.join(_HERE, "csrc", "libmi355vits.so")
# the product's own objects + the hooks of include/mi355vits_lab.h (kernel unit tests, box probes): test infrastructure and bench.py's
# box probe; the product path (session.py, Engine) never opens it
HOOKS_LIBRARY = os.path.join(_HERE, "csrc", "libmi355vits_hooks.so")

# every symbol include/mi355vits.h declares (the product ABI)
EXPORTED_SYMBOLS = (
    "mi355vits_version", "mi355vits_device_count", "mi355vits_create", "mi355vits_create_from_buffer", "mi355vits_clone", "mi355vits_destroy",
    "mi355vits_device_result", "mi355vits_set_math", "mi355vits_get_math",
    "mi355vits_get_config", "mi355vits_run", "mi355vits_run_rows", "mi355vits_run_timed", "mi355vits_run_speakers", "mi355vits_run_levels", "mi355vits_run_pitch",
    "mi355vits_get_speaker_embedding", "mi355vits_fetch", "mi355vits_free_result",
    "mi355vits_last_error", "mi355vits_profile_enable", "mi355vits_profile_reset",
    "mi355vits_profile_report", "mi355vits_last_run_ms", "mi355vits_get_tap", "mi355vits_get_tap_rows", "mi355vits_list_taps",
    "mi355vits_run_packed", "mi355vits_fetch_packed", "mi355vits_free_packed",
    "mi355vits_set_output_rate", "mi355vits_get_output_rate",
    "mi355vits_set_output_encoding", "mi355vits_get_output_encoding",
    "mi355vits_set_output_compression", "mi355vits_get_output_compression",
    "mi355vits_fetch_alignment", "mi355vits_free_alignment",
    "mi355vits_set_edge_trim", "mi355vits_get_edge_trim", "mi355vits_fetch_edges", "mi355vits_free_edges",
    "mi355vits_set_loudness_target", "mi355vits_get_loudness_target", "mi355vits_fetch_loudness", "mi355vits_free_loudness",
    "mi355vits_run_streams", "mi355vits_fetch_streams", "mi355vits_free_streams",
    "mi355vits_run_streams2", "mi355vits_fetch_streams2", "mi355vits_free_streams2",
    "mi355vits_set_loudness_limiter", "mi355vits_get_loudness_limiter", "mi355vits_fetch_limiter", "mi355vits_free_limiter",
    "mi355vits_set_loudness_ceiling_mode", "mi355vits_get_loudness_ceiling_mode", "mi355vits_fetch_true_peak", "mi355vits_free_true_peak",
)
# every symbol include/mi355vits_lab.h declares: exported by libmi355vits_hooks.so, the lab build and the CPU model — NOT by the product
LAB_SYMBOLS = (
    "mi355vits_test_conv1d", "mi355vits_test_conv_transpose1d", "mi355vits_test_mfma_layout", "mi355vits_bench_conv1d", "mi355vits_probe_device", "mi355vits_probe_weights",
    "mi355vits_test_rel_attention", "mi355vits_test_fill_workspace", "mi355vits_test_resample",
    "mi355vits_lab_g711_encode", "mi355vits_test_alignment", "mi355vits_lab_edges",
    "mi355vits_lab_loudness", "mi355vits_lab_loudness_plan", "mi355vits_lab_limit",
    "mi355vits_lab_limit_env", "mi355vits_lab_true_peak", "mi355vits_lab_true_peak_plan", "mi355vits_lab_flac", "mi355vits_lab_flac_jobs",
    "mi355vits_test_wn_layer", "mi355vits_lab_wn_plan", "mi355vits_lab_pack_w16", "mi355vits_test_mrf_stage", "mi355vits_lab_mrf_plan",
    "mi355vits_test_dds_stack", "mi355vits_test_spline_inverse", "mi355vits_test_durations", "mi355vits_test_expand_prior",
    "mi355vits_test_fit_durations", "mi355vits_test_speaker_cond", "mi355vits_test_speaker_cond_mix", "mi355vits_test_levels",
    "mi355vits_test_pitch_table", "mi355vits_test_pitch_plan", "mi355vits_test_pitch",
    "mi355vits_lab_conv_plan", "mi355vits_test_enc_o_ln", "mi355vits_test_conv_post",
    "mi355vits_test_embed", "mi355vits_test_layernorm", "mi355vits_test_dp_det", "mi355vits_lab_dp_det_plan", "mi355vits_test_sdp_noise",
    "mi355vits_test_expand_prior_keyed",
)


class NativeError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"mi355vits error {code}: {message}")
        self.code = code


class WnTest(ctypes.Structure):
    """struct mi355vits_wn_test of include/mi355vits_lab.h"""
    _fields_ = [(n, ctypes.c_int32) for n in ("impl", "B", "H", "T", "K", "dilation", "Crs", "skip_init", "math")] + [
        (n, ctypes.POINTER(ctypes.c_float)) for n in ("h_in", "w_in", "b_in", "w_rs", "b_rs", "cond")] + [
        ("len", ctypes.POINTER(ctypes.c_int32)), ("h_out", ctypes.POINTER(ctypes.c_float)), ("skip", ctypes.POINTER(ctypes.c_float))]


class MrfTest(ctypes.Structure):
    """struct mi355vits_mrf_test of include/mi355vits_lab.h"""
    _fields_ = [(n, ctypes.c_int32) for n in ("impl", "B", "C", "T", "nrb", "math", "seg")] + [
        (n, ctypes.c_int32 * 4) for n in ("k", "d1", "d2")] + [
        ("x", ctypes.POINTER(ctypes.c_float)), ("w", (ctypes.POINTER(ctypes.c_float) * 2) * 4),
        ("bias", (ctypes.POINTER(ctypes.c_float) * 2) * 4), ("len", ctypes.POINTER(ctypes.c_int32)),
        ("out_scale", ctypes.c_float), ("y", ctypes.POINTER(ctypes.c_float))]


class DdsStackTest(ctypes.Structure):
    """struct mi355vits_dds_stack_test of include/mi355vits_lab.h"""
    _fields_ = [(n, ctypes.c_int32) for n in ("impl", "math", "B", "C", "T", "K", "n_layers", "pre_mode", "zch", "proj_cout", "spline", "nb")] + [
        ("tail", ctypes.c_float), ("inv_sqrt_fc", ctypes.c_float)] + [
        (n, ctypes.POINTER(ctypes.c_float)) for n in ("src", "pre_w", "pre_b", "cond")] + [
        (n, ctypes.POINTER(ctypes.c_float) * 4) for n in ("dw_w", "dw_b", "g1", "b1", "w1x1", "bias1x1", "g2", "b2")] + [
        ("proj_w", ctypes.POINTER(ctypes.c_float)), ("proj_b", ctypes.POINTER(ctypes.c_float)), ("len", ctypes.POINTER(ctypes.c_int32)),
        ("z", ctypes.POINTER(ctypes.c_float)), ("out", ctypes.POINTER(ctypes.c_float)), ("x_out", ctypes.POINTER(ctypes.c_float))]


class LayerNormTest(ctypes.Structure):
    """struct mi355vits_layernorm_test of include/mi355vits_lab.h"""
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "C", "T", "nparts", "gelu", "alias")] + [("eps", ctypes.c_float), ("part_stride", ctypes.c_int64),
        ("x", ctypes.POINTER(ctypes.c_float)), ("bias", ctypes.POINTER(ctypes.c_float)), ("premask_len", ctypes.POINTER(ctypes.c_int32)),
        ("res", ctypes.POINTER(ctypes.c_float)), ("add_to", ctypes.POINTER(ctypes.c_float)), ("gamma", ctypes.POINTER(ctypes.c_float)),
        ("beta", ctypes.POINTER(ctypes.c_float)), ("out_len", ctypes.POINTER(ctypes.c_int32)), ("y", ctypes.POINTER(ctypes.c_float))]


class DpDetTest(ctypes.Structure):
    """struct mi355vits_dp_det_test of include/mi355vits_lab.h"""
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "H", "F", "K", "T", "math")] + [
        ("x", ctypes.POINTER(ctypes.c_float)), ("cond", ctypes.POINTER(ctypes.c_float)), ("len", ctypes.POINTER(ctypes.c_int32))] + [
        (n, ctypes.POINTER(ctypes.c_float)) for n in ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "proj_w", "proj_b", "logw")]


LN_ALIAS = {None: 0, "x": 1, "res": 2, "add_to": 3}  # mi355vits_layernorm_test.alias
MATH_F32, MATH_BF16X3, MATH_BF16W = 0, 1, 2  # csrc/kernels.h MathMode, MI355VITS_MATH_*


class RunArgs(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32),
        ("tx_max", ctypes.c_int32),
        ("ids", ctypes.POINTER(ctypes.c_int64)),
        ("lengths", ctypes.POINTER(ctypes.c_int64)),
        ("scales", ctypes.POINTER(ctypes.c_float)),
        ("sid", ctypes.POINTER(ctypes.c_int64)),
        ("seed", ctypes.c_uint64),
        ("utterance_base", ctypes.c_uint64),
        ("noise_w", ctypes.POINTER(ctypes.c_float)),
        ("noise_z", ctypes.POINTER(ctypes.c_float)),
        ("noise_z_frames", ctypes.c_int32),
        ("forced_durations", ctypes.POINTER(ctypes.c_int32)),
        ("flags", ctypes.c_uint32),
        ("pcm_volume", ctypes.c_double),
    ]


class RowArgs(ctypes.Structure):
    _fields_ = [
        ("scales", ctypes.POINTER(ctypes.c_float)),
        ("pcm_volume", ctypes.POINTER(ctypes.c_double)),
        ("utterance", ctypes.POINTER(ctypes.c_uint64)),
    ]


class TimingArgs(ctypes.Structure):  # mi355vits_timing_args
    _fields_ = [
        ("stretch", ctypes.POINTER(ctypes.c_float)),
        ("min_frames", ctypes.POINTER(ctypes.c_int32)),
        ("target_frames", ctypes.POINTER(ctypes.c_int32)),
        ("factor_out", ctypes.POINTER(ctypes.c_float)),
        ("reserved", ctypes.c_int32 * 6),
    ]


class SpeakerArgs(ctypes.Structure):  # mi355vits_speaker_args
    _fields_ = [
        ("n_terms", ctypes.c_int32),
        ("mix_sid", ctypes.POINTER(ctypes.c_int64)),
        ("mix_weight", ctypes.POINTER(ctypes.c_float)),
        ("vectors", ctypes.POINTER(ctypes.c_float)),
        ("reserved", ctypes.c_int32 * 6),
    ]


MAX_SPEAKER_TERMS = 8  # MI355VITS_MAX_SPEAKER_TERMS


class LevelArgs(ctypes.Structure):  # mi355vits_level_args
    _fields_ = [
        ("gain", ctypes.POINTER(ctypes.c_float)),
        ("ramp_samples", ctypes.POINTER(ctypes.c_int32)),
        ("reserved", ctypes.c_int32 * 6),
    ]


class PitchArgs(ctypes.Structure):  # mi355vits_pitch_args
    _fields_ = [
        ("ratio", ctypes.POINTER(ctypes.c_float)),
        ("reserved", ctypes.c_int32 * 7),
    ]


class SpeakerMixTest(ctypes.Structure):  # mi355vits_speaker_mix_test (include/mi355vits_lab.h)
    _fields_ = [
        ("B", ctypes.c_int32), ("gin", ctypes.c_int32), ("n_speakers", ctypes.c_int32), ("n_terms", ctypes.c_int32),
        ("n_jobs", ctypes.c_int32),
        ("emb_g", ctypes.POINTER(ctypes.c_float)),
        ("mix_sid", ctypes.POINTER(ctypes.c_int64)),
        ("mix_weight", ctypes.POINTER(ctypes.c_float)),
        ("vectors", ctypes.POINTER(ctypes.c_float)),
        ("w", ctypes.POINTER(ctypes.c_float) * 10),
        ("bias", ctypes.POINTER(ctypes.c_float) * 10),
        ("Cout", ctypes.c_int32 * 10),
        ("out", ctypes.POINTER(ctypes.c_float) * 10),
        ("out_floats", ctypes.c_size_t * 10),
        ("g", ctypes.POINTER(ctypes.c_float)),
        ("g_floats", ctypes.c_size_t),
    ]


def speaker_tables(speakers, n_rows: int, gin: int):
    """``speakers`` (one entry per row: an ``int`` = that speaker as a one-term mix of weight 1, a dict ``{sid: weight}``, or a 1-D
    float array of ``gin`` values) as the tables of ``mi355vits_speaker_args``: ``("mix", sid [B, K] int64, weight [B, K] float32)``
    — dicts and ints padded with zero-weight terms to the longest row, a dict's terms in its own order — or ``("vectors", v [B,
    gin] float32)``.  Entries of both kinds in one call raise ``ValueError``: the ABI takes one kind per call."""
    speakers = list(speakers)
    if len(speakers) != n_rows:
        raise ValueError("speakers must have one entry per row")
    is_mix = [isinstance(e, (dict, int, np.integer)) and not isinstance(e, bool) for e in speakers]
    if all(is_mix):
        rows = [list(e.items()) if isinstance(e, dict) else [(int(e), 1.0)] for e in speakers]
        K = max(len(r) for r in rows)
        if K < 1:
            raise ValueError("a speaker mix needs at least one term")
        if K > MAX_SPEAKER_TERMS:
            raise ValueError(f"a speaker mix takes at most {MAX_SPEAKER_TERMS} terms")
        sid, w = np.zeros((n_rows, K), np.int64), np.zeros((n_rows, K), np.float32)
        for b, r in enumerate(rows):
            for k, (s, x) in enumerate(r):
                sid[b, k], w[b, k] = int(s), np.float32(x)
        return "mix", sid, w
    if any(is_mix):
        raise ValueError("speakers: mixes (int / dict) and vectors go in calls of their own")
    v = [np.asarray(e, np.float32) for e in speakers]
    if any(e.shape != (gin,) for e in v):
        raise ValueError("a speaker vector must be a 1-D array of gin_channels values")
    return "vectors", np.ascontiguousarray(np.stack(v), dtype=np.float32)


class Result(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32),
        ("l_max", ctypes.c_int64),
        ("ty_max", ctypes.c_int64),
        ("audio", ctypes.POINTER(ctypes.c_float)),
        ("pcm", ctypes.POINTER(ctypes.c_int16)),
        ("lengths", ctypes.POINTER(ctypes.c_int64)),
        ("peaks", ctypes.POINTER(ctypes.c_float)),
        ("owner_", ctypes.c_void_p),
    ]


class PackArgs(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int32),
        ("order", ctypes.POINTER(ctypes.c_int32)),
        ("lead_samples", ctypes.POINTER(ctypes.c_int64)),
        ("tail_samples", ctypes.c_int64),
        ("wav_header", ctypes.c_int32),
    ]


class PackedResult(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int32),
        ("total_samples", ctypes.c_int64),
        ("bytes", ctypes.POINTER(ctypes.c_uint8)),
        ("n_bytes", ctypes.c_size_t),
        ("pcm", ctypes.POINTER(ctypes.c_int16)),
        ("offsets", ctypes.POINTER(ctypes.c_int64)),
        ("lengths", ctypes.POINTER(ctypes.c_int64)),
        ("peaks", ctypes.POINTER(ctypes.c_float)),
        ("owner_", ctypes.c_void_p),
    ]


class StreamArgs(ctypes.Structure):
    _fields_ = [
        ("pack", PackArgs),
        ("encoding", ctypes.c_int32),
        ("trim_ratio", ctypes.c_float),
        ("trim_keep_samples", ctypes.c_int32),
        ("target_lufs", ctypes.c_float),
        ("ceiling_dbfs", ctypes.c_float),
    ]


class StreamsResult(ctypes.Structure):
    _fields_ = [
        ("n_streams", ctypes.c_int32),
        ("n_entries", ctypes.c_int32),
        ("bytes", ctypes.POINTER(ctypes.c_uint8)),
        ("n_bytes", ctypes.c_size_t),
        ("stream_offset", ctypes.POINTER(ctypes.c_int64)),
        ("stream_bytes", ctypes.POINTER(ctypes.c_int64)),
        ("data_offset", ctypes.POINTER(ctypes.c_int64)),
        ("total_samples", ctypes.POINTER(ctypes.c_int64)),
        ("encoding", ctypes.POINTER(ctypes.c_int32)),
        ("entry_base", ctypes.POINTER(ctypes.c_int32)),
        ("rows", ctypes.POINTER(ctypes.c_int32)),
        ("offsets", ctypes.POINTER(ctypes.c_int64)),
        ("lengths", ctypes.POINTER(ctypes.c_int64)),
        ("peaks", ctypes.POINTER(ctypes.c_float)),
        ("first", ctypes.POINTER(ctypes.c_int32)),
        ("lufs", ctypes.POINTER(ctypes.c_double)),
        ("gain", ctypes.POINTER(ctypes.c_double)),
        ("limited", ctypes.POINTER(ctypes.c_int32)),
        ("owner_", ctypes.c_void_p),
    ]


class StreamArgs2(ctypes.Structure):
    _fields_ = [
        ("base", StreamArgs),
        ("compression", ctypes.c_int32),
        ("limiter_window_samples", ctypes.c_int32),
        ("ceiling_mode", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 5),
    ]


class StreamsResult2(ctypes.Structure):
    _fields_ = StreamsResult._fields_[:-1] + [
        ("compression", ctypes.POINTER(ctypes.c_int32)),
        ("frames", ctypes.POINTER(ctypes.c_int32)),
        ("uncompressed_bytes", ctypes.c_int64),
        ("owner_", ctypes.c_void_p),
    ]


class AlignmentResult(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32),
        ("tx_max", ctypes.c_int32),
        ("sample_rate", ctypes.c_int32),
        ("frames", ctypes.POINTER(ctypes.c_int32)),
        ("start", ctypes.POINTER(ctypes.c_int32)),
        ("samples", ctypes.POINTER(ctypes.c_int32)),
        ("peak", ctypes.POINTER(ctypes.c_float)),
        ("rms", ctypes.POINTER(ctypes.c_float)),
        ("owner_", ctypes.c_void_p),
    ]


ALIGN_LEVELS = 1


class EdgesResult(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32),
        ("sample_rate", ctypes.c_int32),
        ("ratio", ctypes.c_float),
        ("keep_samples", ctypes.c_int32),
        ("first", ctypes.POINTER(ctypes.c_int32)),
        ("end", ctypes.POINTER(ctypes.c_int32)),
        ("owner_", ctypes.c_void_p),
    ]


class LoudnessResult(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32),
        ("sample_rate", ctypes.c_int32),
        ("target_lufs", ctypes.c_float),
        ("ceiling_dbfs", ctypes.c_float),
        ("lufs", ctypes.POINTER(ctypes.c_double)),
        ("gain", ctypes.POINTER(ctypes.c_double)),
        ("blocks", ctypes.POINTER(ctypes.c_int32)),
        ("gated", ctypes.POINTER(ctypes.c_int32)),
        ("limited", ctypes.POINTER(ctypes.c_int32)),
        ("owner_", ctypes.c_void_p),
    ]


class LimiterResult(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32),
        ("sample_rate", ctypes.c_int32),
        ("window_samples", ctypes.c_int32),
        ("engaged", ctypes.POINTER(ctypes.c_int32)),
        ("reduced_samples", ctypes.POINTER(ctypes.c_int32)),
        ("min_scale", ctypes.POINTER(ctypes.c_double)),
        ("owner_", ctypes.c_void_p),
    ]


class Limiter:
    """What the look-ahead peak limiter does to every row of a run under the handle's target, ceiling and window
    (``mi355vits_fetch_limiter``): ``engaged`` [B] bool where the ceiling would hold the row's gain back (the limiter acts on it),
    ``reduced_samples`` [B] the samples whose scale lies below the row's full gain, ``min_scale`` [B] float64 the smallest factor
    the curve applies on top of the gain (1.0 for a row it leaves alone).  ``window_samples`` 0: off — all zeros / 1.0.  The arrays
    are copies owned by Python."""

    def __init__(self, engaged, reduced_samples, min_scale, window_samples, sample_rate):
        self.engaged, self.reduced_samples, self.min_scale = engaged, reduced_samples, min_scale
        self.window_samples, self.sample_rate = window_samples, sample_rate


LIMITER_MAX_WINDOW = 4096  # samples: mi355vits_set_loudness_limiter


class TruePeakResult(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32),
        ("sample_rate", ctypes.c_int32),
        ("true_peak", ctypes.POINTER(ctypes.c_double)),
        ("peak", ctypes.POINTER(ctypes.c_float)),
        ("owner_", ctypes.c_void_p),
    ]


class TruePeak:
    """The 4x oversampled peak of every row of a run (``mi355vits_fetch_true_peak``): ``true_peak`` [B] float64, linear, ``peak`` [B]
    float32 the rows' sample peaks (bitwise the run's ``peaks``), ``dbtp`` [B] float64 = 20 log10(true_peak) (``-inf`` for 0).
    ``sample_rate`` is the rate the run ran at.  The arrays are copies owned by Python."""

    def __init__(self, true_peak, peak, sample_rate):
        self.true_peak, self.peak, self.sample_rate = true_peak, peak, sample_rate
        with np.errstate(divide="ignore"):
            self.dbtp = 20.0 * np.log10(true_peak)


CEILING_MODES = {"sample": 0, "true_peak": 1}  # mi355vits_set_loudness_ceiling_mode: MI355VITS_CEILING_*


def ceiling_mode_id(mode) -> int:
    """``"sample"`` / ``"true_peak"`` (or ``False`` / ``True``) as the ABI's value; anything else raises ``ValueError`` naming it."""
    if isinstance(mode, (bool, np.bool_)):
        return int(mode)
    if mode not in CEILING_MODES:
        raise ValueError(f"ceiling mode {mode!r} is neither 'sample' nor 'true_peak'")
    return CEILING_MODES[mode]


def limiter_window(ms, rate) -> int:
    """A limiter window in milliseconds as samples at ``rate`` Hz (``round(ms * rate / 1000)``); ``None`` = off = 0.  A window
    outside 1 .. 4096 samples raises ``ValueError`` naming it."""
    if ms is None:
        return 0
    n = float(ms) * float(rate) / 1000.0
    if not (n == n and abs(n) < 1e12) or not 1 <= int(round(n)) <= LIMITER_MAX_WINDOW:
        raise ValueError(f"limiter window of {ms!r} ms is {n:g} samples at {rate} Hz: outside 1 .. {LIMITER_MAX_WINDOW}")
    return int(round(n))


class Loudness:
    """ITU-R BS.1770-4 integrated loudness of every row of a run (``mi355vits_fetch_loudness``): ``lufs`` [B] float64 (``-inf``
    where no block passes the absolute gate), ``blocks`` / ``gated`` [B] the 400 ms blocks of the row and those passing both
    gates, and under the setting ``target_lufs`` / ``ceiling_dbfs`` (target 0.0: off) the linear ``gain`` [B] a packed stream
    applies (0.0 when off) and ``limited`` [B] bool where the ceiling bounded it.  ``sample_rate`` is the rate the run ran at.
    The arrays are copies owned by Python."""

    def __init__(self, lufs, gain, blocks, gated, limited, target_lufs, ceiling_dbfs, sample_rate):
        self.lufs, self.gain, self.blocks, self.gated, self.limited = lufs, gain, blocks, gated, limited
        self.target_lufs, self.ceiling_dbfs, self.sample_rate = target_lufs, ceiling_dbfs, sample_rate


class Edges:
    """The kept part of every row of a run under an edge-trim setting (``mi355vits_fetch_edges``): row b keeps samples
    ``first[b] : end[b]`` at ``sample_rate``, the rate the run ran at; ``ratio`` / ``keep_samples`` the setting the arrays were made
    with (ratio 0: off — ``first`` = 0, ``end`` = the lengths).  The arrays are copies owned by Python."""

    def __init__(self, first, end, ratio, keep_samples, sample_rate):
        self.first, self.end, self.ratio, self.keep_samples, self.sample_rate = first, end, ratio, keep_samples, sample_rate


class Alignment:
    """Where in a run's audio each phoneme sits (``mi355vits_fetch_alignment``): ``frames`` / ``start`` / ``samples`` [B, Tx]
    integer arrays — phoneme t of row b is samples ``start[b, t] : start[b, t] + samples[b, t]`` of that row at ``sample_rate``,
    the rate the run ran at; the spans tile the row — and with levels ``peak`` / ``rms`` [B, Tx] float32 over each span of the
    float waveform (else ``None``).  All arrays are copies owned by Python."""

    def __init__(self, frames, start, samples, peak=None, rms=None, sample_rate=None):
        self.frames, self.start, self.samples, self.peak, self.rms = frames, start, samples, peak, rms
        self.sample_rate = sample_rate


WAV_HEADER_BYTES = 44
WAV_HEADER_BYTES_NON_PCM = 58  # fmt 18 + fact: the header of a packed stream in any encoding but s16le
# mi355vits_set_output_encoding: name -> (MI355VITS_ENC_*, numpy dtype of a sample)
ENCODINGS = {"s16le": (0, "<i2"), "ulaw": (1, "u1"), "alaw": (2, "u1"), "f32le": (3, "<f4")}
_ENCODING_NAMES = {v[0]: k for k, v in ENCODINGS.items()}


# mi355vits_set_output_compression: name -> MI355VITS_COMPRESS_*
COMPRESSIONS = {None: 0, "none": 0, "flac": 1}
FLAC_HEADER_BYTES = 42  # "fLaC" + the STREAMINFO block: the first frame starts here
_HANDLE = object()  # compression=: "whatever the handle's setting is"


def compression_id(compression) -> int:
    """``"flac"`` / ``None`` (or ``"none"``, or the MI355VITS_COMPRESS_* value itself) -> MI355VITS_COMPRESS_*; an unknown name raises
    ``ValueError``, an unknown number is left to the library to refuse."""
    if compression is None or isinstance(compression, str):
        key = compression.lower() if isinstance(compression, str) else None
        if key not in COMPRESSIONS:
            raise ValueError(f"unknown output compression {compression!r} ('flac' or None)")
        return COMPRESSIONS[key]
    return int(compression)


def encoding_id(encoding) -> int:
    """``"s16le"`` / ``"ulaw"`` / ``"alaw"`` / ``"f32le"`` (or the MI355VITS_ENC_* value itself) -> MI355VITS_ENC_*; an unknown
    name raises ``ValueError``, an unknown number is left to the library to refuse."""
    if isinstance(encoding, str):
        if encoding.lower() not in ENCODINGS:
            raise ValueError(f"unknown output encoding {encoding!r} (one of {', '.join(ENCODINGS)})")
        return ENCODINGS[encoding.lower()][0]
    return int(encoding)


class ConvTest(ctypes.Structure):
    _fields_ = [
        ("impl", ctypes.c_int32), ("B", ctypes.c_int32), ("Cin", ctypes.c_int32), ("Cout", ctypes.c_int32),
        ("T", ctypes.c_int32), ("K", ctypes.c_int32), ("dilation", ctypes.c_int32),
        ("x", ctypes.POINTER(ctypes.c_float)), ("w", ctypes.POINTER(ctypes.c_float)),
        ("bias", ctypes.POINTER(ctypes.c_float)), ("res", ctypes.POINTER(ctypes.c_float)),
        ("in_len", ctypes.POINTER(ctypes.c_int32)), ("out_len", ctypes.POINTER(ctypes.c_int32)),
        ("in_slope", ctypes.c_float), ("relu", ctypes.c_int32), ("out_scale", ctypes.c_float),
        ("res_sub", ctypes.c_int32), ("y", ctypes.POINTER(ctypes.c_float)), ("accumulate", ctypes.c_int32),
        ("math", ctypes.c_int32), ("cond", ctypes.POINTER(ctypes.c_float)), ("mask_before_res", ctypes.c_int32),
        ("fixed_rule", ctypes.c_int32),
    ]


class ConvPlan(ctypes.Structure):
    """include/mi355vits_lab.h: mi355vits_conv_plan."""
    _fields_ = [(n, ctypes.c_int32) for n in ("kernel", "cols", "rows", "MT", "NT", "WM", "WN", "chunk", "ring", "rb_loop", "vec", "yvec",
                                                "ovec")] + [("grid", ctypes.c_int32 * 3), ("lds_bytes", ctypes.c_int32)]

    @property
    def tile(self):
        return (self.MT, self.NT, self.WM, self.WN)


# mi355vits_conv_plan.kernel (MI355VITS_CONVK_*)
(CONVK_GENERIC, CONVK_F32_STAGED, CONVK_F32_DIRECT, CONVK_F32_SPLITK, CONVK_B3_STAGED32, CONVK_B3_STAGED64, CONVK_B3_PC, CONVK_ENC_B3,
 CONVK_ENC_B3W8, CONVK_ENC_B3W6, CONVK_RB_CONV, CONVK_RB_CONV_PW, CONVK_UPS_PL, CONVK_UPS64, CONVK_CONVT_GENERIC) = range(15)


def _fptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _ptr(a: Optional[np.ndarray]):
    """The ctypes pointer of an array's own element type (None stays None: an absent optional argument)."""
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


class NativeLibrary:
    """One loaded copy of the C ABI."""

    def __init__(self, path: Optional[str] = None):
        self.path = path or DEFAULT_LIBRARY
        if not os.path.exists(self.path):
            raise RuntimeError(
                f"native library not found: {self.path}. Build it with `python -m mimic3_amd.build hip` "
                "(hipcc --offload-arch=gfx950). The MI355X engine has no CPU fallback."
            )
        self.lib = ctypes.CDLL(self.path)
        L = self.lib
        for sym in EXPORTED_SYMBOLS:
            if not hasattr(L, sym):
                raise RuntimeError(f"{self.path} does not export {sym}")
        H = ctypes.c_void_p
        L.mi355vits_version.restype = ctypes.c_char_p
        L.mi355vits_create.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(H)]
        L.mi355vits_create_from_buffer.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(H)]
        L.mi355vits_clone.argtypes = [H, ctypes.POINTER(H)]
        L.mi355vits_device_result.argtypes = [H, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                              ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
                                              ctypes.POINTER(ctypes.c_void_p)]
        L.mi355vits_set_math.argtypes = [H, ctypes.c_int]
        L.mi355vits_get_math.argtypes = [H]
        L.mi355vits_set_output_rate.argtypes = [H, ctypes.c_int32]
        L.mi355vits_get_output_rate.argtypes = [H]
        L.mi355vits_get_output_rate.restype = ctypes.c_int32
        L.mi355vits_set_output_encoding.argtypes = [H, ctypes.c_int]
        L.mi355vits_get_output_encoding.argtypes = [H]
        L.mi355vits_set_output_compression.argtypes = [H, ctypes.c_int]
        L.mi355vits_get_output_compression.argtypes = [H]
        L.mi355vits_destroy.argtypes = [H]
        L.mi355vits_destroy.restype = None
        L.mi355vits_get_config.argtypes = [H, ctypes.POINTER(CVitsConfig)]
        L.mi355vits_run.argtypes = [H, ctypes.POINTER(RunArgs), ctypes.POINTER(Result)]
        L.mi355vits_run_rows.argtypes = [H, ctypes.POINTER(RunArgs), ctypes.POINTER(RowArgs), ctypes.POINTER(Result)]
        L.mi355vits_run_timed.argtypes = [H, ctypes.POINTER(RunArgs), ctypes.POINTER(RowArgs), ctypes.POINTER(TimingArgs), ctypes.POINTER(Result)]
        L.mi355vits_run_speakers.argtypes = [H, ctypes.POINTER(RunArgs), ctypes.POINTER(RowArgs), ctypes.POINTER(TimingArgs),
                                             ctypes.POINTER(SpeakerArgs), ctypes.POINTER(Result)]
        L.mi355vits_get_speaker_embedding.argtypes = [H, ctypes.c_int64, ctypes.POINTER(ctypes.c_float), ctypes.c_size_t]
        L.mi355vits_run_levels.argtypes = [H, ctypes.POINTER(RunArgs), ctypes.POINTER(RowArgs), ctypes.POINTER(TimingArgs),
                                           ctypes.POINTER(SpeakerArgs), ctypes.POINTER(LevelArgs), ctypes.POINTER(Result)]
        L.mi355vits_run_pitch.argtypes = [H, ctypes.POINTER(RunArgs), ctypes.POINTER(RowArgs), ctypes.POINTER(TimingArgs),
                                          ctypes.POINTER(SpeakerArgs), ctypes.POINTER(LevelArgs), ctypes.POINTER(PitchArgs),
                                          ctypes.POINTER(Result)]
        L.mi355vits_fetch.argtypes = [H, ctypes.c_uint32, ctypes.POINTER(Result)]
        L.mi355vits_free_result.argtypes = [ctypes.POINTER(Result)]
        L.mi355vits_free_result.restype = None
        L.mi355vits_run_packed.argtypes = [H, ctypes.POINTER(RunArgs), ctypes.POINTER(RowArgs), ctypes.POINTER(PackArgs),
                                           ctypes.POINTER(PackedResult)]
        L.mi355vits_fetch_packed.argtypes = [H, ctypes.POINTER(PackArgs), ctypes.POINTER(PackedResult)]
        L.mi355vits_free_packed.argtypes = [ctypes.POINTER(PackedResult)]
        L.mi355vits_free_packed.restype = None
        L.mi355vits_run_streams.argtypes = [H, ctypes.POINTER(RunArgs), ctypes.POINTER(RowArgs), ctypes.POINTER(StreamArgs), ctypes.c_int32,
                                            ctypes.POINTER(StreamsResult)]
        L.mi355vits_fetch_streams.argtypes = [H, ctypes.POINTER(StreamArgs), ctypes.c_int32, ctypes.POINTER(StreamsResult)]
        L.mi355vits_free_streams.argtypes = [ctypes.POINTER(StreamsResult)]
        L.mi355vits_free_streams.restype = None
        L.mi355vits_run_streams2.argtypes = [H, ctypes.POINTER(RunArgs), ctypes.POINTER(RowArgs), ctypes.POINTER(StreamArgs2), ctypes.c_int32,
                                             ctypes.POINTER(StreamsResult2)]
        L.mi355vits_fetch_streams2.argtypes = [H, ctypes.POINTER(StreamArgs2), ctypes.c_int32, ctypes.POINTER(StreamsResult2)]
        L.mi355vits_free_streams2.argtypes = [ctypes.POINTER(StreamsResult2)]
        L.mi355vits_free_streams2.restype = None
        L.mi355vits_fetch_alignment.argtypes = [H, ctypes.c_uint32, ctypes.POINTER(AlignmentResult)]
        L.mi355vits_free_alignment.argtypes = [ctypes.POINTER(AlignmentResult)]
        L.mi355vits_free_alignment.restype = None
        L.mi355vits_set_edge_trim.argtypes = [H, ctypes.c_float, ctypes.c_int32]
        L.mi355vits_get_edge_trim.argtypes = [H, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)]
        L.mi355vits_fetch_edges.argtypes = [H, ctypes.POINTER(EdgesResult)]
        L.mi355vits_free_edges.argtypes = [ctypes.POINTER(EdgesResult)]
        L.mi355vits_free_edges.restype = None
        L.mi355vits_set_loudness_target.argtypes = [H, ctypes.c_float, ctypes.c_float]
        L.mi355vits_get_loudness_target.argtypes = [H, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.mi355vits_fetch_loudness.argtypes = [H, ctypes.POINTER(LoudnessResult)]
        L.mi355vits_free_loudness.argtypes = [ctypes.POINTER(LoudnessResult)]
        L.mi355vits_free_loudness.restype = None
        L.mi355vits_set_loudness_limiter.argtypes = [H, ctypes.c_int32]
        L.mi355vits_get_loudness_limiter.argtypes = [H]
        L.mi355vits_get_loudness_limiter.restype = ctypes.c_int32
        L.mi355vits_fetch_limiter.argtypes = [H, ctypes.POINTER(LimiterResult)]
        L.mi355vits_free_limiter.argtypes = [ctypes.POINTER(LimiterResult)]
        L.mi355vits_free_limiter.restype = None
        L.mi355vits_set_loudness_ceiling_mode.argtypes = [H, ctypes.c_int]
        L.mi355vits_get_loudness_ceiling_mode.argtypes = [H]
        L.mi355vits_fetch_true_peak.argtypes = [H, ctypes.POINTER(TruePeakResult)]
        L.mi355vits_free_true_peak.argtypes = [ctypes.POINTER(TruePeakResult)]
        L.mi355vits_free_true_peak.restype = None
        L.mi355vits_last_error.argtypes = [H]
        L.mi355vits_last_error.restype = ctypes.c_char_p
        L.mi355vits_profile_enable.argtypes = [H, ctypes.c_int]
        L.mi355vits_profile_reset.argtypes = [H]
        L.mi355vits_profile_report.argtypes = [H, ctypes.c_char_p, ctypes.c_size_t]
        L.mi355vits_profile_report.restype = ctypes.c_long
        L.mi355vits_last_run_ms.argtypes = [H]
        L.mi355vits_last_run_ms.restype = ctypes.c_float
        L.mi355vits_get_tap.argtypes = [H, ctypes.c_char_p, ctypes.POINTER(ctypes.c_float), ctypes.c_size_t,
                                        ctypes.POINTER(ctypes.c_int64)]
        L.mi355vits_get_tap.restype = ctypes.c_long
        L.mi355vits_get_tap_rows.argtypes = [H, ctypes.c_char_p, ctypes.c_long, ctypes.c_long, ctypes.POINTER(ctypes.c_float), ctypes.c_size_t,
                                            ctypes.POINTER(ctypes.c_int64)]
        L.mi355vits_get_tap_rows.restype = ctypes.c_long
        L.mi355vits_list_taps.argtypes = [H, ctypes.c_char_p, ctypes.c_size_t]
        L.mi355vits_list_taps.restype = ctypes.c_long
        # the hooks of include/mi355vits_lab.h: all of them or none (the product library has none)
        present = [hasattr(L, sym) for sym in LAB_SYMBOLS]
        if any(present) and not all(present):
            raise RuntimeError(f"{self.path} exports only part of include/mi355vits_lab.h")
        self.has_hooks = all(present)
        if self.has_hooks:
            L.mi355vits_test_conv1d.argtypes = [ctypes.c_int, ctypes.POINTER(ConvTest)]
            L.mi355vits_test_conv_transpose1d.argtypes = [
                ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                ctypes.POINTER(ctypes.c_float), ctypes.c_float, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)]
            L.mi355vits_test_fill_workspace.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
            L.mi355vits_test_mfma_layout.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
            L.mi355vits_bench_conv1d.argtypes = [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_float)]
            L.mi355vits_probe_device.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
            L.mi355vits_probe_weights.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
            L.mi355vits_test_resample.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_float),
                                                  ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                                  ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32),
                                                  ctypes.POINTER(ctypes.c_float)]
            L.mi355vits_lab_g711_encode.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int16), ctypes.c_long, ctypes.POINTER(ctypes.c_uint8)]
            i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
            L.mi355vits_lab_flac.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint8),
                                             ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), i32p]
            L.mi355vits_lab_flac_jobs.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_long), ctypes.c_int32, ctypes.c_int32,
                                                  ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                                  ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
            L.mi355vits_lab_edges.argtypes = [f32p, ctypes.c_long, i32p, f32p, ctypes.c_int, ctypes.c_float, i32p, i32p]
            L.mi355vits_lab_loudness.argtypes = [f32p, ctypes.c_long, i32p, ctypes.c_int, ctypes.c_int32, ctypes.POINTER(ctypes.c_double), i32p, i32p]
            L.mi355vits_lab_loudness_plan.argtypes = [ctypes.c_int32, i32p, i32p, i32p]
            L.mi355vits_lab_limit.argtypes = [f32p, ctypes.c_long, i32p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_double,
                                              ctypes.c_double, ctypes.c_int32, f32p, ctypes.POINTER(ctypes.c_int64), i32p]
            f64p = ctypes.POINTER(ctypes.c_double)
            L.mi355vits_lab_limit_env.argtypes = [f32p, ctypes.c_long, i32p, ctypes.c_int, f64p, ctypes.c_double, ctypes.c_double,
                                                  ctypes.c_int32, f64p, f32p, ctypes.POINTER(ctypes.c_int64), i32p]
            L.mi355vits_lab_true_peak.argtypes = [f32p, ctypes.c_long, i32p, ctypes.c_int, ctypes.c_int32, f64p, f64p]
            L.mi355vits_lab_true_peak_plan.argtypes = [f64p, i32p]
            L.mi355vits_test_alignment.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, i32p, i32p, ctypes.c_int64, f32p, i32p,
                                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, i32p, i32p, i32p, f32p, f32p]
            L.mi355vits_test_rel_attention.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_float)] * 3 + [
                ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)]
            L.mi355vits_test_wn_layer.argtypes = [ctypes.c_int, ctypes.POINTER(WnTest)]
            L.mi355vits_lab_wn_plan.argtypes = [ctypes.c_int] * 4 + [i32p, i32p]
            L.mi355vits_lab_pack_w16.argtypes = [f32p] + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_uint32)]
            L.mi355vits_test_mrf_stage.argtypes = [ctypes.c_int, ctypes.POINTER(MrfTest)]
            L.mi355vits_lab_mrf_plan.argtypes = [ctypes.c_int] * 3 + [i32p] * 7
            L.mi355vits_lab_conv_plan.argtypes = [ctypes.c_int] * 12 + [i32p, ctypes.POINTER(ConvPlan)]
            L.mi355vits_test_enc_o_ln.argtypes = [ctypes.c_int] * 4 + [f32p] * 6 + [ctypes.c_float, i32p, i32p, ctypes.c_int, f32p]
            L.mi355vits_test_conv_post.argtypes = [ctypes.c_int] * 5 + [f32p, f32p, i32p, ctypes.POINTER(ctypes.c_double), f32p, f32p,
                                                   ctypes.POINTER(ctypes.c_int16), i32p]
            L.mi355vits_test_dds_stack.argtypes = [ctypes.c_int, ctypes.POINTER(DdsStackTest)]
            L.mi355vits_test_spline_inverse.argtypes = [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_float, f32p, i32p, f32p]
            L.mi355vits_test_fit_durations.argtypes = [ctypes.c_int] * 3 + [f32p, i32p, i32p, i32p, i32p, i32p, i32p, f32p, i32p]
            L.mi355vits_test_speaker_cond.argtypes = [ctypes.c_int] * 5 + [f32p, ctypes.POINTER(ctypes.c_int64), f32p, f32p, f32p, ctypes.c_size_t]
            L.mi355vits_test_speaker_cond_mix.argtypes = [ctypes.c_int, ctypes.POINTER(SpeakerMixTest)]
            L.mi355vits_test_levels.argtypes = [ctypes.c_int] * 4 + [i32p, i32p, f32p, i32p, i32p, ctypes.c_int64, f32p, ctypes.c_size_t, f32p]
            L.mi355vits_test_pitch_table.argtypes = [f32p, ctypes.c_size_t]
            L.mi355vits_test_pitch_plan.argtypes = [ctypes.c_int] * 4 + [i32p, i32p, f32p, ctypes.POINTER(ctypes.c_int64), i32p, i32p]
            L.mi355vits_test_pitch.argtypes = [ctypes.c_int] * 4 + [i32p, i32p, f32p, f32p, ctypes.c_int64, ctypes.c_size_t, f32p, ctypes.c_int64,
                                               ctypes.c_int32, ctypes.c_size_t, f32p, i32p]
            L.mi355vits_test_durations.argtypes = [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_float, f32p, i32p, i32p, f32p, f32p, i32p, i32p, i32p]
            L.mi355vits_test_expand_prior.argtypes = [ctypes.c_int] * 5 + [f32p, i32p, i32p, f32p, ctypes.c_int, f32p, f32p]
            u64p = ctypes.POINTER(ctypes.c_uint64)
            L.mi355vits_test_expand_prior_keyed.argtypes = [ctypes.c_int] * 5 + [f32p, i32p, i32p, f32p, ctypes.c_uint64, u64p, f32p]
            L.mi355vits_test_sdp_noise.argtypes = [ctypes.c_int] * 3 + [ctypes.c_uint64, u64p, f32p, f32p]
            L.mi355vits_test_embed.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int64), i32p, f32p, ctypes.c_float, f32p]
            L.mi355vits_test_layernorm.argtypes = [ctypes.c_int, ctypes.POINTER(LayerNormTest)]
            L.mi355vits_test_dp_det.argtypes = [ctypes.c_int, ctypes.POINTER(DpDetTest)]
            L.mi355vits_lab_dp_det_plan.argtypes = [ctypes.c_int] * 4 + [i32p, i32p, i32p]

    def _need_hooks(self):
        if not self.has_hooks:
            raise RuntimeError(f"{self.path} is the product library: the hooks of include/mi355vits_lab.h live in "
                               "libmi355vits_hooks.so (mimic3_amd._native.hooks_library()), the lab build and the CPU model")

    def _hook(self, name: str, *args) -> None:
        """One call of a hook of include/mi355vits_lab.h: ``mi355vits_<name>(*args)``; a non-zero code raises with the library's message."""
        self._need_hooks()
        rc = getattr(self.lib, "mi355vits_" + name)(*args)
        if rc != 0:
            raise NativeError(rc, self.create_error())

    def version(self) -> str:
        return self.lib.mi355vits_version().decode()

    def device_count(self) -> int:
        return int(self.lib.mi355vits_device_count())

    def create_error(self) -> str:
        return (self.lib.mi355vits_last_error(None) or b"").decode("utf-8", "replace")

    # ---- kernel unit-test hooks -------------------------------------------------------------
    def lab_g711_encode(self, law, samples) -> np.ndarray:
        """The device's G.711 encoders (the ones of the encoded packed streams) over int16 ``samples``; law "ulaw" / "alaw"."""
        x = np.ascontiguousarray(samples, np.int16).reshape(-1)
        out = np.empty(x.shape[0], np.uint8)
        self._hook("lab_g711_encode", encoding_id(law), _ptr(x), x.shape[0], _ptr(out))
        return out

    def lab_flac(self, samples, rate: int, first_frame: int = 0):
        """The FLAC kernels alone over int16 ``samples`` (a contiguous 1-d int16 array is read where it is: its address modulo 16 is
        the samples' on the device) -> (the complete file as bytes, frame sizes int32 [ceil(n / 4096)])."""
        x = np.asarray(samples)
        if x.dtype != np.int16 or x.ndim != 1 or not x.flags.c_contiguous:
            x = np.ascontiguousarray(samples, np.int16).reshape(-1)
        n = int(x.shape[0])
        frames = (n + 4095) // 4096
        out = np.empty(42 + 16 * frames + 2 * n, np.uint8)
        sizes = np.zeros(max(frames, 1), np.int32)
        got = ctypes.c_size_t(0)
        self._hook("lab_flac", ctypes.c_void_p(x.ctypes.data), n, int(rate), int(first_frame), _ptr(out), out.shape[0], ctypes.byref(got),
                   _ptr(sizes))
        return out[: int(got.value)].tobytes(), sizes[:frames].copy()

    def lab_flac_jobs(self, arrays, rate: int):
        """SEVERAL int16 arrays as FLAC files in ONE block by the kernels of the streams calls alone (``mi355vits_lab_flac_jobs``):
        -> (the block uint8, offsets int64 [J] — multiples of 16 —, sizes int64 [J]); file j = block[offsets[j] : offsets[j] + sizes[j]].
        A contiguous 1-d int16 array is read where it is, as ``lab_flac`` reads it."""
        xs = []
        for a in arrays:
            x = np.asarray(a)
            if x.dtype != np.int16 or x.ndim != 1 or not x.flags.c_contiguous:
                x = np.ascontiguousarray(a, np.int16).reshape(-1)
            xs.append(x)
        J = len(xs)
        ptrs = (ctypes.c_void_p * max(J, 1))(*[x.ctypes.data for x in xs])
        ns = (ctypes.c_long * max(J, 1))(*[int(x.shape[0]) for x in xs])
        cap = sum(((42 + 16 * ((int(x.shape[0]) + 4095) // 4096) + 2 * int(x.shape[0]) + 15) & ~15) for x in xs) + 16
        out = np.empty(cap, np.uint8)
        offsets, sizes = np.zeros(max(J, 1), np.int64), np.zeros(max(J, 1), np.int64)
        got = ctypes.c_size_t(0)
        self._hook("lab_flac_jobs", ptrs, ns, J, int(rate), _ptr(out), cap, ctypes.byref(got), _ptr(offsets), _ptr(sizes))
        return out[: int(got.value)].copy(), offsets[:J].copy(), sizes[:J].copy()

    def lab_edges(self, audio, lengths, peaks, ratio):
        """The edge kernel (k_edges) alone: audio [B, stride] f32 with lengths [B] valid samples each (what lies behind them is never
        looked at), peaks [B] f32, 0 < ratio <= 1 -> (s_first, s_last) int32 [B]: the first / last sample with
        ``abs(y) >= peaks[b] * ratio`` in f32 (lengths[b] / -1 when there is none)."""
        au = np.ascontiguousarray(audio, np.float32)
        ln = np.ascontiguousarray(lengths, np.int32).reshape(-1)
        pk = np.ascontiguousarray(peaks, np.float32).reshape(-1)
        if au.ndim != 2 or ln.shape[0] != au.shape[0] or pk.shape[0] != au.shape[0]:
            raise ValueError("audio [B, stride], lengths [B], peaks [B]")
        B = au.shape[0]
        first, last = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._hook("lab_edges", _ptr(au), au.shape[1], _ptr(ln), _ptr(pk), B, float(ratio), _ptr(first), _ptr(last))
        return first, last

    def lab_loudness(self, audio, lengths, rate):
        """The loudness kernels (k_loud, k_loud_gate) alone: audio [B, stride] f32 with lengths [B] valid samples each at ``rate`` Hz
        (what lies behind them is never looked at) -> (lufs float64 [B], blocks int32 [B], gated int32 [B]) as
        ``mi355vits_fetch_loudness`` defines them."""
        au = np.ascontiguousarray(audio, np.float32)
        ln = np.ascontiguousarray(lengths, np.int32).reshape(-1)
        if au.ndim != 2 or ln.shape[0] != au.shape[0]:
            raise ValueError("audio [B, stride], lengths [B]")
        B = au.shape[0]
        lufs, blocks, gated = np.zeros(B, np.float64), np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._hook("lab_loudness", _ptr(au), au.shape[1], _ptr(ln), B, int(rate), _ptr(lufs), _ptr(blocks), _ptr(gated))
        return lufs, blocks, gated

    def lab_true_peak(self, audio, lengths, offset=0, envelope=True):
        """The true-peak kernels (k_true_peak, k_true_peak_env) alone: audio [B, stride] f32 with lengths [B] valid samples each (what
        lies behind them is never looked at), on the device ``offset`` (0 .. 3) floats behind a 16-byte boundary -> (tp float64 [B],
        e float64 [B, stride] — the rule's ``e[t]`` at a row's valid samples, 0 behind them; ``None`` with ``envelope=False``)."""
        au = np.ascontiguousarray(audio, np.float32)
        ln = np.ascontiguousarray(lengths, np.int32).reshape(-1)
        if au.ndim != 2 or ln.shape[0] != au.shape[0]:
            raise ValueError("audio [B, stride], lengths [B]")
        B = au.shape[0]
        tp = np.zeros(B, np.float64)
        env = np.zeros(au.shape, np.float64) if envelope else None
        self._hook("lab_true_peak", _ptr(au), au.shape[1], _ptr(ln), B, int(offset), _ptr(tp), _ptr(env))
        return tp, env

    def lab_true_peak_plan(self):
        """``(taps float64 [81], tile)``: the library's tap table ``h`` and the samples of a k_true_peak work item.  No kernel runs."""
        taps, tile = np.zeros(81, np.float64), ctypes.c_int32()
        self._hook("lab_true_peak_plan", _ptr(taps), ctypes.byref(tile))
        return taps, int(tile.value)

    def lab_limit(self, audio, lengths, g, c, U, window, envelope=None):
        """The limiter kernel (k_limit) alone: audio [B, stride] f32 with lengths [B] valid samples each (what lies behind them is
        never looked at), g [B] float64 the rows' gains, c the linear ceiling, U the encoding's unit (32767.0 or 1.0), ``window`` = L
        in samples -> (scale float32 [B, stride] — the rule's ``scale[k]`` at a row's valid samples, 0 behind them —, sq_min int64 [B],
        reduced int32 [B]) as ``include/mi355vits.h`` defines them.  Every row is a job, over the ceiling or not.  ``envelope``
        [B, stride] float64: the true-peak form — ``envelope[b, t]`` in place of ``abs(audio[b, t])``."""
        au = np.ascontiguousarray(audio, np.float32)
        ln = np.ascontiguousarray(lengths, np.int32).reshape(-1)
        gg = np.ascontiguousarray(g, np.float64).reshape(-1)
        if au.ndim != 2 or ln.shape[0] != au.shape[0] or gg.shape[0] != au.shape[0]:
            raise ValueError("audio [B, stride], lengths [B], g [B]")
        B = au.shape[0]
        scale = np.zeros(au.shape, np.float32)
        sq_min, reduced = np.zeros(B, np.int64), np.zeros(B, np.int32)
        if envelope is not None:
            ev = np.ascontiguousarray(envelope, np.float64)
            if ev.shape != au.shape:
                raise ValueError("envelope has the audio's shape")
            self._hook("lab_limit_env", _ptr(au), au.shape[1], _ptr(ln), B, _ptr(gg), float(c), float(U), int(window), _ptr(ev), _ptr(scale),
                       _ptr(sq_min), _ptr(reduced))
        else:
            self._hook("lab_limit", _ptr(au), au.shape[1], _ptr(ln), B, _ptr(gg), float(c), float(U), int(window), _ptr(scale), _ptr(sq_min),
                       _ptr(reduced))
        return scale, sq_min, reduced

    def lab_loudness_plan(self, rate):
        """How k_loud cuts a row at ``rate`` Hz: ``(S, W, K)`` — the 100 ms step, the warm-up samples of a work item that starts
        inside a row, and the steps of a work item (an item is ``K * S`` samples of one row).  Host arithmetic only."""
        s, w, k = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._hook("lab_loudness_plan", int(rate), ctypes.byref(s), ctypes.byref(w), ctypes.byref(k))
        return int(s.value), int(w.value), int(k.value)

    def test_conv1d(self, x, w, bias=None, res=None, dilation=1, impl=1, in_len=None, out_len=None, in_slope=1.0,
                    relu=False, out_scale=1.0, res_sub=False, accumulate_into=None, device=0, math=None, cond=None,
                    mask_before_res=False, fixed_rule=False, y_prior=None) -> np.ndarray:
        """One Conv1d through one kernel family (include/mi355vits_lab.h: mi355vits_test_conv1d).  math: MATH_F32 for impl 0 / 1,
        MATH_BF16X3 (the default) or MATH_BF16W for impl 2 / 3, MATH_BF16X3 for impl 4.  cond [B, Cout].  y_prior = what the output
        buffer holds before the launch (zeros) when not accumulating; accumulate_into = the same buffer AND y += ."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        B, Cin, T = x.shape
        Cout, _, K = w.shape
        assert accumulate_into is None or y_prior is None
        prior = accumulate_into if accumulate_into is not None else y_prior
        y = np.zeros((B, Cout, T), np.float32) if prior is None else np.ascontiguousarray(prior, np.float32).copy()
        assert y.shape == (B, Cout, T) and w.shape[1] == Cin
        keep = [x, w, y]
        t = ConvTest()
        t.impl, t.B, t.Cin, t.Cout, t.T, t.K, t.dilation = impl, B, Cin, Cout, T, K, dilation
        t.x, t.w, t.y = _ptr(x), _ptr(w), _ptr(y)
        for name, arr, shape in (("bias", bias, (Cout,)), ("res", res, (B, Cout, T)), ("cond", cond, (B, Cout))):
            if arr is not None:
                a = np.ascontiguousarray(arr, np.float32)
                assert a.shape == shape, (name, a.shape, shape)
                keep.append(a)
                setattr(t, name, _ptr(a))
        for name, arr in (("in_len", in_len), ("out_len", out_len)):
            if arr is not None:
                a = np.ascontiguousarray(arr, np.int32)
                assert a.shape == (B,)
                keep.append(a)
                setattr(t, name, _ptr(a))
        t.in_slope, t.relu, t.out_scale, t.res_sub = in_slope, int(relu), out_scale, int(res_sub)
        t.accumulate = int(accumulate_into is not None)
        t.math = (MATH_F32 if impl in (0, 1) else MATH_BF16X3) if math is None else int(math)
        t.mask_before_res, t.fixed_rule = int(bool(mask_before_res)), int(bool(fixed_rule))
        self._hook("test_conv1d", device, ctypes.byref(t))
        return y

    def test_conv_transpose1d(self, x, w, bias, stride, in_slope=1.0, device=0, impl=0, in_len=None, y_prior=None) -> np.ndarray:
        """in_len [B]: per-row input lengths (impl 3 only; None = every row at full length); output positions at or past
        in_len[b] x stride are left undefined.  y_prior = what the output buffer holds before the launch (zeros)."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        B, Cin, Tin = x.shape
        _, Cout, K = w.shape
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        ln = None if in_len is None else np.ascontiguousarray(in_len, np.int32)
        y = np.zeros((B, Cout, Tin * stride), np.float32) if y_prior is None else np.ascontiguousarray(y_prior, np.float32).copy()
        assert y.shape == (B, Cout, Tin * stride)
        self._hook("test_conv_transpose1d", device, impl, B, Cin, Cout, Tin, K, stride, _ptr(x), _ptr(w), _ptr(b), in_slope, _ptr(ln), _ptr(y))
        return y

    def lab_conv_plan(self, impl, B, Cin, Cout, T, K, dilation=1, stride=0, math=None, fixed_rule=False, has_res=False, has_cond=False,
                      lengths=None) -> "ConvPlan":
        """What the conv launchers would run for a hook call of this shape on the current device (include/mi355vits_lab.h:
        mi355vits_lab_conv_plan): stride = 0: test_conv1d(impl); stride > 0: test_conv_transpose1d(impl) with Tin = T.  No kernel runs."""
        p = ConvPlan()
        ln = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
        m = (MATH_F32 if impl in (0, 1) else MATH_BF16X3) if math is None else int(math)
        self._hook("lab_conv_plan", int(impl), int(B), int(Cin), int(Cout), int(T), int(K), int(dilation), int(stride), m, int(bool(fixed_rule)),
                   int(bool(has_res)), int(bool(has_cond)), _ptr(ln), ctypes.byref(p))
        return p

    def test_enc_o_ln(self, x, w, bias, res, gamma, beta, in_len=None, ln_out_len=None, eps=1e-5, math=MATH_BF16X3, in_place=False,
                      y_prior=None, device=0) -> np.ndarray:
        """launch_enc_o_ln alone (include/mi355vits_lab.h: mi355vits_test_enc_o_ln): y = LN_c(res + conv1x1(x * mask_in) + bias) *
        mask_ln on [B, 192, T]; in_place: the kernel runs with y == res."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        x, w, bias, res, gamma, beta = f(x), f(w), f(bias), f(res), f(gamma), f(beta)
        B, C, T = x.shape
        assert C == 192 and res.shape == x.shape and w.shape == (C, C, 1) and gamma.shape == beta.shape == (C,)
        y = np.zeros_like(x) if y_prior is None else f(y_prior).copy()
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
        il, ol = i32(in_len), i32(ln_out_len)
        self._hook("test_enc_o_ln", device, int(math), B, T, _ptr(x), _ptr(w), _ptr(bias), _ptr(res), _ptr(gamma), _ptr(beta), float(eps), _ptr(il),
                   _ptr(ol), int(bool(in_place)), _ptr(y))
        return y

    def test_conv_post(self, x, w, valid_len, volumes=None, audio_prior=None, pcm_prior=None, device=0):
        """The decoder's tail, launch_conv_post_tanh then launch_pcm16 (include/mi355vits_lab.h: mi355vits_test_conv_post): x [B, Cin, L],
        w [1, Cin, K] -> (audio [B, L] float32, peaks [B] float32, pcm [B, L] int16, the kernel that ran: 0 dpp, 1 vec, 2 staged)."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        B, Cin, L = x.shape
        assert w.shape[:2] == (1, Cin)
        K = w.shape[2]
        vl = np.ascontiguousarray(valid_len, np.int32)
        assert vl.shape == (B,)
        vol = None if volumes is None else np.ascontiguousarray(volumes, np.float64)
        audio = np.zeros((B, L), np.float32) if audio_prior is None else np.ascontiguousarray(audio_prior, np.float32).copy()
        pcm = np.zeros((B, L), np.int16) if pcm_prior is None else np.ascontiguousarray(pcm_prior, np.int16).copy()
        peaks = np.full(B, -1.0, np.float32)
        kernel = ctypes.c_int32(-1)
        self._hook("test_conv_post", device, B, Cin, K, L, _ptr(x), _ptr(w), _ptr(vl), _ptr(vol), _ptr(audio), _ptr(peaks), _ptr(pcm),
                   ctypes.byref(kernel))
        return audio, peaks, pcm, int(kernel.value)

    def emu_set_cu_count(self, n: int) -> None:
        """The compute units the CPU model reports to the grid sizing of every launch after this call (default 8; n < 1 restores it).
        CPU model only: the device libraries report what the device has."""
        if not hasattr(self.lib, "mi355vits_emu_set_cu_count"):
            raise RuntimeError(f"{self.path} is not the CPU model of the kernels")
        self.lib.mi355vits_emu_set_cu_count(ctypes.c_int(int(n)))

    def test_rel_attention(self, qkv, emb_rel_k, emb_rel_v, lengths, n_heads, impl=2, device=0) -> np.ndarray:
        """Relative-position attention through one kernel: impl 0 = VALU, 1 = f32-MFMA (T <= 512), 2 = streamed.
        qkv [B, 3H, T], emb_rel_* [2W+1, H/n_heads], lengths [B] -> [B, H, T]."""
        qkv = np.ascontiguousarray(qkv, np.float32)
        ek = np.ascontiguousarray(emb_rel_k, np.float32)
        ev = np.ascontiguousarray(emb_rel_v, np.float32)
        ln = np.ascontiguousarray(lengths, np.int32)
        B, H3, T = qkv.shape
        H = H3 // 3
        W = (ek.shape[0] - 1) // 2
        out = np.zeros((B, H, T), np.float32)
        self._hook("test_rel_attention", device, impl, B, T, H, n_heads, W, _ptr(qkv), _ptr(ek), _ptr(ev), _ptr(ln), _ptr(out))
        return out

    def test_wn_layer(self, h, skip, w_in, b_in, w_rs, b_rs, lengths, dilation=1, cond=None, skip_init=False, impl=1, math=None,
                      h_out_prior=None, device=0):
        """One WaveNet layer of the coupling flow through one path (include/mi355vits_lab.h: mi355vits_test_wn_layer): impl 0 = the
        two-launch path, 1 = launch_wn_layer (MATH_F32), 2 = launch_wn_layer_b3 (MATH_BF16X3).  h, skip [B, H, T], w_in [2H, H, K],
        w_rs [Crs, H, 1], cond [B, 2H] or None, lengths [B]; h_out_prior = what the output buffer of h' holds before the launch
        (zeros).  Returns (h', skip'); with Crs = H, h' is h_out_prior unchanged."""
        f = lambda a: np.ascontiguousarray(a, np.float32)
        h, w_in, b_in, w_rs, b_rs = f(h), f(w_in), f(b_in), f(w_rs), f(b_rs)
        skip = f(skip).copy()
        B, H, T = h.shape
        ln = np.ascontiguousarray(lengths, np.int32)
        h_out = np.zeros_like(h) if h_out_prior is None else f(h_out_prior).copy()
        assert skip.shape == h.shape == h_out.shape and w_in.shape[:2] == (2 * H, H) and w_rs.shape[1:] == (H, 1) and ln.shape == (B,)
        assert b_in.shape == (2 * H,) and b_rs.shape == (w_rs.shape[0],)
        c = None if cond is None else f(cond)
        assert c is None or c.shape == (B, 2 * H)
        t = WnTest()
        t.impl, t.B, t.H, t.T, t.K, t.dilation, t.Crs, t.skip_init = impl, B, H, T, w_in.shape[2], int(dilation), w_rs.shape[0], int(bool(skip_init))
        t.math = (MATH_BF16X3 if impl == 2 else MATH_F32) if math is None else int(math)
        t.h_in, t.w_in, t.b_in, t.w_rs, t.b_rs, t.cond = _ptr(h), _ptr(w_in), _ptr(b_in), _ptr(w_rs), _ptr(b_rs), _ptr(c)
        t.len, t.h_out, t.skip = _ptr(ln), _ptr(h_out), _ptr(skip)
        self._hook("test_wn_layer", device, ctypes.byref(t))
        return h_out, skip

    def lab_wn_plan(self, B, T, K=5, dilation=1):
        """What the WaveNet launchers pick for a [B, 192, T] layer on the current device: (the columns of a k_wn_layer_b3 tile — 32, 96
        or 128 —, launch_wn_layer's geometry 0 / 1 / 2).  No kernel runs."""
        tile, geom = ctypes.c_int32(), ctypes.c_int32()
        self._hook("lab_wn_plan", int(B), int(T), int(K), int(dilation), ctypes.byref(tile), ctypes.byref(geom))
        return int(tile.value), int(geom.value)

    def lab_pack_w16(self, w, gate=False):
        """k_wn_layer_b3's weight fragments of w [Cout, Cin, K] (include/mi355vits_lab.h: mi355vits_lab_pack_w16) as uint16 bf16 bit
        patterns [Cout / 16, K, Cin / 32, 3 planes, 64 lanes, 8 k-slots]."""
        w = np.ascontiguousarray(w, np.float32)
        Cout, Cin, K = w.shape
        out = np.zeros((Cout // 16, K, Cin // 32, 3, 64, 4), np.uint32)
        self._hook("lab_pack_w16", _ptr(w), Cout, Cin, K, int(bool(gate)), _ptr(out))
        return out.view(np.uint16).reshape(Cout // 16, K, Cin // 32, 3, 64, 8)

    def test_mrf_stage(self, x, ks, d1, d2, weights, biases, lengths, impl=0, math=None, out_scale=0.0, seg=0, y_prior=None, device=0):
        """One multi-receptive-field stage through one kernel (include/mi355vits_lab.h: mi355vits_test_mrf_stage): impl 0 = k_mrf_fused
        (MATH_F32 unless math says MATH_BF16X3), 1 = k_mrf_p, 2 = k_mrf_s with segments of ``seg`` columns.  x [B, C, T];
        weights[j][q] [C, C, ks[j]], biases[j][q] [C]; lengths [B]; y_prior = what the output buffer holds before the launch (zeros)."""
        x = np.ascontiguousarray(x, np.float32)
        B, C, T = x.shape
        ln = np.ascontiguousarray(lengths, np.int32)
        y = np.zeros_like(x) if y_prior is None else np.ascontiguousarray(y_prior, np.float32).copy()
        nrb = len(ks)
        assert y.shape == x.shape and ln.shape == (B,) and 1 <= nrb <= 4 and len(d1) == len(d2) == len(weights) == len(biases) == nrb
        t = MrfTest()
        t.impl, t.B, t.C, t.T, t.nrb, t.seg = impl, B, C, T, nrb, int(seg)
        t.math = (MATH_F32 if impl == 0 else MATH_BF16X3) if math is None else int(math)
        keep = []
        for j in range(nrb):
            t.k[j], t.d1[j], t.d2[j] = int(ks[j]), int(d1[j]), int(d2[j])
            for q in range(2):
                w = np.ascontiguousarray(weights[j][q], np.float32)
                bq = np.ascontiguousarray(biases[j][q], np.float32)
                assert w.shape == (C, C, ks[j]) and bq.shape == (C,)
                keep += [w, bq]
                t.w[j][q], t.bias[j][q] = _ptr(w), _ptr(bq)
        t.x, t.len, t.out_scale, t.y = _ptr(x), _ptr(ln), float(out_scale), _ptr(y)
        self._hook("test_mrf_stage", device, ctypes.byref(t))
        return y

    def lab_mrf_plan(self, impl, C, ks, d1, d2):
        """How MRF kernel ``impl`` (0 fused, 1 k_mrf_p, 2 k_mrf_s) cuts a row: (work-item width, halo, x ring, x1 ring) in columns; the
        rings are the sweep's (0 otherwise).  NativeError where the kernel does not serve the stage.  Host arithmetic only."""
        arr = lambda v: (ctypes.c_int32 * len(v))(*[int(e) for e in v])
        out = [ctypes.c_int32() for _ in range(4)]
        self._hook("lab_mrf_plan", int(impl), int(C), len(ks), arr(ks), arr(d1), arr(d2), *[ctypes.byref(o) for o in out])
        return tuple(int(o.value) for o in out)

    def test_dds_stack(self, src, pre_w, pre_b, layers, lengths, impl=2, math=None, cond=None, z=None, zch=0, proj_w=None, proj_b=None,
                       spline=False, nb=0, tail=0.0, inv_sqrt_fc=0.0, out_prior=None, x_out_prior=None, device=0):
        """One DDS stack of the stochastic duration predictor through one path (include/mi355vits_lab.h: mi355vits_test_dds_stack):
        impl 0 = one launch per piece, 1 = launch_dds_layer per layer, 2 = k_dds_stack<6> (MATH_F32), 3 = k_dds_stack_b3 (MATH_BF16X3,
        or MATH_BF16W through ``math``).  src [B, C, T]; pre_w [C, C, 1] (conv pre, with cond [B, C] or None) or [C] (affine pre on
        z[:, zch]); layers = a list of dicts dw_w [C, 1, K], dw_b, g1, b1, w1x1 [C, C, 1], bias1x1, g2, b2; proj_w [Cp, C, 1] or None;
        z [B, 2, T] or None.  out_prior / x_out_prior = what the output buffers hold before the launch (zeros).
        Returns (x_out, out or None, z or None)."""
        f = lambda a: np.ascontiguousarray(a, np.float32)
        src, pre_w, pre_b = f(src), f(pre_w), f(pre_b)
        B, C, T = src.shape
        ln = np.ascontiguousarray(lengths, np.int32)
        affine = pre_w.ndim == 1
        assert pre_w.shape == ((C,) if affine else (C, C, 1)) and pre_b.shape == (C,) and ln.shape == (B,) and 1 <= len(layers) <= 4
        t = DdsStackTest()
        keep = []
        K = np.asarray(layers[0]["dw_w"]).shape[2]
        for i, lay in enumerate(layers):
            for name, shape in (("dw_w", (C, 1, K)), ("dw_b", (C,)), ("g1", (C,)), ("b1", (C,)), ("w1x1", (C, C, 1)), ("bias1x1", (C,)),
                                ("g2", (C,)), ("b2", (C,))):
                a = f(lay[name])
                assert a.shape == shape, (name, a.shape, shape)
                keep.append(a)
                getattr(t, name)[i] = _ptr(a)
        c = None if cond is None else f(cond)
        assert c is None or c.shape == (B, C)
        zz = None if z is None else f(z).copy()
        assert zz is None or zz.shape == (B, 2, T)
        pw = None if proj_w is None else f(proj_w)
        pb = None if proj_b is None else f(proj_b)
        Cp = 0 if pw is None else pw.shape[0]
        assert pw is None or (pw.shape == (Cp, C, 1) and pb is not None and pb.shape == (Cp,))
        out = None if pw is None else (np.zeros((B, Cp, T), np.float32) if out_prior is None else f(out_prior).copy())
        x_out = np.zeros_like(src) if x_out_prior is None else f(x_out_prior).copy()
        assert x_out.shape == src.shape and (out is None or out.shape == (B, Cp, T))
        t.impl, t.B, t.C, t.T, t.K, t.n_layers, t.pre_mode, t.zch = int(impl), B, C, T, K, len(layers), int(affine), int(zch)
        t.math = (MATH_BF16X3 if impl == 3 else MATH_F32) if math is None else int(math)
        t.proj_cout, t.spline, t.nb, t.tail, t.inv_sqrt_fc = Cp, int(bool(spline)), int(nb), float(tail), float(inv_sqrt_fc)
        t.src, t.pre_w, t.pre_b, t.cond, t.proj_w, t.proj_b = _ptr(src), _ptr(pre_w), _ptr(pre_b), _ptr(c), _ptr(pw), _ptr(pb)
        t.len, t.z, t.out, t.x_out = _ptr(ln), _ptr(zz), _ptr(out), _ptr(x_out)
        self._hook("test_dds_stack", device, ctypes.byref(t))
        return x_out, out, zz

    def test_spline_inverse(self, theta, z, lengths, nb, ch_x0=0, tail=5.0, inv_sqrt_fc=1.0, device=0) -> np.ndarray:
        """launch_spline_inverse alone: theta [B, 3 nb - 1, T], z [B, 2, T], lengths [B] -> the new z (mi355vits_test_spline_inverse)."""
        theta = np.ascontiguousarray(theta, np.float32)
        z = np.ascontiguousarray(z, np.float32).copy()
        ln = np.ascontiguousarray(lengths, np.int32)
        B, _, T = z.shape
        assert z.shape == (B, 2, T) and theta.shape[0] == B and theta.shape[2] == T and ln.shape == (B,)
        assert nb < 1 or theta.shape[1] >= 3 * min(nb, 16) - 1
        self._hook("test_spline_inverse", device, B, T, int(nb), int(ch_x0), float(tail), float(inv_sqrt_fc), _ptr(theta), _ptr(ln), _ptr(z))
        return z

    def test_durations(self, z, lengths, ea_m=0.0, ea_logs=0.0, ch=0, length_scale=1.0, forced=None, device=0):
        """launch_durations alone: z [B, 2, T], lengths [B], length_scale a number or [B], forced [B, T] int32 or None ->
        (logw [B, T], w_ceil [B, T], cum [B, T], ylen [B]) (mi355vits_test_durations).  The outputs start as -77 / -7.5e29."""
        z = np.ascontiguousarray(z, np.float32)
        B, _, T = z.shape
        ln = np.ascontiguousarray(lengths, np.int32)
        sc = np.zeros((B, 3), np.float32)
        sc[:, 1] = np.asarray(length_scale, np.float32)
        fo = None if forced is None else np.ascontiguousarray(forced, np.int32)
        assert z.shape == (B, 2, T) and ln.shape == (B,) and (fo is None or fo.shape == (B, T))
        logw = np.full((B, T), -7.5e29, np.float32)
        w_ceil, cum, ylen = np.full((B, T), -77, np.int32), np.full((B, T), -77, np.int32), np.full(B, -77, np.int32)
        self._hook("test_durations", device, B, T, int(ch), float(ea_m), float(ea_logs), _ptr(z), _ptr(ln), _ptr(fo), _ptr(sc), _ptr(logw),
                   _ptr(w_ceil), _ptr(cum), _ptr(ylen))
        return logw, w_ceil, cum, ylen

    def test_fit_durations(self, u, lengths, min_frames=None, target=None, device=0):
        """The fit stage of launch_durations_timed alone on a given u [B, T]: lengths [B], min_frames [B, T] or None, target [B] or
        None -> (frames [B, T], cum [B, T], ylen [B], factor [B], status [B]) (mi355vits_test_fit_durations).  The outputs start as
        -77 / -7.5e29."""
        u = np.ascontiguousarray(u, np.float32)
        B, T = u.shape
        ln = np.ascontiguousarray(lengths, np.int32)
        mn = None if min_frames is None else np.ascontiguousarray(min_frames, np.int32)
        tg = None if target is None else np.ascontiguousarray(target, np.int32)
        assert ln.shape == (B,) and (mn is None or mn.shape == (B, T)) and (tg is None or tg.shape == (B,))
        frames, cum = np.full((B, T), -77, np.int32), np.full((B, T), -77, np.int32)
        ylen, status, factor = np.full(B, -77, np.int32), np.full(B, -77, np.int32), np.full(B, -7.5e29, np.float32)
        self._hook("test_fit_durations", device, B, T, _ptr(u), _ptr(ln), _ptr(mn), _ptr(tg), _ptr(frames), _ptr(cum), _ptr(ylen), _ptr(factor),
                   _ptr(status))
        return frames, cum, ylen, factor, status

    def test_levels(self, cum, lengths, gain, ramp, hop: int, audio, audio_bs: int, alen, device=0):
        """launch_levels (k_levels) alone, one launch: cum [B, T] int32, lengths [B], gain [B, T], ramp [B] or None, audio a flat array
        of at least B * ``audio_bs`` floats whose row b starts at ``b * audio_bs`` (all of it goes to the device and comes back), alen
        [B] = hop * max(1, c[len - 1]) -> (audio after the launch, peaks [B]) (mi355vits_test_levels)."""
        cum, gain = np.ascontiguousarray(cum, np.int32), np.ascontiguousarray(gain, np.float32)
        B, T = cum.shape
        ln, al = np.ascontiguousarray(lengths, np.int32), np.ascontiguousarray(alen, np.int32)
        rp = None if ramp is None else np.ascontiguousarray(ramp, np.int32)
        out = np.array(audio, np.float32, copy=True).reshape(-1)
        assert gain.shape == (B, T) and ln.shape == (B,) and al.shape == (B,) and (rp is None or rp.shape == (B,)) and out.size >= B * audio_bs
        peaks = np.full(B, -7.5e29, np.float32)
        self._hook("test_levels", device, B, T, int(hop), _ptr(cum), _ptr(ln), _ptr(gain), _ptr(rp), _ptr(al), int(audio_bs), _ptr(out), out.size,
                   _ptr(peaks))
        return out, peaks

    def test_pitch_table(self) -> np.ndarray:
        """The filter table of pitch control, Z P + 2 = 1,538 floats (mi355vits_test_pitch_table)."""
        out = np.zeros(12 * 128 + 2, np.float32)
        self._hook("test_pitch_table", _ptr(out), out.size)
        return out

    def test_pitch_plan(self, cum, lengths, ratio, hop: int, device=0):
        """launch_pitch_plan (k_pitch_plan) alone: cum [B, T] int32, lengths [B], ratio [B, T] or None -> (tq [B, T] int64,
        wc [B, T] int32, wlen [B] int32) (mi355vits_test_pitch_plan)."""
        cum = np.ascontiguousarray(cum, np.int32)
        B, T = cum.shape
        ln = np.ascontiguousarray(lengths, np.int32)
        rt = None if ratio is None else np.ascontiguousarray(ratio, np.float32)
        assert ln.shape == (B,) and (rt is None or rt.shape == (B, T))
        tq, wc, wlen = np.full((B, T), -1, np.int64), np.full((B, T), -1, np.int32), np.full(B, -1, np.int32)
        self._hook("test_pitch_plan", device, B, T, int(hop), _ptr(cum), _ptr(ln), _ptr(rt), _ptr(tq), _ptr(wc), _ptr(wlen))
        return tq, wc, wlen

    def test_pitch(self, cum, lengths, ratio, hop: int, x, x_bs: int, y, y_bs: int, y_ld: int, device=0):
        """The plan, then launch_pitch (k_pitch), on host buffers: x a flat array of at least B * ``x_bs`` floats whose row b starts
        at ``b * x_bs``, y likewise with ``y_bs`` (all of it goes to the device and comes back; ``y_ld`` floats of each row are
        written) -> (y after the launch, peaks [B], wlen [B]) (mi355vits_test_pitch)."""
        cum = np.ascontiguousarray(cum, np.int32)
        B, T = cum.shape
        ln = np.ascontiguousarray(lengths, np.int32)
        rt = None if ratio is None else np.ascontiguousarray(ratio, np.float32)
        xin = np.ascontiguousarray(x, np.float32).reshape(-1)
        out = np.array(y, np.float32, copy=True).reshape(-1)
        assert ln.shape == (B,) and (rt is None or rt.shape == (B, T)) and xin.size >= B * x_bs and out.size >= B * y_bs
        peaks, wlen = np.full(B, -7.5e29, np.float32), np.full(B, -1, np.int32)
        self._hook("test_pitch", device, B, T, int(hop), _ptr(cum), _ptr(ln), _ptr(rt), _ptr(xin), int(x_bs), xin.size,
                   _ptr(out), int(y_bs), int(y_ld), out.size, _ptr(peaks), _ptr(wlen))
        return out, peaks, wlen

    def test_speaker_cond(self, emb_g, sid, w, bias=None, pad: int = 8, device=0) -> np.ndarray:
        """launch_speaker_cond (k_speaker_cond) alone: emb_g [S, gin], sid [B], w [Cout, gin], bias [Cout] or None -> out, B * Cout
        + ``pad`` floats that start as -7.5e29 (mi355vits_test_speaker_cond): ``out[:B * Cout].reshape(B, Cout)`` is the result."""
        emb_g, w = np.ascontiguousarray(emb_g, np.float32), np.ascontiguousarray(w, np.float32)
        sid = np.ascontiguousarray(sid, np.int64).reshape(-1)
        bias = None if bias is None else np.ascontiguousarray(bias, np.float32)
        (S, gin), Cout, B = emb_g.shape, w.shape[0], sid.shape[0]
        assert w.shape == (Cout, gin) and (bias is None or bias.shape == (Cout,))
        out = np.full(B * Cout + pad, -7.5e29, np.float32)
        self._hook("test_speaker_cond", device, B, gin, S, Cout, _ptr(emb_g), _ptr(sid), _ptr(w), _ptr(bias), _ptr(out),
                   out.size)
        return out

    def test_speaker_cond_mix(self, consumers, emb_g=None, sid=None, weight=None, vectors=None, pad: int = 8, device=0):
        """launch_speaker_cond_mix (k_speaker_cond_mix) alone, one launch: ``consumers`` = [(w [Cout, gin], bias [Cout] or None)],
        with emb_g [S, gin], sid / weight [B, K], or vectors [B, gin] -> (g, [out per consumer]): flat arrays of B * gin and B * Cout
        floats + ``pad`` floats each, which start as -7.5e29 (mi355vits_test_speaker_cond_mix)."""
        t, keep = SpeakerMixTest(), []
        if vectors is not None:
            vectors = np.ascontiguousarray(vectors, np.float32)
            B, gin = vectors.shape
            t.vectors = _ptr(vectors)
        else:
            emb_g, weight = np.ascontiguousarray(emb_g, np.float32), np.ascontiguousarray(weight, np.float32)
            sid = np.ascontiguousarray(sid, np.int64)
            (B, K), gin = weight.shape, emb_g.shape[1]
            assert sid.shape == (B, K)
            t.n_speakers, t.n_terms = emb_g.shape[0], K
            t.emb_g, t.mix_weight, t.mix_sid = _ptr(emb_g), _ptr(weight), _ptr(sid)
        t.B, t.gin, t.n_jobs = B, gin, len(consumers)
        outs = []
        for q, (w, bias) in enumerate(consumers):
            w = np.ascontiguousarray(w, np.float32)
            assert w.ndim == 2 and w.shape[1] == gin
            bias = None if bias is None else np.ascontiguousarray(bias, np.float32)
            out = np.full(B * w.shape[0] + pad, -7.5e29, np.float32)
            keep += [w, bias]
            outs.append(out)
            t.w[q], t.Cout[q], t.out[q], t.out_floats[q] = _ptr(w), w.shape[0], _ptr(out), out.size
            if bias is not None:
                t.bias[q] = _ptr(bias)
        g = np.full(B * gin + pad, -7.5e29, np.float32)
        t.g, t.g_floats = _ptr(g), g.size
        self._hook("test_speaker_cond_mix", device, ctypes.byref(t))
        return g, outs

    def test_expand_prior(self, stats, cum, ylen, Ty, noise_scale=0.0, injected=None, z_prior=None, device=0) -> np.ndarray:
        """launch_expand_prior alone with injected noise: stats [B, 2 I, Tx], cum [B, Tx], ylen [B], noise_scale a number or [B],
        injected [B, I, frames >= Ty] or None -> z [B, I, Ty] (mi355vits_test_expand_prior)."""
        stats = np.ascontiguousarray(stats, np.float32)
        B, I2, Tx = stats.shape
        I = I2 // 2
        cum, ylen = np.ascontiguousarray(cum, np.int32), np.ascontiguousarray(ylen, np.int32)
        sc = np.zeros((B, 3), np.float32)
        sc[:, 0] = np.asarray(noise_scale, np.float32)
        inj = None if injected is None else np.ascontiguousarray(injected, np.float32)
        assert cum.shape == (B, Tx) and ylen.shape == (B,) and (inj is None or inj.shape[:2] == (B, I))
        z = np.full((B, I, int(Ty)), -7.5e29, np.float32) if z_prior is None else np.ascontiguousarray(z_prior, np.float32).copy()
        assert z.shape == (B, I, int(Ty))
        self._hook("test_expand_prior", device, B, I, Tx, int(Ty), _ptr(stats), _ptr(cum), _ptr(ylen), _ptr(inj), 0 if inj is None else inj.shape[2],
                   _ptr(sc), _ptr(z))
        return z

    def test_expand_prior_keyed(self, stats, cum, ylen, Ty, noise_scale, seed: int, utt, z_prior=None, device=0) -> np.ndarray:
        """launch_expand_prior alone with the kernel's own Philox noise (tensor id 1) under ``seed`` and utt [B]: stats [B, 2 I, Tx],
        cum [B, Tx], ylen [B], noise_scale a number or [B] -> z [B, I, Ty] (mi355vits_test_expand_prior_keyed)."""
        stats = np.ascontiguousarray(stats, np.float32)
        B, I2, Tx = stats.shape
        I = I2 // 2
        cum, ylen = np.ascontiguousarray(cum, np.int32), np.ascontiguousarray(ylen, np.int32)
        sc = np.zeros((B, 3), np.float32)
        sc[:, 0] = np.asarray(noise_scale, np.float32)
        u = np.ascontiguousarray(utt, np.uint64)
        assert cum.shape == (B, Tx) and ylen.shape == (B,) and u.shape == (B,)
        z = np.full((B, I, int(Ty)), -7.5e29, np.float32) if z_prior is None else np.ascontiguousarray(z_prior, np.float32).copy()
        assert z.shape == (B, I, int(Ty))
        self._hook("test_expand_prior_keyed", device, B, I, Tx, int(Ty), _ptr(stats), _ptr(cum), _ptr(ylen), _ptr(sc), int(seed), _ptr(u), _ptr(z))
        return z

    def test_sdp_noise(self, T: int, seed: int, utt, noise_w, z_prior=None, device=0) -> np.ndarray:
        """launch_sdp_noise alone with the kernel's own Philox noise (tensor id 0): utt [B], noise_w a number or [B] -> z [B, 2, T]
        (mi355vits_test_sdp_noise)."""
        u = np.ascontiguousarray(utt, np.uint64)
        B = u.shape[0]
        sc = np.zeros((B, 3), np.float32)
        sc[:, 2] = np.asarray(noise_w, np.float32)
        z = np.full((B, 2, int(T)), -7.5e29, np.float32) if z_prior is None else np.ascontiguousarray(z_prior, np.float32).copy()
        assert u.shape == (B,) and z.shape == (B, 2, int(T))
        self._hook("test_sdp_noise", device, B, int(T), int(seed), _ptr(u), _ptr(sc), _ptr(z))
        return z

    def test_embed(self, ids, lengths, emb, scale: float, y_prior=None, device=0) -> np.ndarray:
        """launch_embed alone: ids [B, T] int64, lengths [B], emb [num_symbols, H] -> y [B, H, T] (mi355vits_test_embed)."""
        ids = np.ascontiguousarray(ids, np.int64)
        emb = np.ascontiguousarray(emb, np.float32)
        ln = np.ascontiguousarray(lengths, np.int32)
        B, T = ids.shape
        S, H = emb.shape
        y = np.full((B, H, T), -7.5e29, np.float32) if y_prior is None else np.ascontiguousarray(y_prior, np.float32).copy()
        assert ln.shape == (B,) and y.shape == (B, H, T)
        self._hook("test_embed", device, B, T, H, S, _ptr(ids), _ptr(ln), _ptr(emb), float(scale), _ptr(y))
        return y

    def test_layernorm(self, x, gamma, beta, eps=1e-5, bias=None, premask_len=None, res=None, add_to=None, gelu=False, out_len=None,
                       alias=None, part_stride=None, y_prior=None, device=0) -> np.ndarray:
        """launch_layernorm alone (mi355vits_test_layernorm): x [B, C, T], or [nparts, B, C, T] = the partial sums of a split conv (laid
        out ``part_stride`` floats apart, default B C T); alias None / "x" / "res" / "add_to" = which input y is on the device."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
        x = f(x)
        parts = x.shape[0] if x.ndim == 4 else 1
        B, C, T = x.shape[-3:]
        n = B * C * T
        stride = n if part_stride is None else int(part_stride)
        if parts > 1 and stride != n:
            assert stride >= n
            xs = np.full((parts - 1) * stride + n, -7.5e29, np.float32)
            for p in range(parts):
                xs[p * stride:p * stride + n] = x[p].ravel()
            x = xs
        gamma, beta, bias, res, add_to = f(gamma), f(beta), f(bias), f(res), f(add_to)
        pl, ol = i32(premask_len), i32(out_len)
        assert gamma.shape == (C,) and beta.shape == (C,) and (bias is None or bias.shape == (C,))
        assert all(a is None or a.shape == (B, C, T) for a in (res, add_to)) and all(a is None or a.shape == (B,) for a in (pl, ol))
        y = np.full((B, C, T), -7.5e29, np.float32) if y_prior is None else f(y_prior).copy()
        assert y.shape == (B, C, T)
        t = LayerNormTest()
        t.B, t.C, t.T, t.nparts, t.gelu, t.alias, t.eps, t.part_stride = B, C, T, parts, int(bool(gelu)), LN_ALIAS[alias], float(eps), stride
        t.x, t.bias, t.res, t.add_to, t.gamma, t.beta, t.y = _ptr(x), _ptr(bias), _ptr(res), _ptr(add_to), _ptr(gamma), _ptr(beta), _ptr(y)
        t.premask_len = _ptr(pl)
        t.out_len = _ptr(ol)
        self._hook("test_layernorm", device, ctypes.byref(t))
        return y

    def test_dp_det(self, x, lengths, w, cond=None, math=MATH_BF16X3, logw_prior=None, device=0) -> np.ndarray:
        """launch_dp_det alone (mi355vits_test_dp_det): x [B, H, T], lengths [B], w = dict w1 [F, H, K], b1, g1, be1, w2 [F, F, K], b2, g2,
        be2, proj_w [F], proj_b [1]; cond [B, H] or None -> logw [B, T]."""
        f = lambda a: np.ascontiguousarray(a, np.float32)
        x = f(x)
        B, H, T = x.shape
        ln = np.ascontiguousarray(lengths, np.int32)
        ww = {k: f(w[k]) for k in ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "proj_w", "proj_b")}
        F, Hw, K = ww["w1"].shape
        assert Hw == H and ww["w2"].shape == (F, F, K) and ww["proj_w"].size == F and ww["proj_b"].size == 1 and ln.shape == (B,)
        assert all(ww[k].shape == (F,) for k in ("b1", "g1", "be1", "b2", "g2", "be2"))
        c = None if cond is None else f(cond)
        assert c is None or c.shape == (B, H)
        logw = np.full((B, T), -7.5e29, np.float32) if logw_prior is None else f(logw_prior).copy()
        assert logw.shape == (B, T)
        t = DpDetTest()
        t.B, t.H, t.F, t.K, t.T, t.math = B, H, F, K, T, int(math)
        t.x, t.cond, t.len, t.logw = _ptr(x), _ptr(c), _ptr(ln), _ptr(logw)
        for k, v in ww.items():
            setattr(t, k, _ptr(v))
        self._hook("test_dp_det", device, ctypes.byref(t))
        return logw

    def lab_dp_det_plan(self, H, F, K, math=MATH_BF16X3):
        """(output columns of a k_dp_det work item, the two convs' reach 2 (K // 2), the launch's LDS bytes) from the library's own
        functions (mi355vits_lab_dp_det_plan); NativeError where the hook would refuse the shape."""
        cols, halo, lds = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self._hook("lab_dp_det_plan", int(H), int(F), int(K), int(math), ctypes.byref(cols), ctypes.byref(halo), ctypes.byref(lds))
        return cols.value, halo.value, lds.value

    def test_resample(self, x, lengths, in_hz: int, out_hz: int, device=0):
        """The product's resampler launch (k_resample) on caller-given f32 rows: x [B, row_stride], lengths [B] valid samples
        of each row (what lies past them is never looked at) -> (y [B, max n_out] with zeros past a row's output length,
        y_lengths [B], peaks [B])."""
        x = np.ascontiguousarray(x, np.float32)
        ln = np.ascontiguousarray(lengths, np.int32).reshape(-1)
        B, stride = x.shape
        g = int(np.gcd(int(in_hz), int(out_hz))) if in_hz > 0 and out_hz > 0 else 1
        up, down = int(out_hz) // g, int(in_hz) // g
        ys = max(1, int(max(-(-int(n) * up // down) for n in ln))) if up > 0 else 1
        y = np.empty((B, ys), np.float32)
        yl = np.zeros(B, np.int32)
        pk = np.zeros(B, np.float32)
        self._hook("test_resample", device, B, stride, _ptr(x), _ptr(ln), int(in_hz), int(out_hz), ys, _ptr(y), _ptr(yl), _ptr(pk))
        return y, yl, pk

    def test_alignment(self, frames, lengths, audio, alen, hop: int, L: int = 1, M: int = 1, levels: bool = True, device=0) -> Alignment:
        """The product's alignment launch (k_align) alone on caller-given arrays: frames [B, T] int32 (read below lengths[b]
        only), lengths [B] phonemes of a row, audio [B, row_stride] f32 with alen [B] valid samples each (what lies past them is
        never looked at), hop samples per frame, L / M the rate ratio -> ``Alignment`` (``sample_rate`` None)."""
        fr = np.ascontiguousarray(frames, np.int32)
        ln = np.ascontiguousarray(lengths, np.int32).reshape(-1)
        au = np.ascontiguousarray(audio, np.float32)
        al = np.ascontiguousarray(alen, np.int32).reshape(-1)
        B, T = fr.shape
        if au.ndim != 2 or au.shape[0] != B or ln.shape[0] != B or al.shape[0] != B:
            raise ValueError("frames [B, T], lengths [B], audio [B, row_stride], alen [B]")
        o = [np.zeros((B, T), np.int32) for _ in range(3)]
        lv = [np.zeros((B, T), np.float32) for _ in range(2)] if levels else [None, None]
        self._hook("test_alignment", device, B, T, _ptr(fr), _ptr(ln), au.shape[1], _ptr(au), _ptr(al), int(hop), int(L), int(M), _ptr(o[0]),
                   _ptr(o[1]), _ptr(o[2]), _ptr(lv[0]), _ptr(lv[1]))
        return Alignment(o[0], o[1], o[2], lv[0], lv[1], None)

    def bench_conv1d(self, B, Cin, Cout, T, K, dilation=1, epi=0, reps=20, device=0) -> float:
        ms = ctypes.c_float(-1.0)
        self._hook("bench_conv1d", device, B, Cin, Cout, T, K, dilation, epi, reps, ctypes.byref(ms))
        return float(ms.value)

    def probe_device(self, device=0) -> dict:
        """The box probe: what this lease's chip gives the kernels' access patterns (include/mi355vits_lab.h)."""
        self._need_hooks()
        out = (ctypes.c_double * 8)()
        rc = self.lib.mi355vits_probe_device(device, out)
        if rc != 0:
            raise RuntimeError(f"mi355vits_probe_device failed: rc={rc}")
        return {"l2_stream_GBps": round(out[0], 1), "l2_hit_latency_ns": round(out[1], 1), "hbm_copy_GBps": round(out[2], 1), "cus": int(out[3]),
                "l2_stream_beside_copy_GBps": round(out[4], 1), "table_24MB_stream_GBps": round(out[5], 1),
                "latency_32MB_ns": round(out[6], 1), "latency_1GiB_ns": round(out[7], 1)}

    def test_mfma_layout(self, device=0) -> float:
        self._need_hooks()
        err = ctypes.c_float(-1.0)
        rc = self.lib.mi355vits_test_mfma_layout(device, ctypes.byref(err))
        if rc != 0:
            raise NativeError(rc, self.create_error() + f" (max err {err.value})")
        return float(err.value)


_default_lock = threading.Lock()
_default: Optional[NativeLibrary] = None


def default_library() -> NativeLibrary:
    """The product library (gfx950).  Raises when it has not been built."""
    global _default
    with _default_lock:
        if _default is None:
            _default = NativeLibrary(DEFAULT_LIBRARY)
        return _default


_hooks: Optional[NativeLibrary] = None


def hooks_library() -> NativeLibrary:
    """libmi355vits_hooks.so: the product's own object files + the hooks of include/mi355vits_lab.h (kernel unit tests, conv
    micro-benchmark, box probes).  Test infrastructure and bench.py's box probe; nothing on the product path opens it."""
    global _hooks
    with _default_lock:
        if _hooks is None:
            _hooks = NativeLibrary(HOOKS_LIBRARY)
            if not _hooks.has_hooks:
                raise RuntimeError(f"{HOOKS_LIBRARY} does not export include/mi355vits_lab.h")
        return _hooks


class _ResultHolder:
    """Keeps one ``mi355vits_result`` alive for the numpy views made of it; releases it when they are gone."""

    def __init__(self, native: "NativeLibrary", r: Result):
        self._native = native
        self._r = Result()
        ctypes.memmove(ctypes.byref(self._r), ctypes.byref(r), ctypes.sizeof(Result))

    def view(self, ptr, ctype, dtype, B: int, L: int) -> np.ndarray:
        n = int(B) * int(L)
        buf = (ctype * n).from_address(ctypes.addressof(ptr.contents))
        buf._holder = self  # the array's base chain (memoryview -> ctypes array) keeps the holder alive
        return np.frombuffer(buf, dtype=dtype, count=n).reshape(B, L)

    def __del__(self):
        try:
            self._native.lib.mi355vits_free_result(ctypes.byref(self._r))
        except Exception:
            pass


class _BlockHolder:
    """The same for one ``mi355vits_packed_result`` or one streams result: ONE pinned block (shared by the views of all its
    streams) that lives as long as any view of it and then goes back through ``free``, the struct's own free function."""

    def __init__(self, free, r):
        self._free = free
        self._r = type(r)()
        ctypes.memmove(ctypes.byref(self._r), ctypes.byref(r), ctypes.sizeof(type(r)))

    def view(self) -> np.ndarray:
        """Every byte of the block (headers, if any, + data) as one uint8 array that owns the holder."""
        n = int(self._r.n_bytes)
        buf = (ctypes.c_uint8 * n).from_address(ctypes.addressof(self._r.bytes.contents))
        buf._holder = self
        return np.frombuffer(buf, dtype=np.uint8, count=n)

    def __del__(self):
        try:
            self._free(ctypes.byref(self._r))
        except Exception:
            pass


class PackedAudio:
    """A batch's audio as one contiguous stream (``mi355vits_run_packed``).  Everything is a view of ONE pinned block that goes
    back to the library when the last view is gone: ``data`` [total_samples] (silences included) in the stream's ``encoding`` —
    int16 ("s16le"), uint8 G.711 codes ("ulaw" / "alaw") or float32 ("f32le") —, ``rows[i]`` =
    ``data[offsets[i] : offsets[i] + lengths[i]]`` (no copies), ``wav`` the whole file (header + data) as a memoryview, or None
    when no header was asked for; ``offsets`` / ``lengths`` / ``peaks`` [n] per entry, in samples.  ``pcm`` is ``data`` of an
    int16 stream, and raises for any other encoding.  With edge trimming on (``Engine.set_edge_trim``) entry i is samples
    ``first[i] : end[i]`` of its row (``lengths[i] = end[i] - first[i]``); both are ``None`` when trimming is off.  With a loudness
    target (``Engine.set_loudness_target``) ``lufs[i]`` is the entry's row's integrated loudness, ``gain[i]`` the linear gain its
    samples carry and ``limited[i]`` whether the ceiling bounded it; all three are ``None`` when the target is off.
    A compressed stream (``compression == "flac"``): ``flac`` is the complete FLAC file as a memoryview of the block, ``data``,
    ``rows`` and ``wav`` are ``None`` (no decoder is part of the product), and ``offsets`` / ``lengths`` / ``peaks`` /
    ``total_samples`` are those of the same call uncompressed, in samples."""

    def __init__(self, pcm, offsets, lengths, peaks, wav, sample_rate=None, encoding="s16le", first=None, end=None, lufs=None,
                 gain=None, limited=None, compression=None, flac=None, total_samples=None):
        self.compression, self.flac = compression, flac
        self.first, self.end = first, end
        self.lufs, self.gain, self.limited = lufs, gain, limited
        self.alignment: Optional[Alignment] = None  # set by InferenceSession.run_packed(alignment=...): spans in stream samples
        # a stream of Engine.run_streams / fetch_streams: the uint8 block all streams of that call share, and this stream's place in
        # it — block[stream_offset : stream_offset + stream_bytes] = header (if any) + data + pad; data_offset % 16 == 0.  Else None.
        self.block = self.stream_offset = self.stream_bytes = self.data_offset = None
        self.data, self.offsets, self.lengths, self.peaks, self.wav = pcm, offsets, lengths, peaks, wav
        self.encoding = encoding
        self.sample_rate = sample_rate  # of every sample of the stream: the rate the run ran at
        self.total_samples = int(pcm.shape[0]) if pcm is not None else int(total_samples)
        self.rows = None if pcm is None else [pcm[int(o): int(o) + int(n)] for o, n in zip(offsets, lengths)]

    @property
    def pcm(self):
        if self.compression:
            raise ValueError(f"this packed stream is compressed ({self.compression}): read .flac")
        if self.encoding != "s16le":
            raise ValueError(f"this packed stream is {self.encoding}, not int16 PCM: read .data")
        return self.data


class Engine:
    """A voice loaded on one GPU (wraps ``mi355vits_handle``)."""

    def __init__(self, weights, device: int = 0, library: Optional[NativeLibrary] = None):
        """``weights``: path to an ``.m355`` container, its bytes, or another ``Engine`` — then this is a further lane
        on that engine's device sharing its weight replica (``mi355vits_clone``; ``device`` is ignored)."""
        self.native = weights.native if isinstance(weights, Engine) else (library or default_library())
        self._h = ctypes.c_void_p()
        L = self.native.lib
        if isinstance(weights, Engine):
            rc = L.mi355vits_clone(weights._h, ctypes.byref(self._h))
            if rc != 0:
                self._h = ctypes.c_void_p()
                raise NativeError(rc, (L.mi355vits_last_error(weights._h) or b"").decode("utf-8", "replace"))
            device = weights.device
        elif isinstance(weights, (bytes, bytearray, memoryview)):
            buf = bytes(weights)
            rc = L.mi355vits_create_from_buffer(buf, len(buf), device, ctypes.byref(self._h))
        else:
            rc = L.mi355vits_create(os.fsencode(str(weights)), device, ctypes.byref(self._h))
        if rc != 0:
            self._h = ctypes.c_void_p()
            raise NativeError(rc, self.native.create_error())
        c = CVitsConfig()
        self._check(L.mi355vits_get_config(self._h, ctypes.byref(c)))
        self.config = VitsConfig.from_c(c)
        self.device = device
        self._last_batch = 0  # rows of the last completed run (fetch_packed's default pack with a tail or a header)
        self.last_timing_factor = None  # [B] of the last timed run_packed (run returns it as "timing_factor")
        self._last_rate = int(self.config.sample_rate)  # the rate it ran at (results of a run keep it)

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise NativeError(rc, (self.native.lib.mi355vits_last_error(self._h) or b"").decode("utf-8", "replace"))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.native.lib.mi355vits_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- one synthesis call ---------------------------------------------------------------------
    def run(self, ids, lengths, scales, sid=None, *, seed: int = 0, utterance_base: int = 0, noise_w=None,
            noise_z=None, forced_durations=None, want_float: bool = True, want_pcm16: bool = False,
            device_only: bool = False, debug_taps: bool = False, pcm_volume=1.0, utterance_keys=None,
            stretch=None, min_frames=None, target_frames=None, speakers=None, gain=None, ramp_samples=None,
            pitch=None) -> Dict[str, np.ndarray]:
        """One synthesis call.  Per-row settings (``mi355vits_run_rows``): ``scales`` [B, 3], ``pcm_volume`` [B] and
        ``utterance_keys`` [B] (Philox utterance index of each row, instead of ``utterance_base + b``).  Row b is then bitwise
        its own call with scalar settings and ``utterance_base = utterance_keys[b]`` (same phoneme-length class).
        Timing (``mi355vits_run_timed``, when any of the three is given): ``stretch`` [B, Tx] duration multiplier per phoneme,
        ``min_frames`` [B, Tx] frames a phoneme is held at least, ``target_frames`` [B] the row's latent frames (0 = none); the
        result then carries ``"timing_factor"`` [B], the factor s* every row was fitted with (1.0 without a target).
        ``speakers`` (``mi355vits_run_speakers``; a multi-speaker voice): one entry per row in place of ``sid``, which is then not
        read — an ``int`` (that speaker), a dict ``{sid: weight}`` (a blend, terms in the dict's order; weights need not sum to 1) or
        a 1-D float array of ``gin_channels`` values (the caller's own vector); ints and dicts may be mixed in one call, vectors go
        in a call of their own (``ValueError`` otherwise).  ``SpeakerArgs`` itself is taken as it is.
        Levels (``mi355vits_run_levels``, when ``gain`` is given): ``gain`` [B, Tx] linear gain per phoneme (0 .. 1024) and
        ``ramp_samples`` (an int or [B], 0 .. 4096 native-rate samples; default 0) the half-width of the linear ramp across every
        phoneme boundary: the envelope is applied to the native waveform on the device, in front of everything that reads it.
        ``LevelArgs`` itself is taken as ``gain``.
        Pitch (``mi355vits_run_pitch``, when ``pitch`` is given): ``pitch`` [B, Tx] the pitch multiplier of each phoneme (0.5 .. 2);
        the duration is kept (the run stretches each phoneme by its ratio and the device warps the waveform back), except with
        ``forced_durations``, whose frames are the synthesized ones.  This is resampling: formants move with the pitch.
        ``PitchArgs`` itself is taken as it is."""
        timing, tkeep = self._timing_args(np.shape(ids), stretch, min_frames, target_frames)
        spk, skeep = self._speaker_args(np.shape(ids), speakers)
        lvl, lkeep = self._level_args(np.shape(ids), gain, ramp_samples)
        pit, pkeep = self._pitch_args(np.shape(ids), pitch)
        a, rows, per_row, keep = self._args(ids, lengths, scales, sid, seed, utterance_base, noise_w, noise_z, forced_durations,
                                            pcm_volume, utterance_keys)
        a.flags = (WANT_FLOAT if want_float else 0) | (WANT_PCM16 if want_pcm16 else 0) | \
                  (DEVICE_ONLY if device_only else 0) | (DEBUG_TAPS if debug_taps else 0)
        r = Result()
        if pit is not None:
            self._check(self.native.lib.mi355vits_run_pitch(self._h, ctypes.byref(a), ctypes.byref(rows) if per_row else None,
                                                            ctypes.byref(timing) if timing is not None else None,
                                                            ctypes.byref(spk) if spk is not None else None,
                                                            ctypes.byref(lvl) if lvl is not None else None,
                                                            ctypes.byref(pit), ctypes.byref(r)))
        elif lvl is not None:
            self._check(self.native.lib.mi355vits_run_levels(self._h, ctypes.byref(a), ctypes.byref(rows) if per_row else None,
                                                             ctypes.byref(timing) if timing is not None else None,
                                                             ctypes.byref(spk) if spk is not None else None,
                                                             ctypes.byref(lvl), ctypes.byref(r)))
        elif spk is not None:
            self._check(self.native.lib.mi355vits_run_speakers(self._h, ctypes.byref(a), ctypes.byref(rows) if per_row else None,
                                                               ctypes.byref(timing) if timing is not None else None,
                                                               ctypes.byref(spk), ctypes.byref(r)))
        elif timing is not None:
            self._check(self.native.lib.mi355vits_run_timed(self._h, ctypes.byref(a), ctypes.byref(rows) if per_row else None,
                                                            ctypes.byref(timing), ctypes.byref(r)))
        elif per_row:
            self._check(self.native.lib.mi355vits_run_rows(self._h, ctypes.byref(a), ctypes.byref(rows), ctypes.byref(r)))
        else:
            self._check(self.native.lib.mi355vits_run(self._h, ctypes.byref(a), ctypes.byref(r)))
        del keep, skeep, lkeep, pkeep
        self._last_batch = int(a.batch)
        self._last_rate = self.output_rate  # read when the run started; only this thread sets it meanwhile
        out = self._take(r)
        if timing is not None:
            out["timing_factor"] = tkeep[-1]
        return out

    @staticmethod
    def _level_args(shape, gain, ramp_samples):
        """``mi355vits_level_args`` (or None without ``gain``) + the arrays it points into.  Shapes are checked as ``stretch``'s is."""
        if gain is None:
            if ramp_samples is not None:
                raise ValueError("ramp_samples needs gain")
            return None, []
        if isinstance(gain, LevelArgs):
            return gain, []
        if len(shape) != 2:
            raise ValueError("'input' must have shape [batch, phonemes]")
        B, Tx = shape
        v, keep = LevelArgs(), []
        gain = np.ascontiguousarray(gain, dtype=np.float32)
        if gain.shape != (B, Tx):
            raise ValueError("gain must have shape [batch, phonemes]")
        keep.append(gain)
        v.gain = _fptr(gain)
        if ramp_samples is not None:
            if not np.issubdtype(np.asarray(ramp_samples).dtype, np.integer):
                raise ValueError("ramp_samples must hold integers")
            r64 = np.asarray(ramp_samples, dtype=np.int64)
            r64 = np.full(B, int(r64), np.int64) if r64.ndim == 0 else r64
            if r64.shape != (B,):
                raise ValueError("ramp_samples must be an int or have shape [batch]")
            ramp = np.ascontiguousarray(np.clip(r64, -1, 2**31 - 1), dtype=np.int32)  # (out of range either way: the library names the row)
            keep.append(ramp)
            v.ramp_samples = ramp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        return v, keep

    @staticmethod
    def _pitch_args(shape, pitch):
        """``mi355vits_pitch_args`` (or None without ``pitch``) + the array it points into.  The shape is checked as ``stretch``'s is."""
        if pitch is None:
            return None, []
        if isinstance(pitch, PitchArgs):
            return pitch, []
        if len(shape) != 2:
            raise ValueError("'input' must have shape [batch, phonemes]")
        ratio = np.ascontiguousarray(pitch, dtype=np.float32)
        if ratio.shape != tuple(shape):
            raise ValueError("pitch must have shape [batch, phonemes]")
        v = PitchArgs()
        v.ratio = _fptr(ratio)
        return v, [ratio]

    def _speaker_args(self, shape, speakers):
        """``mi355vits_speaker_args`` (or None without ``speakers``) + the arrays it points into (``speaker_tables``)."""
        if speakers is None:
            return None, []
        if isinstance(speakers, SpeakerArgs):
            return speakers, []
        if len(shape) != 2:
            raise ValueError("'input' must have shape [batch, phonemes]")
        tab = speaker_tables(speakers, shape[0], int(self.config.gin_channels))
        s = SpeakerArgs()
        if tab[0] == "mix":
            s.n_terms = tab[1].shape[1]
            s.mix_sid, s.mix_weight = tab[1].ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _fptr(tab[2])
        else:
            s.vectors = _fptr(tab[1])
        return s, list(tab[1:])

    def speaker_embedding(self, sid: int) -> np.ndarray:
        """Row ``sid`` of the voice's speaker table ``emb_g`` [gin_channels] (``mi355vits_get_speaker_embedding``: a host copy, no
        stream work) — the vector ``run(..., speakers=[sid])`` speaks with, to average, interpolate or fit from."""
        out = np.empty(max(int(self.config.gin_channels), 1), np.float32)
        self._check(self.native.lib.mi355vits_get_speaker_embedding(self._h, int(sid), _fptr(out), out.size))
        return out[: int(self.config.gin_channels)]

    @staticmethod
    def _timing_args(shape, stretch, min_frames, target_frames):
        """``mi355vits_timing_args`` (or None without any of the three) + the arrays it points into; the last of them is
        ``factor_out`` [B].  Shapes are checked as ``forced_durations``' is."""
        if stretch is None and min_frames is None and target_frames is None:
            return None, []
        if len(shape) != 2:
            raise ValueError("'input' must have shape [batch, phonemes]")
        B, Tx = shape
        t, keep = TimingArgs(), []
        if stretch is not None:
            stretch = np.ascontiguousarray(stretch, dtype=np.float32)
            if stretch.shape != (B, Tx):
                raise ValueError("stretch must have shape [batch, phonemes]")
            keep.append(stretch)
            t.stretch = _fptr(stretch)
        if min_frames is not None:
            if not np.issubdtype(np.asarray(min_frames).dtype, np.integer):
                raise ValueError("min_frames must hold integers")
            min_frames = np.ascontiguousarray(min_frames, dtype=np.int32)
            if min_frames.shape != (B, Tx):
                raise ValueError("min_frames must have shape [batch, phonemes]")
            keep.append(min_frames)
            t.min_frames = min_frames.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        if target_frames is not None:
            if not np.issubdtype(np.asarray(target_frames).dtype, np.integer):
                raise ValueError("target_frames must hold integers")
            tf64 = np.asarray(target_frames, dtype=np.int64).reshape(-1)
            if tf64.shape != (B,):
                raise ValueError("target_frames must have shape [batch]")
            target_frames = np.ascontiguousarray(np.clip(tf64, -1, 2**31 - 1), dtype=np.int32)  # (out of range either way: the library names the row)
            keep.append(target_frames)
            t.target_frames = target_frames.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        factor = np.full(B, np.nan, np.float32)
        keep.append(factor)
        t.factor_out = _fptr(factor)
        return t, keep

    def _args(self, ids, lengths, scales, sid, seed, utterance_base, noise_w, noise_z, forced_durations, pcm_volume, utterance_keys):
        """The feed as ``mi355vits_run_args`` + ``mi355vits_row_args`` (flags not set): (args, rows, any per-row setting, the
        arrays the two structs point into — keep them alive across the call)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if ids.ndim != 2:
            raise ValueError("'input' must have shape [batch, phonemes]")
        B, Tx = ids.shape
        lengths = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
        if lengths.shape[0] != B:
            raise ValueError("'input_lengths' must have shape [batch]")
        scales = np.ascontiguousarray(scales, dtype=np.float32)
        rows = RowArgs()
        per_row = False
        if scales.ndim == 2:
            if scales.shape != (B, 3):
                raise ValueError("per-row 'scales' must have shape [batch, 3]")
            rows.scales, per_row = _fptr(scales), True
        elif scales.reshape(-1).shape[0] != 3:
            raise ValueError("'scales' must hold [noise_scale, length_scale, noise_w]")
        a = RunArgs()
        keep = [ids, lengths, scales]
        a.batch, a.tx_max = B, Tx
        a.ids = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        a.lengths = lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        if not per_row:
            a.scales = _fptr(scales)
        if np.ndim(pcm_volume) > 0:
            vol = np.ascontiguousarray(pcm_volume, dtype=np.float64).reshape(-1)
            if vol.shape[0] != B:
                raise ValueError("per-row 'pcm_volume' must have shape [batch]")
            keep.append(vol)
            rows.pcm_volume, per_row = vol.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), True
            pcm_volume = 1.0
        if utterance_keys is not None:
            keys = np.array([int(k) & 0xFFFFFFFFFFFFFFFF for k in np.asarray(utterance_keys).reshape(-1).tolist()], np.uint64)
            if keys.shape[0] != B:
                raise ValueError("'utterance_keys' must have shape [batch]")
            keep.append(keys)
            rows.utterance, per_row = keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), True
        if sid is not None:
            sid = np.ascontiguousarray(sid, dtype=np.int64).reshape(-1)
            if sid.shape[0] != B:
                raise ValueError("'sid' must have shape [batch]")
            keep.append(sid)
            a.sid = sid.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        a.seed = seed & 0xFFFFFFFFFFFFFFFF
        a.utterance_base = utterance_base
        if noise_w is not None:
            noise_w = np.ascontiguousarray(noise_w, dtype=np.float32)
            if noise_w.shape != (B, 2, Tx):
                raise ValueError("noise_w must have shape [batch, 2, phonemes]")
            keep.append(noise_w)
            a.noise_w = _fptr(noise_w)
        if noise_z is not None:
            noise_z = np.ascontiguousarray(noise_z, dtype=np.float32)
            if noise_z.ndim != 3 or noise_z.shape[:2] != (B, self.config.inter_channels):
                raise ValueError("noise_z must have shape [batch, inter_channels, frames]")
            keep.append(noise_z)
            a.noise_z = _fptr(noise_z)
            a.noise_z_frames = noise_z.shape[2]
        if forced_durations is not None:
            forced_durations = np.ascontiguousarray(forced_durations, dtype=np.int32)
            if forced_durations.shape != (B, Tx):
                raise ValueError("forced_durations must have shape [batch, phonemes]")
            keep.append(forced_durations)
            a.forced_durations = forced_durations.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        a.pcm_volume = float(pcm_volume)
        return a, rows, per_row, keep

    # ---- the packed stream ----------------------------------------------------------------------
    @staticmethod
    def _pack_args(order, lead_samples, tail_samples, wav):
        """``mi355vits_pack_args`` (or None: the library's default pack) + the arrays it points into."""
        if order is None and lead_samples is None and not tail_samples and not wav:
            return None, []
        p, keep = PackArgs(), []
        for name, arr, dtype, ctype in (("order", order, np.int32, ctypes.c_int32), ("lead_samples", lead_samples, np.int64, ctypes.c_int64)):
            if arr is not None:
                src = np.asarray(arr).reshape(-1)
                if src.size and not np.issubdtype(src.dtype, np.integer):
                    raise ValueError(f"'{name}' must hold integers")
                v = np.ascontiguousarray(src, dtype=dtype)
                keep.append(v)
                setattr(p, name, v.ctypes.data_as(ctypes.POINTER(ctype)))
        sizes = {int(v.shape[0]) for v in keep}
        if len(sizes) > 1:
            raise ValueError("'order' and 'lead_samples' must have the same length")
        p.n = sizes.pop() if sizes else -1  # -1: every row of the batch, filled in by the caller
        p.tail_samples = int(tail_samples)
        p.wav_header = int(bool(wav))
        return p, keep

    def run_packed(self, ids, lengths, scales, sid=None, *, order=None, lead_samples=None, tail_samples: int = 0, wav: bool = False,
                   seed: int = 0, utterance_base: int = 0, noise_w=None, noise_z=None, forced_durations=None,
                   debug_taps: bool = False, pcm_volume=1.0, utterance_keys=None, compression=_HANDLE,
                   stretch=None, min_frames=None, target_frames=None, speakers=None, gain=None, ramp_samples=None,
                   pitch=None) -> PackedAudio:
        """One synthesis call whose result is ONE contiguous stream (``mi355vits_run_packed``; int16 unless
        ``set_output_encoding`` says otherwise — then the header is the 58-byte non-PCM one): entry i = the valid samples
        of row ``order[i]`` (default: every row in order) behind ``lead_samples[i]`` zero samples, ``tail_samples`` zeros after
        the last entry, with ``wav`` a 44-byte RIFF header in front.  Each entry is bitwise that row of
        ``run(..., want_pcm16=True)`` for the same arguments; one kernel, one device-to-host copy of exactly that many bytes.
        ``compression="flac"`` / ``None``: this call's stream compressed or not, whatever ``set_output_compression`` says (the
        setting is put back afterwards); with FLAC the result's ``.flac`` is the file and ``wav=True`` raises ``ValueError``.
        With any of ``stretch`` / ``min_frames`` / ``target_frames`` (see ``run``): a timed run that keeps its audio on the device
        (``mi355vits_run_timed`` with ``MI355VITS_DEVICE_ONLY``), then ``fetch_packed`` of it — one synchronisation more; the
        factors are left in ``last_timing_factor``.  ``speakers`` (see ``run``) goes the same way: a speakers run that keeps its
        audio on the device, then ``fetch_packed``; so do ``gain`` / ``ramp_samples`` (``mi355vits_run_levels``) and ``pitch``
        (``mi355vits_run_pitch``)."""
        if stretch is not None or min_frames is not None or target_frames is not None or speakers is not None or gain is not None or ramp_samples is not None or pitch is not None:
            comp = self._call_compression(compression, wav)  # refuses wav + FLAC before anything runs
            res = self.run(ids, lengths, scales, sid, seed=seed, utterance_base=utterance_base, noise_w=noise_w, noise_z=noise_z,
                           forced_durations=forced_durations, want_float=False, want_pcm16=False, device_only=True,
                           debug_taps=debug_taps, pcm_volume=pcm_volume, utterance_keys=utterance_keys, stretch=stretch,
                           min_frames=min_frames, target_frames=target_frames, speakers=speakers, gain=gain, ramp_samples=ramp_samples,
                           pitch=pitch)
            self.last_timing_factor = res.get("timing_factor", self.last_timing_factor)
            return self.fetch_packed(order=order, lead_samples=lead_samples, tail_samples=tail_samples, wav=wav, compression=compression)
        comp = self._call_compression(compression, wav)
        a, rows, per_row, keep = self._args(ids, lengths, scales, sid, seed, utterance_base, noise_w, noise_z, forced_durations,
                                            pcm_volume, utterance_keys)
        a.flags = DEBUG_TAPS if debug_taps else 0
        p, pkeep = self._pack_args(order, lead_samples, tail_samples, wav)
        if p is not None and p.n < 0:
            p.n = a.batch
        enc = self.output_encoding  # read by the library when the call starts; only this thread sets it meanwhile
        trimmed = self.edge_trim[0] != 0.0  # likewise
        normalised = self.loudness_target[0] != 0.0
        r = PackedResult()
        with self._compression_for_call(compression):
            self._check(self.native.lib.mi355vits_run_packed(self._h, ctypes.byref(a), ctypes.byref(rows) if per_row else None,
                                                             None if p is None else ctypes.byref(p), ctypes.byref(r)))
        del keep, pkeep
        self._last_batch = int(a.batch)
        self._last_rate = self.output_rate
        return self._take_packed(r, bool(wav), enc, order if (trimmed or normalised) else None, trimmed, normalised, comp)

    def fetch_packed(self, *, order=None, lead_samples=None, tail_samples: int = 0, wav: bool = False, compression=_HANDLE) -> PackedAudio:
        """Pack the last completed run of this handle again (``mi355vits_fetch_packed``): that run's rows and per-row volumes,
        another order / silences / header; nothing is synthesised again.  ``compression`` as for ``run_packed``: one synthesis can be
        fetched raw and as FLAC."""
        comp = self._call_compression(compression, wav)
        p, pkeep = self._pack_args(order, lead_samples, tail_samples, wav)
        if p is not None and p.n < 0:
            p.n = self._last_batch  # every row of the last run (0 before the first: the library names the error)
        enc = self.output_encoding
        trimmed = self.edge_trim[0] != 0.0
        normalised = self.loudness_target[0] != 0.0
        r = PackedResult()
        with self._compression_for_call(compression):
            self._check(self.native.lib.mi355vits_fetch_packed(self._h, None if p is None else ctypes.byref(p), ctypes.byref(r)))
        del pkeep
        return self._take_packed(r, bool(wav), enc, order if (trimmed or normalised) else None, trimmed, normalised, comp)

    def _call_compression(self, compression, wav):
        """The compression a packed call will run with (its ``compression=`` or the handle's setting), as a name or None."""
        if compression is _HANDLE:
            comp = self.output_compression
        else:
            comp = {0: None, 1: "flac"}.get(compression_id(compression), compression)  # (an unknown number: the library refuses it)
        if comp == "flac" and wav:
            raise ValueError("wav=True with compression='flac': a FLAC stream carries its own header")
        return comp

    @contextlib.contextmanager
    def _compression_for_call(self, compression):
        """The handle's compression set to ``compression`` inside the ``with`` and put back behind it (nothing for ``_HANDLE``).
        Not safe on a handle that several threads share: as with every setter, one thread owns a handle while it calls."""
        if compression is _HANDLE:
            yield
            return
        before = int(self.native.lib.mi355vits_get_output_compression(self._h))
        self._check(self.native.lib.mi355vits_set_output_compression(self._h, compression_id(compression)))
        try:
            yield
        finally:
            self.native.lib.mi355vits_set_output_compression(self._h, before)

    # ---- several streams out of one run ---------------------------------------------------------
    @staticmethod
    def _stream_args(streams, batch: int):
        """A list of stream dicts — ``order`` (default: every row), ``lead_samples``, ``tail_samples``, ``wav``, ``encoding``
        (default "s16le"), ``trim=(ratio, keep_samples)``, ``loudness=(lufs, ceiling_db)`` — as an array of
        ``mi355vits_stream_args``, their count, what the array points into, and (trimmed, normalised) per stream.  With any of
        ``compression`` / ``limiter`` / ``true_peak`` in any dict: an array of ``mi355vits_stream_args2``."""
        known = {"order", "lead_samples", "tail_samples", "wav", "encoding", "trim", "loudness"} | Engine._STREAM_KEYS2
        streams = list(streams)
        v2 = any(not Engine._STREAM_KEYS2.isdisjoint(st) for st in streams)  # any of the v2 keys: mi355vits_stream_args2, the v2 entry
        arr2 = (StreamArgs2 * max(1, len(streams)))() if v2 else None
        arr, keep, flags = (StreamArgs * max(1, len(streams)))(), [], []
        for i, st in enumerate(streams):
            if set(st) - known:
                raise ValueError(f"stream {i}: unknown key(s) {sorted(set(st) - known)}")
            p, pkeep = Engine._pack_args(st.get("order"), st.get("lead_samples"), st.get("tail_samples", 0) or 0, st.get("wav", False))
            if p is None:
                p = PackArgs()
                p.n = -1
            if p.n < 0:
                p.n = int(batch)
            keep.append(pkeep)
            a = arr2[i].base if v2 else arr[i]
            a.pack = p
            a.encoding = encoding_id(st.get("encoding") or "s16le")
            ratio, tkeep = st.get("trim") or (0.0, 0)
            a.trim_ratio, a.trim_keep_samples = float(ratio or 0.0), int(tkeep)
            lufs, ceiling = st.get("loudness") or (0.0, -1.0)
            a.target_lufs, a.ceiling_dbfs = float(lufs or 0.0), float(-1.0 if ceiling is None else ceiling)
            flags.append((a.trim_ratio != 0.0, a.target_lufs != 0.0))
            if v2:
                arr2[i].compression = compression_id(st.get("compression"))
                arr2[i].limiter_window_samples = int(st.get("limiter") or 0)
                arr2[i].ceiling_mode = 1 if st.get("true_peak") else 0
        return (arr2 if v2 else arr), len(streams), keep, flags

    _STREAM_KEYS2 = frozenset({"compression", "limiter", "true_peak"})

    def run_streams(self, ids, lengths, scales, sid=None, *, streams, seed: int = 0, utterance_base: int = 0, noise_w=None, noise_z=None,
                    forced_durations=None, debug_taps: bool = False, pcm_volume=1.0, utterance_keys=None) -> List["PackedAudio"]:
        """One synthesis call whose result is SEVERAL streams (``mi355vits_run_streams``), one per dict of ``streams``: ``order``
        (the batch rows of the stream; default: all), ``lead_samples``, ``tail_samples``, ``wav``, ``encoding``, ``trim=(ratio,
        keep_samples)``, ``loudness=(lufs, ceiling_db)``.  Stream s is bitwise ``fetch_packed`` of the same pack with the handle set to
        that stream's encoding, trim and target; the handle's own settings are neither read nor changed.  One kernel writes all
        streams into one pinned block, one device-to-host copy brings it; the ``PackedAudio`` returned per stream are views of it.
        If ANY dict has one of the keys ``compression`` (``"flac"`` / ``None``), ``limiter`` (the limiter window in samples, 0 = off)
        or ``true_peak`` (bool), the call is ``mi355vits_run_streams2``: those three come from each stream as well (absent = off) and
        the handle's limiter window and ceiling mode are not read either.  A compressed stream's ``PackedAudio`` has
        ``compression == "flac"``, ``flac`` = a view of its file in the shared block and ``data`` / ``rows`` / ``wav`` = ``None``;
        every stream of such a call (and of no other) also carries ``frames`` and ``uncompressed_bytes`` (the v1 block of the uncompressed streams,
        which come first in the block)."""
        a, rows, per_row, keep = self._args(ids, lengths, scales, sid, seed, utterance_base, noise_w, noise_z, forced_durations,
                                            pcm_volume, utterance_keys)
        a.flags = DEBUG_TAPS if debug_taps else 0
        arr, n, skeep, flags = self._stream_args(streams, int(a.batch))
        v2 = isinstance(arr[0], StreamArgs2)
        r = StreamsResult2() if v2 else StreamsResult()
        call = self.native.lib.mi355vits_run_streams2 if v2 else self.native.lib.mi355vits_run_streams
        self._check(call(self._h, ctypes.byref(a), ctypes.byref(rows) if per_row else None, arr, n, ctypes.byref(r)))
        del keep, skeep
        self._last_batch = int(a.batch)
        self._last_rate = self.output_rate
        return self._take_streams(r, flags)

    def fetch_streams(self, streams) -> List["PackedAudio"]:
        """The last completed run of this handle as streams again (``mi355vits_fetch_streams``); nothing is synthesised again."""
        arr, n, skeep, flags = self._stream_args(streams, self._last_batch)
        v2 = isinstance(arr[0], StreamArgs2)
        r = StreamsResult2() if v2 else StreamsResult()
        self._check((self.native.lib.mi355vits_fetch_streams2 if v2 else self.native.lib.mi355vits_fetch_streams)(self._h, arr, n, ctypes.byref(r)))
        del skeep
        return self._take_streams(r, flags)

    def _take_streams(self, r, flags) -> List["PackedAudio"]:
        """``flags[s]`` = (trimmed, normalised) of stream s: which of ``first`` / ``end`` and ``lufs`` / ``gain`` / ``limited`` it fills."""
        S, E = int(r.n_streams), int(r.n_entries)
        free = self.native.lib.mi355vits_free_streams2 if isinstance(r, StreamsResult2) else self.native.lib.mi355vits_free_streams
        try:
            per_stream = lambda p: np.ctypeslib.as_array(p, shape=(S,)).copy()  # noqa: E731
            per_entry = lambda p: np.ctypeslib.as_array(p, shape=(E,)).copy()  # noqa: E731
            begin, nbytes, data_at, totals, encs = (per_stream(p) for p in (r.stream_offset, r.stream_bytes, r.data_offset, r.total_samples, r.encoding))
            base = np.ctypeslib.as_array(r.entry_base, shape=(S + 1,)).copy()
            offsets, lens, peaks, first = (per_entry(p) for p in (r.offsets, r.lengths, r.peaks, r.first))
            lufs, gain, limited = per_entry(r.lufs), per_entry(r.gain), per_entry(r.limited).astype(bool)
            v2 = isinstance(r, StreamsResult2)
            comps = per_stream(r.compression) if v2 else np.zeros(S, np.int32)
            nframes = per_stream(r.frames) if v2 else np.zeros(S, np.int32)
            plain_bytes = int(r.uncompressed_bytes) if v2 else int(r.n_bytes)
        except BaseException:
            free(ctypes.byref(r))
            raise
        block = _BlockHolder(free, r).view()  # the views below keep the block alive: no per-stream copy
        out = []
        for s in range(S):
            enc = _ENCODING_NAMES[int(encs[s])]
            dtype = np.dtype(ENCODINGS[enc][1])
            e0, e1 = int(base[s]), int(base[s + 1])
            d0 = int(data_at[s])
            flac = int(comps[s]) == 1
            whole = memoryview(block[int(begin[s]): int(begin[s]) + int(nbytes[s])]) if (flac or d0 != int(begin[s])) else None
            pcm = None if flac else block[d0: d0 + dtype.itemsize * int(totals[s])].view(dtype)
            wav = None if flac else whole
            trimmed, normalised = flags[s]
            out.append(PackedAudio(pcm, offsets[e0:e1], lens[e0:e1], peaks[e0:e1], wav, self._last_rate, enc,
                                   first[e0:e1] if trimmed else None, first[e0:e1] + lens[e0:e1].astype(first.dtype) if trimmed else None,
                                   lufs[e0:e1] if normalised else None, gain[e0:e1] if normalised else None,
                                   limited[e0:e1] if normalised else None, "flac" if flac else None, whole if flac else None,
                                   int(totals[s])))
            if v2:
                out[-1].frames, out[-1].uncompressed_bytes = int(nframes[s]), plain_bytes
            # where the stream sits in the block all streams of the call share
            out[-1].block, out[-1].stream_offset, out[-1].stream_bytes, out[-1].data_offset = block, int(begin[s]), int(nbytes[s]), d0
        return out

    def _take_packed(self, r: PackedResult, wav: bool, enc: str = "s16le", order=None, trimmed: bool = False,
                     normalised: bool = False, compression=None) -> PackedAudio:
        n = int(r.n)
        try:
            offsets = np.ctypeslib.as_array(r.offsets, shape=(n,)).copy()
            lens = np.ctypeslib.as_array(r.lengths, shape=(n,)).copy()
            peaks = np.ctypeslib.as_array(r.peaks, shape=(n,)).copy()
            dtype = np.dtype(ENCODINGS[enc][1])
            hdr = (WAV_HEADER_BYTES if enc == "s16le" else WAV_HEADER_BYTES_NON_PCM) if wav else 0
            data = dtype.itemsize * int(r.total_samples)
            total = int(r.total_samples)
            if compression:
                if int(r.n_bytes) < FLAC_HEADER_BYTES:
                    raise RuntimeError("mi355vits_packed_result: a FLAC stream shorter than its header")
            elif int(r.n_bytes) != hdr + data + (data & 1 if wav else 0):  # a WAV's odd data size is followed by one pad byte
                raise RuntimeError("mi355vits_packed_result: n_bytes does not match total_samples")
        except BaseException:
            self.native.lib.mi355vits_free_packed(ctypes.byref(r))
            raise
        block = _BlockHolder(self.native.lib.mi355vits_free_packed, r).view()
        pcm = None if compression else block[hdr: hdr + data].view(dtype)
        first = end = None
        if trimmed:
            # the edges the pack was placed with: the library holds them on the host for this ratio, nothing is launched
            e = self.fetch_edges()
            rows = np.arange(n) if order is None else np.asarray(order, np.int64).reshape(-1)
            first, end = e.first[rows], e.end[rows]
        lufs = gain = limited = None
        if normalised:
            # the measurement the pack was scaled with: the library holds it on the host, nothing is launched
            ld = self.fetch_loudness()
            rows = np.arange(n) if order is None else np.asarray(order, np.int64).reshape(-1)
            lufs, gain, limited = ld.lufs[rows], ld.gain[rows], ld.limited[rows]
        return PackedAudio(pcm, offsets, lens, peaks, memoryview(block) if wav else None, self._last_rate, enc, first, end, lufs,
                           gain, limited, compression or None, memoryview(block) if compression else None, total)

    def set_loudness_target(self, lufs, ceiling_db: float = -1.0) -> None:
        """Scale each entry of the packed streams made after this to ``lufs`` LUFS of ITU-R BS.1770-4 integrated loudness
        (``mi355vits_set_loudness_target``): ``gain = min(10 ** ((lufs - measured) / 20), 10 ** (ceiling_db / 20) / peak)`` takes
        the place of the peak normalisation of the int16 conversion (``"f32le"``: one multiply).  ``None`` / 0 (the default) =
        off; on: -70 <= lufs < 0 with a finite ``ceiling_db`` <= 0 — anything else raises and leaves the setting as it was.  Read by
        ``run_packed``, each ``fetch_packed`` and each ``fetch_loudness``; everything else is unchanged by it."""
        self._check(self.native.lib.mi355vits_set_loudness_target(self._h, float(lufs or 0.0), float(ceiling_db)))

    @property
    def loudness_target(self):
        """``(target_lufs, ceiling_db)`` of ``set_loudness_target``; target 0.0 = off."""
        t, c = ctypes.c_float(), ctypes.c_float()
        self._check(self.native.lib.mi355vits_get_loudness_target(self._h, ctypes.byref(t), ctypes.byref(c)))
        return float(t.value), float(c.value)

    def fetch_loudness(self) -> Loudness:
        """The integrated loudness of every row of the last completed run, and the gains of the current ``set_loudness_target``
        setting (``mi355vits_fetch_loudness``), whatever the run's flags were, at the rate it ran at."""
        r = LoudnessResult()
        self._check(self.native.lib.mi355vits_fetch_loudness(self._h, ctypes.byref(r)))
        try:
            B = int(r.batch)
            take = lambda p: np.ctypeslib.as_array(p, shape=(B,)).copy()  # noqa: E731
            return Loudness(take(r.lufs), take(r.gain), take(r.blocks), take(r.gated), take(r.limited).astype(bool),
                            float(r.target_lufs), float(r.ceiling_dbfs), int(r.sample_rate))
        finally:
            self.native.lib.mi355vits_free_loudness(ctypes.byref(r))

    def set_loudness_limiter(self, window_samples) -> None:
        """Turn the look-ahead peak limiter of the packed streams on (``mi355vits_set_loudness_limiter``): with a loudness target
        set, a row the ceiling would hold back keeps its full gain and only the samples within ``window_samples`` (1 .. 4096, at the
        run's rate) of a peak are turned down — the row reaches its target.  ``None`` / 0 (the default) = off; anything else raises
        and leaves the setting as it was.  Read by ``run_packed``, each ``fetch_packed``, ``run_streams`` / ``fetch_streams`` (for
        every stream with a target), ``fetch_loudness`` and ``fetch_limiter``; without a target it does nothing."""
        self._check(self.native.lib.mi355vits_set_loudness_limiter(self._h, int(window_samples or 0)))

    @property
    def loudness_limiter(self) -> int:
        """The window of ``set_loudness_limiter`` in samples; 0 = off."""
        return int(self.native.lib.mi355vits_get_loudness_limiter(self._h))

    def fetch_limiter(self) -> Limiter:
        """Which rows of the last completed run the limiter engages on under the current target, ceiling and window, and how far
        (``mi355vits_fetch_limiter``)."""
        r = LimiterResult()
        self._check(self.native.lib.mi355vits_fetch_limiter(self._h, ctypes.byref(r)))
        try:
            B = int(r.batch)
            take = lambda p: np.ctypeslib.as_array(p, shape=(B,)).copy()  # noqa: E731
            return Limiter(take(r.engaged).astype(bool), take(r.reduced_samples), take(r.min_scale), int(r.window_samples), int(r.sample_rate))
        finally:
            self.native.lib.mi355vits_free_limiter(ctypes.byref(r))

    def lab_limit(self, audio, lengths, g, c, U, window, envelope=None):
        """``NativeLibrary.lab_limit`` of this engine's library (the hooks library, the lab build or the CPU model)."""
        return self.native.lab_limit(audio, lengths, g, c, U, window, envelope)

    def set_loudness_ceiling_mode(self, mode) -> None:
        """What the ceiling of the loudness target bounds (``mi355vits_set_loudness_ceiling_mode``): ``"sample"`` (the default) the
        row's sample peak, ``"true_peak"`` its 4x oversampled peak — in the gain rule and in what the limiter looks at.  Read where
        the limiter window is read; without a target it does nothing to a pack."""
        self._check(self.native.lib.mi355vits_set_loudness_ceiling_mode(self._h, ceiling_mode_id(mode)))

    @property
    def loudness_ceiling_mode(self) -> str:
        """``"sample"`` or ``"true_peak"``."""
        return "true_peak" if int(self.native.lib.mi355vits_get_loudness_ceiling_mode(self._h)) == 1 else "sample"

    def fetch_true_peak(self) -> TruePeak:
        """The 4x oversampled peak of every row of the last completed run, whatever the mode (``mi355vits_fetch_true_peak``)."""
        r = TruePeakResult()
        self._check(self.native.lib.mi355vits_fetch_true_peak(self._h, ctypes.byref(r)))
        try:
            B = int(r.batch)
            return TruePeak(np.ctypeslib.as_array(r.true_peak, shape=(B,)).copy(), np.ctypeslib.as_array(r.peak, shape=(B,)).copy(),
                            int(r.sample_rate))
        finally:
            self.native.lib.mi355vits_free_true_peak(ctypes.byref(r))

    def set_edge_trim(self, ratio, keep_samples: int = 0) -> None:
        """Trim each entry's quiet edges in the packed streams made after this (``mi355vits_set_edge_trim``): a sample is loud iff
        ``abs(y) >= peak * ratio`` (one f32 multiply), an entry is its row from ``keep_samples`` before the first loud sample to
        ``keep_samples`` behind the last.  ``ratio`` 0 (the default) = off; NaN, < 0, > 1 or a negative keep raise and leave the
        setting as it was.  Read by ``run_packed``, each ``fetch_packed`` and each ``fetch_edges``; the padded results, ``fetch``
        and ``fetch_alignment`` are unchanged by it."""
        self._check(self.native.lib.mi355vits_set_edge_trim(self._h, float(ratio or 0.0), int(keep_samples)))

    @property
    def edge_trim(self):
        """``(ratio, keep_samples)`` of ``set_edge_trim``; ratio 0.0 = off."""
        ratio, keep = ctypes.c_float(), ctypes.c_int32()
        self._check(self.native.lib.mi355vits_get_edge_trim(self._h, ctypes.byref(ratio), ctypes.byref(keep)))
        return float(ratio.value), int(keep.value)

    def fetch_edges(self) -> Edges:
        """``first`` / ``end`` of every row of the last completed run under the current ``set_edge_trim`` setting
        (``mi355vits_fetch_edges``), whatever the run's flags were, at the rate it ran at."""
        r = EdgesResult()
        self._check(self.native.lib.mi355vits_fetch_edges(self._h, ctypes.byref(r)))
        try:
            B = int(r.batch)
            take = lambda p: np.ctypeslib.as_array(p, shape=(B,)).copy()  # noqa: E731
            return Edges(take(r.first), take(r.end), float(r.ratio), int(r.keep_samples), int(r.sample_rate))
        finally:
            self.native.lib.mi355vits_free_edges(ctypes.byref(r))

    def set_output_encoding(self, encoding) -> None:
        """The sample encoding of the packed streams made after this (``mi355vits_set_output_encoding``): ``"s16le"`` (the
        default), ``"ulaw"`` / ``"alaw"`` (G.711, one byte per sample: the codes of ``audioop.lin2ulaw`` / ``lin2alaw`` of the
        int16 stream) or ``"f32le"`` (the float waveform itself; ``pcm_volume`` does not apply).  Read by ``run_packed`` and by
        each ``fetch_packed``; ``run`` / ``fetch`` are unchanged by it."""
        self._check(self.native.lib.mi355vits_set_output_encoding(self._h, encoding_id(encoding)))

    @property
    def output_encoding(self) -> str:
        return _ENCODING_NAMES[int(self.native.lib.mi355vits_get_output_encoding(self._h))]

    def set_output_compression(self, compression) -> None:
        """The compression of the packed stream made after this (``mi355vits_set_output_compression``): ``"flac"`` — the S16LE
        stream as a complete FLAC file, its frames encoded on the GPU, lossless — or ``None`` (the default).  Read by ``run_packed``
        and by each ``fetch_packed``; ``run_streams`` / ``fetch_streams`` and everything else are unchanged by it."""
        self._check(self.native.lib.mi355vits_set_output_compression(self._h, compression_id(compression)))

    @property
    def output_compression(self) -> Optional[str]:
        return "flac" if int(self.native.lib.mi355vits_get_output_compression(self._h)) == 1 else None

    def set_output_rate(self, hz) -> None:
        """The sample rate of every result of the runs that start after this (``mi355vits_set_output_rate``): ``None`` / 0 or
        the voice's own rate = native; else the waveform is resampled on the GPU (``scipy.signal.resample_poly``'s filter and
        output) before the int16 conversion, packing and silences.  A rate whose reduced ratio to the voice's has a term above
        640 raises and leaves the setting as it was."""
        self._check(self.native.lib.mi355vits_set_output_rate(self._h, int(hz or 0)))

    @property
    def output_rate(self) -> int:
        """The effective rate of the next run's results: the voice's own when none is set."""
        return int(self.native.lib.mi355vits_get_output_rate(self._h))

    @property
    def last_rate(self) -> int:
        """The rate the last completed run of this handle ran at: what ``fetch`` / ``fetch_packed`` / ``device_result`` serve."""
        return self._last_rate

    MATH_MODES = {"f32": 0, "bf16x3": 1, "bf16w": 2, "f16x2": 3}

    def set_math(self, mode) -> None:
        """``"f32"`` (f32 MFMA), ``"bf16x3"`` (f32 operands split 3 x bf16, six bf16-MFMA products, f32 accumulate; the
        default), ``"bf16w"`` (bf16-rounded weights x exact activations: reduced precision, BASELINE configs[4]) or ``"f16x2"``
        (experimental, fixed-scale: every kernel of the bf16x3 split — fused MRF stages, WaveNet layers, staged convs, upsamplers —
        with operands as two fp16 terms = 22 significant bits, three products; activations beyond |x| = 4094 clip, a stage with a
        weight |w| >= 7.99 runs as bf16x3; the text encoder / duration predictor as in bf16x3.  See include/mi355vits.h)."""
        self._check(self.native.lib.mi355vits_set_math(self._h, self.MATH_MODES.get(mode, mode)))

    @property
    def math(self) -> str:
        m = int(self.native.lib.mi355vits_get_math(self._h))
        return {v: k for k, v in self.MATH_MODES.items()}.get(m, str(m))

    def clone(self) -> "Engine":
        """Another lane on this engine's device: own stream + workspace, shared weights."""
        return Engine(self)

    def device_result(self) -> Dict[str, object]:
        """Device pointers of the last run's results (``mi355vits_device_result``): ``{"pcm": ptr, "audio": ptr,
        "row_stride": L, "batch": B, "lengths": ptr, "device": d}`` — valid until the next run on this handle."""
        pcm, audio, lens = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        rs, b = ctypes.c_int64(), ctypes.c_int32()
        self._check(self.native.lib.mi355vits_device_result(self._h, ctypes.byref(pcm), ctypes.byref(audio), ctypes.byref(rs),
                                                           ctypes.byref(b), ctypes.byref(lens)))
        return {"pcm": pcm.value, "audio": audio.value, "row_stride": int(rs.value), "batch": int(b.value),
                "lengths": lens.value, "device": self.device}

    def fetch(self, want_float: bool = True, want_pcm16: bool = False) -> Dict[str, np.ndarray]:
        r = Result()
        flags = (WANT_FLOAT if want_float else 0) | (WANT_PCM16 if want_pcm16 else 0)
        self._check(self.native.lib.mi355vits_fetch(self._h, flags, ctypes.byref(r)))
        return self._take(r)

    def fetch_alignment(self, levels: bool = False) -> Alignment:
        """Phoneme timing of the last completed run of this handle (``mi355vits_fetch_alignment``), whatever its flags were, at
        the rate it ran at; ``levels``: also peak and rms of each phoneme's span of the float waveform."""
        r = AlignmentResult()
        self._check(self.native.lib.mi355vits_fetch_alignment(self._h, ALIGN_LEVELS if levels else 0, ctypes.byref(r)))
        try:
            shape = (int(r.batch), int(r.tx_max))
            take = lambda p: np.ctypeslib.as_array(p, shape=shape).copy() if p else None  # noqa: E731
            return Alignment(take(r.frames), take(r.start), take(r.samples), take(r.peak), take(r.rms), int(r.sample_rate))
        finally:
            self.native.lib.mi355vits_free_alignment(ctypes.byref(r))

    def _take(self, r: Result) -> Dict[str, np.ndarray]:
        """Result struct -> numpy.  The waveform arrays are *views of the callee's pinned buffers* that own them: the
        buffers go back to the library (``mi355vits_free_result`` -> pinned pool) when the last array referring to
        them is garbage-collected.  No host-side copy of the audio, no aliasing between calls (a buffer is handed out
        exclusively until released) — "a new ndarray owned by Python", as ``onnx_model.run`` returns."""
        B, L = r.batch, r.l_max
        try:
            out: Dict[str, np.ndarray] = {
                "lengths": np.ctypeslib.as_array(r.lengths, shape=(B,)).copy(),
                "peaks": np.ctypeslib.as_array(r.peaks, shape=(B,)).copy(),
                "l_max": np.int64(L), "ty_max": np.int64(r.ty_max),
            }
        except BaseException:
            self.native.lib.mi355vits_free_result(ctypes.byref(r))
            raise
        if not r.audio and not r.pcm:
            self.native.lib.mi355vits_free_result(ctypes.byref(r))
            return out
        holder = _ResultHolder(self.native, r)
        if r.audio:
            out["audio"] = holder.view(r.audio, ctypes.c_float, np.float32, B, L)
        if r.pcm:
            out["pcm"] = holder.view(r.pcm, ctypes.c_int16, np.int16, B, L)
        return out

    # ---- profiling / debugging ------------------------------------------------------------------
    def last_run_ms(self) -> float:
        return float(self.native.lib.mi355vits_last_run_ms(self._h))

    def probe_weights(self) -> dict:
        """L2 stream over this replica's own weight arena (include/mi355vits_lab.h mi355vits_probe_weights; the handle must come
        from a library that carries the hooks): GB/s min / median / max over 2.6 MB windows, eight loads in flight per lane and one."""
        self.native._need_hooks()
        out = (ctypes.c_double * 8)()
        self._check(self.native.lib.mi355vits_probe_weights(self._h, out))
        return {"arena_stream8_GBps": [round(out[0]), round(out[1]), round(out[2])], "arena_stream1_GBps": [round(out[3]), round(out[4]), round(out[5])],
                "windows": int(out[6]), "arena_addr_low36": hex(int(out[7]))}

    def fill_workspace(self, pattern: int) -> None:
        """Fill both workspace arenas of this handle with a 32-bit pattern (include/mi355vits_lab.h mi355vits_test_fill_workspace; the
        handle must come from a library that carries the hooks).  A later run that does not outgrow the workspace keeps it."""
        self.native._need_hooks()
        self._check(self.native.lib.mi355vits_test_fill_workspace(self._h, ctypes.c_uint32(pattern & 0xFFFFFFFF)))

    def profile_enable(self, on: bool = True) -> None:
        self._check(self.native.lib.mi355vits_profile_enable(self._h, int(on)))

    def profile_reset(self) -> None:
        self._check(self.native.lib.mi355vits_profile_reset(self._h))

    def profile_report(self) -> Dict[str, Dict[str, float]]:
        buf = ctypes.create_string_buffer(1 << 16)
        n = self.native.lib.mi355vits_profile_report(self._h, buf, len(buf))
        if n < 0:
            self._check(int(n))
        rep = {}
        for line in buf.value.decode().splitlines():
            name, calls, ms, flops, nbytes = line.split()
            rep[name] = {"calls": int(calls), "ms": float(ms), "flops": float(flops), "bytes": float(nbytes)}
        return rep

    def taps(self):
        buf = ctypes.create_string_buffer(1 << 14)
        self.native.lib.mi355vits_list_taps(self._h, buf, len(buf))
        return [t for t in buf.value.decode().splitlines() if t]

    def tap(self, name: str, row0: int = 0, nrows: int = -1) -> np.ndarray:
        """The named intermediate of the last ``debug_taps`` run as [B, C, T]; ``row0`` / ``nrows``: those batch rows only."""
        dims = (ctypes.c_int64 * 4)()
        L = self.native.lib
        if nrows < 0:
            get = lambda out, cap: L.mi355vits_get_tap(self._h, name.encode(), out, cap, dims)  # noqa: E731
        else:
            get = lambda out, cap: L.mi355vits_get_tap_rows(self._h, name.encode(), row0, nrows, out, cap, dims)  # noqa: E731
        n = get(None, 0)
        if n < 0:
            self._check(int(n))
        out = np.empty(int(n), np.float32)
        n2 = get(_fptr(out), out.size)
        if n2 < 0:
            self._check(int(n2))
        shape = [int(d) for d in dims][:3]  # taps are [B, C, T]
        return out.reshape(shape)
