"""Device twin of tests/test_levels.py (pytest -m gpu): mi355vits_run_levels and k_levels on the MI355X.  The same checks against
the same yardstick (tests/levels_ref.py), bit for bit, and once the kernel at the released voice's shape: 64 rows, hop 256, 128
phonemes of 0 .. 12 frames."""
import pytest

from mimic3_amd._native import Engine
from mimic3_amd.session import InferenceSession, SessionOptions
from tests.test_levels import (RAMPS, SEED, check_combinations, check_degenerate_rows, check_dense_boundaries, check_downstream, check_errors,
                               check_identity, check_output_rate, check_ramps, check_rows_alone_and_poison, check_rule, check_session,
                               check_special_gains, check_tile_edges, check_unity, check_zero_frame_phonemes, feed, level_inputs,
                               released_shape_rows, run_kernel, voice)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R", RAMPS)
def test_kernel_tile_edges(gpu_hooks, R):
    check_tile_edges(gpu_hooks, R)


def test_kernel_ramps_and_short_phonemes(gpu_hooks):
    check_ramps(gpu_hooks)


@pytest.mark.parametrize("R", (0, 300))
def test_kernel_zero_frame_phonemes(gpu_hooks, R):
    check_zero_frame_phonemes(gpu_hooks, R)


def test_kernel_degenerate_rows(gpu_hooks):
    check_degenerate_rows(gpu_hooks)


def test_kernel_dense_boundaries(gpu_hooks):
    check_dense_boundaries(gpu_hooks)


def test_kernel_special_gains_and_unity(gpu_hooks):
    check_special_gains(gpu_hooks)
    check_unity(gpu_hooks)


def test_kernel_at_the_released_shape(gpu_hooks):
    run_kernel(gpu_hooks, released_shape_rows(), 256, 91, alone=(0, 31, 63))


@pytest.mark.parametrize("kind", ["sdp", "det", "ms"])
def test_identity_rule_and_rows_alone(gpu_hooks, kind):
    cfg, blob = voice(kind)
    eng = Engine(blob, device=0, library=gpu_hooks)
    a = feed(cfg)
    g, ramp = level_inputs(a)
    check_identity(eng, a)
    check_rule(eng, a, g, ramp)
    if kind != "det":
        check_rows_alone_and_poison(lambda: Engine(blob, device=0, library=gpu_hooks), a, g, ramp)
    eng.close()


@pytest.mark.parametrize("kind", ["sdp", "ms"])
def test_levels_with_timing_forced_durations_and_speakers(gpu_lib, kind):
    cfg, blob = voice(kind)
    eng = Engine(blob, device=0, library=gpu_lib)
    a = feed(cfg)
    check_combinations(eng, a, *level_inputs(a), multispeaker=kind == "ms")
    eng.close()


def test_output_rate_and_downstream_forms(gpu_lib, gpu_hooks):
    cfg, blob = voice("sdp")
    eng = Engine(blob, device=0, library=gpu_lib)
    a = feed(cfg)
    g, ramp = level_inputs(a)
    check_output_rate(eng, gpu_hooks, a, g, ramp)
    check_downstream(eng, a, g, ramp)
    eng.close()


def test_errors(gpu_lib):
    cfg, blob = voice("sdp")
    eng = Engine(blob, device=0, library=gpu_lib)
    check_errors(eng, feed(cfg))
    eng.close()


def test_session_keywords(gpu_lib):
    cfg, blob = voice("sdp")
    eng = Engine(blob, device=0, library=gpu_lib)
    so = SessionOptions()
    so.seed = SEED
    so.micro_batch_window_ms = 200.0
    sess = InferenceSession(blob, sess_options=so)
    check_session(sess, eng, cfg)
    sess.close()
    eng.close()
