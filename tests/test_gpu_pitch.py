"""Device twin of tests/test_pitch.py (pytest -m gpu): mi355vits_run_pitch, k_pitch_plan and k_pitch on the MI355X.  The same checks
against the same yardstick (tests/pitch_ref.py), bit for bit, and once the kernel at the released voice's shape: 64 rows, hop 256,
128 phonemes of 0 .. 12 frames, a third of them moved."""
import numpy as np
import pytest

from mimic3_amd._native import Engine
from mimic3_amd.session import InferenceSession, SessionOptions
from tests.test_pitch import (RATIOS, SEED, check_dense_boundaries, check_downstream, check_duration_kept, check_errors, check_far_samples_keep_their_bits,
                              check_identity, check_plan, check_rows_alone_alignment_and_replay, check_rule, check_session,
                              check_small_spans_and_degenerate_rows, check_table, check_tile_edges, check_unit_impulse, check_unity,
                              check_zero_frame_phonemes_change_nothing, feed, pitch_inputs, row, run_kernel, voice)

pytestmark = pytest.mark.gpu


def test_table_is_the_closed_form(gpu_hooks):
    check_table(gpu_hooks)


def test_kernel_tile_edges(gpu_hooks):
    check_tile_edges(gpu_hooks)


def test_kernel_small_spans_and_degenerate_rows(gpu_hooks):
    check_small_spans_and_degenerate_rows(gpu_hooks)
    check_zero_frame_phonemes_change_nothing(gpu_hooks)


def test_kernel_unity_and_far_samples(gpu_hooks):
    check_unity(gpu_hooks)
    check_far_samples_keep_their_bits(gpu_hooks)


def test_kernel_dense_boundaries(gpu_hooks):
    check_dense_boundaries(gpu_hooks)


def test_kernel_unit_impulse(gpu_hooks):
    check_unit_impulse(gpu_hooks)


def test_plan_kernel(gpu_hooks):
    check_plan(gpu_hooks)


def test_kernel_at_the_released_shape(gpu_hooks):
    rng = np.random.default_rng(90)
    rows = []
    for _ in range(64):
        L = int(rng.integers(1, 129))
        rows.append(row(rng.integers(0, 13, L), np.where(rng.random(L) < 1 / 3, rng.choice(RATIOS, L), 1.0).astype(np.float32)))
    run_kernel(gpu_hooks, rows, 256, 91, alone=(0, 31, 63))


@pytest.mark.parametrize("kind", ["sdp", "det", "ms"])
def test_identity_and_rule(gpu_hooks, kind):
    cfg, blob = voice(kind)
    eng = Engine(blob, device=0, library=gpu_hooks)
    a = feed(cfg)
    check_identity(eng, a)
    check_rule(eng, gpu_hooks, a, pitch_inputs(a))
    eng.close()


def test_rows_alone_alignment_and_replay(gpu_hooks):
    cfg, blob = voice("sdp")
    a = feed(cfg)
    check_rows_alone_alignment_and_replay(lambda: Engine(blob, device=0, library=gpu_hooks), a, pitch_inputs(a))


def test_duration_kept_and_downstream_forms(gpu_lib):
    cfg, blob = voice("sdp")
    eng = Engine(blob, device=0, library=gpu_lib)
    a = feed(cfg)
    check_duration_kept(eng, a)
    check_downstream(eng, a, pitch_inputs(a))
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
