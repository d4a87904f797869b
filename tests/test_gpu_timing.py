"""Device twin of tests/test_timing.py (pytest -m gpu): mi355vits_run_timed and k_durations_timed on the MI355X.  The same checks
against the same yardstick (tests/timing_ref.py applied to the dur_float tap of the run itself), bit for bit, and once a batch of 64
rows of 128 phonemes of the released voice's shape with random targets."""
import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from tests import timing_ref as TR
from tests.test_timing import (FIT_T, SCALES, SEED, check_errors, check_fit, check_fit_is_k_durations, check_fit_stage,
                               check_fit_stage_long, check_identity, check_output_forms, check_rows_alone, check_stretch_and_min, feed, voice)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T", FIT_T)
def test_fit_stage_alone(gpu_hooks, T):
    check_fit_stage(gpu_hooks, T)


@pytest.mark.parametrize("T", [16384, 16385])
def test_fit_stage_alone_at_the_lds_limit(gpu_hooks, T):
    check_fit_stage_long(gpu_hooks, T)


def test_fit_stage_without_a_target_is_k_durations(gpu_hooks):
    check_fit_is_k_durations(gpu_hooks)


@pytest.mark.parametrize("kind", ["sdp", "det", "ms"])
def test_identity_fit_replay_and_rows_alone(gpu_lib, kind):
    cfg, blob = voice(kind)
    eng = Engine(blob, device=0, library=gpu_lib)
    a = feed(cfg)
    check_identity(eng, a)
    target, frames, out = check_fit(eng, a)
    check_rows_alone(lambda: Engine(blob, device=0, library=gpu_lib), a, target, out, [0, 1, 4] if kind == "sdp" else [3])
    eng.close()


@pytest.mark.parametrize("kind", ["sdp", "det"])
def test_output_forms_stretch_and_minimum_frames(gpu_lib, kind):
    cfg, blob = voice(kind)
    eng = Engine(blob, device=0, library=gpu_lib)
    a = feed(cfg)
    target, frames, _ = check_fit(eng, a)
    check_output_forms(eng, a, target, frames)
    check_stretch_and_min(eng, a)
    eng.close()


def test_errors(gpu_lib):
    cfg, blob = voice("sdp")
    eng = Engine(blob, device=0, library=gpu_lib)
    check_errors(eng, feed(cfg))
    eng.close()


def test_a_batch_of_64_rows_of_128_phonemes(gpu_lib):
    """B = 64 x Tx = 128, the released single-speaker voice's shape, random targets in [floor, 3 F(1)]: the integers equal the
    yardstick applied to the tap, and four rows of the batch are bitwise the rows alone."""
    cfg = VitsConfig.apope_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=151, frames_per_id=3.0))
    rng = np.random.default_rng(64)
    B, Tx = 64, 128
    lens = rng.integers(1, Tx + 1, B).astype(np.int64)
    lens[0], lens[1] = Tx, 1
    ids = rng.integers(1, cfg.num_symbols, (B, Tx)).astype(np.int64)
    keys = [int(k) for k in rng.integers(0, 1 << 40, B)]
    kw = dict(seed=SEED, utterance_keys=keys, want_float=True, want_pcm16=False)
    eng = Engine(blob, device=0, library=gpu_lib)
    eng.run(ids, lens, SCALES, None, stretch=np.ones((B, Tx), np.float32), debug_taps=True, **kw)
    u = eng.tap("dur_float")[:, 0, :]
    target = np.array([rng.integers(TR.floor_of(u[b], lens[b]), 3 * TR.natural(u[b], lens[b]) + 1) for b in range(B)], np.int32)
    out = eng.run(ids, lens, SCALES, None, target_frames=target, debug_taps=True, **kw)
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}
    assert eng.tap("dur_float")[:, 0, :].tobytes() == u.tobytes()
    frames, _, ylen, factor, status = TR.fit(u, lens, None, target)
    assert not status.any()
    al = eng.fetch_alignment()
    assert al.frames.tobytes() == frames.tobytes() and np.array_equal(al.frames.sum(axis=1), target)
    assert out["timing_factor"].tobytes() == factor.tobytes()
    assert np.array_equal(out["lengths"], target.astype(np.int64) * cfg.hop_length)
    for b in (0, 1, 31, 63):
        one = eng.run(ids[b:b + 1], lens[b:b + 1], SCALES, None, target_frames=target[b:b + 1], seed=SEED, utterance_keys=keys[b:b + 1],
                      want_float=True)
        n = int(out["lengths"][b])
        assert int(one["lengths"][0]) == n and one["audio"][0, :n].tobytes() == out["audio"][b, :n].tobytes()
        assert one["timing_factor"].tobytes() == out["timing_factor"][b:b + 1].tobytes()
    eng.close()
