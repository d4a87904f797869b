"""Device twin of tests/test_alignment.py (pytest -m gpu): mi355vits_fetch_alignment and k_align on the MI355X — 36 ragged rows of
1 .. 96 ids of the released single-speaker voice's shape (synthetic weights, frames_per_id = 3.0: the `_ragged` shape of
test_gpu_resample.py), the kernel alone through the hook, a NaN-filled workspace.  Same yardsticks as the CPU file: the w_ceil tap
or the forced durations, the integer formula in Python ints, fp64 numpy over the WANT_FLOAT audio of the same run."""
import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests.test_alignment import (NAN, RATES, aligned_run, check_errors, check_forced_round_trip, check_kernel_alone, check_levels,
                                  check_nothing_else_moves, check_rows_alone, check_timing, ratio_of, same_alignment)
from tests.test_gpu_resample import B, _ragged
from tests.test_resample import run_at

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voice():
    cfg = VitsConfig.apope_low()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=151, frames_per_id=3.0))


def test_timing_and_levels_at_every_rate(gpu_lib, voice):
    """Criteria 1 and 2: native, 8000 Hz (M > L, a non-integer hop L / M) and 48000 Hz (L > M), natural durations."""
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_lib)
    a = _ragged(cfg, 151)
    for rate in RATES:
        out, al = aligned_run(eng, rate, a)
        assert len({int(x) for x in out["lengths"]}) > B // 2
        print(f"alignment at {rate or cfg.sample_rate} Hz: {int(al.samples.sum())} samples in {int((al.samples > 0).sum())} spans, longest {int(al.samples.max())}")
    _, plain = aligned_run(eng, 8000, a, levels=False)
    assert np.array_equal(plain.samples, aligned_run(eng, 8000, a)[1].samples)
    eng.close()


def test_the_kernel_alone(gpu_hooks):
    """Criterion 3 on the device."""
    check_kernel_alone(gpu_hooks)


@pytest.mark.parametrize("rate", [0, 8000])
def test_batched_is_alone_and_on_a_nan_filled_workspace(gpu_hooks, voice, rate):
    """Criterion 4: rows of the batch bitwise the rows alone; the same bytes on a workspace a larger call sized and a quiet NaN filled."""
    cfg, blob = voice
    a = _ragged(cfg, 131)
    eng = Engine(blob, device=0, library=gpu_hooks)
    _, want = aligned_run(eng, rate, a)
    check_rows_alone(lambda: Engine(blob, device=0, library=gpu_hooks), a, rate, want, [0, 1, B // 2, B - 1, 7])
    rng = np.random.default_rng(3)
    big = dict(ids=rng.integers(1, cfg.num_symbols, (B + 4, 96)), lens=np.full(B + 4, 96), sid=None, scales=[0.667, 1.0, 0.8],
               kw=dict(seed=1, forced_durations=np.full((B + 4, 96), 8, np.int32)))
    assert int(run_at(eng, rate, big)["l_max"]) > int(np.max(want.samples.sum(axis=1)))  # sizes the workspace past what the ragged call needs
    eng.fetch_alignment(levels=True)  # and the alignment's own arena
    eng.fill_workspace(NAN)
    _, got = aligned_run(eng, rate, a)
    same_alignment(got, want)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_nothing_else_moves(gpu_lib, voice, rate):
    """Criterion 5 on the device."""
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_lib)
    check_nothing_else_moves(eng, _ragged(cfg, 17, B=6, hi=40), rate)
    eng.close()


def test_forced_durations_round_trip_and_zero_frames(gpu_lib, voice):
    """Criterion 6, and forced values with zero-frame phonemes and a row of zero frames at the three rates."""
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_lib)
    a = _ragged(cfg, 19, B=6, hi=40)
    for rate in (0, 48000):
        check_forced_round_trip(eng, a, rate)
    forced = np.random.default_rng(19).integers(0, 6, a["ids"].shape).astype(np.int32)
    forced[:, 3] = 0
    forced[2] = 0
    forced[0, 5] = 90  # 23,040 native samples: 360 passes of a wave
    a["kw"]["forced_durations"] = forced
    for rate in RATES:
        out = run_at(eng, rate, a)
        al = eng.fetch_alignment(levels=True)
        L, M = ratio_of(eng, rate)
        st, sm = check_timing(al, forced, a["lens"], out["lengths"], cfg.hop_length, L, M, rate or cfg.sample_rate)
        check_levels(al, out["audio"], out["peaks"], st, sm)
    eng.close()


def test_errors(gpu_lib, voice):
    """Criterion 7 on the device."""
    cfg, blob = voice
    check_errors(lambda: Engine(blob, device=0, library=gpu_lib), _ragged(cfg, 5, B=4, hi=24))


def test_session_alignment_on_the_device(gpu_lib, voice):
    """Criterion 8 on the device (the routing is host code: tests/test_alignment.py): run_pcm16 and run_packed with alignment."""
    cfg, blob = voice
    opts = SessionOptions()
    opts.seed = 5
    sess = InferenceSession(blob, opts, _library=gpu_lib)
    a = _ragged(cfg, 23, B=3, hi=20)
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    rows, lengths, al = sess.run_pcm16(feed, alignment="levels", utterance_keys=[1, 2, 3], sample_rate=8000)
    assert al.sample_rate == 8000 and [int(x) for x in al.samples.sum(axis=1)] == [int(n) for n in lengths] == [r.size for r in rows]
    pk = sess.run_packed(feed, order=[2, 0], lead_ms=[30.0, 12.5], sample_rate=8000, encoding="ulaw", alignment=True, utterance_keys=[1, 2, 3])
    for i, b in enumerate((2, 0)):
        assert np.array_equal(pk.alignment.start[i], al.start[b].astype(np.int64) + int(pk.offsets[i]))
        assert int(pk.alignment.start[i, -1] + pk.alignment.samples[i, -1]) == int(pk.offsets[i] + pk.lengths[i])
    sess.close()
