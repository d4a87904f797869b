"""Device twin of tests/test_loudness.py (pytest -m gpu): mi355vits_set_loudness_target / mi355vits_fetch_loudness and k_loud /
k_loud_gate on the MI355X — 36 ragged rows of 1 .. 96 ids of the released single-speaker voice's shape (synthetic weights,
frames_per_id = 3.0: the `_ragged` shape of test_gpu_resample.py), 6 rows of up to 40 ids where a test repeats runs, the kernels alone
through the hook, a NaN-filled workspace.  The same yardstick and the same tolerances as the CPU file: tests/loudness_ref.py on the
WANT_FLOAT audio and the peaks of the same run."""
import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests.test_gpu_resample import B, _ragged
from tests.test_loudness import (NAN, RATES, check_calibration, check_errors, check_kernel_alone, check_kernel_is_address_independent,
                                 check_normalised_streams, check_nothing_else_moves, check_off_is_off, check_rows_alone, check_session,
                                 normalised_batch, same_stream)
from tests.test_resample import run_at

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voice():
    cfg = VitsConfig.apope_low()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=151, frames_per_id=3.0))


def test_the_kernels_alone(gpu_hooks):
    """Criterion 1 on the device.  This fails without the feature."""
    check_kernel_alone(gpu_hooks)
    check_kernel_is_address_independent(gpu_hooks)


def test_calibration(gpu_hooks):
    """Criterion 2 on the device."""
    check_calibration(gpu_hooks)


def test_off_is_off(gpu_lib, voice):
    """Criterion 3 on the device."""
    cfg, blob = voice
    check_off_is_off(lambda: Engine(blob, device=0, library=gpu_lib), _ragged(cfg, 17, B=6, hi=40))


@pytest.mark.parametrize("rate", RATES)
def test_normalised_streams(gpu_lib, voice, rate):
    """Criterion 4: 36 ragged rows, a permuted order of all of them.  This fails without the feature.  At (-10, -6) all 36 rows of
    this voice are limited (check_normalised_streams says why and by how much); the setting with rows on both sides of the ceiling is
    the derived third one."""
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_lib)
    check_normalised_streams(eng, _ragged(cfg, 151), rate, [int(i) for i in np.random.default_rng(5).permutation(B)],
                             both_at_minus_10=False)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_batched_is_alone_and_on_a_nan_filled_workspace(gpu_hooks, voice, rate):
    """Criterion 5: rows of the batch give alone the lufs bits and entry bytes they give in the batch; the same on a workspace a
    larger call sized and a quiet NaN filled."""
    cfg, blob = voice
    a = _ragged(cfg, 131)
    eng = Engine(blob, device=0, library=gpu_hooks)
    want = normalised_batch(eng, a, rate)
    check_rows_alone(lambda: Engine(blob, device=0, library=gpu_hooks), a, rate, [0, 1, B // 2, B - 1, 7], want)
    rng = np.random.default_rng(3)
    big = dict(ids=rng.integers(1, cfg.num_symbols, (B + 4, 96)), lens=np.full(B + 4, 96), sid=None, scales=[0.667, 1.0, 0.8],
               kw=dict(seed=1, forced_durations=np.full((B + 4, 96), 8, np.int32)))
    assert int(run_at(eng, rate, big)["l_max"]) > int(np.max(want.lengths))  # sizes the workspace past what the ragged call needs
    eng.set_loudness_target(-23.0, -1.0)
    eng.fetch_packed()  # and the measurement's and the pack's own arenas
    eng.fill_workspace(NAN)
    got = normalised_batch(eng, a, rate)
    same_stream(got, want)
    assert got.lufs.tobytes() == want.lufs.tobytes()
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_nothing_else_moves(gpu_lib, voice, rate):
    """Criterion 6 on the device."""
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_lib)
    check_nothing_else_moves(eng, _ragged(cfg, 17, B=6, hi=40), rate)
    eng.close()


def test_errors(gpu_lib, voice):
    """Criterion 7 on the device."""
    cfg, blob = voice
    check_errors(lambda: Engine(blob, device=0, library=gpu_lib), _ragged(cfg, 5, B=4, hi=24))


def test_session_routing(gpu_lib, voice):
    """Criterion 7's routing on the device (it is host code: tests/test_loudness.py)."""
    cfg, blob = voice
    opts = SessionOptions()
    opts.seed = 5
    sess = InferenceSession(blob, opts, _library=gpu_lib)
    check_session(sess, _ragged(cfg, 23, B=3, hi=20), rate=8000)
    sess.close()
