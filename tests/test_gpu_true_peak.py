"""Device twin of tests/test_true_peak.py (pytest -m gpu): mi355vits_set_loudness_ceiling_mode / mi355vits_fetch_true_peak,
k_true_peak, k_true_peak_env and k_limit<true> on the MI355X — the constructed rows through the hooks, ragged rows of the released
single-speaker voice's shape (synthetic weights, frames_per_id = 3.0: the `_ragged` shape of test_gpu_resample.py) through the
product and the hooks library, a NaN-filled workspace.  The same yardstick and the same exact comparisons as the CPU file:
tests/true_peak_ref.py on the WANT_FLOAT audio of the same run."""
import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests.test_gpu_resample import _ragged
from tests.test_limiter import check_rows_alone, limited_batch, same_batch
from tests.test_loudness import NAN
from tests.test_resample import run_at
from tests.test_true_peak import (check_errors, check_kernel_alone, check_limiter_with_envelope, check_micro_batcher_keeps_modes_apart,
                                  check_off_is_off, check_packs, check_streams, library_taps, true_peak_setting)

pytestmark = pytest.mark.gpu
B = 12
WINDOW = 110  # 5 ms at the voice's 22,050 Hz
SEED = 151    # the ragged batch with rows over in true-peak mode only, in both modes and in neither at both rates (asserted by check_packs)


@pytest.fixture(scope="module")
def voice():
    cfg = VitsConfig.apope_low()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=151, frames_per_id=3.0))


def true_peak_engine(blob, lib):
    eng = Engine(blob, device=0, library=lib)
    eng.set_loudness_ceiling_mode("true_peak")
    return eng


def test_the_kernel_alone(gpu_hooks):
    """This fails without the feature."""
    check_kernel_alone(gpu_hooks)


def test_limiter_with_an_envelope(gpu_hooks):
    """This fails without the feature."""
    check_limiter_with_envelope(gpu_hooks)


@pytest.mark.parametrize("rate", [0, 8000])
def test_packs(gpu_hooks, voice, rate):
    """Ragged rows, a permuted order of all of them.  This fails without the feature."""
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_hooks)
    check_packs(eng, _ragged(cfg, SEED, B=B, hi=60), rate, [int(i) for i in np.random.default_rng(5).permutation(B)],
                library_taps(gpu_hooks), L=WINDOW)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_batched_is_alone_and_on_a_nan_filled_workspace(gpu_hooks, voice, rate):
    cfg, blob = voice
    a = _ragged(cfg, SEED, B=B, hi=60)
    eng = true_peak_engine(blob, gpu_hooks)
    target, ceiling = true_peak_setting(run_at(eng, rate, a), rate or cfg.sample_rate, library_taps(gpu_hooks))
    want = limited_batch(eng, a, rate, target, ceiling, WINDOW)
    assert want[1].engaged.any() and not want[1].engaged.all()
    over, rest = np.nonzero(want[1].engaged)[0], np.nonzero(~want[1].engaged)[0]
    check_rows_alone(lambda: true_peak_engine(blob, gpu_hooks), a, rate, [int(over[0]), int(over[-1]), int(rest[0])], want[0], want[1],
                     target, ceiling, WINDOW)
    rng = np.random.default_rng(3)
    big = dict(ids=rng.integers(1, cfg.num_symbols, (B + 4, 64)), lens=np.full(B + 4, 64), sid=None, scales=[0.667, 1.0, 0.8],
               kw=dict(seed=1, forced_durations=np.full((B + 4, 64), 8, np.int32)))
    assert int(run_at(eng, rate, big)["l_max"]) > int(np.max(want[0]["s16le"].lengths))  # sizes the workspace past what the ragged call needs
    limited_batch(eng, big, rate, -3.0, -6.0, WINDOW)  # and the measurement's, the limiter's and the pack's own arenas
    eng.fill_workspace(NAN)
    same_batch(limited_batch(eng, a, rate, target, ceiling, WINDOW), want)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_streams(gpu_hooks, voice, rate):
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_hooks)
    check_streams(eng, _ragged(cfg, SEED, B=B, hi=60), rate, library_taps(gpu_hooks), L=WINDOW)
    eng.close()


def test_off_is_off(gpu_hooks, voice):
    cfg, blob = voice
    check_off_is_off(lambda: Engine(blob, device=0, library=gpu_hooks), _ragged(cfg, SEED, B=B, hi=60), 8000, library_taps(gpu_hooks), L=WINDOW)


def test_errors(gpu_lib, voice):
    cfg, blob = voice
    check_errors(lambda: Engine(blob, device=0, library=gpu_lib), _ragged(cfg, 5, B=4, hi=24))


def test_session_routing(gpu_lib, gpu_hooks, voice):
    """true_peak= through the session and the micro-batcher on the device (host code: tests/test_true_peak.py)."""
    cfg, blob = voice
    opts = SessionOptions()
    opts.seed = 5
    opts.micro_batch_window_ms = 5.0
    opts.micro_batch_max = 16
    sess = InferenceSession(blob, opts, _library=gpu_lib)
    check_micro_batcher_keeps_modes_apart(sess, _ragged(cfg, 23, B=3, hi=20), library_taps(gpu_hooks), rate=8000)
    sess.close()
