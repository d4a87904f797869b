"""Device twin of tests/test_edge_trim.py (pytest -m gpu): mi355vits_set_edge_trim / mi355vits_fetch_edges and k_edges on the
MI355X — 36 ragged rows of 1 .. 96 ids of the released single-speaker voice's shape (synthetic weights, frames_per_id = 3.0: the
`_ragged` shape of test_gpu_resample.py), 6 rows of up to 40 ids where a test repeats runs, the kernel alone through the hook, a
NaN-filled workspace.  The same yardstick as the CPU file: numpy on the WANT_FLOAT audio and the peaks of the same run, bit for bit.

Not tested here either: a size limit that only the untrimmed stream exceeds (no hook forces small limits)."""
import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests.test_edge_trim import (NAN, RATES, check_errors, check_kernel_alone, check_nothing_else_moves, check_off_is_off,
                                  check_rows_alone, check_session, check_trimmed_streams, same_stream, trimmed_batch)
from tests.test_gpu_resample import B, _ragged
from tests.test_resample import run_at

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voice():
    cfg = VitsConfig.apope_low()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=151, frames_per_id=3.0))


def test_the_kernel_alone(gpu_hooks):
    """Criterion 1 on the device."""
    check_kernel_alone(gpu_hooks)


def test_off_is_off(gpu_lib, voice):
    """Criterion 2 on the device."""
    cfg, blob = voice
    check_off_is_off(lambda: Engine(blob, device=0, library=gpu_lib), _ragged(cfg, 17, B=6, hi=40))


@pytest.mark.parametrize("rate", RATES)
def test_trimmed_streams(gpu_lib, voice, rate):
    """Criterion 3: 36 ragged rows, a permuted order of all of them.  This fails without the feature."""
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_lib)
    check_trimmed_streams(eng, _ragged(cfg, 151), rate, [int(i) for i in np.random.default_rng(5).permutation(B)])
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_batched_is_alone_and_on_a_nan_filled_workspace(gpu_hooks, voice, rate):
    """Criterion 4: rows of the batch give alone the first / end and entry bytes they give in the batch; the same bytes on a
    workspace a larger call sized and a quiet NaN filled."""
    cfg, blob = voice
    a = _ragged(cfg, 131)
    eng = Engine(blob, device=0, library=gpu_hooks)
    want = trimmed_batch(eng, a, rate)
    check_rows_alone(lambda: Engine(blob, device=0, library=gpu_hooks), a, rate, [0, 1, B // 2, B - 1, 7], want)
    rng = np.random.default_rng(3)
    big = dict(ids=rng.integers(1, cfg.num_symbols, (B + 4, 96)), lens=np.full(B + 4, 96), sid=None, scales=[0.667, 1.0, 0.8],
               kw=dict(seed=1, forced_durations=np.full((B + 4, 96), 8, np.int32)))
    assert int(run_at(eng, rate, big)["l_max"]) > int(np.max(want.end))  # sizes the workspace past what the ragged call needs
    eng.set_edge_trim(0.9, 5)
    eng.fetch_packed()  # and the edges' and the pack's own arenas
    eng.fill_workspace(NAN)
    got = trimmed_batch(eng, a, rate)
    same_stream(got, want)
    assert np.array_equal(got.first, want.first) and np.array_equal(got.end, want.end)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_nothing_else_moves(gpu_lib, voice, rate):
    """Criterion 5 on the device."""
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_lib)
    check_nothing_else_moves(eng, _ragged(cfg, 17, B=6, hi=40), rate)
    eng.close()


def test_errors(gpu_lib, voice):
    """Criterion 7 on the device."""
    cfg, blob = voice
    check_errors(lambda: Engine(blob, device=0, library=gpu_lib), _ragged(cfg, 5, B=4, hi=24))


def test_session_trim_and_alignment_in_a_trimmed_stream(gpu_lib, voice):
    """Criterion 6 on the device (the routing is host code: tests/test_edge_trim.py)."""
    cfg, blob = voice
    opts = SessionOptions()
    opts.seed = 5
    sess = InferenceSession(blob, opts, _library=gpu_lib)
    check_session(sess, _ragged(cfg, 23, B=3, hi=20), rate=8000)
    sess.close()
