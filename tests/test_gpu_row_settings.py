"""Per-row synthesis settings (mi355vits_run_rows) on the MI355X: every row of a mixed batch is bitwise its own call with
scalar settings and utterance_base = its key (pytest -m gpu).  tests/test_row_settings.py checks the same on the CPU model."""
import threading

import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from oracle.vits_oracle import VitsOracle
from tests.util import TIGHT_REL_RMS_TOL, rel_rms

pytestmark = pytest.mark.gpu

SEED = 0x5EED5
# eight settings triples: noise on all but the two deterministic ones, length_scale 0.7 .. 1.6
SETTINGS = np.array([[0.667, 1.0, 0.8], [0.5, 0.8, 0.8], [0.0, 1.2, 0.0], [0.667, 1.5, 0.3], [0.9, 0.7, 1.0],
                     [0.333, 1.6, 0.0], [0.0, 0.9, 0.0], [0.6, 1.1, 0.6]], np.float32)
VOLUMES = np.array([1.0, 0.5, 1.5, 3.0, 0.075, 1.0, 2.0, 0.8])


def _batch(cfg, B, lo, hi, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=B).astype(np.int64)
    lens[0] = hi
    ids = np.zeros((B, hi), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    keys = [int(k) for k in rng.permutation(10 * B)[:B] * 7919 + 13]  # distinct, non-consecutive, out of order
    which = np.arange(B) % len(SETTINGS)
    sid = (rng.integers(0, cfg.n_speakers, size=B)).astype(np.int64) if cfg.is_multispeaker else None
    return ids, lens, keys, which, sid


def _check_rows(eng, ids, lens, keys, which, sid, rows):
    """The mixed batch, then each row in `rows` alone (padded to the batch's length: the same encoder length class)."""
    full = eng.run(ids, lens, SETTINGS[which], sid, seed=SEED, utterance_keys=keys, pcm_volume=VOLUMES[which], want_pcm16=True)
    for b in rows:
        one = eng.run(ids[b:b + 1], lens[b:b + 1], SETTINGS[which[b]], None if sid is None else sid[b:b + 1], seed=SEED,
                      utterance_base=keys[b], pcm_volume=float(VOLUMES[which[b]]), want_pcm16=True)
        L = int(one["lengths"][0])
        assert L == int(full["lengths"][b]), b
        assert np.array_equal(one["audio"][0, :L], full["audio"][b, :L]), b
        assert np.array_equal(one["pcm"][0, :L], full["pcm"][b, :L]), b
        assert one["peaks"][0].tobytes() == full["peaks"][b].tobytes(), b
    return full


@pytest.mark.parametrize("math", [None, "f32"])
def test_apope_low_mixed_batch_rows_are_their_solo_runs(gpu_lib, math):
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=61, frames_per_id=3.0)), device=0)
    if math:
        eng.set_math(math)
    ids, lens, keys, which, sid = _batch(cfg, 64, 20, 180, seed=61)
    _check_rows(eng, ids, lens, keys, which, sid, range(64))
    eng.close()


def test_vctk_low_mixed_speakers_and_settings(gpu_lib):
    cfg = VitsConfig.vctk_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=62, frames_per_id=2.5)), device=0)
    ids, lens, keys, which, sid = _batch(cfg, 24, 20, 120, seed=62)
    assert len(set(sid.tolist())) > 4
    _check_rows(eng, ids, lens, keys, which, sid, range(24))
    eng.close()


def test_256_row_mixed_batch_spot_rows_and_oracle(gpu_lib):
    cfg = VitsConfig.apope_low()
    w = W.synthetic_weights(cfg, seed=63, frames_per_id=3.0)
    eng = Engine(W.pack(cfg, w), device=0)
    ids, lens, keys, which, sid = _batch(cfg, 256, 20, 120, seed=63)
    spot = sorted(set(np.random.default_rng(63).choice(256, 14, replace=False).tolist()) | {0, 255})[:16]
    full = _check_rows(eng, ids, lens, keys, which, sid, spot)
    det = [b for b in range(256) if SETTINGS[which[b], 0] == 0 and SETTINGS[which[b], 2] == 0][:2]
    ora = VitsOracle(cfg, w)
    for b in det:
        n = int(lens[b])
        ref = ora.infer(ids[b:b + 1, :n], np.array([n]), SETTINGS[which[b]])
        L = int(full["lengths"][b])
        assert L == int(ref["audio_lengths"][0])
        assert rel_rms(full["audio"][b, :L], ref["audio"][0, 0, :L]) < TIGHT_REL_RMS_TOL
    eng.close()


def test_micro_batcher_merges_mixed_settings_on_the_device(gpu_lib):
    cfg = VitsConfig.apope_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=64, frames_per_id=3.0))
    plain = InferenceSession(blob)
    so = SessionOptions()
    so.micro_batch_window_ms = 200.0
    so.micro_batch_max = 16
    mb = InferenceSession(blob, sess_options=so)
    rng = np.random.default_rng(64)
    settings = [(np.array([0.0, ls, 0.0], np.float32), vol) for ls in (0.8, 1.0, 1.2, 1.5) for vol in (50.0, 100.0, 150.0)]
    feeds = []
    for k in range(12):
        n = int(rng.integers(30, 120))
        feeds.append({"input": rng.integers(1, cfg.num_symbols, (1, n)).astype(np.int64),
                      "input_lengths": np.array([n], np.int64), "scales": settings[k][0]})
    expect = [plain.run_pcm16(feeds[k], volume=settings[k][1])[0][0].copy() for k in range(12)]
    got = [None] * 12
    errs = []
    gate = threading.Barrier(12)

    def client(k):
        try:
            gate.wait()
            got[k] = mb.run_pcm16(feeds[k], volume=settings[k][1])[0][0].copy()
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)

    ts = [threading.Thread(target=client, args=(k,)) for k in range(12)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for k in range(12):
        assert np.array_equal(got[k], expect[k]), k
    assert mb._batcher.requests == 12 and mb._batcher.batches < len(settings), mb._batcher.batches
    mb.close()
    plain.close()
