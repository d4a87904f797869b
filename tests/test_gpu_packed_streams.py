"""Device twin of tests/test_packed_streams.py (pytest -m gpu): mi355vits_run_streams / mi355vits_fetch_streams and k_pack_streams
on the MI355X at sizes a user runs, and InferenceSession.run_stream through the micro-batcher.  The yardstick is the device's own
single-stream path — ``fetch_packed`` under the setters, the padded int16 rows of ``fetch``, ``run_packed`` of a session —, bitwise."""
import threading

import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests.test_packed_streams import LOUD, TRIM, check_against_twins, twin

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE
ENCODINGS = ("s16le", "ulaw", "alaw", "f32le")


def _ragged(cfg, B, lo, hi, seed):
    """B ragged rows of lo .. hi ids with per-row scales (noise on), volumes (3.0 clips) and keys."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, B).astype(np.int64)
    lens[0], lens[B // 2] = hi, lo
    ids = np.zeros((B, hi), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    sid = (np.arange(B) % cfg.n_speakers).astype(np.int64) if cfg.is_multispeaker else None
    scales = np.stack([rng.uniform(0.3, 0.9, B), rng.uniform(0.8, 1.3, B), rng.uniform(0.2, 1.0, B)], axis=1).astype(np.float32)
    vol = rng.choice([0.5, 1.0, 1.5, 3.0, 0.075], B)
    keys = [int(k) for k in rng.integers(0, 1 << 40, B)]
    return ids, lens, sid, scales, vol, keys


@pytest.fixture(scope="module")
def voice():
    cfg = VitsConfig.apope_low()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=151, frames_per_id=3.0))


def _twelve(groups):
    """12 streams of 4 rows, cycling the four encodings; half with headers, every third trimmed, every fourth normalised."""
    rng = np.random.default_rng(12)
    streams = []
    for s, rows in enumerate(groups):
        st = dict(order=[int(r) for r in rows], lead_samples=[int(x) for x in rng.integers(0, 3000, len(rows))], tail_samples=int(rng.integers(0, 500)),
                  wav=bool(s % 2), encoding=ENCODINGS[s % 4])
        if s % 3 == 0:
            st["trim"] = TRIM if s % 2 else (0.25, 3)  # two distinct ratios in one call
        if s % 4 == 0:
            st["loudness"] = LOUD
        streams.append(st)
    return streams


@pytest.mark.parametrize("rate", [None, 8000])
def test_48_ragged_rows_as_12_streams(gpu_lib, voice, rate):
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_lib)
    eng.set_output_rate(rate)
    ids, lens, sid, scales, vol, keys = _ragged(cfg, 48, 20, 128, seed=151)
    rng = np.random.default_rng(5)
    streams = _twelve(rng.permutation(48).reshape(12, 4))
    got = eng.run_streams(ids, lens, scales, sid, streams=streams, seed=SEED, utterance_keys=keys, pcm_volume=vol)
    assert [pa.sample_rate for pa in got] == [rate or cfg.sample_rate] * 12
    check_against_twins(eng, streams, got)  # each stream its fetch_packed twin, the gaps zero
    eng.profile_enable(True)
    eng.profile_reset()
    regrouped = _twelve(rng.permutation(48).reshape(12, 4))[::-1] + [dict(order=[7, 7 + 1], encoding="f32le", wav=True)]
    again = eng.fetch_streams(regrouped)
    check_against_twins(eng, regrouped, again)
    rep = eng.profile_report()
    assert rep["pack.streams"]["calls"] == 1 and set(rep) <= {"pack.streams", "edges", "loudness"} | {"pcm16.pack", "pack.ulaw", "pack.alaw", "pack.f32"}, sorted(rep)  # (the twins' own packs) no synthesis repeated
    eng.close()


def test_256_rows_one_file_each(gpu_lib, voice):
    cfg, blob = voice
    eng = Engine(blob, device=0, library=gpu_lib)
    B = 256
    ids, lens, sid, scales, _, keys = _ragged(cfg, B, 20, 64, seed=152)
    streams = [dict(order=[b], wav=True) for b in range(B)]
    # (volume 100 %: the padded int16 rows a fetch makes after a run that made none carry no volume, as after a DEVICE_ONLY run)
    got = eng.run_streams(ids, lens, scales, sid, streams=streams, seed=SEED, utterance_keys=keys)
    full = eng.fetch(want_float=False, want_pcm16=True)
    block = got[0].block
    outside = np.ones(block.shape[0], bool)
    for b, pa in enumerate(got):
        n = int(full["lengths"][b])
        assert pa.total_samples == n and pa.data_offset % 16 == 0 and pa.data_offset - pa.stream_offset == 44, b
        assert pa.data.tobytes() == full["pcm"][b, :n].tobytes(), b
        outside[pa.stream_offset: pa.stream_offset + pa.stream_bytes] = False
    assert not block[outside].any()
    for b in (0, 1, 63, 64, 127, 128, 200, 255):
        assert bytes(got[b].wav) == bytes(twin(eng, streams[b]).wav), b
    eng.close()


def test_run_stream_micro_batched_on_two_lanes(voice):
    cfg, blob = voice
    so = SessionOptions()
    so.seed = 9
    plain = InferenceSession(blob, sess_options=so)
    so = SessionOptions()
    so.seed = 9
    so.lanes = 2
    so.micro_batch_window_ms = 2.0
    so.micro_batch_max = 64
    sess = InferenceSession(blob, sess_options=so)
    rng = np.random.default_rng(153)
    reqs = []
    for i in range(32):
        tx = int(rng.integers(20, 64))
        lens = np.array([tx, int(rng.integers(20, tx + 1))], np.int64)
        ids = np.zeros((2, tx), np.int64)
        for b in range(2):
            ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
        kw = dict(utterance_keys=[5000 + 2 * i, 5001 + 2 * i], encoding=ENCODINGS[i % 4], wav=bool(i % 2), lead_ms=[0.0, 150.0], volume=[100.0, 60.0] if i % 3 == 0 else None)
        if i % 5 == 0:
            kw.update(trim_db=-30.0, trim_keep_ms=2.0)
        if i % 7 == 0:
            kw.update(loudness=-23.0)
        reqs.append(({"input": ids, "input_lengths": lens, "scales": np.array([0.667, 1.0, 0.8], np.float32)}, kw))
    got, errs = [None] * 32, [None] * 32
    gate = threading.Barrier(32)

    def work(i):
        gate.wait()
        try:
            got[i] = sess.run_stream(reqs[i][0], **reqs[i][1])
        except BaseException as e:  # noqa: BLE001
            errs[i] = e

    ts = [threading.Thread(target=work, args=(i,)) for i in range(32)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert errs == [None] * 32
    assert sess._batcher.requests == 32 and sess._batcher.batches < 32
    for i, (feed, kw) in enumerate(reqs):
        want = plain.run_packed(feed, **kw)
        assert got[i].data.tobytes() == want.data.tobytes(), i
        assert (want.wav is None) == (got[i].wav is None) and (want.wav is None or bytes(got[i].wav) == bytes(want.wav)), i
        for k in ("offsets", "lengths", "peaks"):
            assert getattr(got[i], k).tobytes() == getattr(want, k).tobytes(), (i, k)
    sess.close()
    plain.close()
