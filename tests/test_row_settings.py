"""Per-row synthesis settings in one batched call (mi355vits_run_rows): scales [B,3], PCM volume [B] and Philox noise keys
[B].  On the CPU model of the kernels (tests/emu); test_gpu_row_settings.py runs the same contract on the MI355X.

The contract (include/mi355vits.h): row b of a batch is bitwise its own call with scalar settings and
utterance_base = its key, as long as the padded phoneme length stays in the row's encoder length class."""
import audioop
import ctypes
import threading

import numpy as np
import pytest

from mimic3_amd import sharding
from mimic3_amd import streaming as ST
from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError, Result, RowArgs, RunArgs, WANT_FLOAT, WANT_PCM16, _fptr
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from oracle.vits_oracle import VitsOracle
from tests.util import parity_tol, rel_rms

SEED = 0xC0FFEE
# five ragged rows: most with noise, one deterministic; length_scale 0.7 .. 1.6; keys far apart and out of order
SCALES = np.array([[0.667, 1.0, 0.8], [0.0, 1.6, 0.0], [0.5, 0.7, 0.3], [0.9, 1.2, 1.1], [0.333, 0.85, 0.0]], np.float32)
KEYS = [7, 1_000_003, 42, (1 << 40) + 5, 3]
VOLUMES = [50.0, 100.0, 150.0, 300.0, 7.5]  # percent; 300 % clips


def _inputs(cfg, B, Tx, seed):
    rng = np.random.default_rng(seed)
    lens = np.array([Tx] + list(rng.integers(2, Tx, size=B - 1)), np.int64)
    ids = np.zeros((B, Tx), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    sid = (np.arange(B) % cfg.n_speakers).astype(np.int64) if cfg.is_multispeaker else None
    return ids, lens, sid


def _same_row(full, b, one):
    L = int(one["lengths"][0])
    assert L == int(full["lengths"][b]), (b, L, int(full["lengths"][b]))
    assert np.array_equal(one["audio"][0, :L], full["audio"][b, :L]), b
    assert np.array_equal(one["pcm"][0, :L], full["pcm"][b, :L]), b
    assert one["peaks"][0].tobytes() == full["peaks"][b].tobytes(), b


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("n_speakers", [1, 4])
def test_every_row_is_its_solo_run(emu_lib, math, n_speakers):
    cfg = VitsConfig.tiny(n_speakers=n_speakers) if n_speakers > 1 else VitsConfig.tiny()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=21)), library=emu_lib)
    eng.set_math(math)
    ids, lens, sid = _inputs(cfg, 5, 12, seed=21)
    vol = np.array(VOLUMES) / 100.0
    full = eng.run(ids, lens, SCALES, sid, seed=SEED, utterance_keys=KEYS, pcm_volume=vol, want_pcm16=True)
    for b in range(5):
        n = int(lens[b])
        one = eng.run(ids[b:b + 1, :n], [n], SCALES[b], None if sid is None else sid[b:b + 1], seed=SEED,
                      utterance_base=KEYS[b], pcm_volume=float(vol[b]), want_pcm16=True)
        _same_row(full, b, one)
    eng.close()


def _run_rows_null(eng, ids, lens, scales, seed, base, volume):
    """mi355vits_run_rows with a row_args struct whose pointers are all NULL."""
    ids = np.ascontiguousarray(ids, np.int64)
    lens = np.ascontiguousarray(lens, np.int64)
    scales = np.ascontiguousarray(scales, np.float32)
    a = RunArgs()
    a.batch, a.tx_max = ids.shape
    a.ids = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    a.lengths = lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    a.scales = _fptr(scales)
    a.seed, a.utterance_base = seed, base
    a.flags = WANT_FLOAT | WANT_PCM16
    a.pcm_volume = volume
    r = Result()
    eng._check(eng.native.lib.mi355vits_run_rows(eng._h, ctypes.byref(a), ctypes.byref(RowArgs()), ctypes.byref(r)))
    return eng._take(r)


def test_broadcast_rows_are_the_plain_call(emu_lib):
    cfg = VitsConfig.tiny()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=22)), library=emu_lib)
    ids, lens, _ = _inputs(cfg, 4, 10, seed=22)
    sc = np.array([0.667, 1.1, 0.8], np.float32)
    plain = eng.run(ids, lens, sc, seed=SEED, utterance_base=900, pcm_volume=1.5, want_pcm16=True)
    null_rows = _run_rows_null(eng, ids, lens, sc, SEED, 900, 1.5)
    explicit = eng.run(ids, lens, np.tile(sc, (4, 1)), seed=SEED, utterance_keys=900 + np.arange(4),
                       pcm_volume=np.full(4, 1.5), want_pcm16=True)
    for got in (null_rows, explicit):
        for k in ("lengths", "audio", "pcm", "peaks"):
            assert got[k].tobytes() == plain[k].tobytes(), k
    eng.close()


def test_deterministic_rows_match_the_oracle_and_volume_is_audioop(emu_lib):
    cfg = VitsConfig.tiny()
    w = W.synthetic_weights(cfg, seed=23, frames_per_id=2.5)
    eng = Engine(W.pack(cfg, w), library=emu_lib)
    ora = VitsOracle(cfg, w)
    ids, lens, _ = _inputs(cfg, 4, 11, seed=23)
    scales = np.array([[0.0, ls, 0.0] for ls in (0.7, 1.0, 1.3, 1.6)], np.float32)
    vols = [50.0, 100.0, 300.0, 7.5]
    full = eng.run(ids, lens, scales, pcm_volume=np.array(vols) / 100.0, want_pcm16=True)
    unit = eng.run(ids, lens, scales, want_pcm16=True)  # the same rows at volume 1
    tol = parity_tol(eng)
    for b in range(4):
        n = int(lens[b])
        ref = ora.infer(ids[b:b + 1, :n], np.array([n]), scales[b])
        L = int(full["lengths"][b])
        assert L == int(ref["audio_lengths"][0])
        assert rel_rms(full["audio"][b, :L], ref["audio"][0, 0, :L]) < tol
        want = np.frombuffer(audioop.mul(unit["pcm"][b, :L].tobytes(), 2, vols[b] / 100.0), np.int16)
        assert np.array_equal(full["pcm"][b, :L], want), b
    assert len({int(x) for x in full["lengths"]}) > 1  # the length scales took effect per row
    eng.close()


@pytest.mark.parametrize("bad,what", [((float("nan"), 1.0, 0.5), "finite"), ((0.5, 0.0, 0.5), "length_scale"),
                                      ((0.5, -1.0, 0.5), "length_scale"), ((-0.1, 1.0, 0.5), "noise"),
                                      ((0.5, 1.0, -0.2), "noise")])
def test_a_bad_row_is_named_and_the_handle_survives(emu_lib, bad, what):
    cfg = VitsConfig.tiny()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=24)), library=emu_lib)
    ids, lens, _ = _inputs(cfg, 4, 9, seed=24)
    good = np.tile(np.array([0.667, 1.0, 0.8], np.float32), (4, 1))
    before = eng.run(ids, lens, good, seed=SEED, want_pcm16=True)
    scales = good.copy()
    scales[2] = bad
    with pytest.raises(NativeError, match=f"row 2: .*{what}") as ei:
        eng.run(ids, lens, scales, seed=SEED)
    assert ei.value.code == -1
    after = eng.run(ids, lens, good, seed=SEED, want_pcm16=True)
    for k in ("lengths", "audio", "pcm", "peaks"):
        assert after[k].tobytes() == before[k].tobytes(), k
    eng.close()


def test_micro_batcher_merges_mixed_settings(emu_lib):
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=25, frames_per_id=2.0))
    plain = InferenceSession(blob, _library=emu_lib)
    so = SessionOptions()
    so.micro_batch_window_ms = 200.0
    so.micro_batch_max = 16
    mb = InferenceSession(blob, sess_options=so, _library=emu_lib)
    rng = np.random.default_rng(25)
    settings = [(np.array([0.0, ls, 0.0], np.float32), vol) for ls in (0.8, 1.0, 1.2, 1.5) for vol in (50.0, 100.0, 150.0)]
    feeds = []
    for k in range(12):
        n = int(rng.integers(4, 14))
        feeds.append({"input": rng.integers(1, cfg.num_symbols, (1, n)).astype(np.int64),
                      "input_lengths": np.array([n], np.int64), "scales": settings[k][0]})
    expect = [plain.run_pcm16(feeds[k], volume=settings[k][1])[0][0] for k in range(12)]
    got = [None] * 12
    errs = []
    gate = threading.Barrier(12)

    def client(k):
        try:
            gate.wait()
            got[k] = mb.run_pcm16(feeds[k], volume=settings[k][1])[0][0]
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)

    ts = [threading.Thread(target=client, args=(k,)) for k in range(12)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for k in range(12):
        assert np.array_equal(got[k], expect[k]), k
    groups = len({(tuple(s.tolist()), v) for s, v in settings})
    assert mb._batcher.requests == 12 and mb._batcher.batches < groups, (mb._batcher.batches, groups)
    mb.close()
    plain.close()


def test_streams_are_identical_across_modes_at_stochastic_scales(emu_lib):
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=26, frames_per_id=2.0))
    so = SessionOptions()
    so.seed = 77
    so.lanes = 2
    so.micro_batch_window_ms = 5.0
    sess = InferenceSession(blob, sess_options=so, _library=emu_lib)
    rng = np.random.default_rng(26)
    sentences = [rng.integers(1, cfg.num_symbols, int(rng.integers(3, 20))).tolist() for _ in range(11)]
    sc = (0.667, 1.0, 0.8)
    K = 5000
    planned = list(ST.stream_sentences(sess, sentences, scales=sc, look_ahead=4, utterance_base=K))
    lazy = list(ST.stream_sentences(sess, iter(sentences), scales=sc, look_ahead=4, utterance_base=K))
    single = [sess.run_pcm16(ST._feed(s, sc, None), utterance_keys=[K + i])[0][0] for i, s in enumerate(sentences)]
    assert len(planned) == len(lazy) == len(single) == len(sentences)
    for i in range(len(sentences)):
        assert np.array_equal(planned[i], single[i]), i
        assert np.array_equal(lazy[i], single[i]), i
    other = sess.run_pcm16(ST._feed(sentences[3], sc, None), utterance_keys=[K + 4])[0][0]
    assert not np.array_equal(other, single[3])  # the key is what decides the noise
    sess.close()


def test_shard_feed_slices_per_row_scales_and_session_takes_them(emu_lib):
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=27, frames_per_id=2.0))
    ids, lens, _ = _inputs(cfg, 5, 10, seed=27)
    scales = np.array([[0.0, ls, 0.0] for ls in (0.7, 0.9, 1.1, 1.3, 1.5)], np.float32)
    feed = {"input": ids, "input_lengths": lens, "scales": scales}
    for rank in range(2):
        part, rows = sharding.shard_feed(feed, 2, rank)
        assert np.array_equal(part["scales"], scales[rows])
    uniform = dict(feed, scales=scales[0])
    assert sharding.shard_feed(uniform, 2, 1)[0]["scales"] is uniform["scales"]
    sess = InferenceSession(blob, _library=emu_lib)
    full = sess.run(None, feed)[0]
    full_len = sess.last_lengths.copy()
    for b in range(5):
        n = int(lens[b])
        one = sess.run(None, {"input": ids[b:b + 1, :n], "input_lengths": lens[b:b + 1], "scales": scales[b]})[0]
        L = int(sess.last_lengths[0])
        assert L == int(full_len[b])
        assert np.array_equal(one[0, 0, :L], full[b, 0, :L]), b
    sess.close()


def test_reserve_utterances_advances_the_session_count(emu_lib):
    cfg = VitsConfig.tiny()
    sess = InferenceSession(W.pack(cfg, W.synthetic_weights(cfg, seed=28)), _library=emu_lib)
    a = sess.reserve_utterances(3)
    b = sess.reserve_utterances(2)
    assert b == a + 3 and sess._utterances == a + 5
    sess.close()
