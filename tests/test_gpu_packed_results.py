"""Device twin of tests/test_packed_results.py (pytest -m gpu): mi355vits_run_packed / mi355vits_fetch_packed and k_pack<S16> on
the MI355X at sizes a user runs — ragged batches of the released voices' shapes (synthetic weights), the benchmark's headline
shape, one utterance of the streamed-attention class, and a NaN-filled workspace.  The yardstick is the padded call
(Engine.run(..., want_pcm16=True)) on the same engine + host numpy / postprocess.wav_bytes."""
import io
import wave

import numpy as np
import pytest

from mimic3_amd import postprocess as PP
from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from tests.test_packed_results import CHUNK, _assert_entries, _chunks

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE


def _ragged(cfg, B, lo, hi, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, B).astype(np.int64)
    lens[0], lens[B // 2] = hi, lo
    ids = np.zeros((B, hi), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    sid = (np.arange(B) % cfg.n_speakers).astype(np.int64) if cfg.is_multispeaker else None
    scales = np.stack([rng.uniform(0.3, 0.9, B), rng.uniform(0.8, 1.3, B), rng.uniform(0.2, 1.0, B)], axis=1).astype(np.float32)
    vol = rng.choice([0.5, 1.0, 1.5, 3.0, 0.075], B)  # 3.0 clips
    keys = [int(k) for k in rng.integers(0, 1 << 40, B)]
    return ids, lens, sid, scales, vol, keys


@pytest.mark.parametrize("math", ["bf16x3", "f32", "bf16w"])
@pytest.mark.parametrize("voice", ["apope_low", "vctk_low"])
def test_48_ragged_rows_packed(gpu_lib, voice, math):
    """48 ragged rows of 20 .. 128 ids with natural durations, noise on, per-row scales, volumes and keys: the default pack, a
    permutation with silences behind a header, and fetch_packed after the padded call."""
    cfg = getattr(VitsConfig, voice)()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=141, frames_per_id=3.0)), device=0, library=gpu_lib)
    eng.set_math(math)
    B = 48
    ids, lens, sid, scales, vol, keys = _ragged(cfg, B, 20, 128, seed=141)
    kw = dict(seed=SEED, utterance_keys=keys, pcm_volume=vol)
    full = eng.run(ids, lens, scales, sid, want_pcm16=True, **kw)
    padded = {k: full[k].copy() for k in ("pcm", "lengths", "peaks")}
    assert len({int(x) for x in full["lengths"]}) > B // 2
    # 1. the default pack
    pk = eng.run_packed(ids, lens, scales, sid, **kw)
    assert int(pk.offsets[0]) == 0 and pk.wav is None
    assert np.array_equal(pk.offsets[1:], np.cumsum(full["lengths"])[:-1])
    assert pk.total_samples == int(np.sum(full["lengths"]))
    assert pk.lengths.tobytes() == full["lengths"].tobytes() and pk.peaks.tobytes() == full["peaks"].tobytes()
    _assert_entries(pk, full, range(B))
    # 2. a permutation that drops a row; silences of 0, 1, odd counts and more than a chunk; a tail; a header
    rng = np.random.default_rng(7)
    order = [int(b) for b in rng.permutation(B) if b != 17]
    lead = [int(x) for x in rng.integers(0, 3 * CHUNK, len(order))]
    lead[:4] = [0, 1, 777, CHUNK + 453]
    spec = dict(order=order, lead_samples=lead, tail_samples=2205, wav=True)
    pk2 = eng.run_packed(ids, lens, scales, sid, **spec, **kw)
    want = PP.wav_bytes(_chunks(full, order, lead, 2205), cfg.sample_rate)
    assert bytes(pk2.wav) == want
    _assert_entries(pk2, full, order)
    with wave.open(io.BytesIO(bytes(pk2.wav)), "rb") as wf:
        assert (wf.getframerate(), wf.getnchannels(), wf.getsampwidth(), wf.getnframes()) == (cfg.sample_rate, 1, 2, pk2.total_samples)
    one = eng.run_packed(ids, lens, scales, sid, order=[B // 2], lead_samples=[3], wav=True, **kw)
    assert bytes(one.wav) == PP.wav_bytes(_chunks(full, [B // 2], [3]), cfg.sample_rate)
    # 3. fetch_packed after the padded call: two specs in a row, the padded result unchanged in between
    eng.run(ids, lens, scales, sid, want_pcm16=True, **kw)
    spec_b = dict(order=order[::-1][:20], lead_samples=lead[:20], tail_samples=1, wav=False)
    for s, ref in ((spec, want), (spec_b, np.concatenate(_chunks(full, spec_b["order"], spec_b["lead_samples"], 1)).tobytes())):
        got = eng.fetch_packed(**s)
        assert (bytes(got.wav) if got.wav is not None else got.pcm.tobytes()) == ref
        between = eng.fetch(want_float=False, want_pcm16=True)
        for k in padded:
            assert between[k].tobytes() == padded[k].tobytes(), k
    eng.close()


def test_headline_shape_packed_and_its_profile_line(gpu_lib):
    """256 rows x 128 ids x 6 forced frames (the benchmark's headline): packed rows bitwise the padded rows; with profiling on
    the packed call's report has pcm16.pack with 4 x sum(lengths) + 2 x total_samples bytes and no pcm16 line."""
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0)), device=0, library=gpu_lib)
    B, Tx = 256, 128
    rng = np.random.default_rng(1)
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    lens = np.full(B, Tx, np.int64)
    forced = np.full((B, Tx), 6, np.int32)
    sc = [0.667, 1.0, 0.8]
    full = eng.run(ids, lens, sc, forced_durations=forced, seed=1, want_float=False, want_pcm16=True)
    assert int(full["lengths"][0]) == Tx * 6 * cfg.hop_length
    eng.profile_enable(True)
    eng.profile_reset()
    pk = eng.run_packed(ids, lens, sc, forced_durations=forced, seed=1)
    rep = eng.profile_report()
    eng.profile_enable(False)
    assert "pcm16.pack" in rep and "pcm16" not in rep, sorted(rep)
    assert rep["pcm16.pack"]["calls"] == 1
    assert rep["pcm16.pack"]["bytes"] == 4.0 * float(np.sum(full["lengths"])) + 2.0 * pk.total_samples
    print(f"pcm16.pack at the headline shape: {rep['pcm16.pack']['ms']:.4f} ms")
    assert pk.total_samples == B * int(full["lengths"][0])
    assert np.array_equal(pk.pcm.reshape(B, -1), full["pcm"])
    eng.close()


def test_one_4300_id_utterance_packed_with_a_header(gpu_lib):
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=8, frames_per_id=3.0)), device=0, library=gpu_lib)
    rng = np.random.default_rng(8)
    ids = rng.integers(1, cfg.num_symbols, (1, 4300))
    full = eng.run(ids, [4300], [0.667, 1.0, 0.8], seed=11, want_pcm16=True, pcm_volume=0.8)
    pk = eng.run_packed(ids, [4300], [0.667, 1.0, 0.8], seed=11, pcm_volume=0.8, lead_samples=[5], tail_samples=11, wav=True)
    assert bytes(pk.wav) == PP.wav_bytes(_chunks(full, [0], [5], 11), cfg.sample_rate)
    eng.close()


def test_packed_stream_on_a_nan_filled_workspace(gpu_hooks):
    """apope_low, 24 ragged rows, on a handle whose workspace a larger packed call sized first and a quiet NaN then filled: the
    same bytes as a fresh handle's (the silences are zeros because the kernel wrote them)."""
    cfg = VitsConfig.apope_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=131, frames_per_id=3.0))
    rng = np.random.default_rng(131)
    B, Tx = 24, 64
    lengths = rng.integers(1, Tx + 1, B)
    lengths[0], lengths[5] = Tx, 1
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    scales = [0.667, 1.0, 0.8]
    order = [int(b) for b in rng.permutation(B)]
    lead = [int(x) for x in rng.integers(0, 2 * CHUNK, B)]
    spec = dict(order=order, lead_samples=lead, tail_samples=4097, wav=True)
    kw = dict(seed=SEED, pcm_volume=np.linspace(0.5, 3.0, B))
    fresh = Engine(blob, device=0, library=gpu_hooks)
    want = bytes(fresh.run_packed(ids, lengths, scales, **spec, **kw).wav)
    full = fresh.run(ids, lengths, scales, want_pcm16=True, **kw)
    assert want == PP.wav_bytes(_chunks(full, order, lead, 4097), cfg.sample_rate)
    fresh.close()
    eng = Engine(blob, device=0, library=gpu_hooks)
    big = eng.run_packed(rng.integers(1, cfg.num_symbols, (B + 4, Tx)), np.full(B + 4, Tx), scales,
                         forced_durations=np.full((B + 4, Tx), 8, np.int32), lead_samples=[4 * CHUNK] * (B + 4),
                         tail_samples=8 * CHUNK)  # sizes the workspace past what the ragged call needs
    assert big.total_samples > len(want) // 2
    del big
    eng.fill_workspace(0x7FC00000)
    assert bytes(eng.run_packed(ids, lengths, scales, **spec, **kw).wav) == want
    eng.fill_workspace(0x7FC00000)
    eng.run(ids, lengths, scales, device_only=True, **kw)
    assert bytes(eng.fetch_packed(**spec).wav) == want
    eng.close()
