"""Utterances above the VALU attention kernel's length cap on the MI355X (pytest -m gpu): the streamed attention kernel
(k_rel_attention_stream) against the oracle and fp64, its padding independence and determinism, and the batched / streamed
paths in the fifth encoder length class.  tests/test_long_utterance.py checks the same kernel on the CPU model."""
import numpy as np
import pytest

from mimic3_amd import streaming as ST
from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession
from oracle.vits_oracle import VitsOracle
from tests.test_long_utterance import attention_case, check_stream_vs_fp64, rel_attention_fp64
from tests.util import TIGHT_REL_RMS_TOL, check_parity, rel_rms

pytestmark = pytest.mark.gpu


def _ids(cfg, lens, tx=None, seed=0):
    rng = np.random.default_rng(seed)
    tx = tx or max(lens)
    ids = np.zeros((len(lens), tx), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(1, cfg.num_symbols, size=n)
    return ids, np.asarray(lens, np.int64)


def test_tiny_h192_rows_above_the_cap_with_noise(gpu_lib):
    cfg = VitsConfig.tiny_h192()
    assert cfg.attention_cap == 3991
    ids, lens = _ids(cfg, [4500, 4200], seed=1)
    check_parity(gpu_lib, cfg, ids=ids, lengths=lens, noise=True, seed=4)


def test_tiny_h192_8192_ids(gpu_lib):
    cfg = VitsConfig.tiny_h192()
    ids, lens = _ids(cfg, [8192], seed=2)
    check_parity(gpu_lib, cfg, ids=ids, lengths=lens, forced=np.ones((1, 8192), np.int32), seed=5)


def test_apope_low_4500_ids_default_math(gpu_lib):
    cfg = VitsConfig.apope_low()
    ids, lens = _ids(cfg, [4500], seed=3)
    check_parity(gpu_lib, cfg, ids=ids, lengths=lens, forced=np.full((1, 4500), 2, np.int32), seed=6, frames_per_id=3.0)


def test_apope_low_4500_ids_f32_encoder(gpu_lib):
    cfg = VitsConfig.apope_low()
    w = W.synthetic_weights(cfg, seed=106, frames_per_id=3.0)
    ids, lens = _ids(cfg, [4500], seed=3)
    eng = Engine(W.pack(cfg, w), device=0)
    eng.set_math("f32")
    forced = np.full((1, 4500), 2, np.int32)
    eng.run(ids, lens, [0.0, 1.0, 0.0], forced_durations=forced, debug_taps=True)
    ref = VitsOracle(cfg, w).infer(ids, lens, [0.0, 1.0, 0.0], forced_durations=forced)
    st = eng.tap("stats")
    I = cfg.inter_channels
    for name, got, r in (("x", eng.tap("x"), ref["x"]), ("m_p", st[:, :I], ref["m_p"]), ("logs_p", st[:, I:], ref["logs_p"])):
        assert rel_rms(got, r) < TIGHT_REL_RMS_TOL, (name, rel_rms(got, r))
    eng.close()


@pytest.mark.parametrize("T", [33, 600, 3991, 4500, 8192])
def test_stream_attention_hook_vs_fp64(gpu_hooks, T):
    lengths = sorted({T, 1, min(T, 17), max(1, T - 100)}, reverse=True)
    got = check_stream_vs_fp64(gpu_hooks, T, 96, lengths)
    if T <= VitsConfig.apope_low().attention_cap:  # the VALU kernel on the same input: within the f32 tolerance
        qkv, ek, ev, ln = attention_case(T, 96, lengths)
        valu = gpu_hooks.test_rel_attention(qkv, ek, ev, ln, 2, impl=0)
        ref = rel_attention_fp64(qkv, ek, ev, ln, 2)
        for b, L in enumerate(ln):
            scale = np.abs(ref[b, :, :L]).max()
            assert np.abs(got[b, :, :L] - valu[b, :, :L]).max() / scale < 4e-6, (T, b)
    again = check_stream_vs_fp64(gpu_hooks, T, 96, lengths)
    assert np.array_equal(got, again)  # deterministic


def test_row_does_not_depend_on_padding_above_the_cap(gpu_lib):
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=8, frames_per_id=3.0)), device=0)
    ids, lens = _ids(cfg, [4300], seed=8)
    a = eng.run(ids, lens, [0.667, 1.0, 0.8], seed=11, want_pcm16=True)
    wide = np.zeros((1, 5000), np.int64)
    wide[:, :4300] = ids
    b = eng.run(wide, lens, [0.667, 1.0, 0.8], seed=11, want_pcm16=True)
    L = int(a["lengths"][0])
    assert L == int(b["lengths"][0]) and L > 0
    assert np.array_equal(a["audio"][0, :L], b["audio"][0, :L])
    assert np.array_equal(a["pcm"][0, :L], b["pcm"][0, :L])
    eng.close()


def test_run_rows_above_the_cap_are_their_solo_calls(gpu_lib):
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=9, frames_per_id=3.0)), device=0)
    lens = [4500, 4100, 4321]
    ids, ln = _ids(cfg, lens, seed=9)
    scales = np.array([[0.667, 1.0, 0.8], [0.0, 1.3, 0.0], [0.5, 0.8, 0.6]], np.float32)
    vols = np.array([1.0, 0.5, 2.0])
    keys = [701, 13, 4242]
    full = eng.run(ids, ln, scales, seed=3, utterance_keys=keys, pcm_volume=vols, want_pcm16=True)
    for b, n in enumerate(lens):
        one = eng.run(ids[b:b + 1, :n], ln[b:b + 1], scales[b], seed=3, utterance_base=keys[b], pcm_volume=float(vols[b]),
                      want_pcm16=True)
        L = int(one["lengths"][0])
        assert L == int(full["lengths"][b]), b
        assert np.array_equal(one["audio"][0, :L], full["audio"][b, :L]), b
        assert np.array_equal(one["pcm"][0, :L], full["pcm"][b, :L]), b
    eng.close()


def test_planned_stream_with_one_long_sentence(gpu_lib):
    cfg = VitsConfig.apope_low()
    sess = InferenceSession(W.pack(cfg, W.synthetic_weights(cfg, seed=10, frames_per_id=3.0)))
    rng = np.random.default_rng(10)
    lens = [int(n) for n in rng.integers(8, 160, size=30)]
    lens[17] = 4500
    lens[5] = 600
    sentences = [list(rng.integers(1, cfg.num_symbols, size=n)) for n in lens]
    chunks = list(ST.stream_planned(sess, sentences, scales=(0.667, 1.0, 0.8), utterance_base=500))
    assert len(chunks) == 30
    for i, s in enumerate(sentences):
        pcm = sess.run_pcm16(ST._feed(s, (0.667, 1.0, 0.8), None), utterance_keys=[500 + i])[0][0]
        assert np.array_equal(np.asarray(chunks[i]), np.asarray(pcm)), i
    sess.close()


def test_limits_still_refuse_before_any_launch(gpu_lib):
    cfg = VitsConfig.tiny()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=12)), device=0)
    B, Tx = 2, (1 << 25) + 1  # B * Tx > 2^26
    ids = np.ones((B, Tx), np.int64)
    with pytest.raises(NativeError, match="too large") as e:
        eng.run(ids, [Tx, Tx], [0.0, 1.0, 0.0])
    assert e.value.code == -1  # MI355VITS_ERR_INVALID
    del ids
    out = eng.run(np.array([[3, 5, 7, 2]], np.int64), [4], [0.0, 1.0, 0.0])  # the handle stays usable
    assert int(out["lengths"][0]) > 0
    eng.close()
