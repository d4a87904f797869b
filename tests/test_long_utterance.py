"""Utterances above the VALU attention kernel's length cap (the streamed attention kernel, k_rel_attention_stream) on the CPU
model of the kernels, and the fifth encoder length class in the batching layers."""
import time

import numpy as np
import pytest

from mimic3_amd import streaming as ST
from mimic3_amd import weights as W
from mimic3_amd.config import VitsConfig, tx_class
from mimic3_amd.session import InferenceSession, SessionOptions

from tests.attention_ref import attention_case, rel_attention_fp64
from tests.util import check_parity


def check_stream_vs_fp64(lib, T, d, lengths, n_heads=2):
    qkv, ek, ev, ln = attention_case(T, d, lengths, n_heads)
    got = lib.test_rel_attention(qkv, ek, ev, ln, n_heads, impl=2)
    ref = rel_attention_fp64(qkv, ek, ev, ln, n_heads)
    for b, L in enumerate(ln):
        assert np.all(got[b, :, L:] == 0.0), (T, d, b, "padded query rows must be zeros")
        if L:
            err = np.abs(got[b, :, :L] - ref[b, :, :L]).max() / np.abs(ref[b, :, :L]).max()
            assert err < 2e-6, (T, d, b, L, err)
    return got


@pytest.mark.parametrize("d", [16, 96])
@pytest.mark.parametrize("T", [1, 31, 33, 300, 600])
def test_stream_attention_hook_vs_fp64(emu_lib, T, d):
    lengths = sorted({T, 1, min(T, 17), max(1, T - 100)}, reverse=True)
    check_stream_vs_fp64(emu_lib, T, d, lengths)


def test_stream_attention_rows_do_not_depend_on_padding(emu_lib):
    qkv, ek, ev, ln = attention_case(200, 16, [150, 70])
    a = emu_lib.test_rel_attention(qkv, ek, ev, ln, 2, impl=2)
    wide = np.zeros((2, qkv.shape[1], 333), np.float32)
    wide[:, :, :200] = qkv
    wide[:, :, 200:] = 1e3  # garbage past every row's length is never read
    b = emu_lib.test_rel_attention(wide, ek, ev, ln, 2, impl=2)
    assert np.array_equal(a, b[:, :, :200])


def test_stream_attention_hook_rejects_unsupported_shapes(emu_lib):
    qkv, ek, ev, ln = attention_case(40, 130, [40], n_heads=1)
    with pytest.raises(Exception, match="streamed"):
        emu_lib.test_rel_attention(qkv, ek, ev, ln, 1, impl=2)
    qkv, ek, ev, ln = attention_case(600, 16, [600])
    with pytest.raises(Exception, match="MFMA"):
        emu_lib.test_rel_attention(qkv, ek, ev, ln, 2, impl=1)


def test_utterance_above_the_cap_matches_the_oracle(emu_lib):
    """One 4,100-id utterance of the tiny voice (cap 4,071): refused before the streamed kernel existed."""
    cfg = VitsConfig.tiny()
    assert cfg.attention_cap == 4071
    Tx = 4100
    forced = np.ones((1, Tx), np.int32)
    out, _ = check_parity(emu_lib, cfg, B=1, Tx=Tx, seed=3, forced=forced, ragged=False)
    assert int(out["lengths"][0]) == Tx * cfg.upsample_factor


def test_length_classes_separate_lengths_above_the_cap():
    cap = VitsConfig.tiny_h192().attention_cap
    assert cap == 3991
    assert [tx_class(n) for n in (128, 129, 256, 257, 512, 513, cap, cap + 1)] == [0, 1, 1, 2, 2, 3, 3, 3]
    assert [tx_class(n, cap) for n in (512, 513, cap, cap + 1, 9000)] == [2, 3, 3, 4, 4]
    assert ST._tx_class(cap + 1) == 3  # without a cap: the four classes of old
    lens = [5, 600, cap + 1, 600, cap + 1, 700, cap + 50]
    plan = ST.plan_batches(lens, cap=cap)
    assert sorted(i for b in plan for i in b) == list(range(len(lens)))
    for b in plan:
        assert len({tx_class(lens[i], cap) for i in b}) == 1, (b, plan)
    assert [1, 3, 5] in plan and [2, 4, 6] in plan
    assert [1, 2, 3, 4, 5, 6] in ST.plan_batches(lens)  # plan_batches(lengths) keeps its old classes


def test_stream_planned_takes_the_cap_from_the_session():
    cfg = VitsConfig.tiny_h192()
    calls = []

    class Recorder:
        config = cfg

        def run_pcm16(self, feed, volume=None, direct=False, **kw):
            lens = [int(n) for n in feed["input_lengths"]]
            calls.append(lens)
            return [np.full(n, n, np.int16) for n in lens], np.asarray(lens)

    sentences = [[1] * n for n in (4, 600, 4500, 620, 4200)]
    chunks = list(ST.stream_planned(Recorder(), sentences, scales=(0.0, 1.0, 0.0)))
    assert [len(c) for c in chunks] == [4, 600, 4500, 620, 4200]
    assert sorted(calls) == sorted([[4], [600, 620], [4500, 4200]])


def test_micro_batcher_keeps_lengths_above_the_cap_apart(emu_lib):
    cfg = VitsConfig.tiny()
    cap = cfg.attention_cap
    so = SessionOptions()
    so.micro_batch_window_ms = 50.0
    so.micro_batch_max = 8
    sess = InferenceSession(W.pack(cfg, W.synthetic_weights(cfg, seed=9)), sess_options=so, _library=emu_lib)
    mb = sess._batcher
    groups = []

    def record(group, lane_done=None):  # the grouping only: no synthesis
        groups.append([int(g[1][0]) for g in group])
        for g in group:
            g[5].set_result(None)

    mb._run_group = record
    with mb._inflight_cv:
        mb._inflight = mb._lanes  # every lane busy: the dispatcher collects everything submitted below into one round
    lens = [600, cap + 1, 620, cap + 30]
    futs = [mb.submit(np.zeros((1, n), np.int64), np.array([n], np.int64), np.array([0.0, 1.0, 0.0], np.float32), None, {})
            for n in lens]
    time.sleep(0.3)
    with mb._inflight_cv:
        mb._inflight = 0
        mb._inflight_cv.notify_all()
    for f in futs:
        f.result(timeout=30)
    assert sorted(sorted(g) for g in groups) == [[600, 620], [cap + 1, cap + 30]], groups
