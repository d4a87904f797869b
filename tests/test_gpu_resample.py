"""Device twin of tests/test_resample.py (pytest -m gpu): mi355vits_set_output_rate and k_resample on the MI355X at sizes a user
runs — a ragged batch of the released single-speaker voice's shape (synthetic weights) with a one-phoneme row, the kernel alone
through the hook, a NaN-filled workspace, the packed stream at 16 kHz.  Same yardstick as the CPU file: tests/resample_ref.py on the
native f32 audio of the same engine, the oracle's audio_float_to_int16, postprocess, the stdlib wave module."""
import io
import wave

import numpy as np
import pytest

from mimic3_amd import postprocess as PP
from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError
from mimic3_amd.config import VitsConfig
from tests import resample_ref as R
from tests.test_packed_results import CHUNK, _chunks
from tests.test_resample import (FI, HOOK_RATES, RATES, check_accuracy, check_int16, check_kernel_alone, check_lengths_and_padding,
                                 check_native_untouched, check_rows_alone, run_at)

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE
B = 36


def _ragged(cfg, seed, B=B, lo=1, hi=96):
    rng = np.random.default_rng(seed)
    lens = rng.integers(8, hi + 1, B).astype(np.int64)
    lens[0], lens[B // 2] = hi, lo  # the longest row and a one-phoneme row
    ids = np.zeros((B, hi), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    scales = np.stack([rng.uniform(0.3, 0.9, B), rng.uniform(0.8, 1.3, B), rng.uniform(0.2, 1.0, B)], axis=1).astype(np.float32)
    vol = rng.choice([0.5, 1.0, 1.0, 1.5, 3.0], B)  # 3.0 clips
    vol[0], vol[B // 2] = 1.0, 1.0
    keys = [int(k) for k in rng.integers(0, 1 << 40, B)]
    return dict(ids=ids, lens=lens, sid=None, scales=scales, kw=dict(seed=SEED, utterance_keys=keys, pcm_volume=vol))


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
def test_ragged_batch_at_every_rate(gpu_lib, math):
    """Criteria 1 - 4 on 36 ragged rows of 1 .. 96 ids of apope_low's shape, natural durations, per-row scales / volumes / keys."""
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=141, frames_per_id=3.0)), device=0, library=gpu_lib)
    eng.set_math(math)
    a = _ragged(cfg, 141)
    native = check_native_untouched(eng, a)
    assert len({int(x) for x in native["lengths"]}) > B // 2
    volumes = [100.0 * float(v) for v in a["kw"]["pcm_volume"]]
    eng.profile_enable(True)
    for rate in RATES:
        eng.profile_reset()
        out = run_at(eng, rate, a)
        rep = eng.profile_report()
        assert rep["resample"]["calls"] == 1
        assert rep["resample"]["bytes"] == 4.0 * float(np.sum(native["lengths"])) + 4.0 * float(np.sum(out["lengths"]))
        print(f"resample -> {rate}: {rep['resample']['ms']:.4f} ms for {int(np.sum(out['lengths']))} samples")
        check_lengths_and_padding(out, native, rate)
        check_accuracy(out, native, rate)
        check_int16(out, native, rate, volumes)
    eng.set_output_rate(0)
    again = eng.fetch(want_float=True, want_pcm16=True)  # the last run, at the rate it ran at
    assert again["pcm"].tobytes() == out["pcm"].tobytes() and again["audio"].tobytes() == out["audio"].tobytes()
    back = run_at(eng, 0, a)
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert back[k].tobytes() == native[k].tobytes(), k
    eng.close()


@pytest.mark.parametrize("rate", [16000, 48000])
def test_batched_is_alone_and_on_a_nan_filled_workspace(gpu_hooks, rate):
    """Criterion 5: rows of the batch bitwise the rows alone; the same bytes on a workspace a larger call sized and a quiet NaN filled."""
    cfg = VitsConfig.apope_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=131, frames_per_id=3.0))
    a = _ragged(cfg, 131)
    fresh = Engine(blob, device=0, library=gpu_hooks)
    want = run_at(fresh, rate, a)
    fresh.close()
    check_rows_alone(lambda: Engine(blob, device=0, library=gpu_hooks), a, rate, want, [0, 1, B // 2, B - 1, 7])
    eng = Engine(blob, device=0, library=gpu_hooks)
    rng = np.random.default_rng(3)
    big = dict(ids=rng.integers(1, cfg.num_symbols, (B + 4, 96)), lens=np.full(B + 4, 96), sid=None, scales=[0.667, 1.0, 0.8],
               kw=dict(seed=1, forced_durations=np.full((B + 4, 96), 8, np.int32)))
    assert int(run_at(eng, rate, big)["l_max"]) > int(want["l_max"])  # sizes the workspace past what the ragged call needs
    eng.fill_workspace(0x7FC00000)
    got = run_at(eng, rate, a)
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert got[k].tobytes() == want[k].tobytes(), k
    eng.close()


def test_packed_stream_at_16_khz(gpu_lib):
    """Criterion 6 on the device."""
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=22, frames_per_id=3.0)), device=0, library=gpu_lib)
    a = _ragged(cfg, 22, B=6, hi=40)
    full = run_at(eng, 16000, a)
    order, lead, tail = [3, 0, 4, 1], [1, 0, 777, CHUNK + 453], 5
    pk = eng.run_packed(a["ids"], a["lens"], a["scales"], order=order, lead_samples=lead, tail_samples=tail, wav=True, **a["kw"])
    assert bytes(pk.wav) == PP.wav_bytes(_chunks(full, order, lead, tail), 16000) and pk.sample_rate == 16000
    mask = np.ones(pk.total_samples, bool)
    for i, b in enumerate(order):
        n = int(full["lengths"][b])
        assert int(pk.lengths[i]) == n and pk.rows[i].tobytes() == full["pcm"][b, :n].tobytes()
        mask[int(pk.offsets[i]): int(pk.offsets[i]) + n] = False
    assert not pk.pcm[mask].any()
    with wave.open(io.BytesIO(bytes(pk.wav)), "rb") as wf:
        assert (wf.getframerate(), wf.getnframes()) == (16000, pk.total_samples)
    eng.close()


@pytest.mark.parametrize("rate", HOOK_RATES)
def test_the_kernel_alone(gpu_hooks, rate):
    """Criterion 7 on the device: impulses bitwise the f32-rounded taps, noise / a 9.5 kHz tone / rows of 1, 2 and 37 samples."""
    check_kernel_alone(gpu_hooks, rate, n=70000)


def test_the_kernel_alone_at_the_largest_table_and_an_extreme_ratio(gpu_hooks):
    check_kernel_alone(gpu_hooks, 96000, n=20000)  # 640 phases: 70 KiB of LDS
    check_kernel_alone(gpu_hooks, 50, n=60000)     # 441 : 1, a phase of 8,821 taps


def test_bad_rates_and_clone(gpu_lib):
    """Criterion 8 on the device (the micro-batcher's grouping is host code: tests/test_resample.py)."""
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=5, frames_per_id=3.0)), device=0, library=gpu_lib)
    a = _ragged(cfg, 5, B=4, hi=24)
    before = run_at(eng, 16000, a)
    for hz, message in ((-1, r"output rate -1 Hz"), (22051, r"output rate 22051 Hz = 22051 / 22050")):
        with pytest.raises(NativeError, match=message) as e:
            eng.set_output_rate(hz)
        assert e.value.code == -1 and eng.output_rate == 16000
    lane = eng.clone()
    assert lane.output_rate == 16000
    for e in (eng, lane):
        after = run_at(e, None, a)
        assert after["pcm"].tobytes() == before["pcm"].tobytes() and after["audio"].tobytes() == before["audio"].tobytes()
    assert int(before["lengths"][0]) == R.out_len(int(run_at(eng, 0, a)["lengths"][0]), *R.ratio(FI, 16000))
    lane.close()
    eng.close()
