"""Device twin of tests/test_packed_encodings.py (pytest -m gpu): mi355vits_set_output_encoding and k_pack on the MI355X at
sizes a user runs.  The yardsticks are the device's own int16 packed stream and padded float rows (both older than the setting),
the committed audioop tables (tests/golden/g711_tables.npz) and the header builder of tests/g711_ref.py — neither audioop nor
scipy nor the reference is needed."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g711_ref as G  # noqa: E402

from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from tests.test_gpu_resample import _ragged as _ragged_case  # noqa: E402
from tests.test_packed_encodings import check_every_kernel_form  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE
G711_CHUNK = 4096
LAWS = ("ulaw", "alaw")
ENCODINGS = ("s16le", "ulaw", "alaw", "f32le")
ALL_INT16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)


@pytest.fixture(scope="module")
def tables():
    return G.tables()


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


def _float_stream(pk, audio, lengths, order):
    want = np.zeros(pk.total_samples, np.float32)
    for i, b in enumerate(order):
        n = int(lengths[b])
        assert int(pk.lengths[i]) == n
        want[int(pk.offsets[i]): int(pk.offsets[i]) + n] = audio[b, :n]
    return want


def _check_wav_header(b, encoding, rate, total):
    bps = G.BYTES_PER_SAMPLE[encoding]
    data = bps * total
    pad = data & 1
    assert len(b) == 58 + data + pad
    assert b[:4] == b"RIFF" and struct.unpack_from("<I", b, 4)[0] == 50 + data + pad and b[8:16] == b"WAVEfmt "
    assert struct.unpack_from("<IHHIIHHH", b, 16) == (18, G.FORMAT_TAG[encoding], 1, rate, rate * bps, bps, 8 * bps, 0)
    assert b[38:42] == b"fact" and struct.unpack_from("<II", b, 42) == (4, total)
    assert b[50:54] == b"data" and struct.unpack_from("<I", b, 54)[0] == data
    assert b[:58] == G.wav_header(encoding, rate, total) and b[58 + data:] == b"\0" * pad


@pytest.mark.parametrize("law", LAWS)
def test_device_encoders_over_every_int16_value(gpu_hooks, tables, law):
    got = gpu_hooks.lab_g711_encode(law, ALL_INT16)
    bad = np.nonzero(got != tables[law])[0]
    assert bad.size == 0, (law, [(int(ALL_INT16[i]), int(got[i]), int(tables[law][i])) for i in bad[:8]])


@pytest.mark.parametrize("rate", [None, 8000])
def test_48_ragged_rows_in_every_encoding(gpu_lib, tables, rate):
    """48 ragged rows of 20 .. 128 ids with natural durations, noise on, per-row scales, volumes and keys, at the voice's rate and
    at 8000 Hz: a permutation with silences behind a header in all four encodings, against the device's own int16 stream and float
    rows, bitwise; then the same run served again by fetch_packed in each encoding."""
    cfg = VitsConfig.vctk_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=141, frames_per_id=3.0)), device=0, library=gpu_lib)
    eng.set_output_rate(rate)
    hz = rate or cfg.sample_rate
    B = 48
    ids, lens, sid, scales, vol, keys = _ragged(cfg, B, 20, 128, seed=141)
    kw = dict(seed=SEED, utterance_keys=keys, pcm_volume=vol)
    full = eng.run(ids, lens, scales, sid, want_float=True, want_pcm16=True, **kw)
    audio, pcm, lengths = full["audio"].copy(), full["pcm"].copy(), full["lengths"].copy()
    assert len({int(x) for x in lengths}) > B // 2
    rng = np.random.default_rng(7)
    order = [int(b) for b in rng.permutation(B) if b != 17]
    lead = [int(x) for x in rng.integers(0, 3 * G711_CHUNK, len(order))]
    lead[:4] = [0, 1, 777, G711_CHUNK + 453]
    spec = dict(order=order, lead_samples=lead, tail_samples=2205 + (1 if rate else 0), wav=True)
    streams = {}
    for enc in ENCODINGS:
        eng.set_output_encoding(enc)
        streams[enc] = eng.run_packed(ids, lens, scales, sid, **spec, **kw)
        assert streams[enc].encoding == enc and streams[enc].sample_rate == hz
    s16 = streams["s16le"]
    assert len(s16.wav) == 44 + 2 * s16.total_samples
    for i, b in enumerate(order):
        assert np.array_equal(s16.rows[i], pcm[b, : int(lengths[b])])  # the int16 stream is what it was: the padded call's rows
    gap = np.ones(s16.total_samples, bool)
    for o, n in zip(s16.offsets, s16.lengths):
        gap[int(o): int(o) + int(n)] = False
    assert gap.sum() == sum(lead) + spec["tail_samples"]
    for enc in ("ulaw", "alaw", "f32le"):
        pk = streams[enc]
        assert pk.total_samples == s16.total_samples
        for k in ("offsets", "lengths", "peaks"):
            assert getattr(pk, k).tobytes() == getattr(s16, k).tobytes(), (enc, k)
        _check_wav_header(bytes(pk.wav), enc, hz, pk.total_samples)
    for law in LAWS:
        assert np.array_equal(streams[law].data, G.encode(tables[law], s16.pcm)), law
        assert (streams[law].data[gap] == G.SILENCE[law]).all()
    f32 = streams["f32le"]
    assert f32.data.tobytes() == _float_stream(f32, audio, lengths, order).tobytes()
    assert not f32.data[gap].view(np.uint32).any()
    # one synthesis, every encoding again: s16 -> ulaw -> alaw -> f32
    eng.set_output_encoding("s16le")
    eng.run(ids, lens, scales, sid, want_float=False, want_pcm16=True, **kw)
    for enc in ENCODINGS:
        eng.set_output_encoding(enc)
        got = eng.fetch_packed(**spec)
        assert got.encoding == enc and bytes(got.wav) == bytes(streams[enc].wav), enc
    again = eng.fetch(want_float=True, want_pcm16=True)  # the padded results are not touched by the setting
    assert again["audio"].tobytes() == audio.tobytes() and again["pcm"].tobytes() == pcm.tobytes()
    eng.close()


def test_headline_shape_in_every_encoding_and_the_profile_lines(gpu_lib, tables):
    """256 rows x 128 ids x 6 forced frames (the benchmark's headline): each encoded stream against the int16 stream / the float
    rows; the profile report names the kernel of the encoding with 4 x sum(lengths) + bytes_per_sample x total_samples bytes."""
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0)), device=0, library=gpu_lib)
    B, Tx = 256, 128
    rng = np.random.default_rng(1)
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    lens = np.full(B, Tx, np.int64)
    forced = np.full((B, Tx), 6, np.int32)
    sc = [0.667, 1.0, 0.8]
    full = eng.run(ids, lens, sc, forced_durations=forced, seed=1, want_float=True, want_pcm16=True)
    audio, pcm = full["audio"].copy(), full["pcm"].copy()
    n_audio = float(np.sum(full["lengths"]))
    del full
    eng.profile_enable(True)
    labels = {"s16le": "pcm16.pack", "ulaw": "pack.ulaw", "alaw": "pack.alaw", "f32le": "pack.f32"}
    for enc in ENCODINGS:
        eng.set_output_encoding(enc)
        eng.profile_reset()
        pk = eng.fetch_packed()
        rep = eng.profile_report()
        assert [k for k in rep if k in labels.values()] == [labels[enc]], sorted(rep)
        assert rep[labels[enc]]["calls"] == 1
        assert rep[labels[enc]]["bytes"] == 4.0 * n_audio + float(pk.data.dtype.itemsize) * pk.total_samples
        print(f"{labels[enc]} at the headline shape: {rep[labels[enc]]['ms']:.4f} ms")
        assert pk.total_samples == pcm.size
        if enc == "s16le":
            assert np.array_equal(pk.pcm.reshape(B, -1), pcm)
        elif enc == "f32le":
            assert pk.data.tobytes() == audio.tobytes()
        else:
            assert np.array_equal(pk.data.reshape(B, -1), G.encode(tables[enc], pcm))
    eng.profile_enable(False)
    eng.close()


def test_encoded_streams_on_a_nan_filled_workspace(gpu_hooks, tables):
    """apope_low, 24 ragged rows, on a handle whose workspace a larger float-stream call sized first and a quiet NaN then filled:
    the same bytes as a fresh handle's in every encoding (the silences are 0xFF / 0xD5 / 0.0f because the kernel wrote them)."""
    cfg = VitsConfig.apope_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=131, frames_per_id=3.0))
    rng = np.random.default_rng(131)
    B, Tx = 24, 64
    lengths = rng.integers(1, Tx + 1, B)
    lengths[0], lengths[5] = Tx, 1
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    scales = [0.667, 1.0, 0.8]
    order = [int(b) for b in rng.permutation(B)]
    lead = [int(x) for x in rng.integers(0, 2 * G711_CHUNK, B)]
    spec = dict(order=order, lead_samples=lead, tail_samples=4097, wav=True)
    kw = dict(seed=SEED, pcm_volume=np.linspace(0.5, 3.0, B))
    fresh = Engine(blob, device=0, library=gpu_hooks)
    s16 = fresh.run_packed(ids, lengths, scales, **spec, **kw)
    want = {"s16le": bytes(s16.wav)}
    for enc in ("ulaw", "alaw", "f32le"):
        fresh.set_output_encoding(enc)
        want[enc] = bytes(fresh.fetch_packed(**spec).wav)
    for law in LAWS:
        assert want[law][58: 58 + s16.total_samples] == G.encode(tables[law], s16.pcm).tobytes()
    fresh.close()
    eng = Engine(blob, device=0, library=gpu_hooks)
    eng.set_output_encoding("f32le")
    big = eng.run_packed(rng.integers(1, cfg.num_symbols, (B + 4, Tx)), np.full(B + 4, Tx), scales,
                         forced_durations=np.full((B + 4, Tx), 8, np.int32), lead_samples=[4 * G711_CHUNK] * (B + 4),
                         tail_samples=8 * G711_CHUNK)  # sizes the workspace past what the ragged call needs
    assert 4 * big.total_samples > len(want["f32le"])
    del big
    for enc in ("ulaw", "alaw", "f32le"):
        eng.set_output_encoding(enc)
        eng.fill_workspace(0x7FC00000)
        assert bytes(eng.run_packed(ids, lengths, scales, **spec, **kw).wav) == want[enc], enc
    eng.fill_workspace(0x7FC00000)
    eng.run(ids, lengths, scales, device_only=True, **kw)
    for enc in ENCODINGS:
        eng.set_output_encoding(enc)
        assert bytes(eng.fetch_packed(**spec).wav) == want[enc], enc
    eng.close()


def test_every_kernel_form(gpu_lib, tables):
    """All sixteen forms of the packing kernel (encoding x trimmed x normalised) on the device: six ragged rows of up to 40 ids of
    the released single-speaker voice's shape, one synthesis, sixteen packs (tests/test_packed_encodings.py)."""
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=151, frames_per_id=3.0)), device=0, library=gpu_lib)
    assert len(check_every_kernel_form(eng, _ragged_case(cfg, 17, B=6, hi=40), tables)) == 16
    eng.close()
