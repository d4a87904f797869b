"""The sample encoding of the packed stream (mi355vits_set_output_encoding; k_pack in csrc/kernels_pack.cpp): G.711
mu-law / A-law bytes or the float samples themselves instead of int16, written by the kernel that packs.  On the CPU model of
the kernels (tests/emu); test_gpu_packed_encodings.py runs the same contract on the MI355X.

Yardsticks, never the code under test: the int16 packed stream and the padded float rows of the SAME engine (both existed
before this setting), CPython's audioop as committed tables (tests/golden/g711_tables.npz, tools/make_g711_tables.py), the
numpy restatement and header builder of tests/g711_ref.py, and scipy.io.wavfile where it imports."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g711_ref as G  # noqa: E402

from mimic3_amd import postprocess as PP  # noqa: E402
from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine, NativeError  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from mimic3_amd.session import InferenceSession  # noqa: E402

SEED = 0xC0FFEE
SCALES = np.array([[0.667, 1.0, 0.8], [0.0, 1.6, 0.0], [0.5, 0.7, 0.3], [0.9, 1.2, 1.1], [0.333, 0.85, 0.0]], np.float32)
KEYS = [7, 1_000_003, 42, (1 << 40) + 5, 3]
VOLUMES = [50.0, 100.0, 150.0, 300.0, 7.5]  # percent; 300 % clips
G711_CHUNK = 4096  # output samples of one work item of k_pack in the G.711 forms (256 lanes x 16); the float form: 1024
DEFAULT_CUS = 8
LAWS = ("ulaw", "alaw")
ALL_INT16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
# a permutation without row 2; silences of 1, 0, an odd count and more than a work item: rows start at odd offsets, and one
# lane's 16 samples hold a row's end, a silence and the next row's start
ORDER, LEAD, TAIL = [3, 0, 4, 1], [1, 0, 777, G711_CHUNK + 453], 5


@pytest.fixture(scope="module")
def tables():
    return G.tables()


@pytest.fixture
def cu_count(emu_lib):
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(DEFAULT_CUS)


def _inputs(cfg, B, Tx, seed, one_phoneme_row=None):
    rng = np.random.default_rng(seed)
    lens = np.array([Tx] + list(rng.integers(2, Tx, size=B - 1)), np.int64)
    if one_phoneme_row is not None:
        lens[one_phoneme_row] = 1
    ids = np.zeros((B, Tx), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    sid = (np.arange(B) % cfg.n_speakers).astype(np.int64) if cfg.is_multispeaker else None
    return ids, lens, sid


def _engine(emu_lib, seed, n_speakers=1, **kw):
    cfg = VitsConfig.tiny(n_speakers=n_speakers) if n_speakers > 1 else VitsConfig.tiny()
    return cfg, Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=seed, **kw)), library=emu_lib)


def _gap_mask(pk):
    """True at every sample of the stream that belongs to no entry."""
    gap = np.ones(pk.total_samples, bool)
    for o, n in zip(pk.offsets, pk.lengths):
        gap[int(o): int(o) + int(n)] = False
    return gap


def _same_layout(a, b):
    assert a.total_samples == b.total_samples
    for k in ("offsets", "lengths", "peaks"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def _packed_in(eng, encoding, *args, **kw):
    eng.set_output_encoding(encoding)
    assert eng.output_encoding == encoding
    pk = eng.run_packed(*args, **kw)
    assert pk.encoding == encoding
    return pk


# ---------------------------------------------------------------------------------------------- the encoders themselves
def test_tables_are_the_numpy_restatement_and_audioop(tables):
    assert tables["ulaw"].shape == tables["alaw"].shape == (65536,) and tables["ulaw"].dtype == np.uint8
    assert np.array_equal(G.lin2ulaw(ALL_INT16), tables["ulaw"])
    assert np.array_equal(G.lin2alaw(ALL_INT16), tables["alaw"])
    assert tables["ulaw"][32768] == G.SILENCE["ulaw"] and tables["alaw"][32768] == G.SILENCE["alaw"]
    assert np.array_equal(G.encode(tables["ulaw"], ALL_INT16), tables["ulaw"])
    try:
        import audioop
    except ImportError:
        pytest.skip("audioop is not in this interpreter: the committed tables stand in for it")
    assert audioop.lin2ulaw(ALL_INT16.astype("<i2").tobytes(), 2) == tables["ulaw"].tobytes()
    assert audioop.lin2alaw(ALL_INT16.astype("<i2").tobytes(), 2) == tables["alaw"].tobytes()


@pytest.mark.parametrize("law", LAWS)
def test_device_encoders_over_every_int16_value(emu_lib, tables, law):
    got = emu_lib.lab_g711_encode(law, ALL_INT16)
    bad = np.nonzero(got != tables[law])[0]
    assert bad.size == 0, (law, [(int(ALL_INT16[i]), int(got[i]), int(tables[law][i])) for i in bad[:8]])
    with pytest.raises(NativeError):
        emu_lib.lab_g711_encode(3, ALL_INT16[:4])  # f32le is no law


def test_postprocess_companders_are_the_tables(tables):
    assert np.array_equal(PP.lin2ulaw(ALL_INT16), tables["ulaw"])
    assert np.array_equal(PP.lin2alaw(ALL_INT16), tables["alaw"])
    assert PP.lin2ulaw(ALL_INT16).dtype == np.uint8


# ---------------------------------------------------------------------------------------------- the streams
@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("rate", [None, 8000])
@pytest.mark.parametrize("n_speakers", [1, 4])
def test_g711_streams_are_the_codes_of_the_int16_stream(emu_lib, tables, math, rate, n_speakers):
    cfg, eng = _engine(emu_lib, 22, n_speakers)
    eng.set_math(math)
    eng.set_output_rate(rate)
    ids, lens, sid = _inputs(cfg, 5, 12, seed=22, one_phoneme_row=1)
    kw = dict(order=ORDER, lead_samples=LEAD, tail_samples=TAIL, seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0)
    s16 = _packed_in(eng, "s16le", ids, lens, SCALES, sid, **kw)
    assert any(int(o) % 2 for o in s16.offsets) and any(int(o) % 16 for o in s16.offsets) and int(lens[1]) == 1
    assert np.abs(s16.pcm).max() == 32767  # the 300 % row clips: the codes are those of the samples AFTER the volume
    gap = _gap_mask(s16)
    assert gap.sum() == sum(LEAD) + TAIL and not s16.pcm[gap].any()
    for law in LAWS:
        pk = _packed_in(eng, law, ids, lens, SCALES, sid, **kw)
        assert pk.data.dtype == np.uint8 and pk.data.shape == (s16.total_samples,) and pk.wav is None
        assert np.array_equal(pk.data, G.encode(tables[law], s16.pcm)), law
        assert (pk.data[gap] == G.SILENCE[law]).all()
        _same_layout(pk, s16)
        assert pk.sample_rate == (rate or cfg.sample_rate)
        for i in range(len(ORDER)):
            assert np.array_equal(pk.rows[i], G.encode(tables[law], s16.rows[i])) and np.shares_memory(pk.rows[i], pk.data)
        with pytest.raises(ValueError, match="not int16 PCM"):
            pk.pcm
    eng.close()


@pytest.mark.parametrize("rate", [None, 8000])
@pytest.mark.parametrize("n_speakers", [1, 4])
def test_f32_stream_holds_the_float_rows_bitwise(emu_lib, rate, n_speakers):
    cfg, eng = _engine(emu_lib, 23, n_speakers)
    eng.set_output_rate(rate)
    hz = rate or cfg.sample_rate
    ids, lens, sid = _inputs(cfg, 5, 12, seed=23, one_phoneme_row=1)
    kw = dict(seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0)
    spec = dict(order=ORDER, lead_samples=LEAD, tail_samples=TAIL)
    full = eng.run(ids, lens, SCALES, sid, want_float=True, **kw)
    s16 = _packed_in(eng, "s16le", ids, lens, SCALES, sid, **spec, **kw)
    pk = _packed_in(eng, "f32le", ids, lens, SCALES, sid, wav=True, **spec, **kw)
    assert pk.data.dtype == np.float32
    _same_layout(pk, s16)
    for i, b in enumerate(ORDER):
        n = int(full["lengths"][b])
        assert pk.rows[i].tobytes() == full["audio"][b, :n].tobytes(), (i, b)  # neither normalised nor scaled by the volume
    gap = _gap_mask(pk)
    assert not pk.data[gap].view(np.uint32).any()  # +0.0f, bit for bit
    want = np.zeros(pk.total_samples, np.float32)
    for i, b in enumerate(ORDER):
        want[int(pk.offsets[i]): int(pk.offsets[i]) + int(pk.lengths[i])] = full["audio"][b, : int(pk.lengths[i])]
    assert bytes(pk.wav) == G.wav_file("f32le", hz, want)
    assert bytes(pk.wav) == PP.wav_bytes([want], hz, "f32le")
    assert len(pk.wav) == 58 + 4 * pk.total_samples
    try:
        from scipy.io import wavfile
    except ImportError:
        wavfile = None
    if wavfile is not None:
        buf = io.BytesIO()
        wavfile.write(buf, hz, want)
        assert buf.getvalue() == bytes(pk.wav)
        got_rate, got = wavfile.read(io.BytesIO(bytes(pk.wav)))
        assert got_rate == hz and got.dtype == np.float32 and got.tobytes() == want.tobytes()
    eng.close()


@pytest.mark.parametrize("law", LAWS)
def test_non_pcm_wav_header_field_by_field(emu_lib, tables, law):
    cfg, eng = _engine(emu_lib, 24)
    ids, lens, sid = _inputs(cfg, 3, 9, seed=24)
    kw = dict(seed=SEED, utterance_keys=KEYS[:3])
    seen = set()
    for tail in (4, 5):  # one even and one odd total_samples: without and with the pad byte
        s16 = _packed_in(eng, "s16le", ids, lens, SCALES[:3], sid, lead_samples=[3, 0, 10], tail_samples=tail, **kw)
        pk = _packed_in(eng, law, ids, lens, SCALES[:3], sid, lead_samples=[3, 0, 10], tail_samples=tail, wav=True, **kw)
        total = pk.total_samples
        pad = total & 1
        seen.add(pad)
        b = bytes(pk.wav)
        assert len(b) == 58 + total + pad
        assert b[0:4] == b"RIFF" and struct.unpack_from("<I", b, 4)[0] == 50 + total + pad == len(b) - 8
        assert b[8:12] == b"WAVE" and b[12:16] == b"fmt "
        size, tag, channels, rate, byte_rate, align, bits, cb = struct.unpack_from("<IHHIIHHH", b, 16)
        assert (size, tag, channels, rate, byte_rate, align, bits, cb) == (18, G.FORMAT_TAG[law], 1, cfg.sample_rate, cfg.sample_rate, 1, 8, 0)
        assert b[38:42] == b"fact" and struct.unpack_from("<II", b, 42) == (4, total)
        assert b[50:54] == b"data" and struct.unpack_from("<I", b, 54)[0] == total  # the pad byte is not data
        assert b[58: 58 + total] == pk.data.tobytes() == G.encode(tables[law], s16.pcm).tobytes()
        assert b[58 + total:] == b"\0" * pad
        assert b == G.wav_file(law, cfg.sample_rate, pk.data) == PP.wav_bytes([pk.data], cfg.sample_rate, law)
    assert seen == {0, 1}
    eng.close()


def test_fetch_packed_serves_one_run_in_every_encoding(emu_lib, tables):
    cfg, eng = _engine(emu_lib, 25, n_speakers=4)
    ids, lens, sid = _inputs(cfg, 5, 12, seed=25)
    kw = dict(seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0)
    spec = dict(order=ORDER, lead_samples=LEAD, tail_samples=TAIL, wav=True)
    fresh = {enc: bytes(_packed_in(eng, enc, ids, lens, SCALES, sid, **spec, **kw).wav) for enc in ("s16le", "ulaw", "alaw", "f32le")}
    assert len({len(v) for v in fresh.values()}) == 3
    eng.set_output_encoding("s16le")
    full = eng.run(ids, lens, SCALES, sid, want_pcm16=True, **kw)  # one synthesis; everything below packs it again
    padded = {k: full[k].copy() for k in ("pcm", "audio", "lengths", "peaks")}
    for enc in ("s16le", "ulaw", "alaw", "f32le", "ulaw", "s16le"):
        eng.set_output_encoding(enc)
        got = eng.fetch_packed(**spec)
        assert got.encoding == enc and bytes(got.wav) == fresh[enc], enc
        between = eng.fetch(want_float=True, want_pcm16=True)  # the padded results are not touched by the setting
        for k in padded:
            assert between[k].tobytes() == padded[k].tobytes(), (enc, k)
    eng.close()


def test_fetch_packed_float_stream_outgrows_the_last_runs_workspace(emu_lib):
    """The stream is sized in BYTES: a float stream of 0.7 M samples does not fit the slack behind the last run's layout."""
    cfg, eng = _engine(emu_lib, 27)
    ids, lens, sid = _inputs(cfg, 5, 12, seed=27)
    full = eng.run(ids, lens, SCALES, sid, seed=SEED, utterance_keys=KEYS)
    audio = full["audio"].copy()
    order, lead, tail = [4, 1], [300_001, 150_003], 250_000
    eng.set_output_encoding("f32le")
    for _ in range(2):
        got = eng.fetch_packed(order=order, lead_samples=lead, tail_samples=tail)
        want = np.zeros(got.total_samples, np.float32)
        for i, b in enumerate(order):
            want[int(got.offsets[i]): int(got.offsets[i]) + int(got.lengths[i])] = audio[b, : int(full["lengths"][b])]
        assert got.data.tobytes() == want.tobytes()
        assert eng.fetch(want_float=True)["audio"].tobytes() == audio.tobytes()
    eng.close()


def test_default_and_explicit_s16le_are_the_int16_stream_and_a_clone_inherits(emu_lib, tables):
    cfg, eng = _engine(emu_lib, 26)
    ids, lens, sid = _inputs(cfg, 5, 12, seed=26)
    kw = dict(seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0)
    spec = dict(order=ORDER, lead_samples=LEAD, tail_samples=TAIL, wav=True)
    assert eng.output_encoding == "s16le"  # never set
    full = eng.run(ids, lens, SCALES, sid, want_pcm16=True, **kw)
    parts = []
    for i, b in enumerate(ORDER):
        parts += [np.zeros(LEAD[i], np.int16), full["pcm"][b, : int(full["lengths"][b])]]
    want = PP.wav_bytes(parts + [np.zeros(TAIL, np.int16)], cfg.sample_rate)  # the 44-byte PCM file, as before the setting existed
    eng.profile_enable(True)
    default = eng.run_packed(ids, lens, SCALES, sid, **spec, **kw)
    labels = set(eng.profile_report())
    assert "pcm16.pack" in labels and not any(x.startswith("pack.") for x in labels)
    assert bytes(default.wav) == want and default.encoding == "s16le" and default.pcm is default.data
    eng.set_output_encoding("ulaw")
    lane = eng.clone()
    assert lane.output_encoding == "ulaw"
    eng.profile_reset()
    mu = eng.run_packed(ids, lens, SCALES, sid, **spec, **kw)
    labels = set(eng.profile_report())
    assert "pack.ulaw" in labels and "pcm16.pack" not in labels
    assert bytes(lane.run_packed(ids, lens, SCALES, sid, **spec, **kw).wav) == bytes(mu.wav)
    eng.set_output_encoding("s16le")
    assert lane.output_encoding == "ulaw"  # a lane's setting is its own afterwards
    assert bytes(eng.run_packed(ids, lens, SCALES, sid, **spec, **kw).wav) == want
    assert np.array_equal(mu.data, G.encode(tables["ulaw"], default.pcm))
    lane.close()
    eng.close()


def test_bad_encoding_and_riff_limit(emu_lib):
    cfg, eng = _engine(emu_lib, 28)
    ids, lens, sid = _inputs(cfg, 3, 9, seed=28)
    kw = dict(seed=SEED, utterance_keys=KEYS[:3])
    eng.set_output_encoding("alaw")
    for bad in (4, -1, 77):
        with pytest.raises(NativeError, match=r"output encoding %d\b" % bad) as e:
            eng.set_output_encoding(bad)
        assert e.value.code == -1 and eng.output_encoding == "alaw"
    with pytest.raises(ValueError, match="unknown output encoding 'mp3'"):
        eng.set_output_encoding("mp3")
    assert eng.output_encoding == "alaw"
    before = eng.run(ids, lens, SCALES[:3], sid, want_pcm16=True, **kw)
    # 2^30 float samples of silence fit the sample cap but not RIFF's 32-bit size: refused from the silences alone, before synthesis
    eng.set_output_encoding("f32le")
    big = 1 << 30
    for spec, message in ((dict(order=[0], lead_samples=[big], wav=True), r"pack entry 0: WAV data size does not fit RIFF's 32-bit fields \(50 \+ 4 \* total_samples > 2\^32 - 1\)"),
                          (dict(tail_samples=big, wav=True), r"pack: WAV data size does not fit RIFF's 32-bit fields \(50 \+ 4 \* total_samples")):
        for call in (lambda: eng.run_packed(ids, lens, SCALES[:3], sid, **spec, **kw), lambda: eng.fetch_packed(**spec)):
            with pytest.raises(NativeError, match=message) as e:
                call()
            assert e.value.code == -1
    # (a G.711 file of any permitted sample count fits: 50 + 2^31 - 1 + 1 < 2^32.)  The int16 limit and its message are what they were
    eng.set_output_encoding("s16le")
    with pytest.raises(NativeError, match=r"36 \+ 2 \* total_samples > 2\^32 - 1"):
        eng.fetch_packed(tail_samples=2 ** 31 - 10, wav=True)
    after = eng.run(ids, lens, SCALES[:3], sid, want_pcm16=True, **kw)
    for k in ("lengths", "audio", "pcm", "peaks"):
        assert after[k].tobytes() == before[k].tobytes(), k
    eng.close()


# ---------------------------------------------------------------------------------------------- robustness
POISON = [0x7FC00000, 0xFFFFFFFF, 0x7F800000, 0x7F7FFFFF]  # qNaN, a negative NaN with every mantissa bit, +Inf, the largest float
POISON_ROWS = [24, 3, 13, 1, 0, 17, 9]  # an empty row has one silent frame


def _forced_batch(cfg, lengths, Tx, frames, seed):
    lengths = np.asarray(lengths, np.int64)
    B = len(lengths)
    rng = np.random.default_rng(seed)
    return dict(ids=rng.integers(1, cfg.num_symbols, (B, Tx)), lengths=lengths, forced=np.full((B, Tx), frames, np.int32),
                nw=rng.standard_normal((B, 2, Tx)).astype(np.float32),
                nz=rng.standard_normal((B, cfg.inter_channels, Tx * frames)).astype(np.float32))


def _packed(eng, bt, **spec):
    return eng.run_packed(bt["ids"], bt["lengths"], [0.667, 1.0, 0.8], forced_durations=bt["forced"], noise_w=bt["nw"], noise_z=bt["nz"],
                          pcm_volume=np.linspace(0.5, 3.0, len(bt["lengths"])), **spec)


def test_encoded_streams_on_a_poisoned_workspace(emu_lib, tables):
    """The whole workspace filled with NaN, Inf or the largest float before a ragged packed call: the same bytes as a fresh
    handle's.  A LARGER float-stream call sizes the workspace first, so the poisoned calls cannot reallocate (and zero) it."""
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=91, frames_per_id=2.0))
    bt = _forced_batch(cfg, POISON_ROWS, Tx=24, frames=2, seed=12)
    big = _forced_batch(cfg, [24] * (len(POISON_ROWS) + 2), Tx=24, frames=2, seed=5)
    n = len(POISON_ROWS)
    spec = dict(order=[6, 4, 0, 2, 5, 1, 3], lead_samples=[7, 0, 1, G711_CHUNK + 3, 129, 64, 5], tail_samples=1001, wav=True)
    fresh = Engine(blob, library=emu_lib)
    want = {}
    for enc in ("s16le", "ulaw", "alaw", "f32le"):
        fresh.set_output_encoding(enc)
        want[enc] = bytes(_packed(fresh, bt, **spec).wav)
    fresh.close()
    for law in LAWS:
        assert want[law][58: 58 + (len(want["s16le"]) - 44) // 2] == G.encode(tables[law], np.frombuffer(want["s16le"][44:], "<i2")).tobytes()
    eng = Engine(blob, library=emu_lib)
    eng.set_output_encoding("f32le")
    bigger = _packed(eng, big, lead_samples=[3 * G711_CHUNK] * (n + 2), tail_samples=4 * G711_CHUNK, wav=True)
    assert 4 * bigger.total_samples > 2 * len(want["f32le"])
    del bigger
    for pattern, enc in zip(POISON, ("ulaw", "alaw", "f32le", "ulaw")):
        eng.set_output_encoding(enc)
        eng.fill_workspace(pattern)
        assert bytes(_packed(eng, bt, **spec).wav) == want[enc], (hex(pattern), enc)
        eng.fill_workspace(pattern)  # ... and packed again from the float audio that run left, onto poison as well
        eng.run(bt["ids"], bt["lengths"], [0.667, 1.0, 0.8], forced_durations=bt["forced"], noise_w=bt["nw"], noise_z=bt["nz"],
                pcm_volume=np.linspace(0.5, 3.0, n), device_only=True)
        for other in ("alaw", "f32le", "ulaw"):
            eng.set_output_encoding(other)
            assert bytes(eng.fetch_packed(**spec).wav) == want[other], (hex(pattern), other)
    eng.close()


def test_encoded_streams_do_not_depend_on_the_cu_count(emu_lib, cu_count, tables):
    """k_pack's persistent grid is sized by the compute units: 1, 7 and 256 of them give the default count's bytes — fewer
    workgroups than work items, more than work items, and far more."""
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=33))
    B, Tx = 12, 16
    rng = np.random.default_rng(33)
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    lens = np.array([Tx] + list(rng.integers(Tx // 2, Tx, size=B - 1)), np.int64)
    forced = rng.integers(30, 81, (B, Tx)).astype(np.int32)
    order = [int(b) for b in rng.permutation(B)]
    lead = [int(x) for x in rng.integers(0, 700, B)]
    lead[0], lead[5] = 0, 1
    scales = np.tile(np.array([0.667, 1.0, 0.8], np.float32), (B, 1))
    kw = dict(forced_durations=forced, seed=SEED, utterance_keys=1000 + np.arange(B), pcm_volume=np.linspace(0.4, 3.0, B))
    spec = dict(order=order, lead_samples=lead, tail_samples=11, wav=True)
    want = None
    for cus in (DEFAULT_CUS, 1, 7, 256):
        cu_count(cus)
        eng = Engine(blob, library=emu_lib)
        got = {"ulaw": bytes(_packed_in(eng, "ulaw", ids, lens, scales, **spec, **kw).wav)}
        for enc in ("alaw", "f32le", "s16le"):
            eng.set_output_encoding(enc)
            got[enc] = bytes(eng.fetch_packed(**spec).wav)
        if want is None:
            want = got
            items = -(-(len(got["ulaw"]) - 58) // G711_CHUNK)
            assert items >= 10 and items % 7 and items > 8  # more work items than the one-CU grid has workgroups
            s16 = np.frombuffer(got["s16le"][44:], "<i2")
            for law in LAWS:
                assert got[law][58: 58 + s16.size] == G.encode(tables[law], s16).tobytes()
        assert got == want, cus
        eng.close()


# ---------------------------------------------------------------------------------------------- every form of the kernel
KERNEL_FORM_LEADS = [1, 7, 13, 0, 5, 3, 9, 11]  # with a hop that is a multiple of 8, every entry but the fourth starts at an odd offset
KERNEL_FORM_TAIL = 3
KERNEL_FORM_TRIM, KERNEL_FORM_TARGET = (0.9, 3), (-23.0, -1.0)
KERNEL_FORM_ENCODINGS = ("s16le", "ulaw", "alaw", "f32le")
SILENCE_BITS = {"s16le": 0, "ulaw": G.SILENCE["ulaw"], "alaw": G.SILENCE["alaw"], "f32le": 0}


def _kernel_form_streams(eng, a):
    """ONE synthesis of the batch `a` on `eng`, then a fetch_packed in each of the sixteen forms — a permuted order, odd leading
    silences, a tail, no header: (the pack arguments, the run's lengths per entry, {(encoding, trimmed, normalised): PackedAudio})."""
    n = len(a["lens"])
    assert n <= len(KERNEL_FORM_LEADS)
    order = [int(b) for b in np.random.default_rng(n).permutation(n)]
    assert order != sorted(order)
    spec = dict(order=order, lead_samples=KERNEL_FORM_LEADS[:n], tail_samples=KERNEL_FORM_TAIL)
    eng.set_edge_trim(0.0)
    eng.set_loudness_target(None)
    full = eng.run(a["ids"], a["lens"], a["scales"], a.get("sid"), want_float=False, **a["kw"])
    lengths = [int(full["lengths"][b]) for b in order]
    got = {}
    for enc in KERNEL_FORM_ENCODINGS:
        eng.set_output_encoding(enc)
        for trim in (False, True):
            eng.set_edge_trim(*(KERNEL_FORM_TRIM if trim else (0.0,)))
            for norm in (False, True):
                eng.set_loudness_target(*(KERNEL_FORM_TARGET if norm else (None,)))
                got[enc, trim, norm] = pk = eng.fetch_packed(**spec)
                assert pk.encoding == enc and pk.wav is None
    eng.set_edge_trim(0.0)
    eng.set_loudness_target(None)
    eng.set_output_encoding("s16le")
    return spec, lengths, got


def check_every_kernel_form(eng, a, tables):
    """The packing kernel is one template over (encoding, trimmed, normalised): sixteen forms.  One synthesis of the batch `a` on
    `eng` and a fetch_packed in each form (_kernel_form_streams), and bit for bit:
      * early against late route: the plain stream of each encoding is what run_packed returns on a fresh lane;
      * trimmed against untrimmed: entry i is [first[i], end[i]) of the untrimmed entry of the same encoding and target, and
        offsets / lengths are the running sums of the leads and end - first;
      * the G.711 entries of every trim / target setting are the table codes of the int16 entries of the same setting;
      * every sample outside the entries holds the encoding's silence code.
    Returns {(encoding, trimmed, normalised): the stream's bytes}."""
    encodings = KERNEL_FORM_ENCODINGS
    spec, lengths, got = _kernel_form_streams(eng, a)
    n, lead = len(lengths), spec["lead_samples"]
    # silence: every sample that belongs to no entry
    for (enc, trim, norm), pk in got.items():
        gap = _gap_mask(pk)
        bits = pk.data.view(np.uint32) if enc == "f32le" else pk.data
        assert gap.sum() == sum(lead) + KERNEL_FORM_TAIL and (bits[gap] == SILENCE_BITS[enc]).all(), (enc, trim, norm)
    # early against late route
    fresh = Engine(eng)  # another lane: no completed run, the same weights
    fresh.set_edge_trim(0.0)
    fresh.set_loudness_target(None)
    for enc in encodings:
        early = _packed_in(fresh, enc, a["ids"], a["lens"], a["scales"], a.get("sid"), **spec, **a["kw"])
        late = got[enc, False, False]
        assert early.data.tobytes() == late.data.tobytes(), enc
        _same_layout(early, late)
        assert [int(x) for x in late.lengths] == lengths
    fresh.close()
    # trimmed against untrimmed
    shorter = 0
    for enc in encodings:
        for norm in (False, True):
            whole, cut = got[enc, False, norm], got[enc, True, norm]
            first, end = cut.first.astype(np.int64), cut.end.astype(np.int64)
            pos, offsets = 0, []
            for i in range(n):
                assert cut.rows[i].tobytes() == whole.rows[i][int(first[i]): int(end[i])].tobytes(), (enc, norm, i)
                offsets.append(pos + lead[i])
                pos = offsets[-1] + int(end[i] - first[i])
            assert [int(x) for x in cut.offsets] == offsets and [int(x) for x in cut.lengths] == [int(x) for x in end - first]
            assert cut.total_samples == pos + KERNEL_FORM_TAIL
            shorter += cut.total_samples < whole.total_samples
    assert shorter == 8  # (the batch's side) trimming at 0.9 of the peak takes something away
    # G.711 codes of the int16 entries of the same setting
    for trim in (False, True):
        for norm in (False, True):
            s16 = got["s16le", trim, norm]
            for law in LAWS:
                pk = got[law, trim, norm]
                _same_layout(pk, s16)
                assert np.array_equal(pk.data, G.encode(tables[law], s16.pcm)), (law, trim, norm)
    assert got["s16le", False, True].data.tobytes() != got["s16le", False, False].data.tobytes()  # the target does something
    return {k: v.data.tobytes() for k, v in got.items()}


def _kernel_form_batch(cfg):
    """Forced durations on the tiny voice (hop 8): a row of one phoneme x one frame — 8 samples: exactly one int16 lane store,
    half a G.711 one, two float ones —, a row of 4,224 samples — more than one 4,096-sample G.711 work item, so the chunk cursor
    and the aligned fast path both run —, and three rows in between."""
    phonemes, frames = [24, 1, 5, 11, 17], [22, 1, 3, 7, 2]
    B, Tx = len(phonemes), max(phonemes)
    rng = np.random.default_rng(29)
    ids = np.zeros((B, Tx), np.int64)
    forced = np.zeros((B, Tx), np.int32)
    for b in range(B):
        ids[b, : phonemes[b]] = rng.integers(1, cfg.num_symbols, phonemes[b])
        forced[b, : phonemes[b]] = frames[b]
    assert phonemes[0] * frames[0] * cfg.hop_length >= 4200 > G711_CHUNK and phonemes[1] * frames[1] * cfg.hop_length == 8
    return dict(ids=ids, lens=np.array(phonemes, np.int64), sid=None, scales=SCALES,
                kw=dict(seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0, forced_durations=forced))


def test_every_kernel_form(emu_lib, cu_count, tables):
    """check_every_kernel_form at the smallest shapes the walk can go wrong at; the sixteen streams again with 1 and 13 emulated
    compute units: the bytes do not move."""
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=29))
    a = _kernel_form_batch(cfg)
    eng = Engine(blob, library=emu_lib)
    want = check_every_kernel_form(eng, a, tables)
    eng.close()
    assert len(want) == 16
    for cus in (1, 13):
        cu_count(cus)
        eng = Engine(blob, library=emu_lib)
        got = {k: v.data.tobytes() for k, v in _kernel_form_streams(eng, a)[2].items()}
        eng.close()
        assert got == want, cus


# ---------------------------------------------------------------------------------------------- the Python layer
def test_session_and_request_wav_encodings(emu_lib, tables):
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=25, frames_per_id=2.0))
    sess = InferenceSession(blob, _library=emu_lib)
    assert sess.output_encoding == "s16le"
    ids, lens, _ = _inputs(cfg, 4, 11, seed=25)
    feed = {"input": ids, "input_lengths": lens, "scales": SCALES[:4]}
    keys, vols, ms = [11, 5, 70_000, 2], [100.0, 300.0, 50.0, 120.0], [0, 1, 333.3, 1000]
    common = dict(lead_ms=ms, tail_ms=2.5, volume=vols, utterance_keys=keys)
    s16 = sess.run_packed(feed, **common)
    assert s16.encoding == "s16le"
    for law in LAWS:
        pk = sess.run_packed(feed, encoding=law, **common)
        assert pk.encoding == law and np.array_equal(pk.data, G.encode(tables[law], s16.pcm))
        _same_layout(pk, s16)
    f32 = sess.run_packed(feed, encoding="f32le", sample_rate=8000, wav=True, **common)
    assert f32.encoding == "f32le" and f32.sample_rate == 8000 and bytes(f32.wav) == G.wav_file("f32le", 8000, f32.data)
    assert sess.run_packed(feed, **common).pcm.tobytes() == s16.pcm.tobytes()  # a call's encoding is the call's alone
    with pytest.raises(ValueError, match="unknown output encoding 'opus'"):
        sess.run_packed(feed, encoding="opus")
    with pytest.raises(ValueError, match="unknown output encoding"):
        InferenceSession(blob, _library=emu_lib, output_encoding="g722")
    # a session whose streams are mu-law unless a call says otherwise
    mu = InferenceSession(blob, _library=emu_lib, output_encoding="ulaw", output_sample_rate=8000)
    assert mu.output_encoding == "ulaw"
    a = mu.run_packed(feed, wav=True, **common)
    b = mu.run_packed(feed, wav=True, encoding="s16le", **common)
    assert a.encoding == "ulaw" and a.sample_rate == 8000 and np.array_equal(a.data, G.encode(tables["ulaw"], b.pcm))
    assert bytes(a.wav) == G.wav_file("ulaw", 8000, a.data)
    rows, _ = mu.run_pcm16(feed, volume=vols, utterance_keys=keys)  # padded results: int16 whatever the setting
    assert all(np.array_equal(G.encode(tables["ulaw"], rows[i]), a.rows[i]) for i in range(4))
    mu.close()
    # request_wav: the telephony file in one call == mu-law of the int16 request at that rate
    rng = np.random.default_rng(8000)
    sentences = [rng.integers(1, cfg.num_symbols, int(n)).tolist() for n in (7, 1, 11, 4)]
    settings = dict(break_ms=250.0, scales=(0.667, 1.1, 0.8), volume=150.0, utterance_keys=[901, 17, 33, 5], sample_rate=8000)
    pcm_file = PP.request_wav(sess, sentences, **settings)
    got = PP.request_wav(sess, sentences, encoding="ulaw", **settings)
    pcm = np.frombuffer(pcm_file[44:], "<i2")
    assert got == G.wav_file("ulaw", 8000, G.encode(tables["ulaw"], pcm)) == PP.wav_bytes([PP.lin2ulaw(pcm)], 8000, "ulaw")
    sess.close()


def test_plain_c99_client_of_the_encoding_calls(emu_lib, tmp_path, tables):
    """tests/abi/abi_encoding_client.c: the new declarations are C99, and sizes / pointers / header of an encoded stream hold from C."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_encoding_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_encoding_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir], check=True)
    cfg = VitsConfig.tiny()
    w = W.synthetic_weights(cfg, seed=17)
    W.save(str(tmp_path / "voice.m355"), cfg, w)
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355"), str(tmp_path / "out_ulaw.wav"), str(tmp_path / "out_f32.wav")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "expected failure rc=-1 msg=output encoding 9 unknown" in p.stdout
    ids = np.array([[3, 7, 1, 9, 4], [5, 2, 0, 0, 0], [8, 6, 4, 2, 0]])
    eng = Engine(W.pack(cfg, w), library=emu_lib)
    full = eng.run(ids, [5, 2, 4], [0, 1, 0], want_pcm16=True, want_float=True)
    eng.close()
    pcm, flt = [], []
    for b, lead in ((2, 3), (0, 101)):
        n = int(full["lengths"][b])
        pcm += [np.zeros(lead, np.int16), full["pcm"][b, :n]]
        flt += [np.zeros(lead, np.float32), full["audio"][b, :n]]
    pcm, flt = np.concatenate(pcm + [np.zeros(7, np.int16)]), np.concatenate(flt + [np.zeros(7, np.float32)])
    assert (tmp_path / "out_ulaw.wav").read_bytes() == G.wav_file("ulaw", cfg.sample_rate, G.encode(tables["ulaw"], pcm))
    assert (tmp_path / "out_f32.wav").read_bytes() == G.wav_file("f32le", cfg.sample_rate, flt)
