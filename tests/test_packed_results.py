"""Packed results (mi355vits_run_packed / mi355vits_fetch_packed, k_pack<S16>): a batch's int16 audio as ONE contiguous
stream — only the valid samples of each row, rows in the order the caller names, break silences between them, optionally
behind a RIFF header.  On the CPU model of the kernels (tests/emu); test_gpu_packed_results.py runs the same contract on the
MI355X.

The yardstick is always the EXISTING padded call on the same engine (Engine.run(..., want_pcm16=True)) and host numpy /
postprocess.wav_bytes / the stdlib wave module, never the code under test."""
import io
import os
import subprocess
import wave

import numpy as np
import pytest

from mimic3_amd import postprocess as PP
from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession

SEED = 0xC0FFEE
# five ragged rows: most with noise, one deterministic; length_scale 0.7 .. 1.6; keys far apart and out of order
SCALES = np.array([[0.667, 1.0, 0.8], [0.0, 1.6, 0.0], [0.5, 0.7, 0.3], [0.9, 1.2, 1.1], [0.333, 0.85, 0.0]], np.float32)
KEYS = [7, 1_000_003, 42, (1 << 40) + 5, 3]
VOLUMES = [50.0, 100.0, 150.0, 300.0, 7.5]  # percent; 300 % clips
CHUNK = 2048  # output samples of one work item of k_pack in its int16 form (csrc/kernels_pack.cpp: 256 lanes x 8)
DEFAULT_CUS = 8  # what the CPU model reports unless a test sets another count


@pytest.fixture
def cu_count(emu_lib):
    """Sets the compute units the CPU model reports (create engine handles after setting it); restores the default afterwards."""
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


def _chunks(full, order=None, lead=None, tail=0):
    """The stream assembled on the host from the padded call's rows and np.zeros silences."""
    B = len(full["lengths"])
    order = list(range(B)) if order is None else list(order)
    parts = []
    for i, b in enumerate(order):
        if lead is not None and lead[i]:
            parts.append(np.zeros(int(lead[i]), np.int16))
        parts.append(full["pcm"][b, : int(full["lengths"][b])])
    if tail:
        parts.append(np.zeros(int(tail), np.int16))
    return parts


def _assert_entries(pk, full, order):
    for i, b in enumerate(order):
        L = int(full["lengths"][b])
        assert int(pk.lengths[i]) == L, (i, b)
        assert pk.peaks[i].tobytes() == full["peaks"][b].tobytes(), (i, b)
        assert pk.rows[i].shape == (L,) and np.array_equal(pk.rows[i], full["pcm"][b, :L]), (i, b)
        assert np.shares_memory(pk.rows[i], pk.pcm)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("n_speakers", [1, 4])
def test_default_pack_holds_the_padded_calls_rows(emu_lib, math, n_speakers):
    cfg = VitsConfig.tiny(n_speakers=n_speakers) if n_speakers > 1 else VitsConfig.tiny()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=21)), library=emu_lib)
    eng.set_math(math)
    ids, lens, sid = _inputs(cfg, 5, 12, seed=21)
    kw = dict(seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0)
    full = eng.run(ids, lens, SCALES, sid, want_pcm16=True, **kw)
    pk = eng.run_packed(ids, lens, SCALES, sid, **kw)
    assert len(pk.rows) == 5 and pk.wav is None
    assert int(pk.offsets[0]) == 0
    for i in range(4):
        assert int(pk.offsets[i + 1]) == int(pk.offsets[i]) + int(pk.lengths[i])
    assert pk.total_samples == int(np.sum(full["lengths"])) == pk.pcm.shape[0]
    assert pk.lengths.tobytes() == full["lengths"].tobytes() and pk.peaks.tobytes() == full["peaks"].tobytes()
    _assert_entries(pk, full, range(5))
    assert len({int(x) for x in full["lengths"]}) > 1  # ragged
    # after a packed call the padded forms are served from the float audio, as after a device-only run
    again = eng.fetch(want_float=True, want_pcm16=False)
    assert again["audio"].tobytes() == full["audio"].tobytes()
    eng.close()


@pytest.mark.parametrize("n_speakers", [1, 4])
def test_order_silences_and_header(emu_lib, n_speakers):
    cfg = VitsConfig.tiny(n_speakers=n_speakers) if n_speakers > 1 else VitsConfig.tiny()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=22)), library=emu_lib)
    ids, lens, sid = _inputs(cfg, 5, 12, seed=22, one_phoneme_row=1)
    kw = dict(seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0)
    full = eng.run(ids, lens, SCALES, sid, want_pcm16=True, **kw)
    # a permutation without row 2; silences of 0, 1, an odd count and more than a chunk: rows start at odd and at
    # non-16-byte offsets, and one chunk holds a row's end, a silence and the next row's start
    order, lead, tail = [3, 0, 4, 1], [1, 0, 777, CHUNK + 453], 5
    pk = eng.run_packed(ids, lens, SCALES, sid, order=order, lead_samples=lead, tail_samples=tail, wav=True, **kw)
    want = PP.wav_bytes(_chunks(full, order, lead, tail), cfg.sample_rate)
    assert bytes(pk.wav) == want
    assert len(pk.wav) == 44 + 2 * pk.total_samples
    _assert_entries(pk, full, order)
    pos = 0
    for i, b in enumerate(order):
        pos += lead[i]
        assert int(pk.offsets[i]) == pos
        pos += int(full["lengths"][b])
    assert pk.total_samples == pos + tail
    assert any(int(o) % 2 for o in pk.offsets) and any(int(o) % 8 for o in pk.offsets)
    with wave.open(io.BytesIO(bytes(pk.wav)), "rb") as wf:
        assert (wf.getframerate(), wf.getnchannels(), wf.getsampwidth(), wf.getnframes()) == (cfg.sample_rate, 1, 2, pk.total_samples)
        assert wf.readframes(wf.getnframes()) == pk.pcm.tobytes()
    # the stdlib writes the same file
    buf = io.BytesIO()
    with wave.open(buf, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(cfg.sample_rate)
        wf.writeframes(pk.pcm.tobytes())
    assert buf.getvalue() == bytes(pk.wav)
    # the same without a header; then n == 1: the single-phoneme row alone, behind an odd silence
    raw = eng.run_packed(ids, lens, SCALES, sid, order=order, lead_samples=lead, tail_samples=tail, **kw)
    assert raw.wav is None and raw.pcm.tobytes() == want[44:]
    one = eng.run_packed(ids, lens, SCALES, sid, order=[1], lead_samples=[3], wav=True, **kw)
    assert bytes(one.wav) == PP.wav_bytes(_chunks(full, [1], [3]), cfg.sample_rate)
    assert int(lens[1]) == 1 and len(one.rows) == 1 and int(one.offsets[0]) == 3
    eng.close()


def test_fetch_packed_packs_the_last_run_again(emu_lib):
    cfg = VitsConfig.tiny(n_speakers=4)
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=23)), library=emu_lib)
    ids, lens, sid = _inputs(cfg, 5, 12, seed=23)
    kw = dict(seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0)
    specs = [dict(order=[4, 2, 0], lead_samples=[0, 333, 1], tail_samples=9, wav=True),
             dict(order=[1, 3, 0, 2, 4], lead_samples=[5, 0, CHUNK + 1, 17, 2], tail_samples=0, wav=False),
             dict(tail_samples=3, wav=True)]  # every row, in order
    direct = [eng.run_packed(ids, lens, SCALES, sid, **spec, **kw) for spec in specs]
    direct = [(bytes(d.wav) if d.wav is not None else d.pcm.tobytes(), d.offsets.copy(), d.peaks.copy()) for d in direct]
    full = eng.run(ids, lens, SCALES, sid, want_pcm16=True, **kw)
    padded = {k: full[k].copy() for k in ("pcm", "audio", "lengths", "peaks")}
    for spec, (want, offsets, peaks) in zip(specs, direct):
        got = eng.fetch_packed(**spec)
        assert (bytes(got.wav) if got.wav is not None else got.pcm.tobytes()) == want
        assert got.offsets.tobytes() == offsets.tobytes() and got.peaks.tobytes() == peaks.tobytes()
        order = spec.get("order", range(5))
        assert got.pcm.tobytes() == np.concatenate(_chunks(full, order, spec.get("lead_samples"), spec["tail_samples"])).tobytes()
        between = eng.fetch(want_float=True, want_pcm16=True)  # the padded result is what it was
        for k in padded:
            assert between[k].tobytes() == padded[k].tobytes(), k
    # ... and after a run that asked for nothing on the host
    eng.run(ids, lens, SCALES, sid, device_only=True, want_float=False, **kw)
    got = eng.fetch_packed(**specs[0])
    assert bytes(got.wav) == direct[0][0]
    eng.close()
    fresh = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=23)), library=emu_lib)
    with pytest.raises(NativeError, match="no completed run"):
        fresh.fetch_packed()
    fresh.close()


def test_fetch_packed_outgrows_the_last_runs_workspace(emu_lib):
    """A stream larger than the room behind the last run's frame-side layout (the arena keeps about 1 MiB of slack) must not
    reallocate that arena — the float audio lives there: it goes to an arena of its own, and the padded result stays."""
    cfg = VitsConfig.tiny()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=27)), library=emu_lib)
    ids, lens, sid = _inputs(cfg, 5, 12, seed=27)
    kw = dict(seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0)
    full = eng.run(ids, lens, SCALES, sid, want_pcm16=True, **kw)  # a fresh handle: no packed call has sized anything
    padded = {k: full[k].copy() for k in ("pcm", "audio", "lengths", "peaks")}
    order, lead, tail = [4, 1, 3], [300_001, 0, 400_003], 500_000  # 2.4 MB of stream
    for _ in range(2):
        got = eng.fetch_packed(order=order, lead_samples=lead, tail_samples=tail, wav=True)
        assert bytes(got.wav) == PP.wav_bytes(_chunks(full, order, lead, tail), cfg.sample_rate)
        del got
        again = eng.fetch(want_float=True, want_pcm16=True)
        for k in padded:
            assert again[k].tobytes() == padded[k].tobytes(), k
    eng.close()


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


def test_packed_stream_on_a_poisoned_workspace(emu_lib):
    """The whole workspace filled with NaN, Inf or the largest float before a ragged packed call: the same bytes as a fresh
    handle's — the rows' valid samples only are read, and the silences are zeros because the kernel wrote them.  A LARGER packed
    call (more rows, longer silences) sizes the workspace first, so the poisoned call cannot reallocate (and zero) it."""
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=91, frames_per_id=2.0))
    bt = _forced_batch(cfg, POISON_ROWS, Tx=24, frames=2, seed=12)
    big = _forced_batch(cfg, [24] * (len(POISON_ROWS) + 2), Tx=24, frames=2, seed=5)
    n = len(POISON_ROWS)
    spec = dict(order=[6, 4, 0, 2, 5, 1, 3], lead_samples=[7, 0, 1, CHUNK + 3, 129, 64, 5], tail_samples=1001, wav=True)
    fresh = Engine(blob, library=emu_lib)
    want = bytes(_packed(fresh, bt, **spec).wav)
    full = fresh.run(bt["ids"], bt["lengths"], [0.667, 1.0, 0.8], forced_durations=bt["forced"], noise_w=bt["nw"], noise_z=bt["nz"],
                     pcm_volume=np.linspace(0.5, 3.0, n), want_pcm16=True)
    assert want == PP.wav_bytes(_chunks(full, spec["order"], spec["lead_samples"], spec["tail_samples"]), cfg.sample_rate)
    fresh.close()
    eng = Engine(blob, library=emu_lib)
    bigger = _packed(eng, big, lead_samples=[3 * CHUNK] * (n + 2), tail_samples=4 * CHUNK, wav=True)
    assert bigger.total_samples > 2 * (len(want) // 2)
    del bigger
    for pattern in POISON:
        eng.fill_workspace(pattern)
        assert bytes(_packed(eng, bt, **spec).wav) == want, hex(pattern)
        eng.fill_workspace(pattern)  # ... and packed again from the float audio that run left, onto poison as well
        eng.run(bt["ids"], bt["lengths"], [0.667, 1.0, 0.8], forced_durations=bt["forced"], noise_w=bt["nw"], noise_z=bt["nz"],
                pcm_volume=np.linspace(0.5, 3.0, n), device_only=True)
        assert bytes(eng.fetch_packed(**spec).wav) == want, hex(pattern)
    eng.close()


def test_packed_stream_does_not_depend_on_the_cu_count(emu_lib, cu_count):
    """k_pack's persistent grid is sized by the compute units: 1, 3, 8, 13 and 256 of them give the same bytes.  The tiny
    voice's hop is 8, so forced durations of 30 .. 80 frames per id make the stream at least 40 of the kernel's work items — a
    count that is no multiple of 3, 8 or 13 — from rows of unequal length."""
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=33))
    B, Tx = 12, 16
    rng = np.random.default_rng(33)
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    lens = np.array([Tx] + list(rng.integers(Tx // 2, Tx, size=B - 1)), np.int64)
    forced = rng.integers(30, 81, (B, Tx)).astype(np.int32)
    row_samples = [int(forced[b, : lens[b]].sum()) * cfg.hop_length for b in range(B)]
    assert len(set(row_samples)) == B
    order = [int(b) for b in rng.permutation(B)]
    lead = [int(x) for x in rng.integers(0, 700, B)]
    lead[0], lead[5] = 0, 1
    tail = 11
    items = lambda: -(-(sum(row_samples) + sum(lead) + tail) // CHUNK)  # noqa: E731
    while items() < 40 or any(items() % c == 0 for c in (3, 8, 13)):
        tail += CHUNK
    scales = np.tile(np.array([0.667, 1.0, 0.8], np.float32), (B, 1))
    kw = dict(forced_durations=forced, seed=SEED, utterance_keys=1000 + np.arange(B), pcm_volume=np.linspace(0.4, 3.0, B))
    want = None
    for cus in (DEFAULT_CUS, 1, 3, 13, 256):
        cu_count(cus)
        eng = Engine(blob, library=emu_lib)
        pk = eng.run_packed(ids, lens, scales, order=order, lead_samples=lead, tail_samples=tail, wav=True, **kw)
        assert -(-pk.total_samples // CHUNK) == items()
        if want is None:
            full = eng.run(ids, lens, scales, want_pcm16=True, **kw)
            assert [int(x) for x in full["lengths"]] == row_samples
            want = PP.wav_bytes(_chunks(full, order, lead, tail), cfg.sample_rate)
        assert bytes(pk.wav) == want, cus
        eng.close()


def test_bad_pack_arguments_fail_with_the_entry_named(emu_lib):
    cfg = VitsConfig.tiny()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=24)), library=emu_lib)
    ids, lens, sid = _inputs(cfg, 5, 12, seed=24)
    kw = dict(seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0)
    before = eng.run(ids, lens, SCALES, sid, want_pcm16=True, **kw)
    bad = [
        (dict(order=[0, 9, 1]), r"pack entry 1: row 9 out of range"),
        (dict(order=[0, -1]), r"pack entry 1: row -1 out of range"),
        (dict(order=[0, 2, 4, 2]), r"pack entry 3: row 2 appears twice"),
        (dict(order=[3, 1], lead_samples=[0, -5]), r"pack entry 1: negative silence"),
        (dict(tail_samples=-1), r"negative tail silence"),
        (dict(order=[], lead_samples=[]), r"pack: n = 0 out of range"),
        (dict(order=[0, 1, 2, 3, 4, 0]), r"pack: n = 6 out of range"),
        (dict(tail_samples=2 ** 31), r"total_samples exceeds 2\^31 - 1"),
        (dict(order=[0], lead_samples=[2 ** 31]), r"pack entry 0: total_samples exceeds 2\^31 - 1"),
        (dict(tail_samples=2 ** 31 - 10, wav=True), r"RIFF"),
    ]
    for spec, message in bad:
        for call in (lambda: eng.run_packed(ids, lens, SCALES, sid, **spec, **kw), lambda: eng.fetch_packed(**spec)):
            with pytest.raises(NativeError, match=message) as e:
                call()
            assert e.value.code == -1, spec
    # 2^31 - 10 samples of silence fit the sample cap, hence fail only with a header, and only because of it: without one the
    # call would go on to allocate 4 GiB — not tried here
    after = eng.run(ids, lens, SCALES, sid, want_pcm16=True, **kw)
    for k in ("lengths", "audio", "pcm", "peaks"):
        assert after[k].tobytes() == before[k].tobytes(), k
    pk = eng.run_packed(ids, lens, SCALES, sid, **kw)
    assert pk.pcm.tobytes() == np.concatenate(_chunks(before)).tobytes()
    eng.close()


@pytest.mark.parametrize("rate", [22050, 16000])
def test_session_run_packed_and_request_wav(emu_lib, rate):
    cfg = VitsConfig.tiny()
    cfg.sample_rate = rate
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=25, frames_per_id=2.0))
    sess = InferenceSession(blob, _library=emu_lib)
    assert sess.config.sample_rate == rate
    ids, lens, _ = _inputs(cfg, 4, 11, seed=25)
    feed = {"input": ids, "input_lengths": lens, "scales": SCALES[:4]}
    keys = [11, 5, 70_000, 2]
    vols = [100.0, 300.0, 50.0, 120.0]
    rows, lengths = sess.run_pcm16(feed, volume=vols, utterance_keys=keys)
    ms = [0, 1, 333.3, 1000]
    pk = sess.run_packed(feed, lead_ms=ms, tail_ms=2.5, volume=vols, utterance_keys=keys)
    assert pk.lengths.tobytes() == np.asarray(lengths).tobytes() == np.asarray(sess.last_lengths).tobytes()
    pos = 0
    for i in range(4):
        pos += PP.silence(ms[i], rate).size
        assert int(pk.offsets[i]) == pos, (i, ms[i])
        assert np.array_equal(pk.rows[i], rows[i]) and np.shares_memory(pk.rows[i], pk.pcm)
        pos += rows[i].size
    assert pk.total_samples == pos + PP.silence(2.5, rate).size and pk.wav is None
    chunks = []
    for i in range(4):
        chunks += [PP.silence(ms[i], rate), rows[i]]
    assert pk.pcm.tobytes() == np.concatenate(chunks + [PP.silence(2.5, rate)]).tobytes()
    # order + lead_samples + a header, scalar volume, keys drawn from the session's count like run_pcm16 draws them
    base = sess._utterances
    pk2 = sess.run_packed(feed, order=[2, 0], lead_samples=[0, 9], wav=True, volume=80.0)
    assert sess._utterances == base + 4
    rows2, _ = sess.run_pcm16(feed, volume=80.0, utterance_keys=[base + b for b in range(4)])
    assert bytes(pk2.wav) == PP.wav_bytes([rows2[2], np.zeros(9, np.int16), rows2[0]], rate)
    with pytest.raises(ValueError, match="pack entry 0: row 4 out of range"):
        sess.run_packed(feed, order=[4])
    # request_wav: one call for a request's sentences == utterances_to_wav over per-sentence run_pcm16 calls with the same keys
    rng = np.random.default_rng(rate)
    sentences = [rng.integers(1, cfg.num_symbols, int(n)).tolist() for n in (7, 1, 11, 4)]
    skeys = [901, 17, 33, 5]
    sc = (0.667, 1.1, 0.8)
    per_sentence = []
    for s, k in zip(sentences, skeys):
        # (padded to the request's length class is not needed: every sentence is in the first encoder class)
        f1 = {"input": np.array([s], np.int64), "input_lengths": np.array([len(s)], np.int64), "scales": np.array(sc, np.float32)}
        per_sentence.append(sess.run_pcm16(f1, volume=150.0, utterance_keys=[k])[0][0])
    for break_ms in (None, 250.0):
        got = PP.request_wav(sess, sentences, break_ms=break_ms, scales=sc, volume=150.0, utterance_keys=skeys)
        assert isinstance(got, bytes) and got == PP.utterances_to_wav(per_sentence, rate, break_ms=break_ms)
    sess.close()


def test_plain_c99_client_of_the_packed_calls(emu_lib, tmp_path):
    """tests/abi/abi_packed_client.c, compiled with the flags tests/util.py uses for abi_client.c: the header stays C99-clean and
    the offsets / n_bytes arithmetic holds from C."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_packed_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_packed_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir], check=True)
    cfg = VitsConfig.tiny()
    w = W.synthetic_weights(cfg, seed=17)
    W.save(str(tmp_path / "voice.m355"), cfg, w)
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355"), str(tmp_path / "out.wav")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "expected failure rc=-1 msg=pack entry 1: row 2 appears twice" in p.stdout
    ids = np.array([[3, 7, 1, 9, 4], [5, 2, 0, 0, 0], [8, 6, 4, 2, 0]])
    full = Engine(W.pack(cfg, w), library=emu_lib).run(ids, [5, 2, 4], [0, 1, 0], want_pcm16=True)
    want = PP.wav_bytes(_chunks(full, [2, 0], [3, 101], 7), cfg.sample_rate)
    assert (tmp_path / "out.wav").read_bytes() == want
