"""Phoneme timing and levels of a run (mi355vits_fetch_alignment, k_align) on the CPU model of the kernels;
test_gpu_alignment.py runs the same contract on the MI355X.

Yardsticks, never the code under test: `frames` = the w_ceil debug tap of the same run, or the forced_durations fed in; `start` /
`samples` = the integer formula in Python ints (tests/alignment_ref.py over tests/resample_ref.ratio / out_len); levels = fp64
numpy over the WANT_FLOAT audio of the same run, sliced by the yardstick's own spans."""
import os
import subprocess
import threading

import numpy as np
import pytest

from mimic3_amd import postprocess as PP
from mimic3_amd import weights as W
from mimic3_amd._native import Alignment, Engine, NativeError
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests import alignment_ref as A
from tests import resample_ref as R
from tests.test_resample import FI, SCALES, _case, run_at

RATES = (0, 8000, 48000)  # native; M > L with a non-integer hop L / M; L > M
NAN = 0x7FC00000


# ------------------------------------------------------------------------------------------ checks shared with the GPU twin
def ratio_of(eng, rate):
    return R.ratio(eng.config.sample_rate, rate) if rate else (1, 1)


def check_timing(al, frames, lens, lengths, hop, L, M, rate):
    """Criterion 1: frames / start / samples equal the yardstick element for element; the spans tile each row and sum to
    lengths[b] (a row of zero frames: all-zero spans and one frame of audio); padded positions as specified."""
    lens = [int(n) for n in lens]
    fr, st, sm = A.timing(frames, lens, hop, L, M)
    assert al.sample_rate == rate
    assert al.frames.dtype == al.start.dtype == al.samples.dtype == np.int32 and al.frames.shape == fr.shape
    assert np.array_equal(al.frames, fr) and np.array_equal(al.start, st) and np.array_equal(al.samples, sm)
    for b, n in enumerate(lens):
        assert al.start[b, 0] == 0
        assert np.array_equal(al.start[b, 1:], al.start[b, :-1] + al.samples[b, :-1])  # disjoint, ordered, no gaps
        total = int(al.samples[b].sum())
        if int(al.frames[b].sum()) > 0:
            assert total == int(lengths[b]), b
        else:  # the documented exception: max(1, sum) frames of audio, no span
            assert total == 0 and int(lengths[b]) == R.out_len(hop, L, M), b
        assert not al.frames[b, n:].any() and not al.samples[b, n:].any() and (al.start[b, n:] == total).all()
        zero = al.frames[b, :n] == 0
        assert not al.samples[b, :n][zero].any()  # a phoneme of zero frames: no samples, the next phoneme's start
    return st, sm  # the yardstick's own spans: what the levels are sliced by


def check_levels(al, audio, peaks, st, sm):
    """Criterion 2: peak bitwise the fp64 yardstick's max cast to f32; rms within 1 f32 ulp of the yardstick rounded to f32 (the
    squares are exact in double, the double sum of at most 2^20 terms errs by less than 1e-10 relative, one double rounding
    remains); max_t peak == peaks[b] bitwise for every row with a frame; empty spans and padded positions give 0."""
    assert al.peak.dtype == al.rms.dtype == np.float32
    for b in range(al.frames.shape[0]):
        peak, rms = A.levels(audio[b], st[b], sm[b])
        assert al.peak[b].tobytes() == peak.tobytes(), b
        worst = np.abs(al.rms[b].astype(np.float64) - rms.astype(np.float64)) - np.spacing(rms).astype(np.float64)
        assert (worst <= 0).all(), (b, float(worst.max()))
        empty = al.samples[b] == 0
        assert not al.peak[b][empty].any() and not al.rms[b][empty].any()
        if int(al.frames[b].sum()) > 0:
            assert np.max(al.peak[b]).tobytes() == np.float32(peaks[b]).tobytes(), b


def aligned_run(eng, rate, a, levels=True):
    """One padded call at `rate` with the w_ceil tap, and its alignment checked against the yardsticks."""
    out = run_at(eng, rate, a, debug_taps=True)
    frames = eng.tap("w_ceil")[:, 0, :].astype(np.int64)
    al = eng.fetch_alignment(levels=levels)
    L, M = ratio_of(eng, rate)
    st, sm = check_timing(al, frames, a["lens"], out["lengths"], eng.config.hop_length, L, M, rate or eng.config.sample_rate)
    if levels:
        check_levels(al, out["audio"], out["peaks"], st, sm)
    else:
        assert al.peak is None and al.rms is None
    return out, al


def same_alignment(x, y, rows_x=slice(None), rows_y=slice(None), tx=None):
    for k in ("frames", "start", "samples", "peak", "rms"):
        u, v = getattr(x, k), getattr(y, k)
        assert (u is None) == (v is None), k
        if u is not None:
            assert u[rows_x, :tx].tobytes() == v[rows_y, :tx].tobytes(), k
    assert x.sample_rate == y.sample_rate


def check_kernel_alone(lib):
    """Criterion 3, the kernel through the hook on exact inputs: constant -0.5 audio gives peak = rms = 0.5 exactly for every
    non-empty span; frames mix 0, 1, 40, 0, 0, 3 at hop 256 (a 40-frame span = 10,240 samples: 160 passes of a wave); T = 97; rows
    of 0 and 1 phonemes; alen shorter than the stride with NaN behind it; garbage frames behind a row's count."""
    hop, T = 256, 97
    pattern = np.array([0, 1, 40, 0, 0, 3], np.int32)
    frames = np.tile(pattern, 17)[:T][None, :].repeat(4, 0).copy()
    lens = np.array([T, 0, 1, 50], np.int32)
    frames[2, 0] = 2
    frames[3, 50:] = 1 << 20  # behind the row's count: never looked at
    for (L, M) in ((1, 1), (160, 441), (320, 147)):
        fr, st, sm = A.timing(frames, lens, hop, L, M)
        alen = sm.sum(axis=1).astype(np.int32)
        alen[1] = R.out_len(hop, L, M)  # the row without phonemes still has one frame of audio
        stride = int(alen.max()) + 5
        audio = np.full((4, stride), np.nan, np.float32)
        for b in range(4):
            audio[b, : alen[b]] = -0.5
        al = lib.test_alignment(frames, lens, audio, alen, hop, L, M)
        assert np.array_equal(al.frames, fr) and np.array_equal(al.start, st) and np.array_equal(al.samples, sm), (L, M)
        assert al.samples[0, 2] == R.out_len(41 * hop, L, M) - R.out_len(hop, L, M)
        want = np.where(sm > 0, np.float32(0.5), np.float32(0.0)).astype(np.float32)
        assert al.peak.tobytes() == want.tobytes() and al.rms.tobytes() == want.tobytes(), (L, M)
        assert not al.samples[1].any() and not al.start[1].any() and not al.peak[1].any()
        plain = lib.test_alignment(frames, lens, audio, alen, hop, L, M, levels=False)  # the timing-only form of the kernel
        assert plain.peak is None and np.array_equal(plain.frames, fr) and np.array_equal(plain.start, st) and np.array_equal(plain.samples, sm)
    # levels of varying samples: spans that start on any lane offset, against the fp64 yardstick
    rng = np.random.default_rng(12)
    fr, st, sm = A.timing(frames, lens, 37)
    alen = sm.sum(axis=1).astype(np.int32)
    alen[1] = 37
    audio = np.full((4, int(alen.max()) + 3), np.nan, np.float32)
    for b in range(4):
        audio[b, : alen[b]] = rng.standard_normal(int(alen[b])).astype(np.float32)
    al = lib.test_alignment(frames, lens, audio, alen, 37)
    assert np.array_equal(al.start, st) and np.array_equal(al.samples, sm)
    check_levels(al, audio, [np.max(np.abs(audio[b, : alen[b]])) for b in range(4)], st, sm)


def check_rows_alone(make_engine, a, rate, batched, rows):
    """Criterion 4: a row's alignment in the batch is bitwise the row's alone (its own scales and key)."""
    eng = make_engine()
    eng.set_output_rate(rate)
    for b in rows:
        n = int(a["lens"][b])
        kw = dict(a["kw"])
        kw["utterance_keys"] = [kw["utterance_keys"][b]]
        kw["pcm_volume"] = float(np.asarray(kw["pcm_volume"]).reshape(-1)[b])
        if "forced_durations" in kw:
            kw["forced_durations"] = kw["forced_durations"][b:b + 1, : max(n, 1)]
        eng.run(a["ids"][b:b + 1, : max(n, 1)], [n], a["scales"][b], None, want_float=False, device_only=True, **kw)
        solo = eng.fetch_alignment(levels=True)
        same_alignment(solo, batched, slice(0, 1), slice(b, b + 1), max(n, 1))
        assert not batched.samples[b, max(n, 1):].any() and not batched.peak[b, max(n, 1):].any()
    eng.close()


def check_nothing_else_moves(eng, a, rate):
    """Criterion 5: after fetch_alignment, fetch / fetch_packed / a second fetch_alignment give the bytes they gave before it —
    after a padded run, a DEVICE_ONLY run and a run_packed run; no `align` line unless one was fetched; the profiled bytes."""
    eng.set_output_rate(rate)
    eng.profile_enable(True)
    pack = dict(order=[2, 0], lead_samples=[5, 3], tail_samples=2, wav=True)
    for kind in ("padded", "device_only", "packed"):
        eng.profile_reset()
        if kind == "packed":
            eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **a["kw"])
        else:
            eng.run(a["ids"], a["lens"], a["scales"], a.get("sid"), want_float=True, want_pcm16=True, device_only=kind == "device_only", **a["kw"])
        assert "align" not in eng.profile_report(), kind
        before = eng.fetch(want_float=True, want_pcm16=True)
        before = {k: np.copy(v) for k, v in before.items()}
        packed = bytes(eng.fetch_packed(**pack).wav)
        eng.profile_reset()
        al = eng.fetch_alignment(levels=True)
        B, Tx = a["ids"].shape
        rep = eng.profile_report()
        assert rep["align"]["calls"] == 1 and rep["align"]["bytes"] == 4.0 * float(np.sum(before["lengths"])) + 20.0 * B * Tx, kind
        eng.profile_reset()
        plain = eng.fetch_alignment()
        assert eng.profile_report()["align"]["bytes"] == 12.0 * B * Tx
        assert plain.peak is None and np.array_equal(plain.start, al.start) and np.array_equal(plain.samples, al.samples)
        after = eng.fetch(want_float=True, want_pcm16=True)
        for k in ("audio", "pcm", "lengths", "peaks"):
            assert after[k].tobytes() == before[k].tobytes(), (kind, k)
        assert bytes(eng.fetch_packed(**pack).wav) == packed, kind
        same_alignment(eng.fetch_alignment(levels=True), al)
        assert int(al.samples.sum()) == int(np.sum(before["lengths"]))
    eng.profile_enable(False)


def check_forced_round_trip(eng, a, rate):
    """Criterion 6: run, fetch frames, run again with forced_durations = frames and the same keys: audio and alignment bitwise equal."""
    first = run_at(eng, rate, a)
    al = eng.fetch_alignment(levels=True)
    kw = dict(a["kw"], forced_durations=al.frames)
    again = run_at(eng, rate, dict(a, kw=kw))
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert again[k].tobytes() == first[k].tobytes(), k
    same_alignment(eng.fetch_alignment(levels=True), al)


def check_errors(make_engine, a):
    """Criterion 7."""
    eng = make_engine()
    with pytest.raises(NativeError, match="fetch_alignment: no completed run on this handle") as e:
        eng.fetch_alignment()
    assert e.value.code == -1
    lib = eng.native.lib
    assert lib.mi355vits_fetch_alignment(eng._h, 0, None) == -1
    run_at(eng, 0, a)
    assert lib.mi355vits_fetch_alignment(eng._h, 0, None) == -1
    from mimic3_amd._native import AlignmentResult
    import ctypes

    r = AlignmentResult()
    for want in (2, 0x80000001):
        assert lib.mi355vits_fetch_alignment(eng._h, want, ctypes.byref(r)) == -1
        assert b"unknown bits" in lib.mi355vits_last_error(eng._h) and not r.frames and not r.owner_
    al = eng.fetch_alignment(levels=True)
    # a run refused before anything is launched leaves the previous run served, exactly as fetch behaves
    with pytest.raises(NativeError):
        eng.run(a["ids"], a["lens"], [0.5, -1.0, 0.5], a.get("sid"))
    same_alignment(eng.fetch_alignment(levels=True), al)
    assert eng.fetch()["lengths"].tolist() == [int(x) for x in al.samples.sum(axis=1)]
    # a run that fails after its launch sequence began (a duration past the cap) leaves no result at all
    with pytest.raises(NativeError):
        eng.run(a["ids"], a["lens"], a["scales"], a.get("sid"), forced_durations=np.full(a["ids"].shape, 1 << 23, np.int32))
    with pytest.raises(NativeError, match="fetch: no completed run"):
        eng.fetch()
    with pytest.raises(NativeError, match="fetch_alignment: no completed run on this handle"):
        eng.fetch_alignment()
    eng.close()


# ------------------------------------------------------------------------------------------ the engine on the CPU model
def _engine(emu_lib, seed=71, n_speakers=1, frames_per_id=6.0):
    cfg = VitsConfig.tiny(n_speakers=n_speakers) if n_speakers > 1 else VitsConfig.tiny()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=seed, frames_per_id=frames_per_id))


@pytest.mark.parametrize("n_speakers", [1, 4])
def test_timing_and_levels_at_every_rate(emu_lib, n_speakers):
    """Criteria 1 and 2 on a ragged batch with a one-phoneme row: native, 8000 Hz, 48000 Hz."""
    cfg, blob = _engine(emu_lib, 71, n_speakers)
    eng = Engine(blob, library=emu_lib)
    a = _case(cfg, 71)
    for rate in RATES:
        out, al = aligned_run(eng, rate, a)
        assert len({int(x) for x in out["lengths"]}) > 1
        eng.set_output_rate(0)  # the handle's setting has moved on: the run is served at the rate it ran at
        same_alignment(eng.fetch_alignment(levels=True), al)
        _, plain = aligned_run(eng, rate, a, levels=False)
        assert np.array_equal(plain.start, al.start)
    eng.close()


def test_forced_durations_zero_frames_and_the_empty_row(emu_lib):
    """With forced_durations, frames are the forced values; phonemes of zero frames; a row whose durations sum to 0."""
    cfg, blob = _engine(emu_lib, 72)
    eng = Engine(blob, library=emu_lib)
    a = _case(cfg, 72)
    rng = np.random.default_rng(72)
    forced = rng.integers(0, 9, a["ids"].shape).astype(np.int32)
    forced[:, 3] = 0
    forced[2] = 0  # the documented exception: all-zero spans, one frame of audio
    forced[0, 5] = 300  # a span of several passes of a wave at hop 8
    a["kw"]["forced_durations"] = forced
    for rate in RATES:
        out = run_at(eng, rate, a)
        al = eng.fetch_alignment(levels=True)
        L, M = ratio_of(eng, rate)
        st, sm = check_timing(al, forced, a["lens"], out["lengths"], cfg.hop_length, L, M, rate or FI)
        check_levels(al, out["audio"], out["peaks"], st, sm)
        assert not al.samples[2].any() and int(out["lengths"][2]) == R.out_len(cfg.hop_length, L, M)
    eng.close()


def test_the_kernel_alone(emu_lib):
    check_kernel_alone(emu_lib)
    with pytest.raises(NativeError):
        emu_lib.test_alignment(np.ones((1, 4), np.int32), [5], np.zeros((1, 8), np.float32), [8], 2)
    with pytest.raises(NativeError):  # alen past the stride: refused before anything is launched
        emu_lib.test_alignment(np.ones((1, 4), np.int32), [4], np.zeros((1, 8), np.float32), [9], 2)


@pytest.mark.parametrize("rate", [0, 8000])
def test_batched_is_alone_and_on_a_poisoned_workspace(emu_lib, rate):
    """Criterion 4: the rows of a ragged batch of 5 are bitwise the rows alone; again on a workspace a larger call sized and a quiet
    NaN filled."""
    cfg, blob = _engine(emu_lib, 73)
    a = _case(cfg, 73)
    a["kw"]["forced_durations"] = np.random.default_rng(73).integers(0, 40, a["ids"].shape).astype(np.int32)
    eng = Engine(blob, library=emu_lib)
    _, want = aligned_run(eng, rate, a)
    check_rows_alone(lambda: Engine(blob, library=emu_lib), a, rate, want, range(5))
    big = dict(a, ids=np.tile(a["ids"], (2, 2)), lens=np.tile(a["lens"] * 2, 2), scales=np.tile(SCALES, (2, 1)), sid=None,
               kw=dict(seed=1, forced_durations=np.full((10, 24), 40, np.int32)))
    run_at(eng, rate, big)
    eng.fetch_alignment(levels=True)  # sizes the alignment's own arena past what the batch needs
    eng.fill_workspace(NAN)
    _, got = aligned_run(eng, rate, a)
    same_alignment(got, want)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_nothing_else_moves(emu_lib, rate):
    cfg, blob = _engine(emu_lib, 74)
    eng = Engine(blob, library=emu_lib)
    check_nothing_else_moves(eng, _case(cfg, 74), rate)
    eng.close()


def test_forced_durations_round_trip(emu_lib):
    cfg, blob = _engine(emu_lib, 75)
    eng = Engine(blob, library=emu_lib)
    for rate in (0, 48000):
        check_forced_round_trip(eng, _case(cfg, 75), rate)
    eng.close()


def test_errors(emu_lib):
    cfg, blob = _engine(emu_lib, 76)
    check_errors(lambda: Engine(blob, library=emu_lib), _case(cfg, 76))


# ------------------------------------------------------------------------------------------ Python surface
def _feed(ids, n):
    return {"input": np.asarray(ids, np.int64)[None, :], "input_lengths": np.array([n], np.int64), "scales": np.array([0.667, 1.0, 0.8], np.float32)}


def test_run_pcm16_alignment_under_concurrent_threads(emu_lib):
    """Criterion 8: micro-batcher on, two lanes, 8 concurrent threads — each caller's alignment matches its own rows (the lengths
    tile); unset, the return value is the 2-tuple it was."""
    cfg, blob = _engine(emu_lib, 77, frames_per_id=4.0)
    opts = SessionOptions()
    opts.micro_batch_window_ms = 2.0
    opts.lanes = 2
    opts.seed = 5
    sess = InferenceSession(blob, opts, _library=emu_lib)
    rng = np.random.default_rng(77)
    sizes = [3, 12, 7, 1, 9, 5, 11, 2]
    feeds = [_feed(rng.integers(1, cfg.num_symbols, n), n) for n in sizes]
    results = [None] * len(feeds)

    def work(i):
        results[i] = sess.run_pcm16(feeds[i], utterance_keys=[500 + i], alignment="levels", sample_rate=8000 if i % 2 else None)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(feeds))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i, res in enumerate(results):
        assert res is not None and len(res) == 3, i
        rows, lengths, al = res
        assert isinstance(al, Alignment) and al.frames.shape == (1, sizes[i]) and al.sample_rate == (8000 if i % 2 else FI)
        assert int(al.samples.sum()) == int(lengths[0]) == rows[0].size, i
        plain = sess.run_pcm16(feeds[i], utterance_keys=[500 + i], sample_rate=8000 if i % 2 else None)
        assert isinstance(plain, tuple) and len(plain) == 2 and np.array_equal(plain[0][0], rows[0])
        solo = sess.run_pcm16(feeds[i], utterance_keys=[500 + i], sample_rate=8000 if i % 2 else None, alignment=True, direct=True)
        assert solo[2].peak is None and np.array_equal(solo[2].start, al.start) and np.array_equal(solo[2].frames, al.frames)
    with pytest.raises(ValueError):
        sess.run_pcm16(feeds[0], alignment="loud")
    sess.close()


def test_run_packed_alignment_in_stream_coordinates(emu_lib):
    """Criterion 8: run_packed(order=[2, 0], lead_ms, 8000 Hz, mu-law, alignment=True): the spans land inside their entries."""
    cfg, blob = _engine(emu_lib, 78, frames_per_id=4.0)
    opts = SessionOptions()
    opts.seed = 5
    sess = InferenceSession(blob, opts, _library=emu_lib)
    a = _case(cfg, 78, B=3, Tx=9)
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    keys = [11, 12, 13]
    pk = sess.run_packed(feed, order=[2, 0], lead_ms=[30.0, 12.5], sample_rate=8000, encoding="ulaw", alignment=True, utterance_keys=keys)
    assert sess.run_packed(feed, order=[2, 0], utterance_keys=keys).alignment is None
    al = pk.alignment
    assert pk.encoding == "ulaw" and al.sample_rate == 8000 == pk.sample_rate and al.peak is None and al.start.shape == (2, 9)
    rows, lengths, padded = sess.run_pcm16(feed, sample_rate=8000, alignment="levels", utterance_keys=keys)
    lead = [int((ms / 1000.0) * 8000) for ms in (30.0, 12.5)]  # add_break's rule at the stream's rate
    assert [int(o) for o in pk.offsets] == [lead[0], lead[0] + int(lengths[2]) + lead[1]]
    for i, b in enumerate((2, 0)):
        assert np.array_equal(al.frames[i], padded.frames[b]) and np.array_equal(al.samples[i], padded.samples[b])
        assert np.array_equal(al.start[i], padded.start[b].astype(np.int64) + int(pk.offsets[i]))
        assert int(al.start[i, 0]) == int(pk.offsets[i]) and int(al.start[i, -1] + al.samples[i, -1]) == int(pk.offsets[i] + pk.lengths[i])
        for t in range(int(a["lens"][b])):  # phoneme t of entry i, in the stream's own encoding
            s, n = int(al.start[i, t]), int(al.samples[i, t])
            assert np.array_equal(pk.data[s: s + n], PP.lin2ulaw(rows[b][int(padded.start[b, t]): int(padded.start[b, t]) + n]))
    lv = sess.run_packed(feed, alignment="levels", utterance_keys=keys).alignment
    assert lv.peak is not None and lv.start.dtype == np.int64 and lv.sample_rate == FI
    sess.close()


def test_marks_on_a_three_span_example():
    """Criterion 8: postprocess.marks against hand-computed values."""
    al = Alignment(frames=np.array([[1, 2, 0, 3, 1, 0]], np.int32), start=np.array([[0, 100, 300, 300, 600, 700]], np.int32),
                   samples=np.array([[100, 200, 0, 300, 100, 0]], np.int32),
                   peak=np.array([[0.5, 0.25, 0.0, 0.75, 0.125, 0.0]], np.float32), rms=np.array([[0.3, 0.1, 0.0, 0.4, 0.05, 0.0]], np.float32),
                   sample_rate=1000)
    got = PP.marks(al, 0, [("one", 0, 2), ("pause", 2, 3), ("two", 3, 5)])
    assert [m["label"] for m in got] == ["one", "pause", "two"]
    assert [(m["start_sample"], m["end_sample"]) for m in got] == [(0, 300), (300, 300), (300, 700)]
    assert [(m["start_s"], m["end_s"]) for m in got] == [(0.0, 0.3), (0.3, 0.3), (0.3, 0.7)]
    assert [m["peak"] for m in got] == [0.5, 0.0, 0.75]
    r = lambda pairs: float(np.sqrt(sum(float(np.float32(x)) ** 2 * n for x, n in pairs) / sum(n for _, n in pairs)))  # noqa: E731
    assert got[0]["rms"] == pytest.approx(r([(0.3, 100), (0.1, 200)]), rel=1e-12) and got[1]["rms"] == 0.0
    assert got[2]["rms"] == pytest.approx(r([(0.4, 300), (0.05, 100)]), rel=1e-12)
    plain = PP.marks(Alignment(al.frames, al.start, al.samples, sample_rate=1000), 0, [("all", 0, 6), ("end", 6, 6)])
    assert plain == [{"label": "all", "start_sample": 0, "end_sample": 700, "start_s": 0.0, "end_s": 0.7},
                     {"label": "end", "start_sample": 700, "end_sample": 700, "start_s": 0.7, "end_s": 0.7}]
    with pytest.raises(ValueError):
        PP.marks(al, 0, [("bad", 4, 7)])


def test_plain_c99_client(emu_lib, tmp_path):
    """Criterion 9: a C99 client runs a tiny voice, fetches with levels, checks the tiling sum against lengths and frees the result."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_alignment_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_alignment_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir], check=True)
    cfg = VitsConfig.tiny()
    W.save(str(tmp_path / "voice.m355"), cfg, W.synthetic_weights(cfg, seed=17))
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "expected failure rc=-1 msg=fetch_alignment: no completed run on this handle" in p.stdout
    assert "alignment ok" in p.stdout
