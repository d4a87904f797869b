"""Output at a requested sample rate (mi355vits_set_output_rate, k_resample) on the CPU model of the kernels;
test_gpu_resample.py runs the same contract on the MI355X.

The yardstick is tests/resample_ref.py (scipy.signal.resample_poly's filter and output restated in numpy, fp64 and plain f32),
applied to the NATIVE f32 audio of the same engine for the same arguments, plus oracle.vits_oracle.audio_float_to_int16 /
postprocess.apply_volume / postprocess.wav_bytes / the stdlib wave module — never the code under test."""
import io
import os
import subprocess
import threading
import wave

import numpy as np
import pytest

from mimic3_amd import postprocess as PP
from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import _ROW_SETTINGS, InferenceSession, InvalidArgument, SessionOptions
from oracle.vits_oracle import audio_float_to_int16
from tests import resample_ref as R
from tests.test_packed_results import CHUNK, DEFAULT_CUS, _chunks, _inputs

SEED = 0xC0FFEE
RATES = (8000, 11025, 16000, 24000, 44100, 48000)
HOOK_RATES = (8000, 16000, 44100, 48000)
SCALES = np.array([[0.667, 1.0, 0.8], [0.0, 1.6, 0.0], [0.5, 0.7, 0.3], [0.9, 1.2, 1.1], [0.333, 0.85, 0.0]], np.float32)
KEYS = [7, 1_000_003, 42, (1 << 40) + 5, 3]
VOLUMES = [50.0, 100.0, 150.0, 300.0, 100.0]  # percent; 300 % clips
FI = 22050


@pytest.fixture
def cu_count(emu_lib):
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(DEFAULT_CUS)


# ------------------------------------------------------------------------------------------ checks shared with the GPU twin
def run_at(eng, rate, a, **flags):
    """One padded call at `rate` (None: whatever the handle has)."""
    if rate is not None:
        eng.set_output_rate(rate)
    out = eng.run(a["ids"], a["lens"], a["scales"], a.get("sid"), want_float=True, want_pcm16=True, **a["kw"], **flags)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def check_native_untouched(eng, a):
    """Criterion 1: unset, 0 and the voice's own rate give the same bytes, and no `resample` line is profiled."""
    eng.profile_enable(True)
    eng.profile_reset()
    first = run_at(eng, None, a)
    assert eng.output_rate == eng.config.sample_rate
    for hz in (0, eng.config.sample_rate):
        again = run_at(eng, hz, a)
        assert eng.output_rate == eng.config.sample_rate
        for k in ("audio", "pcm", "lengths", "peaks"):
            assert again[k].tobytes() == first[k].tobytes(), (hz, k)
        assert int(again["l_max"]) == int(first["l_max"]) and eng.last_rate == eng.config.sample_rate
        assert sorted(again) == sorted(("audio", "pcm", "lengths", "peaks", "l_max", "ty_max"))  # the result's fields are what they were
    assert "resample" not in eng.profile_report()
    eng.profile_enable(False)
    return first


def check_lengths_and_padding(out, native, rate, fi=FI):
    """Criterion 2."""
    L, M = R.ratio(fi, rate)
    want = [R.out_len(int(n), L, M) for n in native["lengths"]]
    assert [int(x) for x in out["lengths"]] == want, rate
    assert int(out["l_max"]) == max(want) == out["audio"].shape[1] == out["pcm"].shape[1]
    assert int(out["ty_max"]) == int(native["ty_max"])
    for b, n in enumerate(want):
        assert not out["audio"][b, n:].any() and not out["pcm"][b, n:].any(), (rate, b)


def check_accuracy(out, native, rate, fi=FI, report=None):
    """Criterion 3: worst-row rel. RMS of the engine's rows against the fp64 yardstick <= 3 x the f32 yardstick's own."""
    L, M = R.ratio(fi, rate)
    worst_e = worst_f = 0.0
    for b, n in enumerate(native["lengths"]):
        e, f = R.errors(out["audio"][b, : int(out["lengths"][b])], native["audio"][b, : int(n)], L, M)
        worst_e, worst_f = max(worst_e, e), max(worst_f, f)
    print(f"resample {fi} -> {rate}: engine {worst_e:.3e}  plain f32 {worst_f:.3e}  ratio {worst_e / worst_f:.2f}")
    if report is not None:
        report.append((rate, worst_e, worst_f))
    assert worst_e <= 3.0 * worst_f, (rate, worst_e, worst_f)


def check_int16(out, native, rate, volumes, fi=FI):
    """Criterion 4: the int16 is the reference's conversion of the engine's own float; peaks are max |audio|; against the int16 of
    the fp64 yardstick every sample of a row at 100 % volume is within 1 LSB."""
    L, M = R.ratio(fi, rate)
    for b, n in enumerate(out["lengths"]):
        n = int(n)
        y = out["audio"][b, :n]
        assert out["peaks"][b].tobytes() == np.max(np.abs(y)).astype(np.float32).tobytes(), (rate, b)
        want = audio_float_to_int16(y)
        if volumes[b] != 100.0:
            want = PP.apply_volume(want, volumes[b])
        assert out["pcm"][b, :n].tobytes() == want.tobytes(), (rate, b)
        if volumes[b] == 100.0:
            ref = R.resample(native["audio"][b, : int(native["lengths"][b])].astype(np.float64), L, M)
            peak = max(0.01, float(np.max(np.abs(ref))))
            ref16 = np.clip(ref * (32767.0 / peak), -32767.0, 32767.0).astype(np.int16)
            assert int(np.max(np.abs(out["pcm"][b, :n].astype(np.int32) - ref16.astype(np.int32)))) <= 1, (rate, b)


def check_rows_alone(make_engine, a, rate, batched, rows):
    """Criterion 5: a row of the batch is bitwise the row alone (its own scales, volume and key)."""
    eng = make_engine()
    eng.set_output_rate(rate)
    for b in rows:
        n = int(a["lens"][b])
        kw = dict(a["kw"])
        kw["utterance_keys"] = [kw["utterance_keys"][b]]
        kw["pcm_volume"] = float(np.asarray(kw["pcm_volume"]).reshape(-1)[b])
        if "forced_durations" in kw:
            kw["forced_durations"] = kw["forced_durations"][b:b + 1, : max(n, 1)]
        sid = None if a.get("sid") is None else a["sid"][b:b + 1]
        solo = eng.run(a["ids"][b:b + 1, : max(n, 1)], [n], a["scales"][b], sid, want_float=True, want_pcm16=True, **kw)
        L = int(batched["lengths"][b])
        assert int(solo["lengths"][0]) == L, b
        assert solo["audio"][0, :L].tobytes() == batched["audio"][b, :L].tobytes(), b
        assert solo["pcm"][0, :L].tobytes() == batched["pcm"][b, :L].tobytes(), b
        assert solo["peaks"][0].tobytes() == batched["peaks"][b].tobytes(), b
    eng.close()


def signals(n, rng):
    t = np.arange(n, dtype=np.float64)
    return {"noise": rng.standard_normal(n).astype(np.float32),
            "tone_9500": (0.8 * np.sin(2 * np.pi * 9500.0 / FI * t)).astype(np.float32)}


def check_kernel_alone(lib, rate, n=6000):
    """Criterion 7 through the hook: impulses bitwise the f32-rounded taps; noise, a tone above the new Nyquist frequency and rows of
    1, 2 and 37 samples against the yardstick; a ragged batch equals its rows one by one with NaN in the input's padding."""
    L, M = R.ratio(FI, rate)
    h32 = R.taps(L, M).astype(np.float32)
    half = (h32.shape[0] - 1) // 2
    for j0 in (0, n // 2, n - 1):  # (a)
        x = np.zeros((1, n), np.float32)
        x[0, j0] = 1.0
        y, yl, pk = lib.test_resample(x, [n], FI, rate)
        assert int(yl[0]) == R.out_len(n, L, M) == y.shape[1]
        t = np.arange(yl[0], dtype=np.int64) * M - j0 * L + half
        want = np.where((t >= 0) & (t <= 2 * half), h32[np.clip(t, 0, 2 * half)], np.float32(0)).astype(np.float32)
        assert np.array_equal(y[0], want), (rate, j0)
        assert pk[0] == np.max(np.abs(want))
    rng = np.random.default_rng(rate)
    rows = list(signals(n, rng).values()) + [rng.standard_normal(k).astype(np.float32) for k in (1, 2, 37)]
    lens = [len(r) for r in rows]
    x = np.full((len(rows), n + 3), np.nan, np.float32)  # NaN wherever no row has a sample; an odd stride: the unaligned staging path
    for b, r in enumerate(rows):
        x[b, : len(r)] = r
    y, yl, pk = lib.test_resample(x, lens, FI, rate)  # (b), (c)
    assert y.shape[1] == max(int(v) for v in yl)
    # criterion 3 is worst row against worst row (as tests/util.py::f32_grade_vs_fp64): a row of one or two samples has one or two
    # outputs of one or two products each, and the ratio of two such roundings is no statistic.  The tone is judged on its own: its
    # error is of another scale (the output is a fraction of a percent of the input), and it must not hide the other rows'.
    worst = {"tone": [0.0, 0.0], "rest": [0.0, 0.0]}
    for b, r in enumerate(rows):
        no = R.out_len(len(r), L, M)
        assert int(yl[b]) == no and not y[b, no:].any() and np.isfinite(y[b]).all()
        e, f = R.errors(y[b, :no], r, L, M)
        print(f"k_resample {FI} -> {rate} row {b} ({len(r)} samples): engine {e:.3e}  plain f32 {f:.3e}")
        w = worst["tone" if b == 1 else "rest"]
        w[0], w[1] = max(w[0], e), max(w[1], f)
    for name, (e, f) in worst.items():
        assert e <= 3.0 * f, (rate, name, e, f)
    for b, r in enumerate(rows):
        no = R.out_len(len(r), L, M)
        assert pk[b].tobytes() == np.max(np.abs(y[b, :no])).astype(np.float32).tobytes()
        solo, sl, sp = lib.test_resample(np.ascontiguousarray(r[None, :]), [len(r)], FI, rate)  # an aligned, exact-fit row
        assert int(sl[0]) == no and solo[0].tobytes() == y[b, :no].tobytes() and sp[0].tobytes() == pk[b].tobytes(), (rate, b)


def _case(cfg, seed, B=5, Tx=12, one_phoneme_row=1):
    ids, lens, sid = _inputs(cfg, B, Tx, seed=seed, one_phoneme_row=one_phoneme_row)
    return dict(ids=ids, lens=lens, sid=sid, scales=SCALES,
                kw=dict(seed=SEED, utterance_keys=KEYS, pcm_volume=np.array(VOLUMES) / 100.0))


# ------------------------------------------------------------------------------------------ the yardstick itself
def test_the_yardstick_is_scipys_resample_poly():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(5)
    x = rng.standard_normal(3001)
    for rate in RATES + (32000, 88200, 96000):
        L, M = R.ratio(FI, rate)
        mx = max(L, M)
        assert np.max(np.abs(R.taps(L, M) - signal.firwin(20 * mx + 1, 1.0 / mx, window=("kaiser", 5.0)) * L)) <= 1e-12
        for n in (3001, 37, 1):
            want = signal.resample_poly(x[:n], L, M)
            got = R.resample(x[:n], L, M)
            assert got.shape == want.shape == (R.out_len(n, L, M),)
            assert R.rel_rms(got, want) <= 1e-12, (rate, n)


# ------------------------------------------------------------------------------------------ the engine
@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("n_speakers", [1, 4])
def test_engine_results_at_an_output_rate(emu_lib, math, n_speakers):
    """Criteria 1 - 4 on a ragged batch with a one-phoneme row."""
    cfg = VitsConfig.tiny(n_speakers=n_speakers) if n_speakers > 1 else VitsConfig.tiny()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=61, frames_per_id=6.0)), library=emu_lib)
    eng.set_math(math)
    a = _case(cfg, 61)
    native = check_native_untouched(eng, a)
    assert len({int(x) for x in native["lengths"]}) > 1
    eng.profile_enable(True)
    for rate in RATES:
        eng.profile_reset()
        out = run_at(eng, rate, a)
        rep = eng.profile_report()
        assert eng.output_rate == rate == eng.last_rate and rep["resample"]["calls"] == 1
        assert rep["resample"]["bytes"] == 4.0 * float(np.sum(native["lengths"])) + 4.0 * float(np.sum(out["lengths"]))
        check_lengths_and_padding(out, native, rate)
        check_accuracy(out, native, rate)
        check_int16(out, native, rate, VOLUMES)
        # fetch serves the run at the rate it ran at, whatever the handle is set to by then
        eng.set_output_rate(0)
        again = eng.fetch(want_float=True, want_pcm16=True)
        for k in ("audio", "pcm", "lengths", "peaks"):
            assert again[k].tobytes() == out[k].tobytes(), (rate, k)
    back = run_at(eng, 0, a)
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert back[k].tobytes() == native[k].tobytes(), k
    assert eng.config.sample_rate == FI
    eng.close()


@pytest.mark.parametrize("rate", [16000, 48000])
def test_batched_is_alone_at_any_cu_count_and_on_poison(emu_lib, cu_count, rate):
    """Criterion 5: per row bitwise the row alone, at two CU counts (one not a multiple of 8), and the same bytes after the
    workspace was filled with NaN — the edge taps select zeros, they do not read the row's neighbourhood."""
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=62))
    a = _case(cfg, 62)
    forced = np.random.default_rng(62).integers(30, 81, a["ids"].shape).astype(np.int32)  # hop 8: rows of several work items
    a["kw"]["forced_durations"] = forced
    want = None
    for cus in (DEFAULT_CUS, 3):
        cu_count(cus)
        eng = Engine(blob, library=emu_lib)
        big = dict(a, ids=np.tile(a["ids"], (2, 2)), lens=np.tile(a["lens"] * 2, 2), scales=np.tile(SCALES, (2, 1)), sid=None,
                   kw=dict(seed=SEED, utterance_keys=KEYS + KEYS, pcm_volume=np.tile(a["kw"]["pcm_volume"], 2),
                           forced_durations=np.full((10, 24), 80, np.int32)))
        run_at(eng, rate, big)  # sizes the workspace past what the batch needs: the poisoned call cannot reallocate it
        out = run_at(eng, rate, a)
        assert int(np.max(out["lengths"])) > 2 * 1024  # more than two work items in the longest row
        if want is None:
            want = out
            check_rows_alone(lambda: Engine(blob, library=emu_lib), a, rate, out, range(5))
        for pattern in (0x7FC00000, 0xFFFFFFFF):
            eng.fill_workspace(pattern)
            got = run_at(eng, rate, a)
            for k in ("audio", "pcm", "lengths", "peaks"):
                assert got[k].tobytes() == want[k].tobytes(), (cus, hex(pattern), k)
        eng.close()


def test_packed_stream_at_16_khz(emu_lib):
    """Criterion 6: the shapes of test_packed_results.py::test_order_silences_and_header at 16 kHz."""
    cfg = VitsConfig.tiny(n_speakers=4)
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=22, frames_per_id=6.0)), library=emu_lib)
    a = _case(cfg, 22)
    full = run_at(eng, 16000, a)
    order, lead, tail = [3, 0, 4, 1], [1, 0, 777, CHUNK + 453], 5
    pk = eng.run_packed(a["ids"], a["lens"], SCALES, a["sid"], order=order, lead_samples=lead, tail_samples=tail, wav=True, **a["kw"])
    assert pk.sample_rate == 16000
    want = PP.wav_bytes(_chunks(full, order, lead, tail), 16000)
    assert bytes(pk.wav) == want
    pos = 0
    for i, b in enumerate(order):
        pos += lead[i]
        L = int(full["lengths"][b])
        assert int(pk.offsets[i]) == pos and int(pk.lengths[i]) == L
        assert pk.rows[i].tobytes() == full["pcm"][b, :L].tobytes() and pk.peaks[i].tobytes() == full["peaks"][b].tobytes()
        pos += L
    assert pk.total_samples == pos + tail
    mask = np.ones(pk.total_samples, bool)
    for o, n in zip(pk.offsets, pk.lengths):
        mask[int(o): int(o) + int(n)] = False
    assert not pk.pcm[mask].any()
    with wave.open(io.BytesIO(bytes(pk.wav)), "rb") as wf:
        assert (wf.getframerate(), wf.getnchannels(), wf.getsampwidth(), wf.getnframes()) == (16000, 1, 2, pk.total_samples)
        assert wf.readframes(wf.getnframes()) == pk.pcm.tobytes()
    # packed again from the run's float audio, with the handle set back to native meanwhile: still that run's rate
    eng.set_output_rate(0)
    got = eng.fetch_packed(order=order, lead_samples=lead, tail_samples=tail, wav=True)
    assert bytes(got.wav) == want and got.sample_rate == 16000
    # the size limits hold on the resampled sizes, before anything is launched
    eng.set_output_rate(16000)
    with pytest.raises(NativeError, match=r"total_samples exceeds 2\^31 - 1"):
        eng.run_packed(a["ids"], a["lens"], SCALES, a["sid"], tail_samples=2 ** 31 - 1 - int(np.sum(full["lengths"])) + 1, **a["kw"])
    eng.close()


def test_request_wav_counts_breaks_at_the_output_rate(emu_lib):
    cfg = VitsConfig.tiny()
    opts = SessionOptions()
    opts.seed = 11  # both sessions below draw the same noise
    sess = InferenceSession(W.pack(cfg, W.synthetic_weights(cfg, seed=25, frames_per_id=4.0)), opts, _library=emu_lib)
    rng = np.random.default_rng(3)
    sentences = [rng.integers(1, cfg.num_symbols, int(n)).tolist() for n in (7, 1, 11)]
    keys = [901, 17, 33]
    sc = (0.667, 1.1, 0.8)
    rows = []
    for s, k in zip(sentences, keys):
        f1 = {"input": np.array([s], np.int64), "input_lengths": np.array([len(s)], np.int64), "scales": np.array(sc, np.float32)}
        rows.append(sess.run_pcm16(f1, volume=150.0, utterance_keys=[k], sample_rate=8000)[0][0])
    got = PP.request_wav(sess, sentences, break_ms=250.0, scales=sc, volume=150.0, utterance_keys=keys, sample_rate=8000)
    assert got == PP.utterances_to_wav(rows, 8000, break_ms=250.0)
    with wave.open(io.BytesIO(got), "rb") as wf:
        assert wf.getframerate() == 8000
        pcm = np.frombuffer(wf.readframes(wf.getnframes()), "<i2")
    gap = pcm[rows[0].size: rows[0].size + 2000]
    assert gap.size == 2000 and not gap.any() and np.array_equal(pcm[rows[0].size + 2000: rows[0].size + 2000 + rows[1].size], rows[1])
    # the session default: run() and run_pcm16 follow it, a call's sample_rate goes before it
    feed = {"input": np.array([sentences[0]], np.int64), "input_lengths": np.array([7], np.int64), "scales": np.array(sc, np.float32)}
    s16 = InferenceSession(W.pack(cfg, W.synthetic_weights(cfg, seed=25, frames_per_id=4.0)), opts, _library=emu_lib, output_sample_rate=16000)
    native = sess.run_pcm16(feed, utterance_keys=[5])[0][0]
    at16 = s16.run_pcm16(feed, utterance_keys=[5])[0][0]
    assert at16.size == R.out_len(native.size, *R.ratio(FI, 16000))
    assert np.array_equal(at16, sess.run_pcm16(feed, utterance_keys=[5], sample_rate=16000)[0][0])
    assert np.array_equal(native, s16.run_pcm16(feed, utterance_keys=[5], sample_rate=FI)[0][0])
    det = dict(feed, scales=np.array([0.0, 1.1, 0.0], np.float32))  # run() draws its own key: no noise, equal durations
    assert s16.run(None, det)[0].shape == (1, 1, R.out_len(sess.run(None, det)[0].shape[2], *R.ratio(FI, 16000)))
    pk = s16.run_packed(feed, lead_ms=[250.0], utterance_keys=[5])
    assert pk.sample_rate == 16000 and int(pk.offsets[0]) == 4000 and np.array_equal(pk.rows[0], at16)
    with pytest.raises(InvalidArgument, match="22051"):
        InferenceSession(W.pack(cfg, W.synthetic_weights(cfg, seed=25)), _library=emu_lib, output_sample_rate=22051)
    sess.close()
    s16.close()


@pytest.mark.parametrize("rate", HOOK_RATES)
def test_the_kernel_alone(emu_lib, rate):
    check_kernel_alone(emu_lib, rate)


def test_the_kernel_alone_at_an_extreme_ratio(emu_lib, cu_count):
    """441 : 1 (50 Hz): a phase of 8,821 taps and tiles of a few dozen outputs; and 96 kHz, the largest table, at an odd CU count."""
    check_kernel_alone(emu_lib, 50, n=30000)
    cu_count(5)
    check_kernel_alone(emu_lib, 96000, n=3000)
    with pytest.raises(NativeError):
        emu_lib.test_resample(np.zeros((1, 8), np.float32), [8], FI, 22051)


def test_bad_rates_clone_and_the_micro_batcher(emu_lib):
    """Criterion 8."""
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=63, frames_per_id=4.0))
    eng = Engine(blob, library=emu_lib)
    a = _case(cfg, 63)
    eng.set_output_rate(16000)
    before = run_at(eng, None, a)
    for hz, message in ((-1, r"output rate -1 Hz"), (22051, r"output rate 22051 Hz = 22051 / 22050"), (7, r"output rate 7 Hz = 1 / 3150")):
        with pytest.raises(NativeError, match=message) as e:
            eng.set_output_rate(hz)
        assert e.value.code == -1 and eng.output_rate == 16000
    after = run_at(eng, None, a)
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert after[k].tobytes() == before[k].tobytes(), k
    lane = eng.clone()
    assert lane.output_rate == 16000
    cloned = run_at(lane, None, a)
    assert cloned["pcm"].tobytes() == before["pcm"].tobytes()
    lane.set_output_rate(0)
    assert lane.output_rate == FI and eng.output_rate == 16000
    lane.close()
    eng.close()
    # the rate is not a per-row setting: requests of different rates never share an engine call
    assert "sample_rate" not in _ROW_SETTINGS
    opts = SessionOptions()
    opts.micro_batch_window_ms = 200.0
    sess = InferenceSession(blob, opts, _library=emu_lib)
    calls = []
    inner = sess._engine_run

    def spy(ids, lengths, scales, sid, **kw):
        calls.append((int(ids.shape[0]), kw.get("sample_rate")))
        return inner(ids, lengths, scales, sid, **kw)

    sess._engine_run = spy
    rng = np.random.default_rng(9)
    reqs = [(rng.integers(1, cfg.num_symbols, (1, 9)), rate, 100 + i) for i, rate in enumerate([None, 16000, 8000, 16000, None, 8000])]
    feeds = [{"input": ids, "input_lengths": np.array([9], np.int64), "scales": np.array([0.667, 1.0, 0.8], np.float32)} for ids, _, _ in reqs]
    sess.run_pcm16(feeds[0], utterance_keys=[1])  # a first call: the dispatcher is no longer idle-fresh
    results = [None] * len(reqs)
    hold = sess._free_lanes.acquire()  # every request queues behind the one lane, so the dispatcher sees them together

    def work(i):
        results[i] = sess.run_pcm16(feeds[i], utterance_keys=[reqs[i][2]], sample_rate=reqs[i][1])[0][0]

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(reqs))]
    calls.clear()
    for t in threads:
        t.start()
    import time

    time.sleep(0.5)
    sess._free_lanes.release(hold)
    for t in threads:
        t.join()
    rows_at = {}
    for n, r in calls:  # an engine call has ONE rate: its rows are all requests of that rate
        rows_at[r] = rows_at.get(r, 0) + n
    assert rows_at == {None: 2, 16000: 2, 8000: 2} and len(calls) < len(reqs), calls  # batched, never across rates
    sess._engine_run = inner
    for i, (ids, rate, key) in enumerate(reqs):
        solo = sess.run_pcm16(feeds[i], utterance_keys=[key], sample_rate=rate, direct=True)[0][0]
        assert np.array_equal(results[i], solo), i
        L, M = R.ratio(FI, rate or FI)
        native = sess.run_pcm16(feeds[i], utterance_keys=[key], direct=True)[0][0]
        assert solo.size == R.out_len(native.size, L, M)
    sess.close()


def test_plain_c99_clients(emu_lib, tmp_path):
    """Criterion 9: a C99 client sets 16 kHz and checks lengths and the WAV header's rate field; the header stays C99-clean."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_rate_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_rate_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir], check=True)
    cfg = VitsConfig.tiny()
    w = W.synthetic_weights(cfg, seed=17)
    W.save(str(tmp_path / "voice.m355"), cfg, w)
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355"), str(tmp_path / "out.wav")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "expected failure rc=-1" in p.stdout and "22051 / 22050" in p.stdout
    ids = np.array([[3, 7, 1, 9, 4], [5, 2, 0, 0, 0], [8, 6, 4, 2, 0]])
    eng = Engine(W.pack(cfg, w), library=emu_lib)
    eng.set_output_rate(16000)
    full = eng.run(ids, [5, 2, 4], [0, 1, 0], want_pcm16=True)
    assert open(tmp_path / "out.wav", "rb").read() == PP.wav_bytes(_chunks(full, [2, 0], [3, 101], 7), 16000)
    eng.close()
