"""Edge trimming of the packed streams (mi355vits_set_edge_trim / mi355vits_fetch_edges, k_edges) on the CPU model of the kernels;
test_gpu_edge_trim.py runs the same contract on the MI355X.

The yardstick, never the code under test: numpy on the WANT_FLOAT audio and the peaks OF THE SAME RUN —
``np.flatnonzero(np.abs(y) >= np.float32(p) * np.float32(ratio))``, one f32 multiply and f32 compares, then ``keep`` and the clamps
in Python ints.  A trimmed entry is compared bit for bit with the slice of the UNTRIMMED ``fetch_packed`` stream of the same run; a
trimmed file with the one ``postprocess.wav_bytes`` builds from those slices.  Everything is exact: there is no tolerance in this file.

Not tested: a size limit (2^31 - 1 samples, RIFF's 32-bit fields) that only the UNTRIMMED stream exceeds.  The limits are checked on
the trimmed sizes by the same ``check_pack_size`` calls in ``place_pack``, but there is no hook that forces small limits, and a
stream of 2^31 samples is out of a test's reach."""
import ctypes
import struct

import numpy as np
import pytest

from mimic3_amd import postprocess as PP
from mimic3_amd import weights as W
from mimic3_amd._native import Edges, EdgesResult, Engine, NativeError
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests.test_resample import FI, _case, run_at

RATES = (0, 8000, 48000)
ENCODINGS = ("s16le", "ulaw", "alaw", "f32le")
SILENCE = {"s16le": 0, "ulaw": 0xFF, "alaw": 0xD5, "f32le": 0}  # the code of sample 0; the bits of 0.0f
SETTINGS = ((0.5, 0), (0.5, 37), (0.9, 0), (0.9, 37))
NAN = 0x7FC00000
TILE_SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 70001)


# ------------------------------------------------------------------------------------------ the yardstick
def loud_edges(y, peak, ratio):
    """(s_first, s_last) of one row by the rule: n / -1 when no sample is loud."""
    y = np.asarray(y, np.float32)
    thr = np.float32(peak) * np.float32(ratio)
    assert thr.dtype == np.float32
    loud = np.flatnonzero(np.abs(y) >= thr)
    return (int(loud[0]), int(loud[-1])) if loud.size else (int(y.shape[0]), -1)


def rule(out, ratio, keep):
    """first / end [B] of a padded result (WANT_FLOAT audio, lengths, peaks of one run)."""
    first, end = [], []
    for b, n in enumerate(int(x) for x in out["lengths"]):
        s_first, s_last = loud_edges(out["audio"][b, :n], out["peaks"][b], ratio)
        first.append(max(0, s_first - keep))
        end.append(min(n, s_last + 1 + keep))
    return np.array(first, np.int64), np.array(end, np.int64)


# ------------------------------------------------------------------------------------------ checks shared with the GPU twin
def check_kernel_alone(lib):
    """Criterion 1: constructed rows at the tile and lane edges, an odd stride (row bases on every 4-byte alignment), NaN and then
    3e38 behind every row; s_first / s_last equal the numpy rule exactly, and the named cases give the named answers."""
    ratio = np.float32(0.3)
    pk = np.float32(0.7)
    thr = pk * ratio  # of the rows that hold a sample at / just below the threshold
    below = np.nextafter(thr, np.float32(0))
    assert below < thr
    rows = []  # (n, peak, {index: value}, background, expected or None)
    for n in TILE_SIZES:
        rows.append((n, 1.0, {0: 1.0}, 0.29, (0, 0)))                                   # only sample 0 loud
        rows.append((n, 1.0, {n - 1: 1.0}, 0.29, (n - 1, n - 1)))                       # only sample n - 1 loud
        rows.append((n, 1.0, {n // 2: -1.0}, 0.29, (n // 2, n // 2)))                   # a negative loud sample
        rows.append((n, 0.0, {}, 0.0, (0, n - 1)))                                      # all zeros, peak 0: every sample loud
        rows.append((n, float(pk), {n // 3: float(thr)}, 0.0, (n // 3, n // 3)))        # exactly at thr: found
        rows.append((n, float(pk), {n // 3: float(below)}, 0.0, (n, -1)))               # the f32 just below: not found, so none
        if n >= 15:
            rows.append((n, float(pk), {2 * n // 3: -float(thr), n // 5: float(below)}, 0.0, (2 * n // 3, 2 * n // 3)))
        if n > 6144:
            rows.append((n, 1.0, {6144: 1.0}, 0.29, (6144, 6144)))                      # one loud sample in the middle of the second tile
        if n >= 8193:
            rows.append((n, 1.0, {5: 1.0, n - 3: -1.0}, 0.29, (5, n - 3)))              # loud in the first and in the last tile only
        rows.append((n, 1.0, {n // 2: float("nan"), n - 1: 0.5}, 0.29, (n - 1, n - 1)))  # a NaN among the valid samples is not loud
    rows.append((0, 1.0, {}, 0.0, (0, -1)))                                             # an empty row
    B = len(rows)
    stride = max(TILE_SIZES) + 2
    assert stride % 2 == 1
    lens = np.array([r[0] for r in rows], np.int32)
    peaks = np.array([r[1] for r in rows], np.float32)
    for fill in (np.float32("nan"), np.float32(3e38)):
        audio = np.full((B, stride), fill, np.float32)
        for b, (n, _, marks, bg, _) in enumerate(rows):
            audio[b, :n] = bg * np.where(np.arange(n) % 2, -1.0, 1.0)
            for k, v in marks.items():
                audio[b, k] = v
        first, last = lib.lab_edges(audio, lens, peaks, ratio)
        assert first.dtype == last.dtype == np.int32
        for b, (n, p, _, _, expected) in enumerate(rows):
            want = loud_edges(audio[b, :n], p, ratio)
            assert want == expected, (b, n, want, expected)  # the yardstick agrees with the construction
            assert (int(first[b]), int(last[b])) == want, (b, n, rows[b][2], (int(first[b]), int(last[b])), want)
    # random rows, a ratio of 1 (only the peak itself) and one close to 0
    rng = np.random.default_rng(7)
    lens = np.array([4097, 9000, 33, 12288, 5], np.int32)
    audio = np.full((5, 12291), np.nan, np.float32)
    for b, n in enumerate(lens):
        audio[b, :n] = rng.standard_normal(int(n)).astype(np.float32)
    peaks = np.array([np.max(np.abs(audio[b, :n])) for b, n in enumerate(lens)], np.float32)
    for r in (1.0, 0.75, 1e-6):
        first, last = lib.lab_edges(audio, lens, peaks, r)
        for b, n in enumerate(lens):
            assert (int(first[b]), int(last[b])) == loud_edges(audio[b, :n], peaks[b], r), (r, b)
        if r == 1.0:
            assert all(abs(audio[b, first[b]]) == peaks[b] for b in range(5))


def packs_of(eng, pack):
    """fetch_packed of the last run in the four encodings under the engine's current trim setting."""
    out = {}
    for enc in ENCODINGS:
        eng.set_output_encoding(enc)
        out[enc] = eng.fetch_packed(**pack)
    eng.set_output_encoding("s16le")
    return out


def same_stream(x, y):
    assert bytes(x.wav if x.wav is not None else x.data) == bytes(y.wav if y.wav is not None else y.data)
    assert x.data.tobytes() == y.data.tobytes()
    assert np.array_equal(x.offsets, y.offsets) and np.array_equal(x.lengths, y.lengths) and x.peaks.tobytes() == y.peaks.tobytes()
    assert x.total_samples == y.total_samples and x.encoding == y.encoding and x.sample_rate == y.sample_rate


def check_off_is_off(make_engine, a):
    """Criterion 2: unset, and set and then set back to 0 — run_packed and fetch_packed are those of a fresh handle in the four
    encodings, no `edges` line is profiled, fetch_edges gives first = 0 and end = lengths."""
    pack = dict(order=[2, 0, 1], lead_samples=[5, 0, 3], tail_samples=2, wav=True)
    fresh, eng = make_engine(), make_engine()
    assert eng.edge_trim == (0.0, 0)
    eng.set_edge_trim(0.5, 9)
    assert eng.edge_trim == (0.5, 9)
    eng.set_edge_trim(0.0, 0)
    eng.profile_enable(True)
    eng.profile_reset()
    for enc in ENCODINGS:
        for e in (fresh, eng):
            e.set_output_encoding(enc)
        want = fresh.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **a["kw"])
        got = eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **a["kw"])
        same_stream(got, want)
        same_stream(eng.fetch_packed(**pack), fresh.fetch_packed(**pack))
        assert got.first is None and got.end is None
    e = eng.fetch_edges()
    assert isinstance(e, Edges) and e.ratio == 0.0 and e.keep_samples == 0 and e.sample_rate == eng.config.sample_rate
    assert not e.first.any() and np.array_equal(e.end, eng.fetch(want_float=False)["lengths"])
    assert "edges" not in eng.profile_report()
    eng.set_edge_trim(0.0, 12)  # a ratio of 0 is off whatever keep says
    same_stream(eng.fetch_packed(**pack), fresh.fetch_packed(**pack))
    assert "edges" not in eng.profile_report()
    eng.profile_enable(False)
    fresh.close()
    eng.close()


def wav_fields(wav, enc):
    """(RIFF size, fact count or None, data size) of a packed file's header."""
    wav = bytes(wav)
    assert wav[:4] == b"RIFF" and wav[8:12] == b"WAVE"
    riff = struct.unpack_from("<I", wav, 4)[0]
    if enc == "s16le":
        assert wav[36:40] == b"data"
        return riff, None, struct.unpack_from("<I", wav, 40)[0]
    assert wav[38:42] == b"fact" and wav[50:54] == b"data"
    return riff, struct.unpack_from("<I", wav, 46)[0], struct.unpack_from("<I", wav, 54)[0]


def check_trimmed_pack(got, plain, first, end, order, lead, tail, enc, rate):
    """One trimmed stream against the untrimmed stream of the same run and the edges of the numpy rule."""
    n = len(order)
    f, e = first[order], end[order]
    assert np.array_equal(got.first, f) and np.array_equal(got.end, e)
    assert np.array_equal(got.lengths, e - f)
    offsets = np.cumsum(np.asarray(lead, np.int64) + np.concatenate(([0], (e - f)[:-1])))
    assert np.array_equal(got.offsets, offsets)
    total = int(offsets[-1] + (e - f)[-1] + tail)
    assert got.total_samples == total == got.data.shape[0]
    assert got.peaks.tobytes() == plain.peaks.tobytes()  # the row's peak as before
    chunks, covered = [], np.zeros(total, bool)
    for i in range(n):
        want = plain.rows[i][int(f[i]): int(e[i])]
        assert got.rows[i].tobytes() == want.tobytes(), (enc, i)  # bitwise [first, end) of the untrimmed entry
        covered[int(offsets[i]): int(offsets[i] + e[i] - f[i])] = True
        chunks += [np.full(int(lead[i]), SILENCE[enc], got.data.dtype), want]
    chunks.append(np.full(int(tail), SILENCE[enc], got.data.dtype))
    rest = got.data[~covered]
    assert rest.size == int(np.sum(lead)) + tail and (rest.view(np.uint32 if enc == "f32le" else rest.dtype) == SILENCE[enc]).all()
    bps = got.data.dtype.itemsize
    riff, fact, data = wav_fields(got.wav, enc)
    pad = (bps * total) & 1
    assert data == bps * total and len(got.wav) == (44 if enc == "s16le" else 58) + data + pad
    assert riff == len(got.wav) - 8 and (fact is None if enc == "s16le" else fact == total)
    assert bytes(got.wav) == PP.wav_bytes(chunks, rate, enc)  # the file a host builds by slicing and re-joining


def check_trimmed_streams(eng, a, rate, order, vacuity=True):
    """Criterion 3 at one rate: the edges equal the numpy rule; every trimmed stream (two ratios x two keeps x four encodings, a
    permuted order with lead / tail silences and a header) is the untrimmed one cut; a trimmed run_packed is the trimmed
    fetch_packed; keep = 10^6 cuts nothing; ratio = 1."""
    out = run_at(eng, rate, a)
    hz = rate or eng.config.sample_rate
    n = len(order)
    rng = np.random.default_rng(n)
    lead = [int(x) for x in rng.integers(0, 50, n)]
    lead[1] = 0
    pack = dict(order=order, lead_samples=lead, tail_samples=7, wav=True)
    order = np.asarray(order)
    eng.set_edge_trim(0.0)
    plain = packs_of(eng, pack)
    lengths = out["lengths"].astype(np.int64)
    for ratio, keep in SETTINGS + ((1.0, 0), (0.5, 10 ** 6)):
        first, end = rule(out, ratio, keep)
        assert (end - first >= 1).all()
        if vacuity and keep == 0 and ratio == 0.5:  # what keeps this test from passing vacuously, on the numpy side
            assert np.count_nonzero((first > 0) & (end < lengths)) * 4 >= 3 * len(lengths), (first, lengths - end)
        if vacuity and keep == 0 and ratio == 0.9:
            assert max(int(first.max()), int((lengths - end).max())) > 1024, (first, lengths - end)
        print(f"{hz} Hz ratio {ratio} keep {keep}: cut {int(first.min())} .. {int(first.max())} in front, "
              f"{int((lengths - end).min())} .. {int((lengths - end).max())} behind")
        eng.set_edge_trim(ratio, keep)
        e = eng.fetch_edges()
        assert e.first.dtype == e.end.dtype == np.int32 and e.sample_rate == hz and e.keep_samples == keep
        assert np.float32(e.ratio) == np.float32(ratio)
        assert np.array_equal(e.first, first) and np.array_equal(e.end, end), (ratio, keep)
        got = packs_of(eng, pack)
        for enc in ENCODINGS:
            check_trimmed_pack(got[enc], plain[enc], first, end, order, lead, 7, enc, hz)
            if keep == 10 ** 6:
                same_stream(got[enc], plain[enc])
    # the one-call form: synthesis, edges and pack in one mi355vits_run_packed
    eng.set_edge_trim(0.5, 37)
    want = packs_of(eng, pack)
    for enc in ("s16le", "ulaw"):
        eng.set_output_encoding(enc)
        got = eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **a["kw"])
        same_stream(got, want[enc])
        assert np.array_equal(got.first, want[enc].first) and np.array_equal(got.end, want[enc].end)
    eng.set_output_encoding("s16le")
    after = eng.fetch(want_float=True)  # the run a trimmed run_packed leaves behind is the run itself
    for k in ("audio", "lengths", "peaks"):
        assert after[k].tobytes() == out[k].tobytes(), k
    eng.set_edge_trim(0.0)


def check_rows_alone(make_engine, a, rate, rows, batched, ratio=0.9, keep=5):
    """Criterion 4: a row run alone gives the first / end and the entry bytes it gives in the batch (`batched`: the trimmed int16
    pack of the whole batch in row order)."""
    eng = make_engine()
    eng.set_output_rate(rate)
    eng.set_edge_trim(ratio, keep)
    for b in rows:
        n = int(a["lens"][b])
        kw = dict(a["kw"])
        kw["utterance_keys"] = [kw["utterance_keys"][b]]
        kw["pcm_volume"] = float(np.asarray(kw["pcm_volume"]).reshape(-1)[b])
        if "forced_durations" in kw:
            kw["forced_durations"] = kw["forced_durations"][b:b + 1, : max(n, 1)]
        solo = eng.run_packed(a["ids"][b:b + 1, : max(n, 1)], [n], a["scales"][b], None, **kw)
        assert int(solo.first[0]) == int(batched.first[b]) and int(solo.end[0]) == int(batched.end[b]), b
        assert solo.rows[0].tobytes() == batched.rows[b].tobytes(), b
        e = eng.fetch_edges()
        assert int(e.first[0]) == int(batched.first[b]) and int(e.end[0]) == int(batched.end[b])
    eng.close()


def trimmed_batch(eng, a, rate, ratio=0.9, keep=5):
    """The trimmed int16 pack of a batch in row order, its edges checked against the rule."""
    out = run_at(eng, rate, a)
    eng.set_edge_trim(ratio, keep)
    got = eng.fetch_packed()
    first, end = rule(out, ratio, keep)
    assert np.array_equal(got.first, first) and np.array_equal(got.end, end)
    assert np.count_nonzero((first > 0) & (end < out["lengths"])) * 2 >= len(first)  # (numpy side) most rows lose both edges
    eng.set_edge_trim(0.0)
    return got


def check_nothing_else_moves(eng, a, rate):
    """Criterion 5: with trimming set, run / run_rows (per-row scales), fetch with both flags, fetch_alignment with levels and the
    device_result lengths are bitwise the same handle's with trimming off; unchanged after a fetch_edges and after a trimmed
    fetch_packed; trimmed and untrimmed fetch_packed of one run alternate."""
    def served():
        f = eng.fetch(want_float=True, want_pcm16=True)
        al = eng.fetch_alignment(levels=True)
        d = eng.device_result()
        return ([f[k].tobytes() for k in ("audio", "pcm", "lengths", "peaks")] + [int(f["l_max"])] +
                [getattr(al, k).tobytes() for k in ("frames", "start", "samples", "peak", "rms")] + [d["row_stride"], d["batch"]])

    eng.set_edge_trim(0.0)
    off = run_at(eng, rate, a)
    want = served()
    plain = bytes(eng.fetch_packed(wav=True).wav)
    eng.set_edge_trim(0.9, 3)
    on = run_at(eng, rate, a)
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert on[k].tobytes() == off[k].tobytes(), k
    assert served() == want
    eng.profile_enable(True)
    eng.profile_reset()
    e = eng.fetch_edges()
    rep = eng.profile_report()
    assert rep["edges"]["calls"] == 1 and rep["edges"]["bytes"] == 4.0 * float(np.sum(off["lengths"])) + 8.0 * len(off["lengths"])
    assert served() == want
    trimmed = bytes(eng.fetch_packed(wav=True).wav)
    assert eng.profile_report()["edges"]["calls"] == 1  # the edges of this run at this ratio are held on the host
    eng.profile_enable(False)
    assert len(trimmed) < len(plain) and served() == want
    first, end = rule(off, 0.9, 3)
    assert np.array_equal(e.first, first) and np.array_equal(e.end, end) and int(np.sum(end - first)) < int(np.sum(off["lengths"]))
    for _ in range(2):  # one synthesis, packed trimmed and untrimmed in turn
        eng.set_edge_trim(0.0)
        assert bytes(eng.fetch_packed(wav=True).wav) == plain
        eng.set_edge_trim(0.9, 3)
        assert bytes(eng.fetch_packed(wav=True).wav) == trimmed
    eng.set_edge_trim(0.5, 0)  # another threshold, no synthesis repeated
    f9, e9 = rule(off, 0.5, 0)
    p9 = eng.fetch_packed()
    assert np.array_equal(p9.first, f9) and np.array_equal(p9.end, e9) and served() == want
    eng.set_edge_trim(0.0)


def check_errors(make_engine, a):
    """Criterion 7 at the C ABI."""
    eng = make_engine()
    lib = eng.native.lib
    with pytest.raises(NativeError, match="fetch_edges: no completed run on this handle") as err:
        eng.fetch_edges()
    assert err.value.code == -1
    assert lib.mi355vits_fetch_edges(eng._h, None) == -1
    eng.set_edge_trim(0.25, 5)
    for bad, name in ((float("nan"), "nan"), (-0.1, "-0.1"), (1.5, "1.5")):
        with pytest.raises(NativeError, match="ratio") as err:
            eng.set_edge_trim(bad, 3)
        assert err.value.code == -1 and name in str(err.value).lower()
        assert eng.edge_trim == (0.25, 5)
    with pytest.raises(NativeError, match="keep_samples -2"):
        eng.set_edge_trim(0.5, -2)
    assert eng.edge_trim == (0.25, 5)
    twin = eng.clone()  # a further lane inherits the setting
    assert twin.edge_trim == (0.25, 5)
    twin.close()
    run_at(eng, 0, a)
    assert lib.mi355vits_fetch_edges(eng._h, None) == -1
    r = EdgesResult()
    assert lib.mi355vits_fetch_edges(eng._h, ctypes.byref(r)) == 0 and r.batch == a["ids"].shape[0] and r.keep_samples == 5
    lib.mi355vits_free_edges(ctypes.byref(r))
    assert not r.first and not r.owner_
    lib.mi355vits_free_edges(ctypes.byref(r))  # freeing twice is harmless
    eng.set_edge_trim(1.0, 0)  # the largest ratio is legal
    e = eng.fetch_edges()
    assert (e.end - e.first >= 1).all()
    # a run that fails after its launch sequence began leaves no result: trimmed run_packed as any other run
    with pytest.raises(NativeError):
        eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), forced_durations=np.full(a["ids"].shape, 1 << 23, np.int32))
    with pytest.raises(NativeError, match="fetch_edges: no completed run on this handle"):
        eng.fetch_edges()
    eng.close()


def check_session(sess, a, rate=8000):
    """Criterion 6 and the Python surface: trim_db / trim_keep_ms reach the lane and go back to off; the alignment of a trimmed
    stream follows the cut."""
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    B = a["ids"].shape[0]
    keys = list(range(21, 21 + B))
    order = [2, 0, 1][:B] + list(range(3, B))
    db = -1.0  # the synthetic voices are noise-like: a real voice's -40 dB cuts nothing there
    rows, lengths, al = sess.run_pcm16(feed, sample_rate=rate, alignment="levels", utterance_keys=keys)
    plain = sess.run_packed(feed, order=order, lead_ms=[20.0] * B, sample_rate=rate, utterance_keys=keys, alignment="levels")
    assert plain.first is None and plain.end is None
    got = sess.run_packed(feed, order=order, lead_ms=[20.0] * B, sample_rate=rate, utterance_keys=keys, alignment="levels",
                          trim_db=db, trim_keep_ms=2.0)
    ratio, keep = float(np.float32(10.0 ** (db / 20.0))), int((2.0 / 1000.0) * rate)
    ta = got.alignment
    cut = 0
    for i, b in enumerate(order):
        f, e = int(got.first[i]), int(got.end[i])
        assert got.rows[i].tobytes() == rows[b][f:e].tobytes()
        # the edges are those of the rule over the float waveform: checked at the engine; here the keep and the ratio arrived
        assert int(got.lengths[i]) == e - f and 0 <= f < e <= int(lengths[b])
        assert int(got.offsets[i]) - (int(got.offsets[i - 1] + got.lengths[i - 1]) if i else 0) == int(0.02 * rate)  # the pause asked for
        s, n = ta.start[i].astype(np.int64), ta.samples[i].astype(np.int64)
        assert int(s[0]) == int(got.offsets[i]) and np.array_equal(s[1:], s[:-1] + n[:-1]) and int(n.sum()) == int(got.lengths[i])  # the spans tile the entry
        assert np.array_equal(ta.frames[i], al.frames[b]) and ta.peak[i].tobytes() == al.peak[b].tobytes() and ta.rms[i].tobytes() == al.rms[b].tobytes()
        for t in range(int(a["lens"][b])):
            r0, rn = int(al.start[b, t]), int(al.samples[b, t])
            if r0 >= f and r0 + rn <= e:  # wholly inside: the stream slice is the row slice
                assert int(n[t]) == rn and got.data[int(s[t]): int(s[t]) + rn].tobytes() == rows[b][r0: r0 + rn].tobytes()
            elif r0 + rn <= f or r0 >= e:  # wholly cut
                assert int(n[t]) == 0
                cut += rn > 0
            else:
                assert 0 < int(n[t]) < rn
    assert cut > 0  # some phoneme was cut away entirely
    assert got.total_samples < plain.total_samples
    again = sess.run_packed(feed, order=order, lead_ms=[20.0] * B, sample_rate=rate, utterance_keys=keys)  # the lane is back to off
    assert again.first is None and again.data.tobytes() == plain.data.tobytes()
    e = sess._engines[0].edge_trim
    assert e == (0.0, 0)
    got2 = sess.run_packed(feed, order=order, lead_ms=[20.0] * B, sample_rate=rate, utterance_keys=keys, trim_db=db, trim_keep_ms=2.0)
    assert sess._engines[0].edge_trim == (ratio, keep) and got2.data.tobytes() == got.data.tobytes()
    wav = PP.request_wav(sess, [a["ids"][b, : int(a["lens"][b])] for b in range(B)], break_ms=20.0, sample_rate=rate, utterance_keys=keys,
                         trim_db=db, trim_keep_ms=2.0)
    want = sess.run_packed(feed, lead_ms=[0.0] + [20.0] * (B - 1), wav=True, sample_rate=rate, utterance_keys=keys, trim_db=db, trim_keep_ms=2.0)
    assert wav == bytes(want.wav)
    for bad in (0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sess.run_packed(feed, trim_db=bad)
    with pytest.raises(ValueError):
        sess.run_packed(feed, trim_db=-3.0, trim_keep_ms=-1.0)


# ------------------------------------------------------------------------------------------ the engine on the CPU model
FORCED_SEED = 7


def _engine(seed=81):
    cfg = VitsConfig.tiny()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=seed, frames_per_id=6.0))


def _long_case(cfg, seed, B=5):
    """`_case` with forced durations of 25 .. 70 frames a phoneme: rows of a few thousand samples at the tiny voice's hop of 8, so
    that a cut can pass 1,024 samples and a row several tiles of the kernel."""
    a = _case(cfg, seed, B=B)
    a["kw"]["forced_durations"] = np.random.default_rng(seed + FORCED_SEED).integers(25, 71, a["ids"].shape).astype(np.int32)
    return a


def test_the_kernel_alone(emu_lib):
    check_kernel_alone(emu_lib)
    with pytest.raises(NativeError):  # a length past the stride: refused before anything is launched
        emu_lib.lab_edges(np.zeros((1, 8), np.float32), [9], [1.0], 0.5)
    with pytest.raises(NativeError):
        emu_lib.lab_edges(np.zeros((1, 8), np.float32), [8], [1.0], 0.0)


def test_off_is_off(emu_lib):
    cfg, blob = _engine()
    check_off_is_off(lambda: Engine(blob, library=emu_lib), _case(cfg, 81))


@pytest.mark.parametrize("rate", RATES)
def test_trimmed_streams(emu_lib, rate):
    """Criterion 3.  This fails without the feature."""
    cfg, blob = _engine(82)
    eng = Engine(blob, library=emu_lib)
    check_trimmed_streams(eng, _long_case(cfg, 82), rate, [3, 0, 4, 1, 2])
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_batched_is_alone_and_on_a_poisoned_workspace(emu_lib, rate):
    cfg, blob = _engine(83)
    a = _long_case(cfg, 83)
    eng = Engine(blob, library=emu_lib)
    want = trimmed_batch(eng, a, rate)
    check_rows_alone(lambda: Engine(blob, library=emu_lib), a, rate, range(5), want)
    big = dict(a, ids=np.tile(a["ids"], (2, 2)), lens=np.tile(a["lens"] * 2, 2), scales=np.tile(a["scales"], (2, 1)), sid=None,
               kw=dict(seed=1, forced_durations=np.full((10, 24), 70, np.int32)))
    run_at(eng, rate, big)
    eng.set_edge_trim(0.9, 5)
    eng.fetch_packed()  # sizes the edges' and the pack's own arenas past what the batch needs
    eng.fill_workspace(NAN)
    got = trimmed_batch(eng, a, rate)
    same_stream(got, want)
    assert np.array_equal(got.first, want.first) and np.array_equal(got.end, want.end)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_nothing_else_moves(emu_lib, rate):
    cfg, blob = _engine(84)
    eng = Engine(blob, library=emu_lib)
    check_nothing_else_moves(eng, _long_case(cfg, 84), rate)
    eng.close()


def test_errors(emu_lib):
    cfg, blob = _engine(85)
    check_errors(lambda: Engine(blob, library=emu_lib), _case(cfg, 85))


def test_session_trim_and_alignment_in_a_trimmed_stream(emu_lib):
    cfg, blob = _engine(86)
    opts = SessionOptions()
    opts.seed = 5
    sess = InferenceSession(blob, opts, _library=emu_lib)
    check_session(sess, _case(cfg, 86, B=3, Tx=9), rate=8000)
    sess.close()
    with pytest.raises(ValueError):
        InferenceSession(blob, opts, _library=emu_lib, edge_trim_db=3.0)
    sess = InferenceSession(blob, opts, _library=emu_lib, edge_trim_db=-1.0, edge_trim_keep_ms=1.0)  # the session's own default
    a = _case(cfg, 86, B=3, Tx=9)
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    got = sess.run_packed(feed, utterance_keys=[1, 2, 3])
    assert got.first is not None and sess._engines[0].edge_trim == (float(np.float32(10.0 ** (-1.0 / 20.0))), int(0.001 * FI))
    sess.close()
