"""Loudness of a run's rows and the target gain of the packed streams (mi355vits_set_loudness_target / mi355vits_fetch_loudness,
k_loud / k_loud_gate) on the CPU model of the kernels; test_gpu_loudness.py runs the same contract on the MI355X.

The yardstick is tests/loudness_ref.py — numpy from the definitions of include/mi355vits.h, never the code under test — applied to
the WANT_FLOAT audio and the peaks OF THE SAME RUN.  Tolerances:
 * lufs: 1e-6 LU, derived and not measured: double arithmetic plus the 2^-40 warm-up truncation give dE / E <~ 1e-12, hence
   dL = 4.3 dE / E ~ 1e-11; 1e-6 leaves five orders for summation order and FMA contraction and sits five orders under the 0.1 LU a
   meter displays.  blocks and gated are exact, under the CONDITION (asserted on the reference) that no block of a constructed row
   lies within 1e-3 LU of a gate; in the engine tests a row whose reference has a block within 1e-6 LU of a gate is left out of the
   lufs comparison, at most one row of a batch.
 * gain: relative 1e-12 against the gain rule applied to the FETCHED lufs and peaks (two pow() of different libraries); limited exact.
 * every sample of a stream: bit for bit the numpy pcm16_quant of the run's float samples under np.float32(32767.0 * gain) built
   from the fetched gain, then the G.711 tables of tests/g711_ref.py; f32le is x * np.float32(gain).

Not tested: the number of stream synchronisations of a call (no hook counts them)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mimic3_amd import postprocess as PP
from mimic3_amd import weights as W
from mimic3_amd._native import Engine, Loudness, LoudnessResult, NativeError
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests import g711_ref as G
from tests import loudness_ref as R
from tests.test_resample import DEFAULT_CUS, _case, run_at

RATES = (0, 8000, 48000)
KERNEL_RATES = (8000, 22050, 48000)
ENCODINGS = ("s16le", "ulaw", "alaw", "f32le")
SILENCE = {"s16le": 0, "ulaw": 0xFF, "alaw": 0xD5, "f32le": 0}  # the code of sample 0; the bits of 0.0f
TARGETS = ((-23.0, -1.0), (-10.0, -6.0))
AMPLITUDES = (0.3, 1e-3, 0.3, 0.2, 1e-5, 0.25, 0.3, 0.05, 0.3)
LU_TOL = 1e-6
NAN = 0x7FC00000
FORCED_SEED = 7


# ------------------------------------------------------------------------------------------ the yardstick itself
def test_the_coefficients_at_48_khz_are_the_table_of_bs_1770():
    (b1, a1), (b2, a2) = R.k_weighting(48000)
    assert np.max(np.abs(b1 - [1.53512485958697, -2.69169618940638, 1.19839281085285])) <= 1e-12
    assert np.max(np.abs(a1 - [1.0, -1.69065929318241, 0.73248077421585])) <= 1e-12
    assert np.max(np.abs(b2 - [1.0, -2.0, 1.0])) == 0.0
    assert np.max(np.abs(a2 - [1.0, -1.99004745483398, 0.99007225036621])) <= 1e-12


def test_the_yardsticks_filter_is_scipys_lfilter():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(3)
    for fs in KERNEL_RATES + (96000,):
        (b1, a1), (b2, a2) = R.k_weighting(fs)
        x = rng.standard_normal(3 * fs // 10 + 17)
        want = signal.lfilter(b2, a2, signal.lfilter(b1, a1, x))
        assert np.max(np.abs(R.k_filter(x, fs) - want)) <= 1e-12 * np.max(np.abs(want)), fs


def test_the_yardsticks_gates_and_gain_rule():
    fs, S = 8000, 800
    rng = np.random.default_rng(4)
    loud, quiet = rng.standard_normal(8 * S) * 0.3, rng.standard_normal(8 * S) * 0.003  # 40 dB apart: the relative gate drops the quiet half
    lufs, nb, gated, _ = R.measure(np.concatenate([loud, quiet]), fs)
    # five blocks are all loud, three hold 3/4, 2/4 and 1/4 of it (above -10 LU of the gated mean), five fail the relative gate
    assert nb == 13 and gated == 8 and abs(lufs - R.measure(loud, fs)[0] - 10.0 * np.log10(6.5 / 8.0)) < 0.1
    assert R.measure(np.zeros(5 * S), fs)[:3] == (-np.inf, 2, 0) and R.measure(np.zeros(0), fs)[:3] == (-np.inf, 0, 0)
    assert R.measure(loud[:100], fs)[1:3] == (1, 1)  # shorter than 400 ms: one block over the whole row
    assert R.gain_rule(-20.0, 0.5, -23.0, -1.0) == (10.0 ** (-3.0 / 20.0), False)
    assert R.gain_rule(-30.0, 0.5, -10.0, -6.0) == (10.0 ** (-6.0 / 20.0) / 0.5, True)
    assert R.gain_rule(-np.inf, 0.0, -23.0, -1.0) == (1.0, False)
    q = R.pcm16_quant(np.array([1.0, -1.0, 0.5, 0.99997], np.float32), 32767.0, 1.0)
    assert q.tolist() == [32767, -32767, 16383, 32766]
    assert R.pcm16_quant(np.array([1.0, -1.0, -0.25], np.float32), 32767.0, 1.5).tolist() == [32767, -32768, -12287]  # trunc(-8191.75) = -8191, floor(-12286.5)


# ------------------------------------------------------------------------------------------ checks shared with the GPU twin
def constructed_rows(fs, item):
    """Criterion 1's rows at one rate: (lengths, row content [n]) — Gaussian-noise segments of 4 S + 137 samples at AMPLITUDES, cut
    to n (repeated where n is longer), the whole pattern once, and rows of 1e-5 noise only."""
    S = R.step(fs)
    rng = np.random.default_rng(fs)
    seg = 4 * S + 137
    full = np.concatenate([rng.standard_normal(seg) * a for a in AMPLITUDES]).astype(np.float32)
    ns = [0, 1, S - 1, S, 4 * S - 1, 4 * S, 4 * S + 1, 5 * S - 1, 5 * S, 5 * S + 1, item - 1, item, item + 1, 2 * item + 137, 70001, len(full)]
    rows = [np.resize(full, n) if n else np.zeros(0, np.float32) for n in ns]
    for n in (S - 1, 4 * S + 1, item + 1):  # below the absolute gate everywhere
        rows.append((rng.standard_normal(n) * 1e-5).astype(np.float32))
    return rows


def w_of(fs):
    """W(fs) from the yardstick's impulse response: the smallest W with sum_{k >= W} |h[k]| <= 2^-40 sum |h|."""
    h = np.abs(R.impulse_response(fs))
    tail = np.cumsum(h[::-1])[::-1]  # tail[W] = sum_{k >= W}
    return int(np.argmax(tail <= np.ldexp(h.sum(), -40)))


def check_kernel_alone(lib):
    """Criterion 1: the two kernels alone at three rates over rows at every edge of the step, the block and the work item, an odd
    stride (row bases on every 4-byte alignment), NaN and then 3e38 behind every row."""
    for fs in KERNEL_RATES:
        S, Wm, K = lib.lab_loudness_plan(fs)
        item = K * S
        assert S == R.step(fs) and Wm == w_of(fs) and item >= 4 * Wm and (K - 1) * S < 4 * Wm
        rows = constructed_rows(fs, item)
        lens = np.array([len(r) for r in rows], np.int32)
        stride = int(lens.max()) + 3
        stride += 1 - stride % 2
        want = [R.measure(r, fs) for r in rows]
        # the condition that keeps a gate flip from hiding behind, or excusing, a difference
        assert min(w[3] for w in want) >= 1e-3, [w[3] for w in want]
        if fs == 22050:
            assert want[15][1] == 33
        assert [i for i, w in enumerate(want) if np.isinf(w[0])] == [0, 16, 17, 18]
        assert any(0 < w[2] < w[1] for w in want)  # both gates drop blocks somewhere
        for fill in (np.float32("nan"), np.float32(3e38)):
            audio = np.full((len(rows), stride), fill, np.float32)
            for b, r in enumerate(rows):
                audio[b, : len(r)] = r
            lufs, blocks, gated = lib.lab_loudness(audio, lens, fs)
            assert lufs.dtype == np.float64 and blocks.dtype == gated.dtype == np.int32
            for b, (l, nb, ng, _) in enumerate(want):
                print(f"{fs} Hz n {lens[b]}: {lufs[b]!r} vs {l!r}, blocks {blocks[b]} / {nb}, gated {gated[b]} / {ng}")
                assert (int(blocks[b]), int(gated[b])) == (nb, ng), (fs, b, lens[b])
                if np.isinf(l):
                    assert lufs[b] == -np.inf, (fs, b)
                else:
                    assert abs(lufs[b] - l) <= LU_TOL, (fs, b, lens[b], lufs[b], l)


def check_kernel_is_address_independent(lib, fs=22050):
    """One row of several work items gives the same lufs BITS at every 4-byte alignment of its base, in a batch of ragged
    neighbours and alone: where an item starts and which lane owns which sample depend on (n, fs) only."""
    S, Wm, K = lib.lab_loudness_plan(fs)
    n = 3 * K * S + 1234
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(n) * np.repeat(rng.uniform(0.01, 0.4, n // 1000 + 1), 1000)[:n]).astype(np.float32)
    alone = lib.lab_loudness(x[None, :], [n], fs)[0][0]
    assert abs(alone - R.measure(x, fs)[0]) <= LU_TOL
    stride = n + 5 - (n + 4) % 4
    assert stride % 4 == 1 and stride > n  # row b starts b floats past a 16-byte boundary (mod 4)
    audio = np.full((6, stride), np.nan, np.float32)
    lens = np.array([n, 17, n, n, 4 * S, n], np.int32)
    for b in range(6):
        audio[b, : lens[b]] = x[: lens[b]]
    lufs = lib.lab_loudness(audio, lens, fs)[0]
    for b in (0, 2, 3, 5):
        assert lufs[b].tobytes() == alone.tobytes(), (b, lufs[b], alone)


def check_calibration(lib):
    """Criterion 2, independent of the yardstick: the standard's own anchor, a 997 Hz full-scale sine at 48 kHz, is -3.01 LUFS."""
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(5 * 48000) / 48000.0).astype(np.float32)
    lufs, blocks, gated = lib.lab_loudness(x[None, :], [len(x)], 48000)
    print("997 Hz full scale:", lufs[0])
    assert abs(lufs[0] + 3.01) <= 0.01 and blocks[0] == gated[0] == 47


def packs_of(eng, pack):
    """fetch_packed of the last run in the four encodings under the engine's current settings."""
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


def reference_of(out, hz):
    """The yardstick's (lufs, blocks, gated, margin) of every row of a padded result."""
    return [R.measure(out["audio"][b, : int(n)], hz) for b, n in enumerate(out["lengths"])]


def check_measurement(ld, ref, hz, allow=1):
    """lufs / blocks / gated of a fetch against the yardstick; rows with a block within 1e-6 LU of a gate are left out (<= allow)."""
    left_out = [b for b, r in enumerate(ref) if r[3] < LU_TOL]
    assert len(left_out) <= allow, left_out
    assert ld.sample_rate == hz and ld.lufs.dtype == np.float64 and len(ld.lufs) == len(ref)
    for b, (l, nb, ng, _) in enumerate(ref):
        assert int(ld.blocks[b]) == nb, b
        if b in left_out:
            continue
        assert int(ld.gated[b]) == ng, b
        assert ld.lufs[b] == l if np.isinf(l) else abs(ld.lufs[b] - l) <= LU_TOL, (b, ld.lufs[b], l)


def check_off_is_off(make_engine, a):
    """Criterion 3: unset, and set and then set back to 0 — run_packed and fetch_packed are those of a handle whose setting was never
    touched, in the four encodings, with and without a header; no `loudness` line is profiled; fetch_loudness with the target off
    still measures, with gain 0."""
    fresh, eng = make_engine(), make_engine()
    assert eng.loudness_target[0] == 0.0
    eng.set_loudness_target(-23.0, -2.0)
    assert eng.loudness_target == (-23.0, -2.0)
    eng.set_loudness_target(0.0)
    eng.profile_enable(True)
    eng.profile_reset()
    for wav in (True, False):
        pack = dict(order=[2, 0, 1], lead_samples=[5, 0, 3], tail_samples=2, wav=wav)
        for enc in ENCODINGS:
            for e in (fresh, eng):
                e.set_output_encoding(enc)
            want = fresh.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **a["kw"])
            got = eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **a["kw"])
            same_stream(got, want)
            same_stream(eng.fetch_packed(**pack), fresh.fetch_packed(**pack))
            assert got.lufs is None and got.gain is None and got.limited is None
    eng.set_loudness_target(None)
    same_stream(eng.fetch_packed(**pack), fresh.fetch_packed(**pack))
    assert "loudness" not in eng.profile_report()
    eng.profile_enable(False)
    out = run_at(eng, None, a)
    ld = eng.fetch_loudness()
    assert isinstance(ld, Loudness) and ld.target_lufs == 0.0
    check_measurement(ld, reference_of(out, eng.config.sample_rate), eng.config.sample_rate)
    assert not ld.gain.any() and not ld.limited.any() and ld.gain.dtype == np.float64
    fresh.close()
    eng.close()


def check_normalised_pack(got, out, ld, order, lead, tail, enc, hz, vols, tables, wav):
    """One normalised stream against the float audio of the same run and the fetched gains."""
    n = len(order)
    lens = out["lengths"].astype(np.int64)[order]
    assert np.array_equal(got.lengths, lens)
    offsets = np.cumsum(np.asarray(lead, np.int64) + np.concatenate(([0], lens[:-1])))
    assert np.array_equal(got.offsets, offsets)
    total = int(offsets[-1] + lens[-1] + tail)
    assert got.total_samples == total == got.data.shape[0]
    assert got.peaks.tobytes() == out["peaks"][order].tobytes()  # the row's float peak as before
    assert got.lufs.tobytes() == ld.lufs[order].tobytes() and got.gain.tobytes() == ld.gain[order].tobytes()
    assert np.array_equal(got.limited, ld.limited[order])
    chunks, covered = [], np.zeros(total, bool)
    for i, b in enumerate(order):
        x = out["audio"][b, : int(lens[i])]
        if enc == "f32le":
            want = x * np.float32(ld.gain[b])
            assert want.dtype == np.float32
        else:
            q = R.pcm16_quant(x, np.float32(32767.0 * ld.gain[b]), float(vols[b]))
            want = q if enc == "s16le" else G.encode(tables[enc], q)
        assert got.rows[i].tobytes() == want.tobytes(), (enc, i, b)
        covered[int(offsets[i]): int(offsets[i] + lens[i])] = True
        chunks += [np.full(int(lead[i]), SILENCE[enc], got.data.dtype), want]
    chunks.append(np.full(int(tail), SILENCE[enc], got.data.dtype))
    rest = got.data[~covered]
    assert rest.size == int(np.sum(lead)) + tail and (rest.view(np.uint32 if enc == "f32le" else rest.dtype) == SILENCE[enc]).all()
    if wav:
        assert bytes(got.wav) == PP.wav_bytes(chunks, hz, enc)  # header and sizes are those of the host's own writer
    else:
        assert got.wav is None


def straddling_setting(out, ref):
    """A (target, ceiling) at which the ceiling binds on about half the rows of this run, from the yardstick's side alone: a row is
    limited iff its peak in dBFS lies more than ceiling - target above its loudness, so ceiling - target = the median of that
    difference over the rows, rounded to 0.5 dB, under a target of -23."""
    crest = [20.0 * np.log10(float(p)) - r[0] for p, r in zip(out["peaks"], ref) if np.isfinite(r[0]) and p > 0]
    return -23.0, min(0.0, -23.0 + round(2.0 * float(np.median(crest))) / 2.0)


def check_normalised_streams(eng, a, rate, order, both_at_minus_10=True):
    """Criterion 4 at one rate: lufs against the yardstick on the run's float audio, the gain rule on the fetched lufs and peaks,
    every normalised stream (the targets x four encodings, a permuted order with lead / tail silences, header on and off) sample for
    sample; a normalised run_packed is the normalised fetch_packed.

    The issue expected the (-10, -6) target to bind the ceiling on some rows and not on others.  A row is limited there iff its peak
    lies more than 4 dB above its loudness, and measured on the MI355X every one of the 36 ragged rows of the synthetic apope_low
    voices does (peak - lufs 6.8 .. 9.2 dB native, 11.5 .. 13.5 dB at 8 kHz, 9.2 .. 10.8 dB at 48 kHz for the suite's voice; 5.4 dB at
    the least over four voice / case seeds; with the decoder's last conv scaled up until tanh saturates, still 5.5 dB and more at both
    resampled rates): 36 of 36 rows are limited at (-10, -6) and 0 of 36 at (-23, -1).  `both_at_minus_10` keeps the issue's assertion
    where the inputs allow it (the CPU model's case, chosen for it); everywhere a third setting derived from the run's own reference
    measurement (straddling_setting) is checked in full and must have rows on both sides, so that both branches of min(g, cap) are
    exercised in one stream at every rate."""
    out = run_at(eng, rate, a)
    hz = rate or eng.config.sample_rate
    B = len(out["lengths"])
    n = len(order)
    rng = np.random.default_rng(n)
    lead = [int(x) for x in rng.integers(0, 50, n)]
    lead[1] = 0
    vols = np.broadcast_to(np.asarray(a["kw"].get("pcm_volume", 1.0), np.float64).reshape(-1), (B,))
    tables = G.tables()
    ref = reference_of(out, hz)
    third = straddling_setting(out, ref)
    for target, ceiling in TARGETS + (third,):
        eng.set_loudness_target(target, ceiling)
        ld = eng.fetch_loudness()
        assert (ld.target_lufs, ld.ceiling_dbfs) == (target, ceiling)
        check_measurement(ld, ref, hz)
        for b in range(B):
            g, lim = R.gain_rule(ld.lufs[b], out["peaks"][b], target, ceiling)
            assert abs(ld.gain[b] - g) <= 1e-12 * g and bool(ld.limited[b]) == lim, (b, ld.gain[b], g)
        print(f"{hz} Hz target {target} ceiling {ceiling}: lufs {np.min(ld.lufs):.2f} .. {np.max(ld.lufs):.2f}, "
              f"gain {np.min(ld.gain):.3f} .. {np.max(ld.gain):.3f}, limited {int(ld.limited.sum())} of {B}")
        if (target, ceiling) == third or (both_at_minus_10 and (target, ceiling) == (-10.0, -6.0)):
            assert ld.limited.any() and not ld.limited.all(), (target, ceiling)
        for wav in (True, False):
            pack = dict(order=order, lead_samples=lead, tail_samples=7, wav=wav)
            got = packs_of(eng, pack)
            for enc in ENCODINGS:
                check_normalised_pack(got[enc], out, ld, np.asarray(order), lead, 7, enc, hz, vols, tables, wav)
    # the one-call form: synthesis, measurement and pack in one mi355vits_run_packed
    pack = dict(order=order, lead_samples=lead, tail_samples=7, wav=True)
    want = packs_of(eng, pack)
    for enc in ("s16le", "f32le"):
        eng.set_output_encoding(enc)
        got = eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **a["kw"])
        same_stream(got, want[enc])
        assert got.lufs.tobytes() == want[enc].lufs.tobytes() and got.gain.tobytes() == want[enc].gain.tobytes()
    eng.set_output_encoding("s16le")
    after = eng.fetch(want_float=True)  # the run a normalised run_packed leaves behind is the run itself
    for k in ("audio", "lengths", "peaks"):
        assert after[k].tobytes() == out[k].tobytes(), k
    eng.set_loudness_target(None)


def normalised_batch(eng, a, rate, target=-23.0, ceiling=-1.0):
    """The normalised int16 pack of a batch in row order."""
    run_at(eng, rate, a)
    eng.set_loudness_target(target, ceiling)
    got = eng.fetch_packed()
    eng.set_loudness_target(None)
    return got


def check_rows_alone(make_engine, a, rate, rows, batched, target=-23.0, ceiling=-1.0):
    """Criterion 5: a row run alone gives bitwise the lufs double and the entry bytes it gives in the batch."""
    eng = make_engine()
    eng.set_output_rate(rate)
    eng.set_loudness_target(target, ceiling)
    for b in rows:
        n = int(a["lens"][b])
        kw = dict(a["kw"])
        kw["utterance_keys"] = [kw["utterance_keys"][b]]
        kw["pcm_volume"] = float(np.asarray(kw["pcm_volume"]).reshape(-1)[b])
        if "forced_durations" in kw:
            kw["forced_durations"] = kw["forced_durations"][b:b + 1, : max(n, 1)]
        solo = eng.run_packed(a["ids"][b:b + 1, : max(n, 1)], [n], a["scales"][b], None, **kw)
        assert solo.lufs[0].tobytes() == batched.lufs[b].tobytes(), (b, solo.lufs[0], batched.lufs[b])
        assert solo.gain[0].tobytes() == batched.gain[b].tobytes() and bool(solo.limited[0]) == bool(batched.limited[b])
        assert solo.rows[0].tobytes() == batched.rows[b].tobytes(), b
        assert eng.fetch_loudness().lufs[0].tobytes() == batched.lufs[b].tobytes()
    eng.close()


def check_nothing_else_moves(eng, a, rate):
    """Criterion 6: with a target set, run / fetch with both flags, fetch_alignment with levels, fetch_edges and the device_result
    lengths are bitwise the same handle's with it off; unchanged after a fetch_loudness and after a normalised fetch_packed; with
    trimming and a target both on each entry is [first, end) of the untrimmed normalised entry, and lufs does not move."""
    def served():
        f = eng.fetch(want_float=True, want_pcm16=True)
        al = eng.fetch_alignment(levels=True)
        e = eng.fetch_edges()
        d = eng.device_result()
        return ([f[k].tobytes() for k in ("audio", "pcm", "lengths", "peaks")] + [int(f["l_max"])] +
                [getattr(al, k).tobytes() for k in ("frames", "start", "samples", "peak", "rms")] +
                [e.first.tobytes(), e.end.tobytes(), d["row_stride"], d["batch"]])

    hz = rate or eng.config.sample_rate
    eng.set_loudness_target(None)
    eng.set_edge_trim(0.9, 3)
    off = run_at(eng, rate, a)
    want = served()
    eng.set_edge_trim(0.0)
    plain = bytes(eng.fetch_packed(wav=True).wav)
    eng.set_edge_trim(0.9, 3)
    eng.set_loudness_target(-23.0, -1.0)
    on = run_at(eng, rate, a)
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert on[k].tobytes() == off[k].tobytes(), k
    assert served() == want
    eng.profile_enable(True)
    eng.profile_reset()
    ld = eng.fetch_loudness()
    rep = eng.profile_report()
    S = R.step(hz)
    steps = sum((int(n) + S - 1) // S for n in off["lengths"])
    assert rep["loudness"]["calls"] == 1
    assert rep["loudness"]["bytes"] == 4.0 * float(np.sum(off["lengths"])) + 8.0 * steps + 16.0 * len(off["lengths"])
    assert served() == want
    trimmed = eng.fetch_packed(wav=True)
    eng.set_loudness_target(-16.0, -3.0)  # another target, the measurement is held on the host
    eng.fetch_packed()
    assert eng.fetch_loudness().lufs.tobytes() == ld.lufs.tobytes()
    assert eng.profile_report()["loudness"]["calls"] == 1
    eng.profile_enable(False)
    assert served() == want
    eng.set_loudness_target(-23.0, -1.0)
    eng.set_edge_trim(0.0)
    whole = eng.fetch_packed(wav=True)
    assert whole.lufs.tobytes() == trimmed.lufs.tobytes() == ld.lufs.tobytes()  # lufs does not depend on the trim setting
    assert bytes(whole.wav) != plain and len(bytes(whole.wav)) == len(plain)
    assert int(np.sum(trimmed.lengths)) < int(np.sum(whole.lengths))
    for i in range(len(whole.lengths)):
        assert trimmed.rows[i].tobytes() == whole.rows[i][int(trimmed.first[i]): int(trimmed.end[i])].tobytes(), i
    for _ in range(2):  # one synthesis, packed normalised and un-normalised in turn
        eng.set_loudness_target(None)
        assert bytes(eng.fetch_packed(wav=True).wav) == plain
        eng.set_loudness_target(-23.0, -1.0)
        assert bytes(eng.fetch_packed(wav=True).wav) == bytes(whole.wav)
    assert eng.fetch(want_float=True)["audio"].tobytes() == off["audio"].tobytes()
    eng.set_loudness_target(None)


def check_errors(make_engine, a):
    """Criterion 7 at the C ABI."""
    eng = make_engine()
    lib = eng.native.lib
    with pytest.raises(NativeError, match="fetch_loudness: no completed run on this handle") as err:
        eng.fetch_loudness()
    assert err.value.code == -1
    assert lib.mi355vits_fetch_loudness(eng._h, None) == -1
    eng.set_loudness_target(-18.0, -2.5)
    for bad, ceiling, name in ((0.5, -1.0, "0.5"), (-71.0, -1.0, "-71"), (float("nan"), -1.0, "nan"), (-23.0, 1.0, "1.0"),
                               (-23.0, float("nan"), "nan"), (-23.0, float("-inf"), "inf")):
        with pytest.raises(NativeError, match="set_loudness_target") as err:
            eng.set_loudness_target(bad, ceiling)
        assert err.value.code == -1 and name in str(err.value).lower()
        assert eng.loudness_target == (-18.0, -2.5)
    eng.set_loudness_target(-70.0, 0.0)  # the ends of both ranges are legal
    eng.set_loudness_target(-18.0, -2.5)
    twin = eng.clone()  # a further lane inherits the setting
    assert twin.loudness_target == (-18.0, -2.5)
    twin.close()
    run_at(eng, 0, a)
    assert lib.mi355vits_fetch_loudness(eng._h, None) == -1
    r = LoudnessResult()
    assert lib.mi355vits_fetch_loudness(eng._h, ctypes.byref(r)) == 0 and r.batch == a["ids"].shape[0] and r.target_lufs == -18.0
    assert r.ceiling_dbfs == -2.5 and r.sample_rate == eng.config.sample_rate
    lib.mi355vits_free_loudness(ctypes.byref(r))
    assert not r.lufs and not r.owner_
    lib.mi355vits_free_loudness(ctypes.byref(r))  # freeing twice is harmless
    # a run that fails after its launch sequence began leaves no result: a normalised run_packed as any other run
    with pytest.raises(NativeError):
        eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), forced_durations=np.full(a["ids"].shape, 1 << 23, np.int32))
    with pytest.raises(NativeError, match="fetch_loudness: no completed run on this handle"):
        eng.fetch_loudness()
    eng.close()


def check_session(sess, a, rate=8000):
    """Criterion 7's routing: loudness= / ceiling_db= reach the lane and go back to off for a call that does not ask."""
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    B = a["ids"].shape[0]
    keys = list(range(21, 21 + B))
    order = [2, 0, 1][:B] + list(range(3, B))
    plain = sess.run_packed(feed, order=order, lead_ms=[20.0] * B, sample_rate=rate, utterance_keys=keys)
    assert plain.lufs is None and plain.gain is None and plain.limited is None
    got = sess.run_packed(feed, order=order, lead_ms=[20.0] * B, sample_rate=rate, utterance_keys=keys, loudness=-23, ceiling_db=-2)
    assert sess._engines[0].loudness_target == (-23.0, -2.0)
    assert got.lufs is not None and np.array_equal(got.lengths, plain.lengths) and got.data.tobytes() != plain.data.tobytes()
    for i in range(B):
        g, lim = R.gain_rule(got.lufs[i], got.peaks[i], -23.0, -2.0)
        assert abs(got.gain[i] - g) <= 1e-12 * g and bool(got.limited[i]) == lim
    again = sess.run_packed(feed, order=order, lead_ms=[20.0] * B, sample_rate=rate, utterance_keys=keys)  # the lane is back to off
    assert again.lufs is None and again.data.tobytes() == plain.data.tobytes()
    assert sess._engines[0].loudness_target[0] == 0.0
    wav = PP.request_wav(sess, [a["ids"][b, : int(a["lens"][b])] for b in range(B)], break_ms=20.0, sample_rate=rate, utterance_keys=keys,
                         loudness=-23, ceiling_db=-2)
    want = sess.run_packed(feed, lead_ms=[0.0] + [20.0] * (B - 1), wav=True, sample_rate=rate, utterance_keys=keys, loudness=-23, ceiling_db=-2)
    assert wav == bytes(want.wav)
    for bad in (0.5, 0.0, -71.0, float("nan")):
        with pytest.raises(ValueError):
            sess.run_packed(feed, loudness=bad)
    with pytest.raises(ValueError):
        sess.run_packed(feed, loudness=-23.0, ceiling_db=1.0)


# ------------------------------------------------------------------------------------------ the engine on the CPU model
@pytest.fixture
def cu_count(emu_lib):
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(DEFAULT_CUS)


def _engine(seed=91):
    cfg = VitsConfig.tiny()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=seed, frames_per_id=6.0))


def _long_case(cfg, seed, B=5):
    """`_case` with forced durations of 25 .. 70 frames a phoneme: rows of a few thousand samples at the tiny voice's hop of 8, so
    that a row has several 400 ms blocks at 8 kHz and the gates have something to drop."""
    a = _case(cfg, seed, B=B)
    a["kw"]["forced_durations"] = np.random.default_rng(seed + FORCED_SEED).integers(25, 71, a["ids"].shape).astype(np.int32)
    return a


def test_the_kernels_alone(emu_lib):
    """Criterion 1.  This fails without the feature."""
    check_kernel_alone(emu_lib)
    check_kernel_is_address_independent(emu_lib)
    with pytest.raises(NativeError):  # a length past the stride: refused before anything is launched
        emu_lib.lab_loudness(np.zeros((1, 8), np.float32), [9], 22050)
    with pytest.raises(NativeError):  # below the rate the measure is offered from
        emu_lib.lab_loudness(np.zeros((1, 8), np.float32), [8], 3999)


def test_calibration(emu_lib):
    check_calibration(emu_lib)


def test_off_is_off(emu_lib):
    cfg, blob = _engine()
    check_off_is_off(lambda: Engine(blob, library=emu_lib), _case(cfg, 91))


@pytest.mark.parametrize("rate", RATES)
def test_normalised_streams(emu_lib, rate):
    """Criterion 4 on the small case.  This fails without the feature.  A row is limited iff its peak in dBFS lies more than
    ceiling - target above its loudness — 4 dB at (-10, -6); this voice and case have rows on both sides of that at the three rates
    (a property of the inputs, asserted on the gain rule's side in check_normalised_streams)."""
    cfg, blob = _engine(118)
    eng = Engine(blob, library=emu_lib)
    check_normalised_streams(eng, _case(cfg, 118), rate, [3, 0, 4, 1, 2])
    eng.close()


def test_normalised_streams_of_rows_with_several_blocks(emu_lib):
    cfg, blob = _engine(92)
    eng = Engine(blob, library=emu_lib)
    a = _case(cfg, 92)
    a["kw"]["forced_durations"] = np.random.default_rng(92).integers(150, 251, a["ids"].shape).astype(np.int32)  # ~ 1 s rows
    check_normalised_streams(eng, a, 8000, [3, 0, 4, 1, 2], both_at_minus_10=False)
    assert max(r[1] for r in reference_of(run_at(eng, 8000, a), 8000)) >= 3  # (numpy side) rows of several blocks
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_batched_is_alone_at_any_cu_count_and_on_a_poisoned_workspace(emu_lib, cu_count, rate):
    cfg, blob = _engine(93)
    a = _long_case(cfg, 93)
    eng = Engine(blob, library=emu_lib)
    want = normalised_batch(eng, a, rate)
    check_rows_alone(lambda: Engine(blob, library=emu_lib), a, rate, range(5), want)
    big = dict(a, ids=np.tile(a["ids"], (2, 2)), lens=np.tile(a["lens"] * 2, 2), scales=np.tile(a["scales"], (2, 1)), sid=None,
               kw=dict(seed=1, forced_durations=np.full((10, 24), 70, np.int32)))
    run_at(eng, rate, big)
    eng.set_loudness_target(-23.0, -1.0)
    eng.fetch_packed()  # sizes the measurement's and the pack's own arenas past what the batch needs
    eng.fill_workspace(NAN)
    got = normalised_batch(eng, a, rate)
    same_stream(got, want)
    assert got.lufs.tobytes() == want.lufs.tobytes()
    for cus in (13, 256):
        cu_count(cus)
        got = normalised_batch(eng, a, rate)
        same_stream(got, want)
        assert got.lufs.tobytes() == want.lufs.tobytes(), cus
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_nothing_else_moves(emu_lib, rate):
    cfg, blob = _engine(94)
    eng = Engine(blob, library=emu_lib)
    check_nothing_else_moves(eng, _long_case(cfg, 94), rate)
    eng.close()


def test_errors(emu_lib):
    cfg, blob = _engine(95)
    check_errors(lambda: Engine(blob, library=emu_lib), _case(cfg, 95))


def test_session_routing(emu_lib):
    cfg, blob = _engine(96)
    opts = SessionOptions()
    opts.seed = 5
    sess = InferenceSession(blob, opts, _library=emu_lib)
    check_session(sess, _case(cfg, 96, B=3, Tx=9), rate=8000)
    sess.close()
    for bad in (dict(loudness_lufs=3.0), dict(loudness_lufs=-23.0, loudness_ceiling_db=2.0)):
        with pytest.raises(ValueError):
            InferenceSession(blob, opts, _library=emu_lib, **bad)
    sess = InferenceSession(blob, opts, _library=emu_lib, loudness_lufs=-16.0, loudness_ceiling_db=-3.0)  # the session's own default
    a = _case(cfg, 96, B=3, Tx=9)
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    got = sess.run_packed(feed, utterance_keys=[1, 2, 3])
    assert got.lufs is not None and sess._engines[0].loudness_target == (-16.0, -3.0)
    sess.close()


def test_plain_c99_client(emu_lib, tmp_path):
    """A C99 client measures a tiny voice, packs it at a target and checks every int16 sample against the header's rule."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_loudness_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_loudness_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir, "-lm"], check=True)
    cfg = VitsConfig.tiny()
    W.save(str(tmp_path / "voice.m355"), cfg, W.synthetic_weights(cfg, seed=17))
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "expected failure rc=-1 msg=fetch_loudness: no completed run on this handle" in p.stdout
    assert "loudness ok" in p.stdout
