"""The true-peak ceiling of the loudness chain (mi355vits_set_loudness_ceiling_mode / mi355vits_fetch_true_peak, k_true_peak,
k_true_peak_env, k_limit<true>) on the CPU model of the kernels; test_gpu_true_peak.py runs the same checks on the MI355X.

The yardstick is tests/true_peak_ref.py — numpy from the rule of include/mi355vits.h (resample_ref.resample for the oversampling,
limiter_ref behind the envelope), never the code under test.  The library's literal tap table is compared with numpy's to a relative
2^-50 (i0 / sinc may differ in the last bits between numpy versions) and the yardstick then uses the library's table; everything
behind it — tp, e, rq, the curve, the samples, the statistics — is compared bit for bit.  Comparisons that involve g follow
test_limiter.py: under the gain the library reports, with the gain rule checked to 1e-12.

Not tested: the number of stream synchronisations of a call (no hook counts them); kernel assembly."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from mimic3_amd import _native
from mimic3_amd import postprocess as PP
from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError, TruePeak, TruePeakResult
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests import g711_ref as G
from tests import limiter_ref as M
from tests import loudness_ref as R
from tests import true_peak_ref as TP
from tests.test_limiter import check_rows_alone, limited_batch, same_batch, unit
from tests.test_limiter import want_entry as sample_entry
from tests.test_loudness import ENCODINGS, NAN, _engine, _long_case, packs_of, reference_of, same_stream
from tests.test_resample import DEFAULT_CUS, _case, run_at

TILE = 4096            # samples of a k_true_peak work item (= k_limit's)
WINDOWS = (1, 100, 4096)
ENGINE_WINDOW = 24     # samples: a few milliseconds at the tiny voice's rates
C_LAB = 0.5
G_LAB = 1.2


def library_taps(lib):
    """The library's tap table, checked against numpy's to a relative 2^-50, and its tile."""
    h, tile = lib.lab_true_peak_plan()
    ref = TP.taps()
    assert h.shape == ref.shape == (81,) and tile == TILE
    assert np.max(np.abs(h - ref) / np.abs(ref)) <= 2.0 ** -50
    assert h[40] > 1.0 and np.array_equal(h, h[::-1])  # the centre tap is 1.0006; a symmetric table
    return h


# ------------------------------------------------------------------------------------------ the yardstick itself
def test_the_yardstick_itself():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(777).astype(np.float32)
    try:
        from scipy import signal
    except ImportError:
        signal = None
    if signal is not None:
        for n in (777, 37, 1):
            want = signal.resample_poly(x[:n].astype(np.float64), 4, 1)
            got = TP.oversample(x[:n])
            assert got.shape == want.shape == (4 * n,) and np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    assert TP.oversample(x).tobytes() == TP.oversample(x, TP.taps()).tobytes()  # the two forms of the same passes
    # the fs/4 sine at 45 degrees: every crest falls half way between two samples
    t = np.arange(400, dtype=np.float64)
    s = (0.5 * np.sin(0.5 * np.pi * t + 0.25 * np.pi)).astype(np.float32)
    tp, pk = TP.true_peak(s), float(np.max(np.abs(s)))
    print(f"fs/4 sine: sample peak {pk:.4f}, tp {tp:.4f}, {20 * np.log10(tp / pk):+.2f} dB")
    assert 0.50 <= tp <= 0.52 and 20.0 * np.log10(tp / pk) >= 3.0
    # an isolated impulse: the samples themselves carry the peak
    imp = np.zeros(64, np.float32)
    imp[30] = -0.7
    u = np.abs(TP.oversample(imp))
    assert TP.true_peak(imp) == float(np.float32(0.7)) and 0.75 < np.max(u[np.arange(256) % 4 != 0]) / 0.7 < 0.95
    # max e = tp, e >= |x|, e[t] depends on x[t - 11 .. t + 10] only
    for row in (x, s, imp, TP.burst(300, 150.5), np.zeros(9, np.float32), x[:1], x[:0]):
        e = TP.envelope(row)
        assert e.shape == row.shape and (e >= np.abs(row.astype(np.float64))).all()
        assert (float(e.max()) if len(e) else 0.0) == TP.true_peak(row)
        assert TP.true_peak(row) >= (float(np.max(np.abs(row))) if len(row) else 0.0)
    y = x.copy()
    y[400] += 0.5
    moved = np.nonzero(TP.envelope(y) != TP.envelope(x))[0]
    assert moved.min() >= 400 - 10 and moved.max() <= 400 + 11
    # a NaN is never taken: the row's other samples still speak
    z = x.copy()
    z[100] = np.nan
    assert np.isfinite(TP.envelope(z)).all() and np.isfinite(TP.true_peak(z)) and TP.true_peak(z) > 0
    # the burst of the limiter check: under the ceiling in its samples, over it between them
    b = TP.burst(600, 300.5)
    assert G_LAB * float(np.max(np.abs(b))) < C_LAB < G_LAB * TP.true_peak(b)


# ------------------------------------------------------------------------------------------ checks shared with the GPU twin
def constructed_rows():
    """(name, samples) of the kernel-alone check: lengths around a phase and around the tile, bursts whose maximum lies between the
    last sample of one tile and the first of the next and at the row's two ends, silence, an impulse, a NaN, noise."""
    rng = np.random.default_rng(7)
    noise = lambda n, a=0.1: (rng.standard_normal(n) * a).astype(np.float32)  # noqa: E731
    rows = [(f"n = {n}", noise(n)) for n in (1, 2, 20, 21, TILE - 1, TILE, TILE + 1, 2 * TILE + 37)]
    rows.append(("burst between two tiles", TP.burst(TILE + 300, TILE - 0.5)))
    x = noise(TILE + 40, 0.01)
    x[TILE - 11: TILE + 10] = noise(21, 0.3)
    rows.append(("the 11 samples before and the 10 behind a tile boundary", x))
    rows.append(("burst at the row start", TP.burst(500, 0.5)))
    rows.append(("burst at the row end", TP.burst(500, 498.5)))
    rows.append(("all zero", np.zeros(300, np.float32)))
    x = np.zeros(200, np.float32)
    x[77] = 0.6
    rows.append(("impulse", x))
    x = noise(3000)
    x[100], x[105] = np.nan, 0.9
    rows.append(("a NaN sample", x))
    rows.append(("white noise", noise(TILE + 1, 0.25)))
    rows.append(("empty", np.zeros(0, np.float32)))
    return rows


def check_kernel_alone(lib):
    """k_true_peak / k_true_peak_env alone through the hook: tp and every e[t] of every constructed row bitwise the yardstick's, at
    the four address misalignments of the rows' base, with NaN and then 3e38 behind every row."""
    h = library_taps(lib)
    rows = constructed_rows()
    lens = np.array([len(r[1]) for r in rows], np.int32)
    stride = int(lens.max()) + 3
    stride += (1 - stride) % 4  # 1 mod 4: consecutive rows sit at every 4-byte alignment as well
    want = [(TP.true_peak(r[1], h), TP.envelope(r[1], h)) for r in rows]
    by = {r[0]: w for r, w in zip(rows, want)}
    assert by["impulse"][0] == float(np.float32(0.6)) and by["all zero"][0] == 0.0 and by["empty"][0] == 0.0
    assert by["burst between two tiles"][0] > 1.25 * float(np.max(np.abs(dict(rows)["burst between two tiles"])))
    assert int(np.argmax(by["burst between two tiles"][1])) in (TILE - 1, TILE)
    assert np.isfinite(by["a NaN sample"][1]).all()
    for offset in range(4):
        for fill in (np.float32("nan"), np.float32(3e38)):
            audio = np.full((len(rows), stride), fill, np.float32)
            for b, r in enumerate(rows):
                audio[b, : lens[b]] = r[1]
            tp, e = lib.lab_true_peak(audio, lens, offset)
            assert tp.dtype == np.float64 and e.dtype == np.float64 and e.shape == audio.shape
            for b, r in enumerate(rows):
                n = int(lens[b])
                assert np.float64(tp[b]).tobytes() == np.float64(want[b][0]).tobytes(), (offset, r[0], tp[b], want[b][0])
                assert e[b, :n].tobytes() == want[b][1].tobytes(), (offset, r[0])
                assert not e[b, n:].any(), (offset, r[0])
            only, none = lib.lab_true_peak(audio, lens, offset, envelope=False)
            assert none is None and only.tobytes() == tp.tobytes()
    with pytest.raises(NativeError):  # a length past the stride: refused before anything is launched
        lib.lab_true_peak(np.zeros((1, 8), np.float32), [9])
    with pytest.raises(NativeError):
        lib.lab_true_peak(np.zeros((1, 8), np.float32), [8], 4)


def limiter_rows():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(TILE + 301) * 0.1).astype(np.float32)
    x[TILE - 2] = 0.9
    return [("burst", TP.burst(3000, 1500.5), G_LAB), ("burst between two tiles", TP.burst(TILE + 300, TILE - 0.5), G_LAB),
            ("busy", x, 2.5), ("quiet", (rng.standard_normal(700) * 0.01).astype(np.float32), 2.5), ("n = 1", np.array([0.9], np.float32), 2.5)]


def check_limiter_with_envelope(lib, windows=WINDOWS):
    """k_limit<true> through the hook with the envelope k_true_peak_env makes: curve and statistics bitwise the yardstick's; the burst
    row is over in true-peak mode only, and the true peak of its F32LE output is at most that of sample mode (which leaves it alone)."""
    h = library_taps(lib)
    rows = limiter_rows()
    lens = np.array([len(r[1]) for r in rows], np.int32)
    g = np.array([r[2] for r in rows], np.float64)
    stride = int(lens.max()) + 3
    stride += (1 - stride) % 4
    audio = np.full((len(rows), stride), np.nan, np.float32)
    for b, r in enumerate(rows):
        audio[b, : lens[b]] = r[1]
    tp, env = lib.lab_true_peak(audio, lens)
    for b, r in enumerate(rows):
        assert env[b, : lens[b]].tobytes() == TP.envelope(r[1], h).tobytes(), r[0]
    for L in windows:
        for U in (32767.0, 1.0) if L == 100 else (1.0,):
            scale, sq_min, reduced = lib.lab_limit(audio, lens, g, C_LAB, U, L, envelope=env)
            plain = lib.lab_limit(audio, lens, g, C_LAB, U, L)
            for b, r in enumerate(rows):
                n = int(lens[b])
                want, sq = TP.curve(r[1], r[2], C_LAB, U, L, h)
                st = M.stats(sq, L)
                assert scale[b, :n].tobytes() == want.tobytes(), (L, U, r[0])
                assert not scale[b, n:].any()
                assert (int(sq_min[b]), int(reduced[b])) == st[:2], (L, U, r[0], sq_min[b], reduced[b], st)
                ps, psq = M.curve(r[1], r[2], C_LAB, U, L)
                assert plain[0][b, :n].tobytes() == ps.tobytes() and int(plain[2][b]) == M.stats(psq, L)[1]  # the sample form is what it was
                if r[0].startswith("burst"):
                    over_sample = r[2] * float(np.max(np.abs(r[1]))) > C_LAB
                    over_tp = r[2] * float(tp[b]) > C_LAB
                    assert (over_sample, over_tp) == (False, True) and st[1] > 0 and M.stats(psq, L)[1] == 0, (L, r[0])
                    if U == 1.0:
                        y_tp, y_sample = r[1] * scale[b, :n], r[1] * np.float32(r[2])
                        assert y_tp.dtype == np.float32 and np.max(np.abs(y_tp.astype(np.float64))) <= C_LAB * (1.0 + 2.0 ** -22)
                        a, s = TP.true_peak(y_tp, h), TP.true_peak(y_sample, h)
                        print(f"L {L} {r[0]}: true peak over c {20 * np.log10(a / C_LAB):+.4f} dB limited, {20 * np.log10(s / C_LAB):+.4f} dB in sample mode")
                        assert a <= s
                if r[0] == "quiet":
                    assert st[1] == 0
    with pytest.raises(ValueError):
        lib.lab_limit(audio, lens, g, C_LAB, 1.0, 4, envelope=env[:, :-1])


def true_peak_setting(out, hz, h, target=-23.0):
    """A (target, ceiling) from the run's own audio with the yardstick alone, at which at least one row is over in true-peak mode
    only, one in both modes and one in neither — None when this batch allows none.  A row is over in sample mode iff
    20 log10(peak) - lufs > ceiling - target, in true-peak mode iff 20 log10(tp) - lufs > ceiling - target: the difference D is put in
    the middle of the widest gap between a row's two crests that leaves rows on both sides."""
    B = len(out["lengths"])
    rows = [out["audio"][b, : int(out["lengths"][b])] for b in range(B)]
    lufs = [R.measure(x, hz)[0] for x in rows]
    ok = [b for b in range(B) if np.isfinite(lufs[b]) and out["peaks"][b] > 0]
    cs = {b: 20.0 * np.log10(float(out["peaks"][b])) - lufs[b] for b in ok}
    ct = {b: 20.0 * np.log10(TP.true_peak(rows[b], h)) - lufs[b] for b in ok}
    best = None
    for k in ok:
        D = 0.5 * (cs[k] + ct[k])
        ceiling = float(np.float32(target + D))
        if ceiling > 0.0:
            continue
        D = ceiling - target
        margin = min(min(abs(cs[b] - D), abs(ct[b] - D)) for b in ok)
        both = any(cs[b] > D for b in ok)
        neither = any(ct[b] < D for b in ok)
        only = any(cs[b] < D < ct[b] for b in ok)
        if both and neither and only and margin > 1e-6 and (best is None or margin > best[0]):
            best = (margin, target, ceiling)
    print("crest dB sample / true peak:", " ".join(f"{cs[b]:.2f}/{ct[b]:.2f}" for b in ok), "->", best)
    return None if best is None else best[1:]


def want_entry(x, gain, over, c, enc, L, vol, tables, h):
    """The bytes of one entry in true-peak mode: the envelope's curve for a row that is over, the one scale otherwise."""
    if not over:
        return sample_entry(x, gain, False, c, enc, L, vol, tables)
    scale = TP.curve(x, gain, c, unit(enc), L, h)[0]
    if enc == "f32le":
        y = x * scale
        assert y.dtype == np.float32
        return y
    q = R.pcm16_quant(x, scale, float(vol))
    return q if enc == "s16le" else G.encode(tables[enc], q)


def check_packs(eng, a, rate, order, h, L=ENGINE_WINDOW):
    """The engine at one rate.  tp of fetch_true_peak bitwise; a (target, ceiling) with rows over in true-peak mode only, in both and
    in neither (asserted); gain / limited of both modes; every entry of the four encodings byte for byte with the limiter off and
    on; fetch_loudness / fetch_limiter / fetch_true_peak consistent with the pack; the profile lines; the one-call form."""
    out = run_at(eng, rate, a)
    hz = rate or eng.config.sample_rate
    B = len(out["lengths"])
    rows = [out["audio"][b, : int(out["lengths"][b])] for b in range(B)]
    eng.profile_enable(True)
    eng.profile_reset()
    tpk = eng.fetch_true_peak()
    again = eng.fetch_true_peak()
    rep = eng.profile_report()
    eng.profile_enable(False)
    assert rep["truepeak"]["calls"] == 1 and rep["truepeak"]["bytes"] == 4.0 * float(np.sum(out["lengths"])) + 8.0 * B  # kept on the host
    assert isinstance(tpk, TruePeak) and tpk.sample_rate == hz and tpk.peak.tobytes() == out["peaks"].tobytes()
    assert again.true_peak.tobytes() == tpk.true_peak.tobytes()
    want_tp = np.array([TP.true_peak(x, h) for x in rows])
    assert tpk.true_peak.tobytes() == want_tp.tobytes(), (tpk.true_peak, want_tp)
    assert (tpk.true_peak >= tpk.peak.astype(np.float64)).all() and np.array_equal(tpk.dbtp, 20.0 * np.log10(want_tp))
    setting = true_peak_setting(out, hz, h)
    assert setting is not None, "no ceiling splits this batch into rows over in true-peak mode only, in both modes and in neither"
    target, ceiling = setting
    c = M.ceiling_linear(ceiling)
    vols = np.broadcast_to(np.asarray(a["kw"].get("pcm_volume", 1.0), np.float64).reshape(-1), (B,))
    tables = G.tables()
    lead = [int(v) for v in np.random.default_rng(len(order)).integers(0, 40, len(order))]
    pack = dict(order=order, lead_samples=lead, tail_samples=5, wav=True)
    eng.set_loudness_target(target, ceiling)
    assert eng.loudness_ceiling_mode == "sample"
    ld_s = eng.fetch_loudness()
    sample_packs = packs_of(eng, pack)
    eng.set_loudness_ceiling_mode("true_peak")
    assert eng.loudness_ceiling_mode == "true_peak"
    ld_t = eng.fetch_loudness()
    over_s, over = ld_s.limited, ld_t.limited
    print(f"{hz} Hz: over in sample mode {over_s.astype(int)}, in true-peak mode {over.astype(int)}")
    assert (over & ~over_s).any() and (over & over_s).any() and (~over).any() and not (over_s & ~over).any()
    assert ld_t.lufs.tobytes() == ld_s.lufs.tobytes()
    for b in range(B):
        g = 1.0 if np.isinf(ld_t.lufs[b]) else 10.0 ** ((target - ld_t.lufs[b]) / 20.0)
        cap = c / want_tp[b] if want_tp[b] > 0 else np.inf
        assert abs(ld_t.gain[b] - min(g, cap)) <= 1e-12 * g and bool(over[b]) == bool(cap < g), (b, ld_t.gain[b], g, cap)
        if over[b]:  # consequence 1, in the doubles of the library: the oversampled peak of the scaled row is under the ceiling
            assert ld_t.gain[b] * want_tp[b] <= c * (1.0 + 2.0 ** -50)
    # limiter off: one scale per entry, capped by the true peak
    off = packs_of(eng, pack)
    for enc in ENCODINGS:
        p = off[enc]
        assert p.gain.tobytes() == ld_t.gain[order].tobytes() and np.array_equal(p.limited, over[order])
        for i, b in enumerate(order):
            assert p.rows[i].tobytes() == sample_entry(rows[b], ld_t.gain[b], False, c, enc, L, vols[b], tables).tobytes(), (enc, i, b)
            if not over[b]:
                assert p.rows[i].tobytes() == sample_packs[enc].rows[i].tobytes(), (enc, i, b)  # under both ceilings: the same bytes
        assert p.data.tobytes() != sample_packs[enc].data.tobytes()
    # limiter on
    eng.set_loudness_limiter(L)
    ld = eng.fetch_loudness()
    assert np.array_equal(ld.limited, over)
    for b in range(B):
        g = 1.0 if np.isinf(ld.lufs[b]) else 10.0 ** ((target - ld.lufs[b]) / 20.0)
        assert abs(ld.gain[b] - g) <= 1e-12 * g  # uncapped, over or not
    eng.profile_enable(True)
    eng.profile_reset()
    lim = eng.fetch_limiter()
    rep = eng.profile_report()
    jobs_len = float(np.sum(out["lengths"][over]))
    assert rep["truepeak.env"]["calls"] == 1 and rep["truepeak.env"]["bytes"] == 12.0 * jobs_len and "truepeak" not in rep
    assert rep["limit"]["calls"] == 1 and rep["limit"]["bytes"] == 8.0 * jobs_len + 16.0 * int(over.sum())
    assert lim.window_samples == L and np.array_equal(lim.engaged, over)
    for b in range(B):
        if not over[b]:
            assert (int(lim.reduced_samples[b]), float(lim.min_scale[b])) == (0, 1.0)
            continue
        _, red, ms = M.stats(TP.curve(rows[b], ld.gain[b], c, 1.0, L, h)[1], L)
        assert int(lim.reduced_samples[b]) == red > 0 and np.float64(lim.min_scale[b]).tobytes() == np.float64(ms).tobytes(), b
    eng.profile_reset()
    got = packs_of(eng, pack)
    rep = eng.profile_report()
    eng.profile_enable(False)
    assert rep["truepeak.env"]["calls"] == rep["limit"]["calls"] == len(ENCODINGS) and "truepeak" not in rep and "loudness" not in rep
    bare = packs_of(eng, dict(pack, wav=False))
    for enc in ENCODINGS:
        p, o = got[enc], off[enc]
        assert np.array_equal(p.offsets, o.offsets) and np.array_equal(p.lengths, o.lengths)
        assert p.gain.tobytes() == ld.gain[order].tobytes() and np.array_equal(p.limited, over[order])
        assert bare[enc].wav is None and bare[enc].data.tobytes() == p.data.tobytes()
        for i, b in enumerate(order):
            want = want_entry(rows[b], ld.gain[b], over[b], c, enc, L, vols[b], tables, h)
            assert p.rows[i].tobytes() == want.tobytes(), (enc, i, b)
            if not over[b]:
                assert p.rows[i].tobytes() == o.rows[i].tobytes() == sample_packs[enc].rows[i].tobytes()  # untouched by either mode
            elif enc == "f32le":  # consequence 2: every sample obeys the ceiling
                assert np.max(np.abs(p.rows[i].astype(np.float64))) <= c * (1.0 + 2.0 ** -22), (i, b)
                print(f"{hz} Hz row {b}: true peak of the limited entry {20 * np.log10(TP.true_peak(p.rows[i], h) / c):+.3f} dB over c"
                      f" (sample mode: {20 * np.log10(TP.true_peak(rows[b] * np.float32(ld.gain[b]), h) / c):+.3f} dB uncapped)")
    # the one-call form: the measurement rides in front of the run's own synchronisation
    for enc in ("s16le", "f32le"):
        eng.set_output_encoding(enc)
        eng.profile_enable(True)
        eng.profile_reset()
        one = eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **a["kw"])
        rep = eng.profile_report()
        eng.profile_enable(False)
        assert rep["truepeak"]["calls"] == 1 and rep["loudness"]["calls"] == 1 and rep["truepeak.env"]["calls"] == 1
        same_stream(one, got[enc])
        assert one.gain.tobytes() == got[enc].gain.tobytes() and np.array_equal(one.limited, got[enc].limited)
    eng.set_output_encoding("s16le")
    eng.set_loudness_limiter(0)
    eng.set_loudness_ceiling_mode("sample")
    eng.set_loudness_target(None)
    return target, ceiling


def check_streams(eng, a, rate, h, L=ENGINE_WINDOW):
    """run_streams / fetch_streams: each stream is bitwise fetch_packed under its own settings plus the handle's mode and window, and
    the handle's own settings are neither read nor changed."""
    out = run_at(eng, rate, a)
    hz = rate or eng.config.sample_rate
    setting = true_peak_setting(out, hz, h)
    assert setting is not None
    target, ceiling = setting
    B = len(out["lengths"])
    order = list(range(B))[::-1]
    specs = [dict(order=order, wav=True, encoding="s16le", loudness=(target, ceiling)),
             dict(order=order, encoding="f32le", loudness=(target + 6.0, ceiling)),
             dict(order=order[:3], wav=True, encoding="ulaw", loudness=(target, ceiling), trim=(0.9, 3), lead_samples=[4, 0, 9]),
             dict(order=order, encoding="alaw"),  # no target: neither the mode nor the window does anything
             dict(order=order[1:], encoding="f32le", loudness=(target, ceiling))]
    eng.set_output_encoding("alaw")
    eng.set_loudness_target(-30.0, -9.0)  # not read by the streams calls
    results = {}
    for window in (0, L):
        eng.set_loudness_limiter(window)
        eng.set_loudness_ceiling_mode("sample")
        plain = eng.fetch_streams(specs)
        eng.set_loudness_ceiling_mode("true_peak")
        got = eng.fetch_streams(specs)
        ran = eng.run_streams(a["ids"], a["lens"], a["scales"], a.get("sid"), streams=specs, **a["kw"])
        assert (eng.output_encoding, eng.loudness_target, eng.loudness_limiter, eng.loudness_ceiling_mode) == ("alaw", (-30.0, -9.0), window, "true_peak")
        differs = 0
        for s, spec in enumerate(specs):
            eng.set_output_encoding(spec["encoding"])
            eng.set_loudness_target(*spec.get("loudness", (None, -1.0)))
            eng.set_edge_trim(*spec.get("trim", (0.0, 0)))
            want = eng.fetch_packed(order=spec["order"], lead_samples=spec.get("lead_samples"), wav=spec.get("wav", False))
            for g in (got[s], ran[s]):
                same_stream(g, want)
                if "loudness" in spec:
                    assert g.gain.tobytes() == want.gain.tobytes() and np.array_equal(g.limited, want.limited)
            if "loudness" in spec:
                differs += got[s].data.tobytes() != plain[s].data.tobytes()
            else:
                assert got[s].data.tobytes() == plain[s].data.tobytes()
        assert differs >= 2  # the mode reached the streams
        eng.set_edge_trim(0.0)
        eng.set_output_encoding("alaw")
        eng.set_loudness_target(-30.0, -9.0)
        results[window] = got
    assert results[0][0].data.tobytes() != results[L][0].data.tobytes()
    eng.set_output_encoding("s16le")
    eng.set_loudness_limiter(0)
    eng.set_loudness_ceiling_mode("sample")
    eng.set_loudness_target(None)


def check_off_is_off(make_engine, a, rate, h, L=ENGINE_WINDOW):
    """Sample mode — never set, and set and put back — gives every packed byte, fetch_loudness, fetch_limiter and the profile's kernel
    list of a handle that never heard of the setting; and in true-peak mode the padded results, fetch, fetch_alignment, fetch_edges
    and device_result never move."""
    fresh, eng = make_engine(), make_engine()
    assert eng.loudness_ceiling_mode == "sample"
    eng.set_loudness_ceiling_mode("true_peak")
    eng.set_loudness_ceiling_mode("sample")
    out = run_at(fresh, rate, a)
    hz = rate or fresh.config.sample_rate
    target, ceiling = true_peak_setting(out, hz, h)
    labels = []
    for e in (fresh, eng):
        e.set_output_rate(rate)
        e.set_loudness_target(target, ceiling)
        e.profile_enable(True)
        e.profile_reset()
    B = len(out["lengths"])
    pack = dict(order=list(range(B))[::-1], lead_samples=[(3 * i) % 7 for i in range(B)], tail_samples=2, wav=True)
    for window in (0, L):
        for e in (fresh, eng):
            e.set_loudness_limiter(window)
        for enc in ENCODINGS:
            for e in (fresh, eng):
                e.set_output_encoding(enc)
            want = fresh.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **a["kw"])
            got = eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **a["kw"])
            same_stream(got, want)
            same_stream(eng.fetch_packed(**pack), fresh.fetch_packed(**pack))
            assert got.gain.tobytes() == want.gain.tobytes() and np.array_equal(got.limited, want.limited) and want.limited.any()
        specs = [dict(order=[1, 0], encoding="s16le", loudness=(target, ceiling), wav=True), dict(encoding="f32le", loudness=(target, ceiling))]
        for x, y in zip(eng.fetch_streams(specs), fresh.fetch_streams(specs)):
            same_stream(x, y)
        lw, lg = fresh.fetch_loudness(), eng.fetch_loudness()
        for k in ("lufs", "gain", "blocks", "gated", "limited"):
            assert getattr(lg, k).tobytes() == getattr(lw, k).tobytes(), k
        mw, mg = fresh.fetch_limiter(), eng.fetch_limiter()
        for k in ("engaged", "reduced_samples", "min_scale"):
            assert getattr(mg, k).tobytes() == getattr(mw, k).tobytes(), k
    for e in (fresh, eng):
        labels.append({k: (v["calls"], v["bytes"]) for k, v in e.profile_report().items()})
        e.profile_enable(False)
    assert labels[0] == labels[1] and "limit" in labels[1] and not any(k.startswith("truepeak") for k in labels[1])
    # the mode without a target does nothing to a pack
    for e in (fresh, eng):
        e.set_loudness_target(None)
        e.set_loudness_limiter(0)
        e.set_output_encoding("s16le")
    eng.set_loudness_ceiling_mode("true_peak")
    eng.profile_enable(True)
    eng.profile_reset()
    same_stream(eng.fetch_packed(wav=True), fresh.fetch_packed(wav=True))
    assert not any(k.startswith("truepeak") or k == "loudness" for k in eng.profile_report())
    eng.profile_enable(False)

    # true-peak mode: nothing outside the packed streams moves
    def served(e):
        f = e.fetch(want_float=True, want_pcm16=True)
        al = e.fetch_alignment(levels=True)
        ed = e.fetch_edges()
        return ([f[k].tobytes() for k in ("audio", "pcm", "lengths", "peaks")] + [int(f["l_max"])] +
                [getattr(al, k).tobytes() for k in ("frames", "start", "samples", "peak", "rms")] +
                [ed.first.tobytes(), ed.end.tobytes(), e.fetch_loudness().lufs.tobytes()])

    for e in (fresh, eng):
        e.set_loudness_target(target, ceiling)
        e.set_loudness_limiter(L)
        e.set_edge_trim(0.9, 3)
    assert served(eng) == served(fresh)
    on = run_at(eng, rate, a)
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert on[k].tobytes() == out[k].tobytes(), k
    run_at(fresh, rate, a)
    want = served(fresh)  # a handle in sample mode after the same padded call
    assert served(eng) == want
    dev = eng.device_result()
    eng.fetch_true_peak()
    eng.fetch_limiter()
    eng.fetch_packed(wav=True)
    assert served(eng) == want and eng.device_result() == dev
    fresh.close()
    eng.close()


def check_errors(make_engine, a):
    """An unknown mode is rejected and the setting stays; fetch_true_peak before a run; NULL out; clone inheritance; the struct's
    free; a run below 4000 Hz with a target, as in sample mode."""
    eng = make_engine()
    lib = eng.native.lib
    with pytest.raises(NativeError, match="fetch_true_peak: no completed run on this handle") as err:
        eng.fetch_true_peak()
    assert err.value.code == -1
    assert lib.mi355vits_fetch_true_peak(eng._h, None) == -1
    eng.set_loudness_ceiling_mode("true_peak")
    for bad in (2, -1, 1 << 20):
        assert lib.mi355vits_set_loudness_ceiling_mode(eng._h, bad) == -1
        msg = (lib.mi355vits_last_error(eng._h) or b"").decode()
        assert "set_loudness_ceiling_mode" in msg and str(bad) in msg
        assert eng.loudness_ceiling_mode == "true_peak" and lib.mi355vits_get_loudness_ceiling_mode(eng._h) == 1
    for bad in ("dbtp", None, 2):
        with pytest.raises(ValueError, match="ceiling mode"):
            eng.set_loudness_ceiling_mode(bad)
    twin = eng.clone()  # a further lane inherits the setting
    assert twin.loudness_ceiling_mode == "true_peak"
    twin.close()
    run_at(eng, 0, a)
    assert lib.mi355vits_fetch_true_peak(eng._h, None) == -1
    r = TruePeakResult()
    assert lib.mi355vits_fetch_true_peak(eng._h, ctypes.byref(r)) == 0 and r.batch == a["ids"].shape[0]
    assert r.sample_rate == eng.config.sample_rate and r.true_peak and r.peak and r.true_peak[0] >= r.peak[0]
    lib.mi355vits_free_true_peak(ctypes.byref(r))
    assert not r.true_peak and not r.peak and not r.owner_
    lib.mi355vits_free_true_peak(ctypes.byref(r))  # freeing twice is harmless
    # below 4000 Hz the loudness is not offered, with either ceiling: the pack with a target fails as it does today
    eng.set_loudness_target(-23.0, -1.0)
    run_at(eng, 3000, a)
    with pytest.raises(NativeError, match="4000"):
        eng.fetch_packed()
    eng.fetch_true_peak()  # the oversampled peak itself has no such limit
    eng.set_loudness_ceiling_mode("sample")
    with pytest.raises(NativeError, match="4000"):
        eng.fetch_packed()
    eng.close()


def check_session(sess, a, h, rate=8000):
    """true_peak= reaches the lane and goes back to the sample peak for a call that does not ask; run_stream and request_wav carry
    it.  -> (keywords, the sample-mode and the true-peak streams)"""
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    B = a["ids"].shape[0]
    keys = list(range(31, 31 + B))
    eng = sess._engines[0]
    probe = sess.run_packed(feed, sample_rate=rate, utterance_keys=keys, loudness=-23)
    # every row over in both modes: a ceiling 3 dB under the smallest sample crest
    crest = 20.0 * np.log10(probe.peaks.astype(np.float64)) - probe.lufs
    kw = dict(sample_rate=rate, utterance_keys=keys, loudness=-23.0, ceiling_db=float(np.floor(-23.0 + np.min(crest) - 3.0)))
    plain = sess.run_packed(feed, **kw)
    assert plain.limited.all() and eng.loudness_ceiling_mode == "sample"
    got = sess.run_packed(feed, true_peak=True, **kw)
    assert eng.loudness_ceiling_mode == "true_peak" and got.limited.all()
    assert (got.gain <= plain.gain).all() and (got.gain < plain.gain).any() and got.data.tobytes() != plain.data.tobytes()
    again = sess.run_packed(feed, **kw)  # the lane is back to the sample peak
    assert eng.loudness_ceiling_mode == "sample" and again.data.tobytes() == plain.data.tobytes()
    assert sess.run_packed(feed, true_peak=False, **kw).data.tobytes() == plain.data.tobytes()
    assert sess.run_stream(feed, true_peak=True, **kw).data.tobytes() == got.data.tobytes()
    assert sess.run_stream(feed, **kw).data.tobytes() == plain.data.tobytes()
    wav = PP.request_wav(sess, [a["ids"][b, : int(a["lens"][b])] for b in range(B)], break_ms=20.0, true_peak=True, **kw)
    assert wav == bytes(sess.run_packed(feed, lead_ms=[0.0] + [20.0] * (B - 1), wav=True, true_peak=True, **kw).wav)
    return feed, kw, plain, got


def check_micro_batcher_keeps_modes_apart(sess, a, h, rate=8000):
    """Requests with different ceiling modes that arrive together never share a run_streams call: each gets the bytes of its own
    run_packed."""
    feed, kw, plain, got = check_session(sess, a, h, rate)
    modes = [None, True, False, True, None, True]
    want = [(got if m else plain).data.tobytes() for m in modes]
    res = [None] * len(modes)
    gate = threading.Barrier(len(modes))

    def work(i):
        gate.wait()
        res[i] = sess.run_stream(feed, true_peak=modes[i], **kw).data.tobytes()

    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(modes))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert res == want


# ------------------------------------------------------------------------------------------ the CPU model
SEED = 93  # the tiny voice and case whose batch has rows over in true-peak mode only, in both modes and in neither at both rates


@pytest.fixture
def cu_count(emu_lib):
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(DEFAULT_CUS)


def true_peak_engine(blob, lib, **kw):
    eng = Engine(blob, library=lib, **kw)
    eng.set_loudness_ceiling_mode("true_peak")
    return eng


def test_the_kernel_alone(emu_lib):
    """This fails without the feature."""
    check_kernel_alone(emu_lib)


def test_limiter_with_an_envelope(emu_lib):
    """This fails without the feature."""
    check_limiter_with_envelope(emu_lib)


@pytest.mark.parametrize("rate", [0, 8000])
def test_packs(emu_lib, rate):
    """This fails without the feature."""
    cfg, blob = _engine(SEED)
    eng = Engine(blob, library=emu_lib)
    check_packs(eng, _long_case(cfg, SEED), rate, [3, 0, 4, 1, 2], library_taps(emu_lib))
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_streams(emu_lib, rate):
    cfg, blob = _engine(SEED)
    eng = Engine(blob, library=emu_lib)
    check_streams(eng, _long_case(cfg, SEED), rate, library_taps(emu_lib))
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_batched_is_alone_at_any_cu_count_and_on_a_poisoned_workspace(emu_lib, cu_count, rate):
    cfg, blob = _engine(SEED)
    a = _long_case(cfg, SEED)
    eng = true_peak_engine(blob, emu_lib)
    target, ceiling = true_peak_setting(run_at(eng, rate, a), rate or cfg.sample_rate, library_taps(emu_lib))
    want = limited_batch(eng, a, rate, target, ceiling)
    assert want[1].engaged.any() and not want[1].engaged.all()
    check_rows_alone(lambda: true_peak_engine(blob, emu_lib), a, rate, range(5), want[0], want[1], target, ceiling)
    big = dict(a, ids=np.tile(a["ids"], (2, 2)), lens=np.tile(a["lens"] * 2, 2), scales=np.tile(a["scales"], (2, 1)), sid=None,
               kw=dict(seed=1, forced_durations=np.full((10, 24), 70, np.int32)))
    limited_batch(eng, big, rate, -3.0, -6.0)  # sizes the measurement's, the limiter's and the pack's own arenas past what the batch needs
    eng.fill_workspace(NAN)
    same_batch(limited_batch(eng, a, rate, target, ceiling), want)
    for cus in (13, 256):
        cu_count(cus)
        same_batch(limited_batch(eng, a, rate, target, ceiling), want)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_off_is_off(emu_lib, rate):
    cfg, blob = _engine(SEED)
    check_off_is_off(lambda: Engine(blob, library=emu_lib), _long_case(cfg, SEED), rate, library_taps(emu_lib))


def test_errors(emu_lib):
    cfg, blob = _engine(95)
    check_errors(lambda: Engine(blob, library=emu_lib), _case(cfg, 95))


def test_session_routing(emu_lib):
    cfg, blob = _engine(SEED)
    opts = SessionOptions()
    opts.seed = 5
    opts.micro_batch_window_ms = 5.0
    opts.micro_batch_max = 16
    a = _long_case(cfg, SEED)
    a = dict(a, ids=a["ids"][:3], lens=a["lens"][:3])
    sess = InferenceSession(blob, opts, _library=emu_lib)
    check_micro_batcher_keeps_modes_apart(sess, a, library_taps(emu_lib))
    sess.close()
    sess = InferenceSession(blob, opts, _library=emu_lib, loudness_lufs=-16.0, loudness_true_peak=True)  # the session's own default
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    sess.run_packed(feed, utterance_keys=[1, 2, 3])
    assert sess._engines[0].loudness_ceiling_mode == "true_peak"
    sess.run_packed(feed, utterance_keys=[1, 2, 3], true_peak=False)
    assert sess._engines[0].loudness_ceiling_mode == "sample"
    sess.close()


def test_plain_c99_client(emu_lib, tmp_path):
    """A C99 client fetches a tiny voice's oversampled peaks and checks the gain rule of both ceiling modes against them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_true_peak_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_true_peak_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir, "-lm"], check=True)
    cfg = VitsConfig.tiny()
    W.save(str(tmp_path / "voice.m355"), cfg, W.synthetic_weights(cfg, seed=17))
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "expected failure rc=-1 msg=fetch_true_peak: no completed run on this handle" in p.stdout
    assert "set_loudness_ceiling_mode: mode 7 unknown" in p.stdout
    assert "true peak ok" in p.stdout
