"""The look-ahead peak limiter of the packed streams (mi355vits_set_loudness_limiter / mi355vits_fetch_limiter, k_limit) on the CPU
model of the kernels; test_gpu_limiter.py runs the same checks on the MI355X.

The yardstick is tests/limiter_ref.py — numpy from the rule of include/mi355vits.h, never the code under test — applied to the
WANT_FLOAT audio OF THE SAME RUN under the gain the library reports (g is made by two pow() of the host's libm: the gain rule is
checked to 1e-12 against numpy as in test_loudness.py, everything behind it bit for bit).  c = 10 ** (ceiling / 20) is the same
libm call on both sides.  Every comparison of samples, scales and statistics is exact.

Not tested: the number of stream synchronisations of a call (no hook counts them)."""
import ctypes
import threading

import numpy as np
import pytest

from mimic3_amd import _native
from mimic3_amd import postprocess as PP
from mimic3_amd._native import Engine, Limiter, LimiterResult, NativeError
from mimic3_amd.session import InferenceSession, SessionOptions
from tests import g711_ref as G
from tests import limiter_ref as M
from tests import loudness_ref as R
from tests.test_loudness import ENCODINGS, NAN, _engine, _long_case, packs_of, reference_of, same_stream, straddling_setting
from tests.test_resample import DEFAULT_CUS, _case, run_at

TILE = 4096                          # samples of a k_limit work item
WINDOWS = (1, 7, 100, 255, 4096)     # 100: not one less than a power of two
ENGINE_WINDOW = 24                   # samples: a few milliseconds at the tiny voice's rates
C_LAB = 0.5


def unit(enc):
    return 1.0 if enc == "f32le" else 32767.0


# ------------------------------------------------------------------------------------------ the yardstick itself
def test_the_yardsticks_three_consequences():
    """By brute force on small arrays: the ceiling bound, the bit identity away from peaks, sliding sums = direct sums."""
    rng = np.random.default_rng(1)
    for L in (1, 7, 64, 220):
        for g in (1.0, 2.5, 40.0):
            c = 10.0 ** (-1.5 / 20.0)
            n = 1500
            x = (rng.standard_normal(n) * (0.15 / g)).astype(np.float32)  # g |x| stays under c: only the peaks are over
            x[rng.integers(0, n, 4)] = rng.uniform(0.5, 1.0, 4).astype(np.float32)
            x[5:800] = 0.0  # a stretch whose middle is further than L from every sample that is over
            x[0], x[n - 1] = 0.9, -0.95
            mq = M.mq_of(M.rq_of(x, g, c), L)
            small = M.rq_of(x[:260], g, c)  # the window minimum itself against one min() per window (the doubling scheme is k_limit's too)
            assert np.array_equal(M.mq_of(small, L), M.mq_direct(small, L))
            assert len(mq) == n + L and np.array_equal(M.sq_sliding(mq, L), M.sq_direct(mq, L))
            worst = 0.0
            for U in (1.0, 32767.0):
                scale, sq = M.curve(x, g, c, U, L)
                assert scale.dtype == np.float32 and sq.dtype == np.int64 and sq.max() <= (L + 1) * M.ONE and sq.min() >= 0
                full = sq == (L + 1) * M.ONE
                assert full.any() and not full.all()
                # 2. where the whole window is ONE the scale is bitwise what an uncapped gain writes
                assert (scale[full].view(np.uint32) == np.float32(U * g).view(np.uint32)).all()
                if U == 1.0:  # 1. the ceiling holds
                    y = x * scale
                    assert y.dtype == np.float32
                    worst = max(worst, float(np.max(np.abs(y.astype(np.float64))) / c - 1.0))
                    assert np.max(np.abs(y.astype(np.float64))) <= c * (1.0 + 2.0 ** -22)
                else:
                    q = R.pcm16_quant(x, scale, 1.0).astype(np.int64)
                    assert np.max(np.abs(q)) <= np.floor(32767.0 * c) + 1
            print(f"L {L} g {g}: excess over c {worst:.2e}")
    # samples that are not over leave everything alone; a NaN is not over
    x = np.array([0.1, np.nan, -0.2, 0.0], np.float32)
    scale, sq = M.curve(x, 2.0, 0.5, 32767.0, 3)
    assert (sq == 4 * M.ONE).all() and (scale.view(np.uint32) == np.float32(32767.0 * 2.0).view(np.uint32)).all()
    assert M.stats(sq, 3) == (4 * M.ONE, 0, 1.0) and M.stats(np.zeros(0, np.int64), 3) == (4 * M.ONE, 0, 1.0)


# ------------------------------------------------------------------------------------------ checks shared with the GPU twin
def constructed_rows(L):
    """The rows of the kernel-alone check at window L: (name, samples, g).  Quiet noise (never over at g = 2.5, c = 0.5) with peaks of
    0.9 placed where the kernel could go wrong; a few thousand samples each."""
    rng = np.random.default_rng(L)
    quiet = lambda n: (rng.standard_normal(n) * 0.01).astype(np.float32)  # noqa: E731
    busy = lambda n: (rng.standard_normal(n) * 0.1).astype(np.float32)    # noqa: E731  (g |x| > c at two sigma: a few percent over)
    rows = []

    def add(name, x, g=2.5):
        rows.append((name, np.asarray(x, np.float32), g))

    x = quiet(6000)
    x[0], x[-1] = 0.9, -0.9
    add("peaks at 0 and n - 1", x)
    n = TILE + L + 37
    for p in (TILE - 1, TILE, TILE + 1, TILE - L, TILE + L):
        x = quiet(n)
        x[p] = 0.9
        add(f"peak at {p}", x)
    add("n = 1, over", [0.9])
    add("n = 1, not over", [0.01])
    x = quiet(max(1, L - 1))
    x[len(x) // 2] = -0.9
    add("n < L", x)
    for n in (TILE - 1, TILE, TILE + 1):
        add(f"n = {n}", busy(n))
    add("every sample over", (rng.uniform(0.5, 0.9, 3000) * rng.choice([-1.0, 1.0], 3000)).astype(np.float32))
    x = quiet(3000)
    x[1500] = 0.9
    add("a single over sample", x)
    x = busy(3000)
    x[100], x[105] = np.nan, 0.9
    add("a NaN sample", x)
    add("all zero", np.zeros(3000, np.float32))
    add("a large gain", busy(2500), 40.0)
    x = busy(TILE + 301)
    x[TILE - 2] = 0.9
    for k in range(4):  # the same row at four consecutive places: with a stride of 1 mod 4 floats, at every 4-byte alignment of its base
        add(f"alignment {k}", x)
    return rows


def check_kernel_alone(lib, windows=WINDOWS):
    """k_limit alone through the hook, bitwise against the yardstick: scale, min sq and the reduced count of every constructed row, with
    NaN and then 3e38 behind every row, at U = 32767 and (one window) U = 1."""
    for L in windows:
        rows = constructed_rows(L)
        lens = np.array([len(r[1]) for r in rows], np.int32)
        g = np.array([r[2] for r in rows], np.float64)
        stride = int(lens.max()) + 3
        stride += (1 - stride) % 4
        assert stride % 4 == 1
        for U in (32767.0, 1.0) if L == 100 else (32767.0,):
            want = [M.curve(r[1], r[2], C_LAB, U, L) for r in rows]
            st = [M.stats(w[1], L) for w in want]
            assert any(0 < s[1] < n for s, n in zip(st, lens)) and any(s[1] == 0 for s in st)
            for fill in (np.float32("nan"), np.float32(3e38)):
                audio = np.full((len(rows), stride), fill, np.float32)
                for b, r in enumerate(rows):
                    audio[b, : lens[b]] = r[1]
                scale, sq_min, reduced = lib.lab_limit(audio, lens, g, C_LAB, U, L)
                assert scale.dtype == np.float32 and sq_min.dtype == np.int64 and reduced.dtype == np.int32
                for b, r in enumerate(rows):
                    n = int(lens[b])
                    assert scale[b, :n].tobytes() == want[b][0].tobytes(), (L, U, r[0])
                    assert not scale[b, n:].any(), (L, r[0])
                    assert (int(sq_min[b]), int(reduced[b])) == st[b][:2], (L, U, r[0], sq_min[b], reduced[b], st[b])
            al = [b for b, r in enumerate(rows) if r[0].startswith("alignment")]
            assert len(al) == 4 and all(want[b][0].tobytes() == want[al[0]][0].tobytes() for b in al)
    with pytest.raises(NativeError):  # a length past the stride: refused before anything is launched
        lib.lab_limit(np.zeros((1, 8), np.float32), [9], [1.0], 0.5, 1.0, 4)
    for bad in (0, 4097):
        with pytest.raises(NativeError):
            lib.lab_limit(np.zeros((1, 8), np.float32), [8], [1.0], 0.5, 1.0, bad)
    empty = lib.lab_limit(np.full((2, 8), np.nan, np.float32), [0, 0], [1.0, 1.0], 0.5, 1.0, 4)
    assert not empty[0].any() and empty[1].tolist() == [5 * M.ONE] * 2 and empty[2].tolist() == [0, 0]


def over_setting(eng, a, rate):
    """One padded run at `rate` and a (target, ceiling) at which some of its rows are over and some are not (straddling_setting: from
    the yardstick's side alone).  -> (out, hz, target, ceiling)"""
    out = run_at(eng, rate, a)
    hz = rate or eng.config.sample_rate
    target, ceiling = straddling_setting(out, reference_of(out, hz))
    return out, hz, target, ceiling


def want_entry(x, gain, over, c, enc, L, vol, tables):
    """The bytes of one entry from the row's float samples: the curve for a row that is over, the one scale otherwise."""
    U = unit(enc)
    scale = M.curve(x, gain, c, U, L)[0] if over else np.float32(U * gain)
    if enc == "f32le":
        y = x * scale
        assert y.dtype == np.float32
        return y
    q = R.pcm16_quant(x, scale, float(vol))
    return q if enc == "s16le" else G.encode(tables[enc], q)


def check_limited_packs(eng, a, rate, order, L=ENGINE_WINDOW):
    """The engine at one rate: gain / limited with the limiter on, fetch_limiter against the yardstick's statistics, every entry of
    the four encodings byte for byte, rows that are not over = the limiter off, the ceiling bounds, trimmed = slice of untrimmed, the
    `limit` profile line, and the one-call form."""
    out, hz, target, ceiling = over_setting(eng, a, rate)
    B = len(out["lengths"])
    c = M.ceiling_linear(ceiling)
    vols = np.broadcast_to(np.asarray(a["kw"].get("pcm_volume", 1.0), np.float64).reshape(-1), (B,))
    tables = G.tables()
    lead = [int(v) for v in np.random.default_rng(len(order)).integers(0, 40, len(order))]
    pack = dict(order=order, lead_samples=lead, tail_samples=5, wav=True)
    eng.set_loudness_target(target, ceiling)
    eng.set_loudness_limiter(0)
    ld0 = eng.fetch_loudness()
    off = packs_of(eng, pack)
    eng.set_loudness_limiter(L)
    assert eng.loudness_limiter == L
    ld = eng.fetch_loudness()
    over = ld.limited
    assert np.array_equal(over, ld0.limited) and ld.lufs.tobytes() == ld0.lufs.tobytes()
    assert over.any() and not over.all(), (target, ceiling, over)  # both kinds of row exist
    for b in range(B):
        g = 1.0 if np.isinf(ld.lufs[b]) else 10.0 ** ((target - ld.lufs[b]) / 20.0)
        assert abs(ld.gain[b] - g) <= 1e-12 * g, (b, ld.gain[b], g)  # uncapped, over or not
        assert (ld.gain[b].tobytes() == ld0.gain[b].tobytes()) == (not over[b])
    # fetch_limiter = the yardstick's statistics
    eng.profile_enable(True)
    eng.profile_reset()
    lim = eng.fetch_limiter()
    rep = eng.profile_report()
    eng.profile_enable(False)
    assert isinstance(lim, Limiter) and lim.window_samples == L and lim.sample_rate == hz and np.array_equal(lim.engaged, over)
    partly = 0
    for b in range(B):
        n = int(out["lengths"][b])
        if not over[b]:
            assert (int(lim.reduced_samples[b]), float(lim.min_scale[b])) == (0, 1.0)
            continue
        _, red, ms = M.stats(M.curve(out["audio"][b, :n], ld.gain[b], c, 1.0, L)[1], L)
        print(f"{hz} Hz row {b}: n {n}, reduced {lim.reduced_samples[b]} / {red}, min scale {lim.min_scale[b]!r} / {ms!r}")
        assert int(lim.reduced_samples[b]) == red and np.float64(lim.min_scale[b]).tobytes() == np.float64(ms).tobytes(), b
        partly += 0 < red < n
    assert partly >= 1  # the curve both acts and lets go somewhere: nothing below passes vacuously
    jobs = int(over.sum())
    assert rep["limit"]["calls"] == 1 and rep["limit"]["bytes"] == 8.0 * float(np.sum(out["lengths"][over])) + 16.0 * jobs
    # every entry of every encoding, with and without a header
    eng.profile_enable(True)
    eng.profile_reset()
    got = packs_of(eng, pack)
    assert eng.profile_report()["limit"]["calls"] == len(ENCODINGS)  # the curve is made per pack
    eng.profile_enable(False)
    bare = packs_of(eng, dict(pack, wav=False))
    for enc in ENCODINGS:
        p, o = got[enc], off[enc]
        assert np.array_equal(p.offsets, o.offsets) and np.array_equal(p.lengths, o.lengths) and len(bytes(p.wav)) == len(bytes(o.wav))
        assert p.gain.tobytes() == ld.gain[order].tobytes() and np.array_equal(p.limited, over[order])
        assert bare[enc].wav is None and bare[enc].data.tobytes() == p.data.tobytes()
        for i, b in enumerate(order):
            x = out["audio"][b, : int(out["lengths"][b])]
            want = want_entry(x, ld.gain[b], over[b], c, enc, L, vols[b], tables)
            assert p.rows[i].tobytes() == want.tobytes(), (enc, i, b)
            if not over[b]:
                assert p.rows[i].tobytes() == o.rows[i].tobytes(), (enc, i, b)  # untouched: the bytes of the limiter off
            elif enc == "f32le":
                assert p.rows[i].tobytes() != o.rows[i].tobytes()
                assert np.max(np.abs(p.rows[i].astype(np.float64))) <= c * (1.0 + 2.0 ** -22), (i, b)
                assert np.max(np.abs(p.rows[i])) > np.max(np.abs(o.rows[i])) * 0.999  # the peak sits at the ceiling, the body is louder
            elif enc == "s16le" and vols[b] == 1.0:
                assert np.max(np.abs(p.rows[i].astype(np.int64))) <= np.floor(32767.0 * c) + 1, (i, b)
        silent = np.ones(p.total_samples, bool)
        for i in range(len(order)):
            silent[int(p.offsets[i]): int(p.offsets[i] + p.lengths[i])] = False
        assert p.data[silent].tobytes() == o.data[silent].tobytes()
    # trimmed = [first, end) of untrimmed: the curve is made on the whole row
    eng.set_edge_trim(0.9, 3)
    for enc in ("s16le", "f32le"):
        eng.set_output_encoding(enc)
        t = eng.fetch_packed(**pack)
        assert int(np.sum(t.lengths)) < int(np.sum(got[enc].lengths))
        for i in range(len(order)):
            assert t.rows[i].tobytes() == got[enc].rows[i][int(t.first[i]): int(t.end[i])].tobytes(), (enc, i)
    eng.set_edge_trim(0.0)
    # the one-call form
    for enc in ("s16le", "ulaw"):
        eng.set_output_encoding(enc)
        one = eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **a["kw"])
        same_stream(one, got[enc])
        assert one.gain.tobytes() == got[enc].gain.tobytes()
    eng.set_output_encoding("s16le")
    # the int16 bound of consequence 1 on EVERY over row: the same call at volume 1 (the float audio does not depend on the volume)
    one = eng.run_packed(a["ids"], a["lens"], a["scales"], a.get("sid"), **pack, **dict(a["kw"], pcm_volume=1.0))
    assert np.array_equal(one.limited, over[order]) and one.gain.tobytes() == ld.gain[order].tobytes()
    checked = 0
    for i, b in enumerate(order):
        x = out["audio"][b, : int(out["lengths"][b])]
        assert one.rows[i].tobytes() == want_entry(x, ld.gain[b], over[b], c, "s16le", L, 1.0, tables).tobytes(), (i, b)
        if over[b]:
            peak = int(np.max(np.abs(one.rows[i].astype(np.int64))))
            assert peak <= np.floor(32767.0 * c) + 1, (i, b, peak)
            assert peak >= np.floor(32767.0 * c) - 1, (i, b, peak)  # and the row's peak does reach the ceiling
            checked += 1
    assert checked == int(over.sum()) >= 1
    eng.set_loudness_limiter(0)
    eng.set_loudness_target(None)
    return target, ceiling


def limited_batch(eng, a, rate, target, ceiling, L=ENGINE_WINDOW):
    """The limited f32le and int16 packs of a batch in row order, and its statistics."""
    run_at(eng, rate, a)
    eng.set_loudness_target(target, ceiling)
    eng.set_loudness_limiter(L)
    got = packs_of(eng, {})
    lim = eng.fetch_limiter()
    eng.set_loudness_limiter(0)
    eng.set_loudness_target(None)
    return got, lim


def check_rows_alone(make_engine, a, rate, rows, batched, lim, target, ceiling, L=ENGINE_WINDOW):
    """A row run alone gives bitwise the entry bytes and the statistics it gives in the batch."""
    eng = make_engine()
    eng.set_output_rate(rate)
    eng.set_loudness_target(target, ceiling)
    eng.set_loudness_limiter(L)
    for b in rows:
        n = int(a["lens"][b])
        kw = dict(a["kw"])
        kw["utterance_keys"] = [kw["utterance_keys"][b]]
        kw["pcm_volume"] = float(np.asarray(kw["pcm_volume"]).reshape(-1)[b])
        if "forced_durations" in kw:
            kw["forced_durations"] = kw["forced_durations"][b:b + 1, : max(n, 1)]
        for enc in ("s16le", "f32le"):
            eng.set_output_encoding(enc)
            solo = eng.run_packed(a["ids"][b:b + 1, : max(n, 1)], [n], a["scales"][b], None, **kw)
            assert solo.rows[0].tobytes() == batched[enc].rows[b].tobytes(), (enc, b)
            assert solo.gain[0].tobytes() == batched[enc].gain[b].tobytes() and bool(solo.limited[0]) == bool(batched[enc].limited[b])
        one = eng.fetch_limiter()
        assert (bool(one.engaged[0]), int(one.reduced_samples[0])) == (bool(lim.engaged[b]), int(lim.reduced_samples[b]))
        assert one.min_scale[0].tobytes() == lim.min_scale[b].tobytes()
    eng.close()


def same_batch(x, y):
    for enc in ENCODINGS:
        same_stream(x[0][enc], y[0][enc])
    for k in ("engaged", "reduced_samples", "min_scale"):
        assert getattr(x[1], k).tobytes() == getattr(y[1], k).tobytes(), k


def check_streams(eng, a, rate, L=ENGINE_WINDOW):
    """run_streams / fetch_streams with two targets over the same rows: each stream is bitwise fetch_packed under that stream's
    settings plus the handle's limiter window, and the handle's own settings are neither read nor changed."""
    out, hz, target, ceiling = over_setting(eng, a, rate)
    B = len(out["lengths"])
    order = list(range(B))[::-1]
    specs = [dict(order=order, wav=True, encoding="s16le", loudness=(target, ceiling)),
             dict(order=order, encoding="f32le", loudness=(target + 6.0, ceiling)),  # 6 dB up: more rows over, other gains
             dict(order=order[:3], wav=True, encoding="ulaw", loudness=(target, ceiling), trim=(0.9, 3), lead_samples=[4, 0, 9]),
             dict(order=order, encoding="alaw"),  # no target: the window does nothing
             dict(order=order[1:], encoding="f32le", loudness=(target, ceiling))]  # shares its rows' curves with no other stream's unit
    eng.set_output_encoding("alaw")
    eng.set_loudness_target(-30.0, -9.0)  # not read by the streams calls
    eng.set_loudness_limiter(L)
    eng.profile_enable(True)
    eng.profile_reset()
    got = eng.fetch_streams(specs)
    rep = eng.profile_report()
    eng.profile_enable(False)
    assert rep["limit"]["calls"] == 1 and rep["pack.streams"]["calls"] == 1
    ran = eng.run_streams(a["ids"], a["lens"], a["scales"], a.get("sid"), streams=specs, **a["kw"])
    assert (eng.output_encoding, eng.loudness_target, eng.loudness_limiter) == ("alaw", (-30.0, -9.0), L)
    eng.set_loudness_limiter(0)
    plain = eng.fetch_streams(specs)
    eng.set_loudness_limiter(L)
    jobs = set()
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
            assert want.limited.any() or s == 2
            assert (got[s].data.tobytes() != plain[s].data.tobytes()) == bool(want.limited.any())
            jobs |= {(int(b), spec["loudness"], unit(spec["encoding"])) for b, lim in zip(spec["order"], want.limited) if lim}
        else:
            assert got[s].data.tobytes() == plain[s].data.tobytes()
    # one job per distinct (row, target, ceiling, U) among the over entries
    assert rep["limit"]["bytes"] == 8.0 * sum(float(out["lengths"][b]) for b, _, _ in jobs) + 16.0 * len(jobs)
    eng.set_edge_trim(0.0)
    eng.set_output_encoding("s16le")
    eng.set_loudness_limiter(0)
    eng.set_loudness_target(None)


def check_off_is_off(make_engine, a, rate):
    """With the window at 0 — never set, and set and put back — every pack, fetch_loudness, fetch_limiter and the profiled labels of
    a run are those of a handle that never heard of the limiter."""
    fresh, eng = make_engine(), make_engine()
    assert eng.loudness_limiter == 0
    eng.set_loudness_limiter(64)
    eng.set_loudness_limiter(None)
    assert eng.loudness_limiter == 0
    out, hz, target, ceiling = over_setting(fresh, a, rate)
    labels = []
    for e in (fresh, eng):
        e.set_output_rate(rate)
        e.set_loudness_target(target, ceiling)
        e.profile_enable(True)
        e.profile_reset()
    for wav in (True, False):
        pack = dict(order=[2, 0, 1, 4, 3], lead_samples=[5, 0, 3, 1, 0], tail_samples=2, wav=wav)
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
    lim = eng.fetch_limiter()
    assert lim.window_samples == 0 and not lim.engaged.any() and not lim.reduced_samples.any() and (lim.min_scale == 1.0).all()
    for e in (fresh, eng):
        labels.append({k: (v["calls"], v["bytes"]) for k, v in e.profile_report().items()})
    assert labels[0] == labels[1] and "limit" not in labels[1]  # the same launches, by label, count and bytes
    # the window without a target does nothing either
    eng.set_loudness_target(None)
    fresh.set_loudness_target(None)
    eng.set_loudness_limiter(32)
    eng.profile_reset()
    same_stream(eng.fetch_packed(wav=True), fresh.fetch_packed(wav=True))
    lim = eng.fetch_limiter()
    assert lim.window_samples == 32 and not lim.engaged.any() and (lim.min_scale == 1.0).all()
    assert "limit" not in eng.profile_report() and "loudness" not in eng.profile_report()
    # nor does it where the ceiling binds on no row
    eng.set_loudness_target(-60.0, 0.0)
    fresh.set_loudness_target(-60.0, 0.0)
    got, want = eng.fetch_packed(wav=True), fresh.fetch_packed(wav=True)
    same_stream(got, want)
    assert not got.limited.any() and "limit" not in eng.profile_report()
    fresh.close()
    eng.close()


def check_nothing_else_moves(eng, a, rate, L=ENGINE_WINDOW):
    """The padded results, alignment, edges and fetch_loudness.lufs are identical with the limiter on."""
    def served():
        f = eng.fetch(want_float=True, want_pcm16=True)
        al = eng.fetch_alignment(levels=True)
        e = eng.fetch_edges()
        return ([f[k].tobytes() for k in ("audio", "pcm", "lengths", "peaks")] + [int(f["l_max"])] +
                [getattr(al, k).tobytes() for k in ("frames", "start", "samples", "peak", "rms")] +
                [e.first.tobytes(), e.end.tobytes(), eng.fetch_loudness().lufs.tobytes()])

    out, hz, target, ceiling = over_setting(eng, a, rate)
    eng.set_loudness_target(target, ceiling)
    eng.set_edge_trim(0.9, 3)
    want = served()
    eng.set_loudness_limiter(L)
    assert served() == want
    on = run_at(eng, rate, a)
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert on[k].tobytes() == out[k].tobytes(), k
    assert served() == want
    eng.fetch_limiter()
    eng.fetch_packed(wav=True)
    assert served() == want
    eng.set_edge_trim(0.0)
    eng.set_loudness_limiter(0)
    eng.set_loudness_target(None)


def check_errors(make_engine, a):
    """The setter's range and messages, fetch_limiter before a run, clone inheritance, the struct's free."""
    eng = make_engine()
    lib = eng.native.lib
    with pytest.raises(NativeError, match="fetch_limiter: no completed run on this handle") as err:
        eng.fetch_limiter()
    assert err.value.code == -1
    assert lib.mi355vits_fetch_limiter(eng._h, None) == -1
    eng.set_loudness_limiter(48)
    for bad in (-1, 4097, 1 << 20, -(1 << 31)):
        with pytest.raises(NativeError, match="set_loudness_limiter") as err:
            eng.set_loudness_limiter(bad)
        assert err.value.code == -1 and str(bad) in str(err.value)
        assert eng.loudness_limiter == 48
    for ok in (1, 4096, 48):
        eng.set_loudness_limiter(ok)
        assert eng.loudness_limiter == ok
    twin = eng.clone()  # a further lane inherits the setting
    assert twin.loudness_limiter == 48
    twin.close()
    run_at(eng, 0, a)
    assert lib.mi355vits_fetch_limiter(eng._h, None) == -1
    r = LimiterResult()
    assert lib.mi355vits_fetch_limiter(eng._h, ctypes.byref(r)) == 0 and r.batch == a["ids"].shape[0] and r.window_samples == 48
    assert r.sample_rate == eng.config.sample_rate and r.engaged and r.min_scale[0] == 1.0
    lib.mi355vits_free_limiter(ctypes.byref(r))
    assert not r.engaged and not r.owner_
    lib.mi355vits_free_limiter(ctypes.byref(r))  # freeing twice is harmless
    eng.close()


def check_session(sess, a, rate=8000):
    """limiter_ms= reaches the lane as samples at the run's rate and goes back to off for a call that does not ask; run_stream and
    request_wav carry it; a window outside 1 .. 4096 samples is a ValueError that names it."""
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    B = a["ids"].shape[0]
    keys = list(range(31, 31 + B))
    eng = sess._engines[0]
    probe = sess.run_packed(feed, sample_rate=rate, utterance_keys=keys, loudness=-23)
    # a row is over iff its peak in dBFS lies more than ceiling - target above its loudness: the median of that difference splits the rows
    crest = 20.0 * np.log10(probe.peaks.astype(np.float64)) - probe.lufs
    target = min(-0.5, round(2.0 * (-1.0 - float(np.median(crest)))) / 2.0)
    kw = dict(sample_rate=rate, utterance_keys=keys, loudness=target, ceiling_db=-1.0)
    plain = sess.run_packed(feed, **kw)
    assert plain.limited.any() and not plain.limited.all() and eng.loudness_limiter == 0
    got = sess.run_packed(feed, limiter_ms=3.0, **kw)
    assert eng.loudness_limiter == round(3.0 * rate / 1000.0) == _native.limiter_window(3.0, rate)
    assert np.array_equal(got.limited, plain.limited) and got.data.tobytes() != plain.data.tobytes()
    for i in range(B):
        g = 10.0 ** ((target - got.lufs[i]) / 20.0)
        assert abs(got.gain[i] - g) <= 1e-12 * g
    again = sess.run_packed(feed, **kw)  # the lane is back to off
    assert eng.loudness_limiter == 0 and again.data.tobytes() == plain.data.tobytes()
    shared = sess.run_stream(feed, limiter_ms=3.0, **kw)
    assert shared.data.tobytes() == got.data.tobytes()
    assert sess.run_stream(feed, **kw).data.tobytes() == plain.data.tobytes()
    wav = PP.request_wav(sess, [a["ids"][b, : int(a["lens"][b])] for b in range(B)], break_ms=20.0, limiter_ms=3.0, **kw)
    want = sess.run_packed(feed, lead_ms=[0.0] + [20.0] * (B - 1), wav=True, limiter_ms=3.0, **kw)
    assert wav == bytes(want.wav)
    for bad in (0.0, 0.01, -1.0, 1000.0, float("nan")):
        with pytest.raises(ValueError, match="limiter window"):
            sess.run_packed(feed, limiter_ms=bad, **kw)
        with pytest.raises(ValueError, match="limiter window"):
            sess.run_stream(feed, limiter_ms=bad, **kw)
    return kw, plain, got


def check_micro_batcher_keeps_windows_apart(sess, a, rate=8000):
    """Requests with different limiter windows that arrive together never share a run_streams call: each gets the bytes of its own
    run_packed."""
    B = a["ids"].shape[0]
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    kw, plain, _ = check_session(sess, a, rate)
    windows = [None, 1.0, 3.0, 3.0, None, 5.0]
    want = [sess.run_packed(feed, limiter_ms=w, **kw).data.tobytes() for w in windows]
    assert len(set(want)) == 4
    got = [None] * len(windows)
    gate = threading.Barrier(len(windows))

    def work(i):
        gate.wait()
        got[i] = sess.run_stream(feed, limiter_ms=windows[i], **kw).data.tobytes()

    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(windows))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == want


# ------------------------------------------------------------------------------------------ the CPU model
@pytest.fixture
def cu_count(emu_lib):
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(DEFAULT_CUS)


def test_the_kernel_alone(emu_lib):
    """This fails without the feature."""
    check_kernel_alone(emu_lib)


@pytest.mark.parametrize("rate", [0, 8000])
def test_limited_packs(emu_lib, rate):
    """This fails without the feature."""
    cfg, blob = _engine(93)
    eng = Engine(blob, library=emu_lib)
    check_limited_packs(eng, _long_case(cfg, 93), rate, [3, 0, 4, 1, 2])
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_batched_is_alone_at_any_cu_count_and_on_a_poisoned_workspace(emu_lib, cu_count, rate):
    cfg, blob = _engine(93)
    a = _long_case(cfg, 93)
    eng = Engine(blob, library=emu_lib)
    _, _, target, ceiling = over_setting(eng, a, rate)
    want = limited_batch(eng, a, rate, target, ceiling)
    assert want[1].engaged.any() and not want[1].engaged.all()
    check_rows_alone(lambda: Engine(blob, library=emu_lib), a, rate, range(5), want[0], want[1], target, ceiling)
    big = dict(a, ids=np.tile(a["ids"], (2, 2)), lens=np.tile(a["lens"] * 2, 2), scales=np.tile(a["scales"], (2, 1)), sid=None,
               kw=dict(seed=1, forced_durations=np.full((10, 24), 70, np.int32)))
    limited_batch(eng, big, rate, -3.0, -6.0)  # sizes the limiter's and the pack's own arenas past what the batch needs
    eng.fill_workspace(NAN)
    same_batch(limited_batch(eng, a, rate, target, ceiling), want)
    for cus in (13, 256):
        cu_count(cus)
        same_batch(limited_batch(eng, a, rate, target, ceiling), want)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_streams(emu_lib, rate):
    cfg, blob = _engine(93)
    eng = Engine(blob, library=emu_lib)
    check_streams(eng, _long_case(cfg, 93), rate)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000])
def test_off_is_off(emu_lib, rate):
    cfg, blob = _engine(93)
    check_off_is_off(lambda: Engine(blob, library=emu_lib), _long_case(cfg, 93), rate)


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
    cfg, blob = _engine(93)
    opts = SessionOptions()
    opts.seed = 5
    opts.micro_batch_window_ms = 5.0
    opts.micro_batch_max = 16
    a = _long_case(cfg, 93)
    a = dict(a, ids=a["ids"][:3], lens=a["lens"][:3])
    sess = InferenceSession(blob, opts, _library=emu_lib)
    check_micro_batcher_keeps_windows_apart(sess, a)
    sess.close()
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            InferenceSession(blob, opts, _library=emu_lib, loudness_limiter_ms=bad)
    sess = InferenceSession(blob, opts, _library=emu_lib, loudness_lufs=-16.0, loudness_limiter_ms=2.0)  # the session's own default
    feed = {"input": a["ids"], "input_lengths": a["lens"], "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    sess.run_packed(feed, utterance_keys=[1, 2, 3])
    assert sess._engines[0].loudness_limiter == round(2.0 * cfg.sample_rate / 1000.0)
    with pytest.raises(ValueError, match="limiter window"):  # the session's 2 ms are no sample at 100 Hz... nor is 2 s a window
        sess.run_packed(feed, utterance_keys=[1, 2, 3], limiter_ms=2000.0)
    sess.close()
