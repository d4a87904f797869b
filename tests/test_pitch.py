"""Pitch control in one run (mi355vits_run_pitch, k_pitch_plan, k_pitch) on the CPU model of the kernels; test_gpu_pitch.py runs the
same checks on the MI355X.

The yardstick is tests/pitch_ref.py: the rule of include/mi355vits.h in int64 and numpy f32.  Every comparison is bit for bit
(pitch_ref.same_bits: a NaN equals a NaN); the rule has no tolerance.  The bitwise checks use the engine's own filter table, which
is pinned to numpy's closed form within one f32 ulp."""
import ctypes

import numpy as np
import pytest

from mimic3_amd import postprocess as PP
from mimic3_amd._native import Engine, NativeError, PitchArgs, Result, WANT_FLOAT, WANT_PCM16
from mimic3_amd.session import InferenceSession, SessionOptions
from tests import pitch_ref as PR
from tests.test_levels import first_difference, plant
from tests.test_timing import KEYS, LENS, SCALES, SEED, calls, feed, run, same_run, voice
from tests.util import audio_float_to_int16

POISON = np.float32(-7.5e29)
RATIOS = np.array([0.5, 2.0, 1.0, 1.0 + 2.0 ** -23, 0.75, 1.0595, 1.25, 0.8], np.float32)
_TABLE = {}


def table_of(lib):
    if id(lib) not in _TABLE:
        _TABLE[id(lib)] = lib.test_pitch_table()
    return _TABLE[id(lib)]


# ------------------------------------------------------------------------------------------ the yardstick itself
def tone_snr(f, p, n=6000, edge=200):
    """A tone of f cycles per source sample through a constant ratio p -> (SNR against the analytic sine of f p cycles per output
    sample, the output's power over the input's), both in dB, the edges left out."""
    h = PR.table()
    x = np.sin(2 * np.pi * f * np.arange(n)).astype(np.float32)
    y = PR.warp(x, [n], 1, np.array([p], np.float32), 1, h).astype(np.float64)
    inv = int(PR.inv_of(np.float32(p)))
    want = np.sin(2 * np.pi * f * PR.position(np.arange(y.size), inv))
    e, w = (y - want)[edge:-edge], want[edge:-edge]
    return 10 * np.log10((w ** 2).mean() / max((e ** 2).mean(), 1e-300)), 10 * np.log10(max((y[edge:-edge] ** 2).mean(), 1e-300) / 0.5)


TONES = [(f, p) for f in (0.01, 0.05, 0.15, 0.3) for p in (0.5, 0.8, 1.0595, 1.25, 2.0) if f * p < 0.45]


@pytest.mark.parametrize("f,p", TONES)
def test_yardstick_tones_come_out_at_the_new_pitch(f, p):
    snr, _ = tone_snr(f, p)
    print("tone %.2f x %.4f: SNR %.1f dB" % (f, p, snr))
    assert snr >= 80.0, snr


def test_yardstick_does_not_alias():
    _, left = tone_snr(0.4, 2.0)
    print("0.4 cycles under p = 2 leaves %.1f dB" % left)
    assert left <= -90.0, left


def test_yardstick_on_a_row_worked_by_hand():
    """hop 2, frames 1, 0, 2 at ratios 1, 2, 0.5: inv = ONE, ONE / 2, 2 ONE; Tq = 2, 2, 10 (x ONE): 10 outputs; the first two are the
    first two input samples, bits in, bits out; the even outputs of the slowed span sit on source samples."""
    assert PR.inv_of(np.array([0.5, 1.0, 2.0, 1.0 + 2.0 ** -23, 0.75], np.float32)).tolist() == [2 << 20, 1 << 20, 1 << 19, 1 << 20, 1398101]
    tq, wc, wlen = PR.plan([1, 0, 2], 3, np.array([1, 2, 0.5], np.float32), 2)
    assert (tq // PR.ONE).tolist() == [2, 2, 10] and wc.tolist() == [2, 2, 10] and wlen == 10
    x = np.array([0.5, -0.25, 1.0, 2.0, 3.0, 4.0], np.float32)
    y = PR.warp(x, [1, 0, 2], 3, np.array([1, 2, 0.5], np.float32), 2, PR.table())
    assert y.size == 10 and y[:2].tobytes() == x[:2].tobytes() and y[2::2].tolist() == [1.0, 2.0, 3.0, 4.0]
    assert PR.plan([0, 0], 2, None, 4)[2] == 4 and PR.plan([], 0, None, 4)[2] == 4  # no frames: one pseudo-phoneme of hop samples
    assert PR.peak(np.array([np.nan, -2.0, 1.0], np.float32)) == 2.0


def test_table_is_the_closed_form(emu_lib):
    check_table(emu_lib)


def check_table(lib):
    h, want = table_of(lib), PR.table()
    assert h.shape == (PR.Z * PR.P + 2,) and h[0] == 1.0 and not h[PR.P::PR.P].any() and not h[PR.Z * PR.P:].any()
    ulps = np.abs(h.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, ulps.max()


# ------------------------------------------------------------------------------------------ the kernels alone
def row(frames, ratio=None, x=None):
    return dict(frames=np.asarray(frames, np.int64).reshape(-1), ratio=ratio, x=x)


def run_kernel(lib, rows, hop, seed, alone=None, special=True):
    """The hook on a batch of rows and on each row alone (or those of `alone`): the warped samples bitwise the yardstick's, zeros up
    to y_ld, the floats behind every row's y_ld and behind the last row still poison, peaks bitwise max |y|, wlen the plan's.
    -> [(x, y, peak)] per row"""
    rng = np.random.default_rng(seed)
    h = table_of(lib)
    B, T = len(rows), max(1, max(len(r["frames"]) for r in rows))
    cum, ratio = np.full((B, T), -77, np.int32), np.full((B, T), np.nan, np.float32)  # behind a row: never read
    lens = np.array([len(r["frames"]) for r in rows], np.int32)
    for b, r in enumerate(rows):
        L = int(lens[b])
        cum[b, :L] = np.cumsum(r["frames"])
        ratio[b, :L] = rng.choice(RATIOS, L) if r["ratio"] is None else np.asarray(r["ratio"], np.float32)
    alen = np.array([PR.valid_samples(rows[b]["frames"], int(lens[b]), hop) for b in range(B)], np.int64)
    wlen = np.array([PR.plan(rows[b]["frames"], int(lens[b]), ratio[b], hop)[2] for b in range(B)], np.int64)
    x_bs, y_ld = (int(alen.max()) + 6) | 1, int(wlen.max()) + 5  # odd strides: the rows' bases take every alignment
    y_bs = (y_ld + 4) | 1
    xs = np.full(B * x_bs + 11, POISON, np.float32)  # behind a row: never read
    ys = np.full(B * y_bs + 37, POISON, np.float32)
    want, want_pk, out = ys.copy(), np.zeros(B, np.float32), []
    for b in range(B):
        n = int(alen[b])
        x = rows[b]["x"]
        if x is None:
            x = rng.standard_normal(n).astype(np.float32)
            x = plant(x, b, rng) if special else x
        x = np.asarray(x, np.float32)
        y = PR.warp(x, rows[b]["frames"], int(lens[b]), ratio[b], hop, h)
        assert y.size == wlen[b]
        xs[b * x_bs: b * x_bs + n] = x
        want[b * y_bs: b * y_bs + y_ld] = 0.0
        want[b * y_bs: b * y_bs + y.size], want_pk[b] = y, PR.peak(y)
        out.append((x, y, want_pk[b]))
    got, pk, wl = lib.test_pitch(cum, lens, ratio, hop, xs, x_bs, ys, y_bs, y_ld)
    assert wl.tolist() == wlen.tolist()
    assert PR.same_bits(got, want), first_difference(got, want)
    assert pk.tobytes() == want_pk.tobytes(), (pk, want_pk)
    for b in (range(B) if alone is None else alone):
        if B == 1:
            break
        y1 = np.full(y_bs + 9, POISON, np.float32)
        got1, pk1, wl1 = lib.test_pitch(cum[b:b + 1], lens[b:b + 1], ratio[b:b + 1], hop, xs[b * x_bs: (b + 1) * x_bs], x_bs, y1, y_bs, y_ld)
        want1 = np.concatenate([want[b * y_bs: (b + 1) * y_bs], np.full(9, POISON, np.float32)])
        assert PR.same_bits(got1, want1), (b, first_difference(got1, want1))
        assert pk1.tobytes() == want_pk[b:b + 1].tobytes() and int(wl1[0]) == wlen[b], b
    return out


def check_tile_edges(lib):
    """hop = 1: rows of 1,023 / 1,024 / 1,025 / 2,049 outputs; a pitch step (0.5 <-> 2, 1 <-> 1.0595) exactly on a tile edge and one
    sample either side of it.  hop = 256: rows of 4 and 9 frames, a step mid-row."""
    e = np.float32(1.0 + 2.0 ** -23)
    rows = [row([a, b, c], [1.0, 0.5, e]) for a, b, c in ((23, 400, 200), (24, 400, 200), (25, 400, 200), (49, 900, 200))]  # a + 2 b + c outputs
    rows += [row([1, 511, 700], [1.0, 0.5, 2.0]), row([512, 700], [0.5, 2.0]), row([1, 512, 700], [1.0, 0.5, 2.0])]  # 0.5 -> 2 at 1023, 1024, 1025
    rows += [row([2046, 300], [2.0, 0.5]), row([2048, 300], [2.0, 0.5]), row([2048, 1, 300], [2.0, 1.0, 0.5])]  # 2 -> 0.5 likewise
    rows += [row([n, 700], [1.0, 1.0595]) for n in (1023, 1024, 1025)] + [row([700, 1100], [1.0595, 1.0])]
    out = run_kernel(lib, rows, 1, 10, alone=(0, 3, 5, 9))
    assert [o[1].size for o in out[:4]] == [1023, 1024, 1025, 2049]
    rows = [row([1, 3], [1.0, 2.0]), row([2, 2], [0.5, 2.0]), row([4, 5], [1.0595, 1.0]), row([3, 1, 5], [0.75, 2.0, 0.5]), row([9], [2.0])]
    run_kernel(lib, rows, 256, 11)


def check_small_spans_and_degenerate_rows(lib):
    """A span of one source sample; zero-frame phonemes between spans; L = 0; a row whose durations sum to 0 (each keeps its one
    frame of audio, bit for bit)."""
    for hop in (1, 8, 256):
        rows = [row([5, 1, 5], [1.0, 2.0, 1.0]), row([0, 0, 3, 0, 0, 0, 2, 1, 0], [2.0, 0.5, 0.5, 2.0, 2.0, 0.5, 2.0, 0.75, 0.5]), row([]),
                row([0, 0, 0, 0], [2.0, 0.5, 1.0, 2.0]), row([1], [0.5]), row([1, 1, 1, 1, 1, 1], [2.0, 2.0, 0.5, 2.0, 2.0, 2.0])]
        out = run_kernel(lib, rows, hop, 20 + hop)
        for b in (2, 3):
            assert out[b][0].size == hop and PR.same_bits(out[b][1], out[b][0]) and out[b][2] == PR.peak(out[b][0])


def check_zero_frame_phonemes_change_nothing(lib):
    """Zero-frame phonemes own no sample, whatever their ratio: the row is bitwise the row without them."""
    frames = np.array([0, 0, 2, 0, 0, 0, 3, 1, 0, 0])
    ratio = np.where(frames == 0, 2.0, [9, 9, 0.5, 9, 9, 9, 2.0, 0.75, 9, 9]).astype(np.float32)
    full = run_kernel(lib, [row(frames, ratio)], 256, 30)
    keep = frames > 0
    bare = run_kernel(lib, [row(frames[keep], ratio[keep])], 256, 30)  # the same seed: the same samples
    assert full[0][0].tobytes() == bare[0][0].tobytes() and PR.same_bits(full[0][1], bare[0][1]) and full[0][2] == bare[0][2]


def check_unity(lib):
    """Every ratio 1 (or 1 + 2^-23, which rounds to inv = ONE), zero-frame phonemes between the spans: bits in, bits out, NaN and
    Inf included, and the peak is the input's."""
    rng = np.random.default_rng(40)
    e = np.float32(1.0 + 2.0 ** -23)
    for hop, rows in ((256, [row(rng.integers(0, 5, 12), np.ones(12)), row([3, 0, 2], [e, 1.0, e])]),
                      (1, [row(rng.integers(0, 300, 15), rng.choice([1.0, e], 15)), row([0, 0], [1.0, 1.0])])):
        for x, y, pk in run_kernel(lib, rows, hop, 41 + hop):
            assert PR.same_bits(y, x) and pk == PR.peak(x)


def check_far_samples_keep_their_bits(lib):
    """Samples further than Z source samples from a span with p != 1 keep their bits."""
    (x, y, _), = run_kernel(lib, [row([300, 40, 300], [1.0, 0.75, 1.0])], 1, 50, special=False)
    assert PR.same_bits(y[: 300 - PR.Z], x[: 300 - PR.Z]) and not PR.same_bits(y[300:330], x[300:330])
    (x, y, _), = run_kernel(lib, [row([300, 40, 300], [1.0, 0.5, 1.0])], 1, 51, special=False)  # inv = 2 ONE: the phase comes back to 0
    assert PR.same_bits(y[: 300 - PR.Z], x[: 300 - PR.Z]) and PR.same_bits(y[380 + PR.Z:], x[340 + PR.Z:])


def check_dense_boundaries(lib):
    """hop = 1, one-sample phonemes: a tile reaches more phonemes than the LDS table holds (256): 512 at ratio 0.5, 2,048 at ratio
    2, runs of zero-frame phonemes among them."""
    rng = np.random.default_rng(60)
    rows = [row(np.ones(1500, np.int64), np.full(1500, 0.5)), row(np.ones(5000, np.int64), np.full(5000, 2.0)), row(np.ones(3000, np.int64)),
            row(np.arange(4000) % 2, rng.choice(RATIOS, 4000)), row(np.ones(257, np.int64), np.full(257, 1.0))]
    run_kernel(lib, rows, 1, 61, alone=(1, 3))


def check_unit_impulse(lib):
    """A unit impulse returns bitwise the interpolated coefficients."""
    h = table_of(lib)
    n, m = 400, 200
    x = np.zeros(n, np.float32)
    x[m] = 1.0
    for p in (0.75, 0.5, 0.8):  # inv >= ONE: D = inv
        (_, y, pk), = run_kernel(lib, [row([n], [p], x)], 1, 70)
        inv = int(PR.inv_of(np.float32(p)))
        k = np.arange(y.size, dtype=np.int64)
        q, r = np.divmod(k * PR.ONE, inv)
        a = np.abs((q - m) * inv + r)
        on = a < PR.Z * inv
        idx, rem = np.divmod(np.where(on, a, 0) * PR.P, inv)
        coef = h[idx] + (rem.astype(np.float32) / np.float32(inv)) * (h[idx + 1] - h[idx])
        assert np.array_equal(np.where(on, coef, np.float32(0.0)).astype(np.float32), y) and pk == np.abs(y).max() and on.sum() > 20
    for p in (2.0, 1.25):  # inv < ONE: the prototype stretched, the sum scaled
        (_, y, pk), = run_kernel(lib, [row([n], [p], x)], 1, 71)
        inv = int(PR.inv_of(np.float32(p)))
        k = np.arange(y.size, dtype=np.int64)
        q, r = np.divmod(k * PR.ONE, inv)
        a = np.abs((q - m) * inv + r)
        on = a < PR.Z * PR.ONE
        idx, rem = np.divmod(np.where(on, a, 0) * PR.P, PR.ONE)
        coef = h[idx] + (rem.astype(np.float32) / np.float32(PR.ONE)) * (h[idx + 1] - h[idx])
        want = (np.float32(inv) * np.float32(2.0 ** -20)) * np.where(on, coef, np.float32(0.0)).astype(np.float32)
        assert np.array_equal(want.astype(np.float32), y) and on.sum() >= 12


def check_plan(lib):
    """k_pitch_plan's Tq / wc / wlen against the yardstick: ragged rows, L = 0, no frames, more phonemes than a pass (256), and a row
    whose warped length does not fit 32 bits (wc and wlen saturate)."""
    rng = np.random.default_rng(80)
    B, T = 6, 700
    frames = rng.integers(0, 9, (B, T))
    lens = np.array([700, 0, 255, 257, 3, 512], np.int32)
    frames[4, :3] = 0
    frames[5, 10] = 4_200_000  # x hop 256 x 2 (ratio 0.5) > 2^31
    ratio = rng.choice(RATIOS, (B, T)).astype(np.float32)
    ratio[5, 10] = 0.5
    cum = np.cumsum(frames, axis=1).astype(np.int32)
    for b in range(B):
        cum[b, lens[b]:] = -77
        ratio[b, lens[b]:] = np.nan
    for rt in (ratio, None):
        tq, wc, wlen = lib.test_pitch_plan(cum, lens, rt, 256)
        for b in range(B):
            wtq, wwc, wwl = PR.plan(frames[b], int(lens[b]), None if rt is None else rt[b], 256)
            assert np.array_equal(tq[b], wtq) and np.array_equal(wc[b], wwc) and int(wlen[b]) == wwl, b
    tq, wc, wlen = lib.test_pitch_plan(cum, lens, ratio, 256)
    assert int(wlen[5]) == PR.SAT and int(wc[5, 9]) < PR.SAT and int(wc[5, 10]) == PR.SAT and int(wlen[1]) == 256 and int(wlen[4]) == 256


def test_kernel_tile_edges(emu_lib):
    check_tile_edges(emu_lib)


def test_kernel_small_spans_and_degenerate_rows(emu_lib):
    check_small_spans_and_degenerate_rows(emu_lib)
    check_zero_frame_phonemes_change_nothing(emu_lib)


def test_kernel_unity_and_far_samples(emu_lib):
    check_unity(emu_lib)
    check_far_samples_keep_their_bits(emu_lib)


def test_kernel_dense_boundaries(emu_lib):
    check_dense_boundaries(emu_lib)


def test_kernel_unit_impulse(emu_lib):
    check_unit_impulse(emu_lib)


def test_plan_kernel(emu_lib):
    check_plan(emu_lib)


# ------------------------------------------------------------------------------------------ through the C ABI
VOLUMES = np.array([100.0, 50.0, 100.0, 130.0, 100.0])
SEMITONE2 = np.float32(2.0 ** (2.0 / 12.0))


def pitch_inputs(a, seed=5):
    """A ratio for every phoneme of the feed: a third of them moved (+2 semitones, the ends of the range and odd values among them)."""
    rng = np.random.default_rng(seed)
    B, Tx = a["ids"].shape
    p = np.where(rng.random((B, Tx)) < 1 / 3, rng.choice(np.array([SEMITONE2, 0.5, 2.0, 0.75, 1.0595, 1.25], np.float32), (B, Tx)), 1.0).astype(np.float32)
    p[0, 3], p[0, 4], p[3, 7] = 2.0, 0.5, SEMITONE2
    p[np.arange(Tx)[None, :] >= a["lens"][:, None]] = np.nan  # behind a row: never looked at
    return p


def forced_of(a, seed=4):
    B, Tx = a["ids"].shape
    forced = np.random.default_rng(seed).integers(0, 7, (B, Tx)).astype(np.int32)
    forced[2, : int(a["lens"][2])] = 0  # a row of no frames: one frame of audio, untouched
    return forced


def same_rows(x, y):
    """Lengths and peaks, and the valid samples of every row of audio and pcm, bit for bit (behind a row's length a pitch run leaves
    zeros, the plain run what its last kernel computed there)."""
    assert x["lengths"].tobytes() == y["lengths"].tobytes() and x["peaks"].tobytes() == y["peaks"].tobytes()
    for b, n in enumerate(int(n) for n in x["lengths"]):
        assert PR.same_bits(x["audio"][b, :n], y["audio"][b, :n]) and x["pcm"][b, :n].tobytes() == y["pcm"][b, :n].tobytes(), b


def run_pitch_raw(eng, a, pitch):
    """mi355vits_run_pitch itself with `pitch` = None (NULL) or a PitchArgs."""
    args, rows, per_row, keep = eng._args(a["ids"], a["lens"], SCALES, a["sid"], SEED, 0, None, None, None, 1.0, KEYS)
    args.flags = WANT_FLOAT | WANT_PCM16
    r = Result()
    rc = eng.native.lib.mi355vits_run_pitch(eng._h, ctypes.byref(args), ctypes.byref(rows) if per_row else None, None, None, None,
                                            None if pitch is None else ctypes.byref(pitch), ctypes.byref(r))
    if rc != 0:
        eng._check(rc)
    out = eng._take(r)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def check_identity(eng, a):
    """NULL pitch and a struct without a ratio ARE the levels run: the same launches, the same bytes.  Every ratio 1 is bitwise the
    plain run, as a timed run with the two pitch kernels."""
    B, Tx = a["ids"].shape
    eng.profile_enable(True)
    eng.profile_reset()
    plain = run(eng, a)
    want_calls = calls(eng)
    assert "pitch" not in want_calls and "pitch.plan" not in want_calls
    for pa in (None, PitchArgs()):
        eng.profile_reset()
        same_run(run_pitch_raw(eng, a, pa), plain)
        assert calls(eng) == want_calls
    eng.profile_reset()
    ones = run(eng, a, pitch=np.ones((B, Tx), np.float32))
    same_rows(ones, plain)
    assert ones["audio"].shape == plain["audio"].shape
    got = calls(eng)
    assert got.pop("pitch.plan") == 1 and got.pop("pitch") == 1 and got.pop("durations.timed") == 1
    assert got == {k: v for k, v in want_calls.items() if k != "durations"}
    forced = forced_of(a)
    same_rows(run(eng, a, pitch=np.ones((B, Tx), np.float32), forced_durations=forced), run(eng, a, forced_durations=forced))
    eng.profile_enable(False)
    return plain


def check_rule(eng, hooks, a, p, rate=16000):
    """With forced_durations and the taps on: the yardstick applied to the audio_synth tap is bitwise the result — lengths, peaks, the
    int16 rows with their volumes, the rows behind their lengths zero; the same at a 16 kHz output rate (the resampler's result of
    the warped native row) and in a packed WAV."""
    hop, h = eng.config.hop_length, table_of(hooks)
    B, Tx = a["ids"].shape
    forced = forced_of(a)
    kw = dict(forced_durations=forced, pcm_volume=VOLUMES[:B] / 100.0)
    plain = run(eng, a, **kw)
    got = run(eng, a, pitch=p, debug_taps=True, **kw)
    synth = eng.tap("audio_synth")
    assert synth.shape == (B, 1, plain["audio"].shape[-1])
    native, moved = [], 0
    for b in range(B):
        L = int(a["lens"][b])
        n = PR.valid_samples(forced[b], L, hop)
        assert int(plain["lengths"][b]) == n and PR.same_bits(synth[b, 0, :n], plain["audio"][b, :n])
        y = PR.warp(synth[b, 0, :n], forced[b], L, p[b], hop, h)
        assert int(got["lengths"][b]) == y.size, b
        assert PR.same_bits(got["audio"][b, : y.size], y), (b, first_difference(got["audio"][b, : y.size], y))
        assert not got["audio"][b, y.size:].any()
        assert got["peaks"][b].tobytes() == PR.peak(y).tobytes(), b
        want = PP.apply_volume(audio_float_to_int16(got["audio"][b, : y.size]), VOLUMES[b])
        assert got["pcm"][b, : y.size].tobytes() == want.tobytes(), b
        native.append(y)
        moved += int(y.size != n)
    assert moved >= 3 and got["audio"].shape[-1] == max(y.size for y in native)
    eng.set_output_rate(rate)
    try:
        shaped = run(eng, a, pitch=p, **kw)
        al = eng.fetch_alignment()
    finally:
        eng.set_output_rate(0)
    for b, y in enumerate(native):
        solo, sl, sp = hooks.test_resample(np.ascontiguousarray(y[None, :]), [y.size], eng.config.sample_rate, rate)
        no = int(shaped["lengths"][b])
        assert int(sl[0]) == no and solo[0, :no].tobytes() == shaped["audio"][b, :no].tobytes() and sp[0].tobytes() == shaped["peaks"][b].tobytes(), b
    check_spans_tile(al, a, shaped["lengths"])
    pk = eng.run_packed(a["ids"], a["lens"], SCALES, a["sid"], seed=SEED, utterance_keys=KEYS[:B], wav=True, pitch=p, **kw)
    assert bytes(pk.wav[:4]) == b"RIFF" and pk.lengths.tolist() == [y.size for y in native]
    for b, y in enumerate(native):
        assert pk.rows[b].tobytes() == got["pcm"][b, : y.size].tobytes(), b
    return got


def check_spans_tile(al, a, lengths):
    for b in range(len(lengths)):
        L = int(a["lens"][b])
        st, sm = al.start[b].astype(np.int64), al.samples[b].astype(np.int64)
        assert L == 0 or st[0] == 0
        assert np.array_equal(st[1:L], (st + sm)[: max(L - 1, 0)]) and (sm >= 0).all()
        if al.frames[b, :L].sum() > 0:
            assert int(sm[:L].sum()) == int(lengths[b]), b


def check_rows_alone_alignment_and_replay(make, a, p):
    """Without forced_durations (the stretched, timed run): a row of the ragged batch is bitwise the row alone; a poisoned workspace
    changes nothing; the alignment's spans tile the rows; the reported frames fed back as forced_durations give the same bytes."""
    eng = make()
    batched = run(eng, a, pitch=p)
    al = eng.fetch_alignment()
    check_spans_tile(al, a, batched["lengths"])
    frames = al.frames.astype(np.int32)
    for b in range(a["ids"].shape[0]):
        one = run(eng, a, rows=slice(b, b + 1), pitch=p[b:b + 1])
        n = int(batched["lengths"][b])
        assert int(one["lengths"][0]) == n
        assert PR.same_bits(one["audio"][0, :n], batched["audio"][b, :n]) and one["pcm"][0, :n].tobytes() == batched["pcm"][b, :n].tobytes()
        assert one["peaks"].tobytes() == batched["peaks"][b:b + 1].tobytes()
    same_run(run(eng, a, pitch=p, forced_durations=frames), batched)
    for pattern in (0x7FC00000, 0xFFFFFFFF):
        eng.fill_workspace(pattern)
        same_run(run(eng, a, pitch=p), batched)
    eng.close()


def check_duration_kept(eng, a):
    """A constant ratio keeps the duration: every phoneme is synthesized ceil(w p) frames long and played back p times faster, so a
    row ends within hop (#phonemes + 1) samples of the plain run's."""
    hop = eng.config.hop_length
    plain = run(eng, a)
    for c in (1.25, 0.8, float(SEMITONE2)):
        out = run(eng, a, pitch=np.full(a["ids"].shape, c, np.float32))
        d = np.abs(out["lengths"].astype(np.int64) - plain["lengths"].astype(np.int64))
        print("ratio %.4f: lengths %s against %s" % (c, out["lengths"].tolist(), plain["lengths"].tolist()))
        assert (d <= hop * (a["lens"] + 1)).all(), (c, d)
        assert out["audio"].tobytes() != plain["audio"].tobytes()


def check_downstream(eng, a, p):
    """After a pitch run that keeps its audio on the device: the packed entries are the int16 rows, the alignment's largest phoneme
    peak is the row peak, the loudness is the yardstick's of the warped audio."""
    from tests.test_loudness import check_measurement, reference_of

    B = a["ids"].shape[0]
    kw = dict(seed=SEED, utterance_keys=KEYS[:B], pitch=p, forced_durations=np.full(a["ids"].shape, 40, np.int32))
    eng.run(a["ids"], a["lens"], SCALES, a["sid"], want_float=False, device_only=True, **kw)
    pk = eng.fetch_packed()
    al = eng.fetch_alignment(levels=True)
    ld = eng.fetch_loudness()
    out = eng.fetch(want_float=True, want_pcm16=True)
    same_run(out, run(eng, a, **{k: v for k, v in kw.items() if k not in ("seed", "utterance_keys")}))
    for b, n in enumerate(int(n) for n in out["lengths"]):
        assert pk.rows[b].tobytes() == out["pcm"][b, :n].tobytes(), b
        assert al.peak[b].max().tobytes() == out["peaks"][b].tobytes(), b
    check_measurement(ld, reference_of(out, eng.config.sample_rate), eng.config.sample_rate)


def check_errors(eng, a):
    """Every refusal names what is wrong, comes before anything is launched and leaves the previous run served."""
    B, Tx = a["ids"].shape
    p = pitch_inputs(a)
    kept = run(eng, a)
    served = lambda: same_run({**eng.fetch(want_float=True, want_pcm16=True)}, kept)  # noqa: E731

    def refused(match, **kw):
        with pytest.raises(NativeError, match=match) as err:
            run(eng, a, **kw)
        assert err.value.code == -1
        served()

    for v in (np.nan, 0.49, np.inf, -np.inf, 2.01, -1.0, 0.0):
        bad = p.copy()
        bad[2, 4] = v
        refused("row 2, phoneme 4: pitch ratio must be finite and within 0.5 .. 2", pitch=bad)
    stretch = np.ones((B, Tx), np.float32)
    stretch[1, 0] = 2.0 ** 20
    bad = np.ones((B, Tx), np.float32)
    bad[1, 0] = 1.5
    refused(r"row 1, phoneme 0: stretch times pitch ratio is above 2\^20", pitch=bad, stretch=stretch)
    target = np.zeros(B, np.int32)
    target[3] = 200
    bad = np.ones((B, Tx), np.float32)
    bad[3, 5] = 1.25
    refused("row 3: a fitted length and a pitch ratio exclude each other", pitch=bad, target_frames=target)
    bad[3, 5], bad[0, 5] = 1.0, 1.25  # another row's ratio: the fitted row is all ones
    assert int(run(eng, a, pitch=bad, target_frames=target)["lengths"][3]) == 200 * eng.config.hop_length
    kept = run(eng, a)
    pa = PitchArgs()
    pa.reserved[6] = 1
    with pytest.raises(NativeError, match="pitch: reserved fields must be 0"):
        run_pitch_raw(eng, a, pa)
    served()
    for kw in (dict(pitch=p[:, :-1]), dict(pitch=p[:-1])):
        with pytest.raises(ValueError):
            run(eng, a, **kw)
        served()


def check_session(sess, eng, cfg):
    """pitch / pitch_semitones give the bytes of the _native call with the converted array; straight to a lane."""
    a = feed(cfg, lens=LENS[:3])
    fd = {"input": a["ids"], "input_lengths": a["lens"], "scales": SCALES}
    st = [[0.0, 2.0, -3.0, 12.0, -12.0], [7.0], []]
    g = np.ones(a["ids"].shape, np.float32)
    g[0, :5] = np.float32(2.0 ** (np.array(st[0]) / 12.0))
    g[1, 0] = np.float32(2.0 ** (7.0 / 12.0))
    batches = []
    sess._batcher.submit, submit = (lambda *x, **k: batches.append(1) or submit(*x, **k)), sess._batcher.submit
    rows, lengths = sess.run_pcm16(fd, utterance_keys=KEYS[:3], pitch_semitones=st)
    assert not batches
    want = eng.run(a["ids"], a["lens"], SCALES, None, seed=SEED, utterance_keys=KEYS[:3], want_pcm16=True, pitch=g)
    plain = eng.run(a["ids"], a["lens"], SCALES, None, seed=SEED, utterance_keys=KEYS[:3], want_pcm16=True)
    assert want["pcm"].tobytes() != plain["pcm"].tobytes()
    for b in range(3):
        n = int(want["lengths"][b])
        assert int(lengths[b]) == n and rows[b].tobytes() == want["pcm"][b, :n].tobytes()
    rows2, _ = sess.run_pcm16(fd, utterance_keys=KEYS[:3], pitch=[g[0, :5], g[1, :1], []])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(rows, rows2))
    pk = sess.run_packed(fd, utterance_keys=KEYS[:3], pitch_semitones=st, order=[2, 0])
    assert pk.rows[0].tobytes() == rows[2].tobytes() and pk.rows[1].tobytes() == rows[0].tobytes()
    with pytest.raises(ValueError, match="exclude each other"):
        sess.run_pcm16(fd, pitch=g, pitch_semitones=st)
    with pytest.raises(ValueError, match="one entry per row"):
        sess.run_pcm16(fd, pitch_semitones=st[:2])
    with pytest.raises(ValueError, match="finite"):
        sess.run_packed(fd, pitch=[[np.nan], [], []])


@pytest.fixture(scope="module")
def engines(emu_lib):
    made = {}

    def get(kind):
        if kind not in made:
            cfg, blob = voice(kind)
            made[kind] = (cfg, blob, Engine(blob, library=emu_lib))
        return made[kind]

    yield get
    for _, _, e in made.values():
        e.close()


@pytest.mark.parametrize("kind", ["sdp", "det", "ms"])
def test_identity_and_rule(emu_lib, engines, kind):
    cfg, blob, eng = engines(kind)
    a = feed(cfg)
    check_identity(eng, a)
    check_rule(eng, emu_lib, a, pitch_inputs(a))


def test_rows_alone_alignment_and_replay(emu_lib, engines):
    cfg, blob, eng = engines("sdp")
    a = feed(cfg)
    check_rows_alone_alignment_and_replay(lambda: Engine(blob, library=emu_lib), a, pitch_inputs(a))


def test_duration_kept_and_downstream_forms(engines):
    cfg, blob, eng = engines("sdp")
    a = feed(cfg)
    check_duration_kept(eng, a)
    check_downstream(eng, a, pitch_inputs(a))


def test_errors(engines):
    cfg, blob, eng = engines("sdp")
    check_errors(eng, feed(cfg))


def test_session_keywords(emu_lib, engines):
    cfg, blob, eng = engines("sdp")
    so = SessionOptions()
    so.seed = SEED
    so.micro_batch_window_ms = 200.0
    sess = InferenceSession(blob, sess_options=so, _library=emu_lib)
    check_session(sess, eng, cfg)
