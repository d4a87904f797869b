"""Level control in one run (mi355vits_run_levels, k_levels) on the CPU model of the kernels; test_gpu_levels.py runs the same
checks on the MI355X.

The yardstick is tests/levels_ref.py: the rule of include/mi355vits.h in int64 and numpy floats.  Every comparison is bit for bit
(levels_ref.same_bits: a NaN equals a NaN, whose sign and payload IEEE leaves to the platform); the rule has no tolerance."""
import ctypes

import numpy as np
import pytest

from mimic3_amd import postprocess as PP
from mimic3_amd._native import Engine, LevelArgs, NativeError, Result, WANT_FLOAT, WANT_PCM16
from mimic3_amd.session import InferenceSession, SessionOptions
from tests import levels_ref as LR
from tests.test_timing import KEYS, LENS, SCALES, SEED, calls, feed, run, same_run, voice
from tests.util import audio_float_to_int16

POISON = np.float32(-7.5e29)
RAMPS = (0, 1, 255, 4096)
GAINS = np.array([0.0, -0.0, 1.0, 1024.0, 1.0 + 2.0 ** -23, 2.0 ** -21, 3 * 2.0 ** -21, 0.5, 2.0, 0.25, 3.7, 1.0, 1.0], np.float32)


# ------------------------------------------------------------------------------------------ the kernel alone
def row(frames, gain=None, R=0):
    return dict(frames=np.asarray(frames, np.int64).reshape(-1), gain=gain, R=int(R))


def partition(rng, n, parts, planted=()):
    """Frames of `parts` + len(planted) phonemes that sum to n, with boundaries at the planted samples (hop = 1)."""
    cuts = set(int(p) for p in planted if 0 < p < n)
    while len(cuts) < min(parts + len(planted), n) - 1:
        cuts.add(int(rng.integers(1, n)))
    edges = np.array([0] + sorted(cuts) + [n], np.int64)
    return np.diff(edges)


def plant(x, b, rng):
    """-0.0 and a NaN in every row, +-Inf in the odd ones (an even row's peak stays finite)."""
    if x.size >= 16:
        p = rng.permutation(x.size)[:4]
        x[p[0]], x[p[1]] = -0.0, np.nan
        if b % 2:
            x[p[2]], x[p[3]] = np.inf, -np.inf
    return x


def first_difference(got, want):
    d = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))
    return d[:4].tolist(), got[d[:4]].tolist(), want[d[:4]].tolist()


def run_kernel(lib, rows, hop, seed, alone=None):
    """The hook on a batch of rows and on each row alone (or those of `alone`): valid samples bitwise the yardstick's, the floats
    behind every row and behind the last one still poison, peaks bitwise max |y|.  -> [(x, y, peak)] per row"""
    rng = np.random.default_rng(seed)
    B, T = len(rows), max(1, max(len(r["frames"]) for r in rows))
    cum, gain = np.full((B, T), -77, np.int32), np.full((B, T), np.nan, np.float32)  # behind a row: never read
    lens, ramp = np.array([len(r["frames"]) for r in rows], np.int32), np.array([r["R"] for r in rows], np.int32)
    for b, r in enumerate(rows):
        L = int(lens[b])
        cum[b, :L] = np.cumsum(r["frames"])
        gain[b, :L] = rng.choice(GAINS, L) if r["gain"] is None else np.asarray(r["gain"], np.float32)
    alen = np.array([LR.valid_samples(cum[b], int(lens[b]), hop) for b in range(B)], np.int32)
    bs = (int(alen.max()) + 6) | 1  # odd: the rows' bases take every alignment
    audio = np.full(B * bs + 37, POISON, np.float32)
    want, want_pk, out = audio.copy(), np.zeros(B, np.float32), []
    for b in range(B):
        n = int(alen[b])
        x = plant(rng.standard_normal(n).astype(np.float32), b, rng)
        y = LR.apply(x, LR.scale_cum(cum[b], int(lens[b]), gain[b], int(ramp[b]), hop))
        audio[b * bs: b * bs + n], want[b * bs: b * bs + n], want_pk[b] = x, y, LR.peak(y)
        assert b % 2 or n < 16 or (np.isnan(x).any() and np.isfinite(want_pk[b]))
        out.append((x, y, want_pk[b]))
    got, pk = lib.test_levels(cum, lens, gain, ramp, hop, audio, bs, alen)
    assert LR.same_bits(got, want), first_difference(got, want)
    assert pk.tobytes() == want_pk.tobytes(), (pk, want_pk)
    for b in (range(B) if alone is None else alone):
        if B == 1:
            break
        one = np.concatenate([audio[b * bs: (b + 1) * bs], np.full(9, POISON, np.float32)])
        got1, pk1 = lib.test_levels(cum[b:b + 1], lens[b:b + 1], gain[b:b + 1], ramp[b:b + 1], hop, one, bs, alen[b:b + 1])
        want1 = np.concatenate([want[b * bs: (b + 1) * bs], np.full(9, POISON, np.float32)])
        assert LR.same_bits(got1, want1), (b, first_difference(got1, want1))
        assert pk1.tobytes() == want_pk[b:b + 1].tobytes(), b
    return out


def check_tile_edges(lib, R):
    """hop = 1: rows of 4,095 .. 8,193 samples with phoneme boundaries on a tile edge and one sample either side of it; hop = 256:
    rows of 16 and 32 frames, a boundary exactly on the edge."""
    rng = np.random.default_rng(R)
    rows = [row(partition(rng, n, 9, (4095, 4096, 4097, 8191, 8192)), R=R) for n in (4095, 4096, 4097, 8192, 8193)]
    run_kernel(lib, rows, 1, 10 + R)
    rows = [row([3, 5, 8], R=R), row([16, 16], R=R), row([7, 9, 1, 15], R=R), row([16], R=R), row([1, 15, 15, 1], R=R)]
    run_kernel(lib, rows, 256, 20 + R)


def check_ramps(lib):
    """R larger than the row (1 frame at hop 256, R = 4096: the edge values carry the window), phonemes shorter than 2 R + 1, a ramp
    per row."""
    rows = [row([1], [2.0], 4096), row([0, 1, 0], [1024.0, 0.5, 1024.0], 4096), row([1, 1], [0.0, 2.0], 4096), row([1, 2, 1, 3, 1], R=255),
            row([2] * 9, R=1), row([1] * 40, R=300)]
    out = run_kernel(lib, rows, 256, 31)
    assert LR.same_bits(out[0][1], LR.apply(out[0][0], np.float32(2.0)))  # one phoneme: its gain everywhere, whatever R


def check_zero_frame_phonemes(lib, R):
    """Runs of zero-frame phonemes at the start, in the middle and at the end own no sample: with gains of 1024 they change nothing —
    the row is bitwise the row without them."""
    frames = np.array([0, 0, 2, 0, 0, 0, 3, 1, 0, 0])
    gain = np.where(frames == 0, 1024.0, [9, 9, 0.5, 9, 9, 9, 2.0, 0.0, 9, 9]).astype(np.float32)
    full = run_kernel(lib, [row(frames, gain, R)], 256, 40 + R)
    keep = frames > 0
    bare = run_kernel(lib, [row(frames[keep], gain[keep], R)], 256, 40 + R)  # the same seed: the same samples
    assert full[0][0].tobytes() == bare[0][0].tobytes() and LR.same_bits(full[0][1], bare[0][1]) and full[0][2] == bare[0][2]


def check_degenerate_rows(lib):
    """A row whose frames are all 0 and a row of len 0 have one frame of audio and keep it bit for bit; len 1; an empty row inside a
    batch of 5."""
    for hop in (256, 8, 1):
        rows = [row([2, 0, 3], R=5), row([], R=0), row([1, 4], R=4096), row([0, 0, 0, 0], [0.0, 0.0, 0.0, 0.0], 17), row([3], R=100)]
        out = run_kernel(lib, rows, hop, 50 + hop)
        for b in (1, 3):
            assert out[b][0].size == hop and LR.same_bits(out[b][1], out[b][0]) and out[b][2] == LR.peak(out[b][0])


def check_dense_boundaries(lib):
    """hop = 1, every frame 1, Tx = 13,000, R = 4096: a tile's reach holds more than 12,288 non-empty phonemes; hop = 3, Tx = 300."""
    run_kernel(lib, [row(np.ones(13000, np.int64), R=4096)], 1, 60)
    run_kernel(lib, [row(np.ones(300, np.int64), R=4096), row(np.ones(300, np.int64), R=7), row(np.arange(300) % 3, R=2)], 3, 61)
    run_kernel(lib, [row(np.ones(5000, np.int64), R=0), row(np.arange(2400) % 2, R=1)], 1, 62)  # just past one table; runs of zeros in it


def check_special_gains(lib):
    g = np.array([0.0, -0.0, 1.0, 1024.0, 1.0 + 2.0 ** -23, 2.0 ** -21, 3 * 2.0 ** -21], np.float32)
    assert LR.q_of(g).tolist() == [0, 0, 1 << 20, 1 << 30, 1 << 20, 0, 2]  # the two ties go to even
    out = run_kernel(lib, [row([2] * 7, g, 0), row([2] * 7, g, 100), row([2] * 7, g[::-1], 4096)], 256, 70)
    x, y, _ = out[0]
    assert not y[:1024][~np.isnan(y[:1024])].any()  # a mute
    assert LR.same_bits(y[1024:1536], x[1024:1536])  # gain 1 between steps: the samples keep their bits


def check_unity(lib):
    """All gains 1 with any R: the audio keeps its bits and the peak is the input's."""
    rng = np.random.default_rng(80)
    rows = [row(rng.integers(0, 13, 40), np.ones(40), R) for R in RAMPS] + [row(partition(rng, 8193, 30), np.ones(30), 255)]
    for hop, rr in ((256, rows[:4]), (1, rows[4:] + [row([0, 0], [1.0, 1.0], 9)])):
        for x, y, pk in run_kernel(lib, rr, hop, 81 + hop):
            assert LR.same_bits(y, x) and pk == LR.peak(x)


def released_shape_rows(seed=90):
    """64 rows, hop 256, Tx 128, frames 0 .. 12, gains in [0, 4] on a third of the phonemes, a random R per row."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(64):
        L = int(rng.integers(1, 129))
        g = np.where(rng.random(L) < 1 / 3, rng.uniform(0, 4, L), 1.0).astype(np.float32)
        rows.append(row(rng.integers(0, 13, L), g, int(rng.integers(0, 4097))))
    return rows


@pytest.mark.parametrize("R", RAMPS)
def test_kernel_tile_edges(emu_lib, R):
    check_tile_edges(emu_lib, R)


def test_kernel_ramps_and_short_phonemes(emu_lib):
    check_ramps(emu_lib)


@pytest.mark.parametrize("R", (0, 300))
def test_kernel_zero_frame_phonemes(emu_lib, R):
    check_zero_frame_phonemes(emu_lib, R)


def test_kernel_degenerate_rows(emu_lib):
    check_degenerate_rows(emu_lib)


def test_kernel_dense_boundaries(emu_lib):
    check_dense_boundaries(emu_lib)


def test_kernel_special_gains_and_unity(emu_lib):
    check_special_gains(emu_lib)
    check_unity(emu_lib)


def test_the_yardstick_on_a_row_worked_by_hand():
    """hop 2, frames 1, 0, 2, gains 1, 9, 3, R = 1: qs = 1 1 3 3 3 3 (x 2^20), edge values repeat: S = 3 5 7 9 9 9 over 3."""
    s = LR.scale([1, 0, 2], 3, np.array([1, 9, 3], np.float32), 1, 2)
    assert s.tobytes() == (np.array([3, 5, 7, 9, 9, 9], np.float64) / 3).astype(np.float32).tobytes()
    assert LR.scale([0, 0], 2, np.array([5, 5], np.float32), 7, 4).tolist() == [1.0] * 4  # no frames: one frame of audio, ONE
    assert LR.peak(np.array([np.nan, -2.0, 1.0], np.float32)) == 2.0


# ------------------------------------------------------------------------------------------ through the C ABI
VOLUMES = np.array([100.0, 50.0, 100.0, 130.0, 100.0])


def level_inputs(a, seed=3):
    """A gain for every phoneme of the feed (a third of them moved, a mute and a +12 dB among them) and a ramp per row."""
    rng = np.random.default_rng(seed)
    B, Tx = a["ids"].shape
    g = np.where(rng.random((B, Tx)) < 1 / 3, rng.uniform(0, 4, (B, Tx)), 1.0).astype(np.float32)
    g[0, 3], g[0, 4], g[3, 7] = 0.0, 3.98, 1024.0
    g[np.arange(Tx)[None, :] >= a["lens"][:, None]] = np.nan  # behind a row: never looked at
    return g, np.array([0, 3, 40, 4096, 11][:B], np.int32)


def run_levels_raw(eng, a, levels):
    """mi355vits_run_levels itself with `levels` = None (NULL) or a LevelArgs."""
    args, rows, per_row, keep = eng._args(a["ids"], a["lens"], SCALES, a["sid"], SEED, 0, None, None, None, 1.0, KEYS)
    args.flags = WANT_FLOAT | WANT_PCM16
    r = Result()
    rc = eng.native.lib.mi355vits_run_levels(eng._h, ctypes.byref(args), ctypes.byref(rows) if per_row else None, None, None,
                                             None if levels is None else ctypes.byref(levels), ctypes.byref(r))
    if rc != 0:
        eng._check(rc)
    out = eng._take(r)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def check_identity(eng, a):
    """NULL levels, a struct without a gain and all-ones gains (with and without ramps) are bitwise the plain run; only the last two
    launch `levels`."""
    B, Tx = a["ids"].shape
    eng.profile_enable(True)
    eng.profile_reset()
    plain = run(eng, a)
    want_calls = calls(eng)
    assert "levels" not in want_calls
    for lv in (None, LevelArgs()):
        eng.profile_reset()
        same_run(run_levels_raw(eng, a, lv), plain)
        assert calls(eng) == want_calls
    for ramp in (None, 0, [0, 5, 4096, 1, 77][:B]):
        eng.profile_reset()
        same_run(run(eng, a, gain=np.ones((B, Tx), np.float32), ramp_samples=ramp), plain)
        got = calls(eng)
        assert got.pop("levels") == 1 and got == want_calls
    eng.profile_enable(False)
    return plain


def check_rule(eng, a, g, ramp, **kw):
    """Valid samples = plain audio x the yardstick's scale of the run's own frames; peaks = max |y|; the int16 = the int16
    yardstick on the shaped float audio, volumes included; lengths are the plain run's."""
    hop = eng.config.hop_length
    kw = dict(kw, pcm_volume=VOLUMES[: len(ramp)] / 100.0)
    plain = run(eng, a, **kw)
    shaped = run(eng, a, gain=g, ramp_samples=ramp, **kw)
    frames = eng.fetch_alignment().frames
    assert shaped["lengths"].tobytes() == plain["lengths"].tobytes()
    moved = 0
    for b, n in enumerate(int(n) for n in shaped["lengths"]):
        y = LR.apply(plain["audio"][b, :n], LR.scale(frames[b], int(a["lens"][b]), g[b], int(ramp[b]), hop))
        assert LR.same_bits(shaped["audio"][b, :n], y), (b, first_difference(shaped["audio"][b, :n], y))
        assert shaped["audio"][b, n:].tobytes() == plain["audio"][b, n:].tobytes()  # behind the row: what the plain run leaves there
        assert shaped["peaks"][b].tobytes() == LR.peak(y).tobytes(), b
        want = PP.apply_volume(audio_float_to_int16(shaped["audio"][b, :n]), VOLUMES[b])
        assert shaped["pcm"][b, :n].tobytes() == want.tobytes(), b
        moved += int((y != plain["audio"][b, :n]).sum())
    assert moved > 100
    return plain, shaped, frames


def check_rows_alone_and_poison(make, a, g, ramp):
    """A row of the batch is bitwise the row alone; a poisoned workspace changes nothing on the ragged batch."""
    eng = make()
    batched = run(eng, a, gain=g, ramp_samples=ramp)
    for b in range(len(ramp)):
        one = run(eng, a, rows=slice(b, b + 1), gain=g[b:b + 1], ramp_samples=ramp[b:b + 1])
        n = int(batched["lengths"][b])
        assert int(one["lengths"][0]) == n
        assert LR.same_bits(one["audio"][0, :n], batched["audio"][b, :n]) and one["pcm"][0, :n].tobytes() == batched["pcm"][b, :n].tobytes()
        assert one["peaks"].tobytes() == batched["peaks"][b:b + 1].tobytes()
    for pattern in (0x7FC00000, 0xFFFFFFFF):
        eng.fill_workspace(pattern)
        same_run(run(eng, a, gain=g, ramp_samples=ramp), batched)
    eng.close()


def check_combinations(eng, a, g, ramp, multispeaker):
    """The rule on the frames of a fitted run, of forced durations and (a multi-speaker voice) under a speakers mix."""
    B, Tx = a["ids"].shape
    natural = run(eng, a)
    target = (natural["lengths"] // eng.config.hop_length * 13 // 10 + 1).astype(np.int32)
    _, shaped, frames = check_rule(eng, a, g, ramp, target_frames=target)
    assert np.array_equal(frames.sum(axis=1), target)
    forced = np.random.default_rng(4).integers(0, 7, (B, Tx)).astype(np.int32)
    forced[2, : int(a["lens"][2])] = 0  # a row of no frames: one frame of audio, untouched
    _, shaped, frames = check_rule(eng, a, g, ramp, forced_durations=forced)
    assert np.array_equal(frames, np.where(np.arange(Tx)[None, :] < a["lens"][:, None], forced, 0))
    if multispeaker:
        check_rule(eng, a, g, ramp, speakers=[{0: 0.5, 1: 0.5}, 1, {2: 1.25, 0: -0.25}, 0, 2][:B])


def check_output_rate(eng, hooks, a, g, ramp, rate=16000):
    """At another output rate: the lengths of the plain run, and the resampler's result of the shaped native waveform."""
    native = run(eng, a, gain=g, ramp_samples=ramp)
    eng.set_output_rate(rate)
    plain = run(eng, a)
    shaped = run(eng, a, gain=g, ramp_samples=ramp)
    eng.set_output_rate(0)
    assert shaped["lengths"].tobytes() == plain["lengths"].tobytes() and shaped["audio"].tobytes() != plain["audio"].tobytes()
    for b, n in enumerate(int(n) for n in native["lengths"]):
        r = native["audio"][b, :n]
        solo, sl, sp = hooks.test_resample(np.ascontiguousarray(r[None, :]), [n], eng.config.sample_rate, rate)
        no = int(shaped["lengths"][b])
        assert int(sl[0]) == no and solo[0, :no].tobytes() == shaped["audio"][b, :no].tobytes() and sp[0].tobytes() == shaped["peaks"][b].tobytes(), b


def check_downstream(eng, a, g, ramp):
    """After a levels run that keeps its audio on the device: the packed entries are the padded int16 rows, the alignment's largest
    phoneme peak is the row peak, the loudness is the yardstick's of the shaped audio."""
    from tests.test_loudness import check_measurement, reference_of

    kw = dict(seed=SEED, utterance_keys=KEYS[: len(ramp)], gain=g, ramp_samples=ramp, forced_durations=np.full(a["ids"].shape, 40, np.int32))
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
    g, ramp = level_inputs(a)
    kept = run(eng, a)
    served = lambda: same_run({**eng.fetch(want_float=True, want_pcm16=True)}, kept)  # noqa: E731

    def refused(match, **kw):
        with pytest.raises(NativeError, match=match) as err:
            run(eng, a, **kw)
        assert err.value.code == -1
        served()

    for v in (np.nan, -0.5, np.inf, -np.inf, 1024.5):
        bad = g.copy()
        bad[2, 4] = v
        refused("row 2, phoneme 4: gain must be finite and within 0 .. 1024", gain=bad, ramp_samples=ramp)
    for v in (-1, 4097):
        bad = ramp.copy()
        bad[3] = v
        refused("row 3: ramp_samples must be within 0 .. 4096", gain=g, ramp_samples=bad)
    lv = LevelArgs()
    lv.reserved[2] = 1
    with pytest.raises(NativeError, match="levels: reserved fields must be 0"):
        run_levels_raw(eng, a, lv)
    served()
    for kw in (dict(gain=g[:, :-1]), dict(gain=g[:-1]), dict(gain=g, ramp_samples=ramp[:-1]), dict(gain=g, ramp_samples=np.ones(B, np.float32)),
               dict(ramp_samples=ramp)):
        with pytest.raises(ValueError):
            run(eng, a, **kw)
        served()


def check_session(sess, eng, cfg):
    """gain_db / ramp_ms give the bytes of the _native call with the converted arrays; -inf dB mutes; straight to a lane."""
    a = feed(cfg, lens=LENS[:3])
    fd = {"input": a["ids"], "input_lengths": a["lens"], "scales": SCALES}
    db = [[0.0, -6.0, -np.inf, 6.0, 12.0], [3.0], [0.0] * 17]
    g = np.ones(a["ids"].shape, np.float32)
    g[0, :5] = np.float32(10.0 ** (np.array(db[0]) / 20.0))
    g[1, 0] = np.float32(10.0 ** (3.0 / 20.0))
    R = int(round(0.1 / 1000 * cfg.sample_rate))
    batches = []
    sess._batcher.submit, submit = (lambda *x, **k: batches.append(1) or submit(*x, **k)), sess._batcher.submit
    rows, lengths = sess.run_pcm16(fd, utterance_keys=KEYS[:3], gain_db=db, ramp_ms=0.1)
    assert not batches
    want = eng.run(a["ids"], a["lens"], SCALES, None, seed=SEED, utterance_keys=KEYS[:3], want_pcm16=True, gain=g, ramp_samples=R)
    al = eng.fetch_alignment()
    for b in range(3):
        n = int(want["lengths"][b])
        assert int(lengths[b]) == n and rows[b].tobytes() == want["pcm"][b, :n].tobytes()
    mute = LR.scale(al.frames[0], int(a["lens"][0]), g[0], R, cfg.hop_length) == 0
    assert R == 2 and mute.any() and not rows[0][mute].any() and rows[0][~mute].any()  # the muted phoneme
    pk = sess.run_packed(fd, utterance_keys=KEYS[:3], gain_db=np.float64(20.0) * np.log10(np.maximum(g, 1e-30)), ramp_ms=[0.1, 0, 0.1], order=[2, 0])
    assert pk.rows[0].tobytes() == rows[2].tobytes() and pk.rows[1].size == rows[0].size
    with pytest.raises(ValueError, match="needs gain_db"):
        sess.run_pcm16(fd, ramp_ms=2.0)
    with pytest.raises(ValueError, match="one entry per row"):
        sess.run_pcm16(fd, gain_db=db[:2])
    with pytest.raises(ValueError, match="-inf"):
        sess.run_pcm16(fd, gain_db=[[np.inf], [], []])


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
def test_identity_rule_and_rows_alone(emu_lib, engines, kind):
    cfg, blob, eng = engines(kind)
    a = feed(cfg)
    g, ramp = level_inputs(a)
    check_identity(eng, a)
    check_rule(eng, a, g, ramp)
    if kind != "det":
        check_rows_alone_and_poison(lambda: Engine(blob, library=emu_lib), a, g, ramp)


@pytest.mark.parametrize("kind", ["sdp", "ms"])
def test_levels_with_timing_forced_durations_and_speakers(engines, kind):
    cfg, blob, eng = engines(kind)
    a = feed(cfg)
    check_combinations(eng, a, *level_inputs(a), multispeaker=kind == "ms")


def test_output_rate_and_downstream_forms(emu_lib, engines):
    cfg, blob, eng = engines("sdp")
    a = feed(cfg)
    g, ramp = level_inputs(a)
    check_output_rate(eng, emu_lib, a, g, ramp)
    check_downstream(eng, a, g, ramp)


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
    sess.close()
