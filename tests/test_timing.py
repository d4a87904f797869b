"""Timing control in one run (mi355vits_run_timed, k_durations_timed) on the CPU model of the kernels; test_gpu_timing.py runs the
same checks on the MI355X.

The yardstick is tests/timing_ref.py: the rule of include/mi355vits.h in np.float32 products and Python integers, applied to the u[t]
the run itself reports (the dur_float tap: the device's expf is not numpy's).  Everything is compared bit for bit: the rule has no
tolerance."""
import ctypes

import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError, Result, TimingArgs, WANT_FLOAT, WANT_PCM16
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, SessionOptions
from tests import timing_ref as TR
from tests.detdp_util import det_config

CAP = TR.CAP
FIT_T = (1, 2, 63, 64, 65, 255, 256, 257, 600, 4100)
TARGET_KINDS = ("none", "floor", "floor-1", "floor+1", "F1", "F1-1", "F1+1", "3F1", "cap")
MIN_KINDS = ("zeros", "one_large", "sum_is_target", "sum_above_target")
SCALES = np.array([0.667, 1.0, 0.8], np.float32)
LENS = np.array([40, 1, 17, 33, 8], np.int64)  # B = 5 ragged, Tx = 40
KEYS = [7, 1_000_003, 42, (1 << 40) + 5, 3]
SEED = 11


# ------------------------------------------------------------------------------------------ the fit stage alone
def _planted_u(rng, T, big):
    """u log-uniform over [2^-6, 2^6] with planted exact integers, integers +- 1 ulp, zeros, a run of equal values (they step at
    the same s': the index order decides) and, with `big`, one value >= CAP."""
    u = np.exp2(rng.uniform(-6.0, 6.0, T)).astype(np.float32)
    at = rng.permutation(T)
    plant = [np.float32(3.0), np.float32(1.0), np.nextafter(np.float32(5.0), np.float32(9.0)), np.nextafter(np.float32(5.0), np.float32(0.0)),
             np.nextafter(np.float32(2.0), np.float32(0.0)), np.float32(0.0), np.float32(0.0)] + [np.float32(1.7)] * 5
    for i, v in zip(at, plant):
        u[i] = v
    if big and T > len(plant):
        u[at[len(plant)]] = np.float32(CAP) * np.float32(1.5)
    return u


def fit_case(T, seed=0):
    """One batch of rows of T phonemes: every target kind x every min_frames kind, ragged lengths with 0 and T among them, a row of
    zeros with a target (status 2).  -> u, lens, min_frames, target"""
    rng = np.random.default_rng(1000 * seed + T)
    rows = []
    for ti, tk in enumerate(TARGET_KINDS):
        for mi, mk in enumerate(MIN_KINDS):
            big = (ti + mi) % 4 == 3 and tk in ("none", "floor", "floor+1", "floor-1", "cap")
            L = T if (ti + mi) % 3 == 0 else int(rng.integers(1, T + 1))
            u = _planted_u(rng, T, big)
            mn = np.zeros(T, np.int64)
            if mk == "one_large":
                mn[int(rng.integers(0, L))] = 500
            fl, f1 = TR.floor_of(u, L, mn), TR.natural(u, L, mn)
            N = {"none": 0, "floor": fl, "floor-1": fl - 1, "floor+1": fl + 1, "F1": f1, "F1-1": f1 - 1, "F1+1": f1 + 1, "3F1": 3 * f1, "cap": CAP}[tk]
            if not 1 <= N <= CAP:
                N = 0
            if mk in ("sum_is_target", "sum_above_target") and N:
                mn[:L] = N // L  # the minimum frames of the row sum to the target ...
                mn[: N % L] += 1
                if mk == "sum_above_target":
                    mn[L - 1] += 1  # ... or pass it by one: below the floor
            rows.append((u, L, mn, N))
    rows.append((np.zeros(T, np.float32), T, np.zeros(T, np.int64), 17))  # every u = 0: unreachable
    rows.append((_planted_u(rng, T, False), 0, np.zeros(T, np.int64), 5))  # an empty row with a target: unreachable
    rows.append((_planted_u(rng, T, False), 0, np.zeros(T, np.int64), 0))  # an empty row without
    u = np.stack([r[0] for r in rows])
    u[:, :] = np.where(np.arange(T)[None, :] < np.array([r[1] for r in rows])[:, None], u, np.float32(np.nan))  # behind a row: never read
    return (u, np.array([r[1] for r in rows], np.int32), np.stack([r[2] for r in rows]).astype(np.int32),
            np.array([r[3] for r in rows], np.int32))


def check_fit_stage(lib, T):
    u, lens, mn, target = fit_case(T)
    want = TR.fit(u, lens, mn, target)
    got = lib.test_fit_durations(u, lens, mn, target)
    for name, g, w in zip(("frames", "cum", "ylen", "factor", "status"), got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (T, name, np.argwhere(g != w)[:4].tolist())
    st = want[4]
    assert set(st.tolist()) == {0, 1, 2}  # the case holds every status
    ok = (st == 0) & (target > 0)
    assert ok.any() and np.array_equal(want[0][ok].sum(axis=1), target[ok])  # a fitted row sums to its target
    # the plain forms of the optional inputs: no min_frames, no target
    got0 = lib.test_fit_durations(u, lens, None, None)
    want0 = TR.fit(u, lens, None, None)
    for g, w in zip(got0, want0):
        assert g.tobytes() == w.tobytes()


def check_fit_is_k_durations(lib):
    """Without a target and with min_frames 0 the fit stage is k_durations' ceil, scan and row length: u = expf(0) * 1 * length_scale
    exactly, so both kernels see the same float."""
    rng = np.random.default_rng(5)
    B, T = 9, 300
    ls = np.exp2(rng.uniform(-3, 5, B)).astype(np.float32)
    ls[0], ls[1] = np.float32(4.0), np.float32(CAP) * 2
    lens = rng.integers(0, T + 1, B).astype(np.int32)
    lens[2], lens[3] = 0, T
    _, w_ceil, cum, ylen = lib.test_durations(np.zeros((B, 2, T), np.float32), lens, length_scale=ls)
    u = np.repeat(ls[:, None], T, axis=1)
    frames, cum2, ylen2, factor, status = lib.test_fit_durations(u, lens)
    assert frames.tobytes() == w_ceil.tobytes() and cum2.tobytes() == cum.tobytes() and ylen2.tobytes() == ylen.tobytes()
    assert (factor == 1.0).all() and not status.any()


def check_fit_stage_long(lib, T):
    """The longest row that keeps u and min_frames in LDS (16,384 phonemes) and the first that re-reads them from memory: a few rows
    of the same case."""
    u, lens, mn, target = (x[[0, 4, 13, 16, 21, 28, 9, 36]] for x in fit_case(T))
    want = TR.fit(u, lens, mn, target)
    got = lib.test_fit_durations(u, lens, mn, target)
    for name, g, w in zip(("frames", "cum", "ylen", "factor", "status"), got, want):
        assert g.tobytes() == w.tobytes(), (T, name, np.argwhere(g != w)[:4].tolist())
    assert (want[4] == 0).sum() >= 3 and (target[want[4] == 0] > 0).any()


@pytest.mark.parametrize("T", FIT_T)
def test_fit_stage_alone(emu_lib, T):
    check_fit_stage(emu_lib, T)


@pytest.mark.parametrize("T", [16384, 16385])
def test_fit_stage_alone_at_the_lds_limit(emu_lib, T):
    check_fit_stage_long(emu_lib, T)


def test_fit_stage_without_a_target_is_k_durations(emu_lib):
    check_fit_is_k_durations(emu_lib)


def test_the_yardstick_on_a_row_worked_by_hand():
    """u = 1.5, 1.5, 0.25: F(1) = 2 + 2 + 1 = 5.  Target 6: the largest s with F <= 6 is 4/3 rounded down in the sense that
    fl(1.5 s) <= 2 still holds (s* = the f32 just at or below 4/3 whose product rounds to <= 2); at the next float BOTH 1.5s step to 3,
    and the one missing frame goes to the first."""
    fr, s, st = TR.fit_row(np.array([1.5, 1.5, 0.25], np.float32), 3, None, 6)
    assert st == 0 and fr.tolist() == [3, 2, 1]
    assert np.float32(1.5) * s <= np.float32(2.0) < np.float32(1.5) * np.nextafter(s, np.float32(9))
    fr, s, st = TR.fit_row(np.array([1.5, 1.5, 0.25], np.float32), 3, None, 2)
    assert st == 1 and fr.tolist() == [1, 1, 1] and s == TR.S_MIN
    fr, s, st = TR.fit_row(np.array([0, 0, 0], np.float32), 3, np.array([1, 0, 0]), 2)
    assert st == 2 and fr.tolist() == [1, 0, 0]
    fr, s, st = TR.fit_row(np.array([1.5, 1.5, 0.25], np.float32), 2, None, 0)
    assert st == 0 and fr.tolist() == [2, 2, 0] and s == 1.0


# ------------------------------------------------------------------------------------------ through the engine
def voice(kind):
    cfg = {"sdp": VitsConfig.tiny, "det": lambda: det_config(VitsConfig.tiny(), 64), "ms": lambda: VitsConfig.tiny(n_speakers=3)}[kind]()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=31, frames_per_id=3.0))


def feed(cfg, lens=LENS, seed=2):
    rng = np.random.default_rng(seed)
    B, Tx = len(lens), int(max(lens))
    ids = rng.integers(1, cfg.num_symbols, (B, Tx)).astype(np.int64)
    for b, n in enumerate(lens):
        ids[b, int(n):] = 0
    sid = (np.arange(B) % cfg.n_speakers).astype(np.int64) if cfg.n_speakers > 1 else None
    return dict(ids=ids, lens=np.asarray(lens, np.int64), sid=sid)


def run(eng, a, rows=slice(None), **kw):
    sid = None if a["sid"] is None else a["sid"][rows]
    keys = KEYS[rows] if isinstance(rows, slice) else [KEYS[rows]]
    out = eng.run(a["ids"][rows], a["lens"][rows], SCALES, sid, seed=SEED, utterance_keys=keys, want_float=True, want_pcm16=True, **kw)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def same_run(x, y):
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert x[k].tobytes() == y[k].tobytes(), k


def run_timed_raw(eng, a, timing):
    """mi355vits_run_timed itself with `timing` = None (NULL) or a TimingArgs."""
    args, rows, per_row, keep = eng._args(a["ids"], a["lens"], SCALES, a["sid"], SEED, 0, None, None, None, 1.0, KEYS)
    args.flags = WANT_FLOAT | WANT_PCM16
    r = Result()
    rc = eng.native.lib.mi355vits_run_timed(eng._h, ctypes.byref(args), ctypes.byref(rows) if per_row else None,
                                            None if timing is None else ctypes.byref(timing), ctypes.byref(r))
    if rc != 0:
        eng._check(rc)
    out = eng._take(r)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def calls(eng):
    return {k: v["calls"] for k, v in eng.profile_report().items()}


def check_identity(eng, a):
    """run_timed with NULL timing, with a struct of NULL inputs, and with all-ones stretch / zero min_frames / no target are bitwise
    run_rows; the first two launch the same kernels the same number of times."""
    B, Tx = a["ids"].shape
    eng.profile_enable(True)
    eng.profile_reset()
    plain = run(eng, a)
    want_calls = calls(eng)
    assert "durations" in want_calls and "durations.timed" not in want_calls
    for timing in (None, TimingArgs()):
        eng.profile_reset()
        same_run(run_timed_raw(eng, a, timing), plain)
        assert calls(eng) == want_calls
    eng.profile_reset()
    ones = run(eng, a, stretch=np.ones((B, Tx), np.float32), min_frames=np.zeros((B, Tx), np.int32), target_frames=np.zeros(B, np.int32))
    same_run(ones, plain)
    got = calls(eng)
    assert got.pop("durations.timed") == 1 and got == {k: v for k, v in want_calls.items() if k != "durations"}
    assert ones["timing_factor"].tobytes() == np.ones(B, np.float32).tobytes()
    eng.profile_enable(False)
    return plain


def targets_for(eng, a):
    """Targets in frames for every row out of the row's own floor and natural length (the dur_float tap of an all-ones timed run)."""
    B, Tx = a["ids"].shape
    run(eng, a, stretch=np.ones((B, Tx), np.float32), debug_taps=True)
    u = eng.tap("dur_float")[:, 0, :]
    fl = [TR.floor_of(u[b], a["lens"][b]) for b in range(B)]
    f1 = [TR.natural(u[b], a["lens"][b]) for b in range(B)]
    t = [fl[0], f1[1] + 7, 2 * f1[2] + 1, max(fl[3], f1[3] - 3), 3 * f1[4]]
    return np.array(t[:B], np.int32), u


def check_fit(eng, a):
    """lengths = target * hop; the alignment's frames sum to the target and equal the yardstick applied to the dur_float tap of the
    same run; timing_factor is the yardstick's s* bit for bit.  Replay: those frames as forced_durations give bitwise the same audio."""
    B, Tx = a["ids"].shape
    target, u0 = targets_for(eng, a)
    out = run(eng, a, target_frames=target, debug_taps=True)
    u = eng.tap("dur_float")[:, 0, :]
    assert u.tobytes() == u0.tobytes()  # the targets do not move u
    assert "logw" in eng.taps() and "w_ceil" in eng.taps()
    al = eng.fetch_alignment()
    hop = eng.config.hop_length
    assert np.array_equal(out["lengths"], target.astype(np.int64) * hop)
    assert np.array_equal(al.frames.sum(axis=1), target)
    frames, _, ylen, factor, status = TR.fit(u, a["lens"], None, target)
    assert not status.any() and np.array_equal(ylen, target)
    assert al.frames.tobytes() == frames.tobytes()
    assert eng.tap("w_ceil")[:, 0, :].astype(np.int32).tobytes() == frames.tobytes()
    assert out["timing_factor"].tobytes() == factor.tobytes()
    assert len({float(f) for f in factor}) == B and not (factor == 1.0).all()
    replay = run(eng, a, forced_durations=frames)
    same_run(replay, out)
    return target, frames, out


def check_rows_alone(make, a, target, batched, rows):
    """Row b of the timed batch is bitwise the row alone (same Tx)."""
    for b in rows:
        eng = make()
        one = run(eng, a, rows=slice(b, b + 1), target_frames=target[b:b + 1])
        n = int(batched["lengths"][b])
        assert int(one["lengths"][0]) == n
        assert one["audio"][0, :n].tobytes() == batched["audio"][b, :n].tobytes() and one["pcm"][0, :n].tobytes() == batched["pcm"][b, :n].tobytes()
        assert one["peaks"].tobytes() == batched["peaks"][b:b + 1].tobytes() and one["timing_factor"].tobytes() == batched["timing_factor"][b:b + 1].tobytes()
        eng.close()


def check_output_forms(eng, a, target, frames):
    """run_packed(target_frames) is bitwise run_packed(forced_durations = the fitted frames), natively and at another output rate,
    where lengths = ceil(target * hop * L / M)."""
    from tests import resample_ref as R

    kw = dict(seed=SEED, utterance_keys=KEYS, order=[3, 0, 4, 1, 2][: len(target)], lead_samples=[5, 0, 9, 1, 2][: len(target)], wav=True)
    order = kw["order"]
    for rate in (0, 8000):
        eng.set_output_rate(rate)
        timed = eng.run_packed(a["ids"], a["lens"], SCALES, a["sid"], target_frames=target, **kw)
        assert eng.last_timing_factor is not None and eng.last_timing_factor.shape == (len(target),)
        forced = eng.run_packed(a["ids"], a["lens"], SCALES, a["sid"], forced_durations=frames, **kw)
        assert timed.data.tobytes() == forced.data.tobytes() and np.array_equal(timed.offsets, forced.offsets)
        assert np.asarray(timed.wav).tobytes() == np.asarray(forced.wav).tobytes()
        L, M = R.ratio(eng.config.sample_rate, rate) if rate else (1, 1)
        want = [-(-int(target[b]) * eng.config.hop_length * L // M) for b in order]
        assert [int(n) for n in timed.lengths] == want
    eng.set_output_rate(0)


def check_stretch_and_min(eng, a):
    B, Tx = a["ids"].shape
    ones = np.ones((B, Tx), np.float32)
    run(eng, a, stretch=ones, debug_taps=True)
    u0, f0 = eng.tap("dur_float")[:, 0, :], eng.fetch_alignment().frames
    st = ones.copy()
    st[0, 3:9] = 2.0
    st[2, 5] = 0.0  # a phoneme dropped
    st[3, 20:] = 0.37
    st[4, 8:] = np.nan  # behind the row: never looked at
    run(eng, a, stretch=st, debug_taps=True)
    u1, f1 = eng.tap("dur_float")[:, 0, :], eng.fetch_alignment().frames
    valid = np.arange(Tx)[None, :] < a["lens"][:, None]
    want_u = np.where(valid, u0 * np.where(valid, st, 1).astype(np.float32), 0).astype(np.float32)
    assert u1.tobytes() == want_u.tobytes()
    assert np.array_equal(f1, np.where(valid, TR.count(u1), 0))  # exactly c(fl(u * 2)) on the span
    same = st == 1.0
    assert np.array_equal(f1[same & valid], f0[same & valid]) and f1[2, 5] == 0
    assert (f1[0, 3:9] >= 2 * f0[0, 3:9] - 1).all() and (f1[0, 3:9] <= 2 * f0[0, 3:9]).all()  # roughly doubled: ceil(2u) is 2 ceil(u) or one less
    mn = np.zeros((B, Tx), np.int32)
    mn[0, 2], mn[3, 30] = 50, 1
    mn[1, 5] = 77  # behind the row
    out = run(eng, a, min_frames=mn)
    f2 = eng.fetch_alignment().frames
    assert f2[0, 2] == max(50, f0[0, 2]) >= 50 and f2[3, 30] == max(1, f0[3, 30])
    mask = np.ones((B, Tx), bool)
    mask[0, 2] = mask[3, 30] = False
    assert np.array_equal(f2[mask], f0[mask])
    assert np.array_equal(out["lengths"], f2.sum(axis=1).astype(np.int64) * eng.config.hop_length)


def check_errors(eng, a):
    """Every refusal names what is wrong.  What is refused before anything is launched leaves the previous run served; the two the
    device finds (below the floor, unreachable) come at the sizing synchronisation of a run under way and leave the handle as every run
    that fails there does (a predicted duration out of range): nothing served — never partial audio — until the next completed run."""
    B, Tx = a["ids"].shape
    ones = np.ones((B, Tx), np.float32)
    kept = run(eng, a)
    served = lambda: same_run({**eng.fetch(want_float=True, want_pcm16=True)}, kept)  # noqa: E731

    def refused(match, **kw):
        with pytest.raises(NativeError, match=match) as err:
            run(eng, a, **kw)
        assert err.value.code == -1
        served()

    bad = ones.copy()
    bad[2, 4] = np.nan
    refused("row 2, phoneme 4: stretch must be finite and within 0 .. 2\\^20", stretch=bad)
    bad[2, 4] = -0.5
    refused("row 2, phoneme 4: stretch", stretch=bad)
    bad[2, 4] = 2.0 ** 20 * 1.5
    refused("row 2, phoneme 4: stretch", stretch=bad)
    bad[2, 4] = np.inf
    refused("row 2, phoneme 4: stretch", stretch=bad)
    mn = np.zeros((B, Tx), np.int32)
    mn[4, 0] = -1
    refused("row 4, phoneme 0: min_frames must be within 0 .. 4194304", min_frames=mn)
    mn[4, 0] = CAP + 1
    refused("row 4, phoneme 0: min_frames", min_frames=mn)
    tg = np.zeros(B, np.int64)
    tg[1] = CAP + 1
    refused("row 1: target_frames must be 0 \\(none\\) or within 1 .. 4194304", target_frames=tg)
    tg[1] = -3
    refused("row 1: target_frames", target_frames=tg)
    refused("timing and forced_durations exclude each other", stretch=ones, forced_durations=np.full((B, Tx), 2, np.int32))
    t = TimingArgs()
    t.reserved[3] = 1
    with pytest.raises(NativeError, match="timing: reserved fields must be 0"):
        run_timed_raw(eng, a, t)
    served()
    for kw in (dict(stretch=ones[:, :-1]), dict(stretch=ones[:-1]), dict(min_frames=np.zeros((B, Tx + 1), np.int32)), dict(min_frames=np.zeros(B, np.int32)),
               dict(target_frames=np.zeros(B + 1, np.int32)), dict(target_frames=np.zeros((B, 2), np.int32)), dict(min_frames=ones),
               dict(target_frames=np.ones(B, np.float32))):
        with pytest.raises(ValueError):
            run(eng, a, **kw)
        served()
    # found on the device
    target, u = targets_for(eng, a)
    floor3 = TR.floor_of(u[3], a["lens"][3])
    tg = target.copy()
    tg[3] = floor3 - 1
    with pytest.raises(NativeError, match=f"row 3: target of {floor3 - 1} frames is below the {floor3} the row needs at least") as err:
        run(eng, a, target_frames=tg)
    assert err.value.code == -1
    with pytest.raises(NativeError, match="no completed run"):
        eng.fetch(want_float=True)
    same_run(run(eng, a), kept)  # the handle works on
    zero = ones.copy()
    zero[1] = 0.0
    with pytest.raises(NativeError, match="row 1: target of 9 frames cannot be reached") as err:
        run(eng, a, stretch=zero, target_frames=np.array([0, 9, 0, 0, 0][:B], np.int32))
    assert err.value.code == -1
    with pytest.raises(NativeError, match="no completed run"):
        eng.fetch_alignment()
    same_run(run(eng, a), kept)


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
def test_identity_fit_replay_and_rows_alone(emu_lib, engines, kind):
    cfg, blob, eng = engines(kind)
    a = feed(cfg)
    check_identity(eng, a)
    target, frames, out = check_fit(eng, a)
    check_rows_alone(lambda: Engine(blob, library=emu_lib), a, target, out, [0, 1, 4] if kind == "sdp" else [3])


@pytest.mark.parametrize("kind", ["sdp", "det"])
def test_output_forms_stretch_and_minimum_frames(engines, kind):
    cfg, blob, eng = engines(kind)
    a = feed(cfg)
    target, frames, _ = check_fit(eng, a)
    check_output_forms(eng, a, target, frames)
    check_stretch_and_min(eng, a)


def test_errors(engines):
    cfg, blob, eng = engines("sdp")
    check_errors(eng, feed(cfg))


def test_session_keywords(emu_lib):
    """run_pcm16 / run_packed: the three keywords and duration_ms (frames = max(1, round(ms / 1000 * rate / hop)) at the voice's
    native rate); such a call goes straight to a lane, never through the micro-batcher."""
    cfg, blob = voice("sdp")
    so = SessionOptions()
    so.seed = SEED
    so.micro_batch_window_ms = 200.0
    sess = InferenceSession(blob, sess_options=so, _library=emu_lib)
    a = feed(cfg, lens=LENS[:3])
    fd = {"input": a["ids"], "input_lengths": a["lens"], "scales": SCALES}
    ms = [60.0, 0.01, None]  # row 1 has one phoneme: a single frame is its floor
    want = [max(1, int(round(60.0 / 1000 * cfg.sample_rate / cfg.hop_length))), 1, 0]
    assert want[0] == 165
    batches = []
    sess._batcher.submit, submit = (lambda *x, **k: batches.append(1) or submit(*x, **k)), sess._batcher.submit
    rows, lengths = sess.run_pcm16(fd, utterance_keys=KEYS[:3], duration_ms=ms)
    assert not batches
    assert int(lengths[0]) == 165 * cfg.hop_length == rows[0].size and int(lengths[1]) == cfg.hop_length
    assert sess.last_timing_factor.shape == (3,) and sess.last_timing_factor[2] == 1.0
    rows2, lengths2, al = sess.run_pcm16(fd, utterance_keys=KEYS[:3], target_frames=want, alignment=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(rows, rows2)) and al.frames[0].sum() == 165
    pk = sess.run_packed(fd, utterance_keys=KEYS[:3], duration_ms=ms, order=[2, 0])
    assert pk.rows[1].tobytes() == rows[0].tobytes() and pk.rows[0].tobytes() == rows[2].tobytes()
    st = np.ones(a["ids"].shape, np.float32)
    st[2] = 3.0
    rows3, _ = sess.run_pcm16(fd, utterance_keys=KEYS[:3], stretch=st, min_frames=np.zeros(a["ids"].shape, np.int32))
    assert rows3[2].size > rows[2].size and rows3[0].tobytes() != rows[0].tobytes()
    with pytest.raises(ValueError, match="not both"):
        sess.run_pcm16(fd, duration_ms=ms, target_frames=[1, 1, 1])
    with pytest.raises(ValueError, match="shape"):
        sess.run_pcm16(fd, duration_ms=ms[:2])
    with pytest.raises(ValueError, match="finite"):
        sess.run_pcm16(fd, duration_ms=[1.0, -2.0, 3.0])
    sess.close()


def test_plain_c99_client(emu_lib, tmp_path):
    """tests/abi/abi_timing_client.c: the new struct and entry point are C99; identity, fit, factor_out and the refusals hold from C."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_timing_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_timing_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir], check=True)
    cfg = VitsConfig.tiny()
    W.save(str(tmp_path / "voice.m355"), cfg, W.synthetic_weights(cfg, seed=17))
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "expected failure rc=-1 msg=timing and forced_durations exclude each other" in p.stdout
    assert "expected failure rc=-1 msg=timing: reserved fields must be 0" in p.stdout
    assert "expected failure rc=-1 msg=row 2: target of 3 frames is below the 12 the row needs at least" in p.stdout
    assert "timing ok" in p.stdout
