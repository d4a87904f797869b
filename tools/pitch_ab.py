"""What pitch control in one run (mi355vits_run_pitch, k_pitch_plan, k_pitch) costs, the sides alternating in ONE process on one
handle (the numbers of DESIGN.md §4.20).

  python tools/pitch_ab.py [--reps 5] [--out FILE]

1. Kernel times from mi355vits_profile_report on the headline shape (256 rows x 128 ids, apope_low shapes, synthetic weights, a third
   of the phonemes at +2 semitones; output rate 16 kHz, results left on the device): `pitch` (k_pitch) beside `resample` (k_resample)
   of the same run, each per sample it writes.  Kernel gate: pitch per output sample <= 3 x resample per output sample.
2. Host to host, profiler off, on 48 ragged sentences (20 .. 128 ids) with a third of the phonemes at +2 semitones, int16 results
   copied to the host:
     (a) one pitch call;
     (b) the route (a) replaces: a timed float run whose stretch is the ratios, fetch_alignment, the warp in numpy
         (tests/pitch_ref.py, with the handles' own filter table), the peak and the int16 conversion on the host.
   Call gate: median (a) < median (b); the two int16 results are identical (asserted).
Two untimed warm-up rounds; prints min / median / max over the repetitions and says whether each gate holds; the figures stand as
measured."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine, hooks_library  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from tests import pitch_ref as PR  # noqa: E402

SCALES = [0.667, 1.0, 0.8]
SEMITONE2 = np.float32(2.0 ** (2.0 / 12.0))


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def ratios(rng, B, Tx):
    return np.where(rng.random((B, Tx)) < 1 / 3, SEMITONE2, np.float32(1.0)).astype(np.float32)


def host_int16(y):
    """utils.py:237-244 on the host: peak-normalise, clip, truncating cast."""
    peak = np.float32(max(0.01, np.max(np.abs(y)))) if y.size else np.float32(0.01)
    return np.clip(y * (np.float32(32767.0) / peak), -32767.0, 32767.0).astype(np.int16)


def kernels(eng, cfg, reps, say):
    rng = np.random.default_rng(1)
    B, Tx = 256, 128
    ids, lens = rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64)
    p = ratios(rng, B, Tx)
    kw = dict(seed=1, want_float=False, device_only=True)
    native = int(eng.run(ids, lens, SCALES, pitch=p, **kw)["lengths"].sum())
    eng.set_output_rate(16000)
    res = eng.run(ids, lens, SCALES, pitch=p, **kw)
    out16 = int(res["lengths"].sum())
    say(f"headline shape: {B} rows x {Tx} ids, {int((p != 1).sum())} of {B * Tx} phonemes at +2 semitones; {native} warped samples at {cfg.sample_rate} Hz, {out16} at 16000 Hz")
    t = {"pitch": [], "pitch.plan": [], "resample": []}
    eng.profile_enable(True)
    for rep in range(reps + 2):
        eng.profile_reset()
        eng.run(ids, lens, SCALES, pitch=p, **kw)
        rp = eng.profile_report()
        if rep >= 2:
            for k in t:
                t[k].append(rp[k]["ms"])
    eng.profile_enable(False)
    eng.set_output_rate(0)
    say("  kernel times (ms, HIP events around the launch):")
    for k, v in t.items():
        say(f"  {k:12s} {_fmt(v)}")
    per_p, per_r = statistics.median(t["pitch"]) / native * 1e6, statistics.median(t["resample"]) / out16 * 1e6
    say(f"  kernel gate: pitch {per_p:.4f} ns per output sample against 3 x resample's {per_r:.4f} = {3 * per_r:.4f}: {'holds' if per_p <= 3 * per_r else 'FAILS'}")


def host_to_host(eng, cfg, reps, say, h):
    rng = np.random.default_rng(141)
    B = 48
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    p = ratios(rng, B, 128)
    hop = cfg.hop_length

    def a():
        return eng.run(ids, lens, SCALES, seed=1, want_float=False, want_pcm16=True, pitch=p)

    def b():
        out = eng.run(ids, lens, SCALES, seed=1, want_float=True, want_pcm16=False, stretch=p)
        frames = eng.fetch_alignment().frames
        rows = []
        for r in range(B):
            n = int(out["lengths"][r])
            rows.append(host_int16(PR.warp(out["audio"][r, :n], frames[r], int(lens[r]), p[r], hop, h)))
        pcm = np.zeros((B, max(y.size for y in rows)), np.int16)
        for r, y in enumerate(rows):
            pcm[r, : y.size] = y
        return {"pcm": pcm, "lengths": np.array([y.size for y in rows])}

    say(f"48 ragged sentences: {int(a()['lengths'].sum())} warped samples")
    t = {"a": [], "b": []}
    for rep in range(reps + 2):
        got = {}
        for key, fn in (("a", a), ("b", b), ("a", a)):
            t0 = time.perf_counter()
            out = fn()
            ms = (time.perf_counter() - t0) * 1e3
            got[key] = (out["pcm"].copy(), np.asarray(out["lengths"]).astype(np.int64).copy())
            del out
            if rep >= 2:
                t[key].append(ms)
        assert got["a"][1].tolist() == got["b"][1].tolist() and got["a"][0].tobytes() == got["b"][0].tobytes(), "the pitch run and the host route differ"
    say("  host to host (ms), profiler off:")
    say(f"  (a) one pitch call                              {_fmt(t['a'])}")
    say(f"  (b) timed float run, alignment, numpy, int16    {_fmt(t['b'])}")
    ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
    say(f"  call gate: (a) = {ma:.4f} ms against (b) = {mb:.4f} ms ({mb / ma:.2f} x), int16 identical: {'holds' if ma < mb else 'FAILS'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0)), device=0)
    say(f"pitch_ab: {eng.native.version()}, math {eng.math}, reps {args.reps} (times in ms)")
    kernels(eng, cfg, args.reps, say)
    host_to_host(eng, cfg, args.reps, say, hooks_library().test_pitch_table())
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
