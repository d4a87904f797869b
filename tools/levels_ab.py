"""What level control in one run (mi355vits_run_levels, k_levels) costs, the sides alternating in ONE process on one handle (the
numbers of DESIGN.md §4.19).

  python tools/levels_ab.py [--reps 7] [--out FILE]

1. Kernel times from mi355vits_profile_report on the headline shape (256 rows x 128 ids, apope_low shapes, synthetic weights,
   natural durations; results left on the device): `levels` (k_levels; gains on a third of the phonemes, R = 5 ms) beside
   `pack.f32` (k_pack writing the same run's rows as one F32LE stream: the project's existing kernel with the same 8 bytes per
   sample).  Kernel gate: median(levels) <= 2 x median(pack.f32) + (max - min of pack.f32).  Ungated: `levels` at R = 0 and R = 4096.
2. Host to host, profiler off, on 48 ragged sentences (20 .. 128 ids), int16 results copied to the host:
     (a) one levels call;
     (b) the same call without levels;
     (c) the route (a) replaces: a float run, fetch_alignment, the envelope and the product in numpy (tests/levels_ref.py), the
         peak and the int16 conversion on the host.
   Call gate 1: median (a) - median (b) <= (b)'s max - min + the measured median of `levels` on these rows.
   Call gate 2: median (a) < median (c); the two int16 results are identical (asserted).
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
from mimic3_amd._native import Engine  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from tests import levels_ref as LR  # noqa: E402

SCALES = [0.667, 1.0, 0.8]


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def gains(rng, lens, Tx):
    """Gains on a third of the phonemes (uniform in [0, 4], what -inf .. +12 dB spans), 1 elsewhere."""
    g = np.where(rng.random((len(lens), Tx)) < 1 / 3, rng.uniform(0.0, 4.0, (len(lens), Tx)), 1.0).astype(np.float32)
    return g


def host_int16(y):
    """utils.py:237-244 on the host: peak-normalise, clip, truncating cast."""
    peak = np.float32(max(0.01, np.max(np.abs(y)))) if y.size else np.float32(0.01)
    return np.clip(y * (np.float32(32767.0) / peak), -32767.0, 32767.0).astype(np.int16)


def kernels(eng, cfg, reps, say):
    rng = np.random.default_rng(1)
    B, Tx = 256, 128
    ids, lens = rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64)
    g = gains(rng, lens, Tx)
    R5 = int(round(0.005 * cfg.sample_rate))
    kw = dict(seed=1, want_float=False, device_only=True)
    res = eng.run(ids, lens, SCALES, **kw)
    say(f"headline shape: {B} rows x {Tx} ids, {int(res['lengths'].sum())} samples natural, gains on {int((g != 1).sum())} of {B * Tx} phonemes, R = {R5}")
    t = {"levels (R = 5 ms)": [], "pack.f32": [], "levels (R = 0)": [], "levels (R = 4096)": []}
    eng.set_output_encoding("f32le")
    eng.profile_enable(True)
    for rep in range(reps + 2):
        for key, R in (("levels (R = 5 ms)", R5), ("levels (R = 0)", 0), ("levels (R = 4096)", 4096)):
            eng.profile_reset()
            eng.run(ids, lens, SCALES, gain=g, ramp_samples=R, **kw)
            if R == R5:
                pk = eng.fetch_packed()  # k_pack, F32LE, on the same run
                del pk
            rp = eng.profile_report()
            if rep >= 2:
                t[key].append(rp["levels"]["ms"])
                if R == R5:
                    t["pack.f32"].append(rp["pack.f32"]["ms"])
    eng.profile_enable(False)
    eng.set_output_encoding("s16le")
    say("  kernel times (ms, HIP events around the launch):")
    for k, v in t.items():
        say(f"  {k:22s} {_fmt(v)}")
    ml, mp = statistics.median(t["levels (R = 5 ms)"]), statistics.median(t["pack.f32"])
    spread = max(t["pack.f32"]) - min(t["pack.f32"])
    say(f"  kernel gate: levels {ml:.4f} ms against 2 x pack.f32 + its spread = {2 * mp + spread:.4f} ms: {'holds' if ml <= 2 * mp + spread else 'FAILS'}")


def host_to_host(eng, cfg, reps, say):
    rng = np.random.default_rng(141)
    B = 48
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    g = gains(rng, lens, 128)
    R = int(round(0.005 * cfg.sample_rate))
    ramp = np.full(B, R, np.int32)
    kw = dict(seed=1, want_float=False, want_pcm16=True)
    hop = cfg.hop_length

    def a():
        return eng.run(ids, lens, SCALES, gain=g, ramp_samples=ramp, **kw)

    def b():
        return eng.run(ids, lens, SCALES, **kw)

    def c():
        out = eng.run(ids, lens, SCALES, seed=1, want_float=True, want_pcm16=False)
        frames = eng.fetch_alignment().frames
        pcm = np.zeros(out["audio"].shape, np.int16)
        for r in range(B):
            n = int(out["lengths"][r])
            y = LR.apply(out["audio"][r, :n], LR.scale(frames[r], int(lens[r]), g[r], R, hop))
            pcm[r, :n] = host_int16(y)
        return {"pcm": pcm, "lengths": out["lengths"]}

    # the levels kernel on these rows (profiler on for this one measurement only)
    eng.profile_enable(True)
    tk = []
    for rep in range(reps + 2):
        eng.profile_reset()
        a()
        if rep >= 2:
            tk.append(eng.profile_report()["levels"]["ms"])
    eng.profile_enable(False)
    say(f"48 ragged sentences: {int(b()['lengths'].sum())} samples; `levels` on them: {_fmt(tk)}")

    t = {"a": [], "b": [], "c": []}
    for rep in range(reps + 2):
        got = {}
        for key, fn in (("a", a), ("b", b), ("c", c), ("b", b), ("a", a)):
            t0 = time.perf_counter()
            out = fn()
            ms = (time.perf_counter() - t0) * 1e3
            got[key] = out["pcm"].copy()
            del out
            if rep >= 2:
                t[key].append(ms)
        assert got["a"].tobytes() == got["c"].tobytes(), "the levels run and the host route differ"
        assert got["a"].tobytes() != got["b"].tobytes()
    say("  host to host (ms), profiler off:")
    say(f"  (a) one levels call                       {_fmt(t['a'])}")
    say(f"  (b) the same call without levels          {_fmt(t['b'])}")
    say(f"  (c) float run, alignment, numpy, int16    {_fmt(t['c'])}")
    ma, mb, mc = (statistics.median(t[k]) for k in "abc")
    allow = max(t["b"]) - min(t["b"]) + statistics.median(tk)
    say(f"  call gate 1: (a) - (b) = {ma - mb:+.4f} ms against (b)'s spread + the kernel = {allow:.4f} ms: {'holds' if ma - mb <= allow else 'FAILS'}")
    say(f"  call gate 2: (a) = {ma:.4f} ms against (c) = {mc:.4f} ms ({mc / ma:.2f} x), int16 identical: {'holds' if ma < mc else 'FAILS'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0)), device=0)
    say(f"levels_ab: {eng.native.version()}, math {eng.math}, reps {args.reps} (times in ms)")
    kernels(eng, cfg, args.reps, say)
    host_to_host(eng, cfg, args.reps, say)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
