"""What timing control in one run (mi355vits_run_timed, k_durations_timed) costs, the sides alternating in ONE process on one device
(the numbers of DESIGN.md §4.17).

  python tools/timing_ab.py [--reps 7] [--out FILE]

1. Kernel times from mi355vits_profile_report on the headline shape (256 rows x 128 ids, apope_low shapes, synthetic weights,
   natural durations; results left on the device): `durations` (k_durations) of a plain run beside `durations.timed`
   (k_durations_timed) of a run without targets (stretch = 1) and of a run with a target for every row.
2. Host to host on 48 ragged sentences (20 .. 128 ids) fitted to given durations (1.15 x each row's natural length), int16
   results copied to the host:
     (a) one timed call;
     (b) the same frames replayed through forced_durations — the cost floor: only one small kernel differs;
     (c) the route without the feature: run, fetch_alignment, edit the frames on the host, run again with forced_durations.
   Gate 1: median (a) exceeds median (b) by no more than (b)'s own max - min over the repetitions.  Gate 2: median (a) < median (c).
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

SCALES = [0.667, 1.0, 0.8]


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def host_edit(frames, lens, target):
    """What a caller does today between the two runs: scale a row's frames to the target, largest remainders first."""
    out = np.zeros_like(frames)
    for b, n in enumerate(lens):
        f = frames[b, :n].astype(np.float64)
        want = f * (target[b] / max(1.0, f.sum()))
        base = np.floor(want).astype(np.int64)
        order = np.argsort(-(want - base), kind="stable")
        base[order[: int(target[b] - base.sum())]] += 1
        out[b, :n] = base
    return out


def kernels(eng, cfg, reps, say):
    rng = np.random.default_rng(1)
    B, Tx = 256, 128
    ids, lens = rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64)
    kw = dict(seed=1, want_float=False, device_only=True)
    ones = np.ones((B, Tx), np.float32)
    res = eng.run(ids, lens, SCALES, **kw)
    target = (res["lengths"] // cfg.hop_length * 115 // 100).astype(np.int32)
    say(f"headline shape: {B} rows x {Tx} ids, {int(res['lengths'].sum())} samples natural, targets 1.15 x")
    t = {"durations": [], "durations.timed (no target)": [], "durations.timed (targets)": []}
    eng.profile_enable(True)
    for rep in range(reps + 2):
        for key, name, extra in (("durations", "durations", {}), ("durations.timed (no target)", "durations.timed", dict(stretch=ones)),
                                 ("durations.timed (targets)", "durations.timed", dict(target_frames=target))):
            eng.profile_reset()
            eng.run(ids, lens, SCALES, **kw, **extra)
            if rep >= 2:
                t[key].append(eng.profile_report()[name]["ms"])
    eng.profile_enable(False)
    say("  kernel times (ms, HIP events around the launch):")
    for k, v in t.items():
        say(f"  {k:28s} {_fmt(v)}")


def host_to_host(eng, cfg, reps, say):
    rng = np.random.default_rng(141)
    B = 48
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    kw = dict(seed=1, want_float=False, want_pcm16=True)
    res = eng.run(ids, lens, SCALES, **kw)
    target = (res["lengths"] // cfg.hop_length * 115 // 100).astype(np.int32)
    eng.run(ids, lens, SCALES, target_frames=target, **kw)
    fitted = eng.fetch_alignment().frames.copy()
    say(f"48 ragged sentences: {int(res['lengths'].sum())} samples natural, fitted to {int(target.sum()) * cfg.hop_length}")

    def a():
        return eng.run(ids, lens, SCALES, target_frames=target, **kw)

    def b():
        return eng.run(ids, lens, SCALES, forced_durations=fitted, **kw)

    def c():
        eng.run(ids, lens, SCALES, seed=1, want_float=False, device_only=True)
        edited = host_edit(eng.fetch_alignment().frames, lens, target)
        return eng.run(ids, lens, SCALES, forced_durations=edited, **kw)

    t = {"a": [], "b": [], "c": []}
    for rep in range(reps + 2):
        for key, fn in (("a", a), ("b", b), ("c", c), ("b", b), ("a", a)):
            t0 = time.perf_counter()
            out = fn()
            ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(out["lengths"], target.astype(np.int64) * cfg.hop_length)
            del out
            if rep >= 2:
                t[key].append(ms)
    say("  host to host (ms):")
    say(f"  (a) one timed call              {_fmt(t['a'])}")
    say(f"  (b) forced_durations replay     {_fmt(t['b'])}")
    say(f"  (c) run, alignment, edit, run   {_fmt(t['c'])}")
    ma, mb, mc = (statistics.median(t[k]) for k in "abc")
    spread = max(t["b"]) - min(t["b"])
    say(f"  gate 1: (a) - (b) = {ma - mb:+.4f} ms against (b)'s spread of {spread:.4f} ms: {'holds' if ma - mb <= spread else 'FAILS'}")
    say(f"  gate 2: (a) = {ma:.4f} ms against (c) = {mc:.4f} ms ({mc / ma:.2f} x): {'holds' if ma < mc else 'FAILS'}")


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
    say(f"timing_ab: {eng.native.version()}, math {eng.math}, reps {args.reps} (times in ms)")
    kernels(eng, cfg, args.reps, say)
    host_to_host(eng, cfg, args.reps, say)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
