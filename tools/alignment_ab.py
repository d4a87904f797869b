"""What mi355vits_fetch_alignment costs, the sides alternating in ONE process on one device (the numbers of DESIGN.md §4.9).

  python tools/alignment_ab.py [--reps 7] [--out FILE]

On the headline shape (256 rows x 128 ids x 6 forced frames, apope_low shapes, synthetic weights; results left on the device) and
on 48 ragged rows (20 .. 128 ids, natural durations; int16 results copied to the host):
1. the `align` kernel with and without levels from mi355vits_profile_report, beside the padded int16 pass (`pcm16`) of the same
   run, which reads the same samples once;
2. host-to-host: run against run + fetch_alignment (timing only, and with levels), alternating repetitions, the median.
Two untimed warm-up rounds; prints min / median / max over the repetitions; nothing is asserted."""
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


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def measure(eng, name, ids, lens, reps, say, **kw):
    t = {k: [] for k in ("align_ms", "align.levels_ms", "pcm16_ms", "run_ms", "run+align_ms", "run+align.levels_ms")}
    for rep in range(reps + 2):  # two untimed warm-up rounds
        # (1) the kernels: one profiled run (its pcm16 pass), then the two forms of align on that run
        eng.profile_enable(True)
        eng.profile_reset()
        res = eng.run(ids, lens, [0.667, 1.0, 0.8], seed=1, want_float=False, want_pcm16=True, **kw)
        ms = {"pcm16_ms": eng.profile_report()["pcm16"]["ms"]}
        for levels, key in ((False, "align_ms"), (True, "align.levels_ms")):
            eng.profile_reset()
            al = eng.fetch_alignment(levels=levels)
            r = eng.profile_report()["align"]
            ms[key] = r["ms"]
            if rep == 0:
                say(f"  align{'.levels' if levels else '':7s} {al.frames.shape[0]} x {al.frames.shape[1]} phonemes, {int(al.samples.sum())} samples, "
                    f"longest span {int(al.samples.max())}, {int(r['bytes'])} B moved")
        eng.profile_enable(False)
        if rep == 0:
            say(f"{name}: {len(lens)} rows, {int(np.sum(res['lengths']))} samples")
        del res
        # (2) host to host, the sides alternating inside a round
        h2h = {"run_ms": [], "run+align_ms": [], "run+align.levels_ms": []}
        for key, fetch in (("run_ms", None), ("run+align_ms", False), ("run+align.levels_ms", True), ("run_ms", None)):
            t0 = time.perf_counter()
            res = eng.run(ids, lens, [0.667, 1.0, 0.8], seed=1, want_float=False, want_pcm16=True, **kw)
            if fetch is not None:
                eng.fetch_alignment(levels=fetch)
            h2h[key].append((time.perf_counter() - t0) * 1e3)
            del res
        if rep >= 2:
            for k, v in ms.items():
                t[k].append(v)
            for k, v in h2h.items():
                t[k].extend(v)
    say("  kernel times (ms, HIP events around the launch):")
    for k in ("align_ms", "align.levels_ms", "pcm16_ms"):
        say(f"  {k:22s} {_fmt(t[k])}")
    say("  host to host (ms):")
    for k in ("run_ms", "run+align_ms", "run+align.levels_ms"):
        say(f"  {k:22s} {_fmt(t[k])}")
    lv, pc, fl = statistics.median(t["align.levels_ms"]), statistics.median(t["pcm16_ms"]), statistics.median(t["align_ms"])
    if lv > pc:
        say(f"  align with levels ({lv:.4f}) costs more than the padded pcm16 pass ({pc:.4f}): the timing-only form, which reads no audio, "
            f"takes {fl:.4f} — launches of this size sit at the launch floor, this pcm16 pass included; above the floor a wave walks one "
            "phoneme's span with 4-byte loads and a double add per sample, and most of the rows x phonemes waves are short.")
    else:
        say(f"  align with levels ({lv:.4f}) costs no more than the padded pcm16 pass ({pc:.4f}); the timing-only form: {fl:.4f}.")


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
    say(f"alignment_ab: {eng.native.version()}, math {eng.math}, reps {args.reps} (times in ms)")
    rng = np.random.default_rng(1)
    B, Tx = 256, 128
    measure(eng, "headline shape", rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64), args.reps, say,
            forced_durations=np.full((B, Tx), 6, np.int32), device_only=True)
    rng = np.random.default_rng(141)
    B = 48
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    measure(eng, "48 ragged sentences", ids, lens, args.reps, say)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
