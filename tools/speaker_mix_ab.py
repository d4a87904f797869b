"""What the speaker conditioning costs with and without blended speakers (mi355vits_run_speakers, k_speaker_cond_mix), the two sides
alternating in ONE process on one device (the numbers of DESIGN.md §4.18).

  python tools/speaker_mix_ab.py [--reps 9] [--out FILE]

vctk_low shapes (109 speakers, gin 512; synthetic weights), B = 1, 32 and 256 rows of 64 ids, results left on the device.  Per B:
  * `speaker_cond` of a plain sid run from mi355vits_profile_report: ONE record around the 2 + flow_n_flows launches of
    k_speaker_cond — the path a run without speakers takes, unchanged by the feature;
  * `speaker_cond.mix` of a run with a two-term mix per row: the one launch of k_speaker_cond_mix;
  * host-to-host times of both runs with the profiler off (a host clock around a call that ends in the run's synchronisations).
Gate, at B = 32: median speaker_cond.mix <= median speaker_cond + that side's max - min over the repetitions.  B = 1 and 256 are
reported, not gated.  Two untimed warm-up rounds; the figures stand as measured."""
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
GATED_B = 32


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def one_batch(eng, cfg, B, reps, say):
    rng = np.random.default_rng(B)
    Tx = 64
    ids, lens = rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64)
    sid = rng.integers(0, cfg.n_speakers, B).astype(np.int64)
    mixes = [{int(s): 0.7, int((s + 1 + rng.integers(0, cfg.n_speakers - 1)) % cfg.n_speakers): 0.3} for s in sid]
    kw = dict(seed=1, want_float=False, device_only=True)
    sides = (("speaker_cond", "speaker_cond", lambda: eng.run(ids, lens, SCALES, sid, **kw)),
             ("speaker_cond.mix", "speaker_cond.mix", lambda: eng.run(ids, lens, SCALES, None, speakers=mixes, **kw)))
    k = {key: [] for key, _, _ in sides}
    eng.profile_enable(True)
    for rep in range(reps + 2):
        for key, name, fn in sides if rep % 2 == 0 else sides[::-1]:
            eng.profile_reset()
            fn()
            if rep >= 2:
                k[key].append(eng.profile_report()[name]["ms"])
    eng.profile_enable(False)
    h = {key: [] for key, _, _ in sides}
    for rep in range(reps + 2):
        for key, name, fn in sides if rep % 2 == 0 else sides[::-1]:
            t0 = time.perf_counter()
            fn()
            ms = (time.perf_counter() - t0) * 1e3
            if rep >= 2:
                h[key].append(ms)
    say(f"B = {B} x {Tx} ids:")
    say(f"  kernel  speaker_cond (plain sid run)   {_fmt(k['speaker_cond'])}")
    say(f"  kernel  speaker_cond.mix (two terms)   {_fmt(k['speaker_cond.mix'])}")
    say(f"  host to host  plain sid run            {_fmt(h['speaker_cond'])}")
    say(f"  host to host  speakers run             {_fmt(h['speaker_cond.mix'])}")
    if B == GATED_B:
        a, m = k["speaker_cond"], statistics.median(k["speaker_cond.mix"])
        bound = statistics.median(a) + (max(a) - min(a))
        say(f"  gate: speaker_cond.mix {m:.4f} ms against speaker_cond {statistics.median(a):.4f} + spread {max(a) - min(a):.4f} = {bound:.4f} ms: "
            f"{'holds' if m <= bound else 'FAILS'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 32, 256])
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = VitsConfig.vctk_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0)), device=0)
    say(f"speaker_mix_ab: {eng.native.version()}, math {eng.math}, vctk_low shapes, reps {args.reps} (times in ms)")
    for B in args.batches:
        one_batch(eng, cfg, B, args.reps, say)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
