"""Packed results against the padded path, both sides alternating in ONE process on one device (the numbers of DESIGN.md §4.2 / §6).

  python tools/packed_ab.py [--reps 7] [--out FILE]

1. Headline shape (256 rows x 128 ids x 6 forced frames, apope_low shapes, synthetic weights): k_pcm16 (profile label
   `pcm16`) against k_pack<S16> (csrc/kernels_pack.cpp; `pcm16.pack`) from mi355vits_profile_report — both move 6 B per sample there —, and the
   calls' device times (mi355vits_last_run_ms) and host-to-host times.
2. A ragged batch (48 rows of 20 .. 128 ids, natural durations): host-to-host time to one WAV with 250 ms breaks —
   run_packed(wav=True) against the padded int16 call + postprocess.utterances_to_wav — with the bytes each side copies from the
   device beside it.
Prints min / median / max over the repetitions; nothing is asserted."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimic3_amd import postprocess as PP  # noqa: E402
from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def headline(eng, cfg, reps, say):
    B, Tx = 256, 128
    rng = np.random.default_rng(1)
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    lens = np.full(B, Tx, np.int64)
    forced = np.full((B, Tx), 6, np.int32)
    sc = [0.667, 1.0, 0.8]
    t = {k: [] for k in ("pcm16_ms", "pack_ms", "padded_dev_ms", "packed_dev_ms", "padded_host_ms", "packed_host_ms")}
    for rep in range(reps + 2):  # two untimed warm-up rounds
        eng.profile_enable(True)
        eng.profile_reset()
        t0 = time.perf_counter()
        full = eng.run(ids, lens, sc, forced_durations=forced, seed=1, want_float=False, want_pcm16=True)
        t1 = time.perf_counter()
        a = eng.profile_report()["pcm16"]["ms"]
        da = eng.last_run_ms()
        eng.profile_reset()
        t2 = time.perf_counter()
        pk = eng.run_packed(ids, lens, sc, forced_durations=forced, seed=1)
        t3 = time.perf_counter()
        b = eng.profile_report()["pcm16.pack"]["ms"]
        db = eng.last_run_ms()
        eng.profile_enable(False)
        if rep == 0:
            assert np.array_equal(pk.pcm.reshape(B, -1), full["pcm"])
            say(f"headline shape: {B} rows x {int(full['lengths'][0])} samples; D2H padded {full['pcm'].nbytes} B, packed {pk.pcm.nbytes} B")
        del full, pk
        if rep >= 2:
            for k, v in zip(t, (a, b, da, db, (t1 - t0) * 1e3, (t3 - t2) * 1e3)):
                t[k].append(v)
    say("  (profiling on: every launch is bracketed by events; call times below include that)")
    for k, v in t.items():
        say(f"  {k:16s} {_fmt(v)}")


def ragged(eng, cfg, reps, say):
    B = 48
    rng = np.random.default_rng(141)
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    sc = [0.667, 1.0, 0.8]
    break_ms = 250.0
    lead = [0] + [int(break_ms / 1000.0 * cfg.sample_rate)] * (B - 1)
    t = {k: [] for k in ("padded_to_wav_ms", "packed_to_wav_view_ms", "packed_to_wav_bytes_ms", "padded_dev_ms", "packed_dev_ms")}
    for rep in range(reps + 2):
        t0 = time.perf_counter()
        full = eng.run(ids, lens, sc, seed=1, want_float=False, want_pcm16=True)
        rows = [full["pcm"][b, : int(full["lengths"][b])] for b in range(B)]
        wav_a = PP.utterances_to_wav(rows, cfg.sample_rate, break_ms=break_ms)
        t1 = time.perf_counter()
        da = eng.last_run_ms()
        t2 = time.perf_counter()
        pk = eng.run_packed(ids, lens, sc, seed=1, lead_samples=lead, wav=True)
        view = pk.wav
        t3 = time.perf_counter()
        wav_b = bytes(view)
        t4 = time.perf_counter()
        db = eng.last_run_ms()
        if rep == 0:
            assert wav_a == wav_b
            say(f"ragged: {B} rows, l_max {int(full['l_max'])}, sum of rows {int(np.sum(full['lengths']))} samples "
                f"(padding efficiency {float(np.sum(full['lengths'])) / (B * int(full['l_max'])):.3f}); "
                f"D2H padded {full['pcm'].nbytes} B, packed {len(wav_b)} B (silences and header included)")
        del full, rows, pk, view
        if rep >= 2:
            for k, v in zip(t, ((t1 - t0) * 1e3, (t3 - t2) * 1e3, (t4 - t2) * 1e3, da, db)):
                t[k].append(v)
    for k, v in t.items():
        say(f"  {k:24s} {_fmt(v)}")


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
    say(f"packed_ab: {eng.native.version()}, math {eng.math}, reps {args.reps} (times in ms)")
    headline(eng, cfg, args.reps, say)
    ragged(eng, cfg, args.reps, say)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
