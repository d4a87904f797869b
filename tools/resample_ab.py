"""Output at a requested sample rate against the native path, both alternating in ONE process on one handle (the numbers of
DESIGN.md §4.2 / §4.8).

  python tools/resample_ab.py [--reps 7] [--out FILE]

1. Headline shape (256 rows x 128 ids x 6 forced frames = 768 frames a row, apope_low shapes, synthetic weights), host ids in ->
   host int16 out: per rate (8, 16, 48 kHz) the step both ways, native and resampled calls alternating; then, with profiling on,
   k_resample's time (profile label `resample`) and its bytes/s = (4 sum n + 4 sum n_out) / time as a share of 8 TB/s.
2. The ragged 48-sentence request of tools/packed_ab.py to one WAV with 250 ms breaks (run_packed), native against each rate.
3. Accuracy on that ragged batch: worst-row relative RMS of the engine's rows and of plain f32 against the fp64 yardstick
   (tests/resample_ref.py on the engine's own native audio).
Prints min / median / max over the repetitions; nothing is asserted."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from tests import resample_ref as R  # noqa: E402

RATES = (8000, 16000, 48000)
HBM_ROOF = 8.0e12


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def headline(eng, cfg, reps, say):
    B, Tx = 256, 128
    rng = np.random.default_rng(1)
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    lens = np.full(B, Tx, np.int64)
    forced = np.full((B, Tx), 6, np.int32)
    sc = [0.667, 1.0, 0.8]

    def step(rate):
        eng.set_output_rate(rate)
        t0 = time.perf_counter()
        out = eng.run(ids, lens, sc, forced_durations=forced, seed=1, want_float=False, want_pcm16=True)
        t1 = time.perf_counter()
        n = int(out["lengths"][0])
        del out
        return (t1 - t0) * 1e3, eng.last_run_ms(), n

    for rate in (0,) + RATES:  # warm-up: every rate's workspace and filter table
        step(rate)
        step(rate)
    n_native = step(0)[2]
    say(f"headline shape: {B} rows x {n_native} native samples (host ids in -> host int16 out; times in ms)")
    for rate in RATES:
        nat, res, nat_dev, res_dev = [], [], [], []
        for _ in range(reps):
            a = step(0)
            b = step(rate)
            nat.append(a[0]); nat_dev.append(a[1]); res.append(b[0]); res_dev.append(b[1])
            n_out = b[2]
        say(f"  {rate} Hz ({n_out} samples a row), alternating with native:")
        say(f"    native step    host {_fmt(nat)}")
        say(f"                   device {_fmt(nat_dev)}")
        say(f"    resampled step host {_fmt(res)}")
        say(f"                   device {_fmt(res_dev)}")
        say(f"    resampled / native (medians): host {statistics.median(res) / statistics.median(nat):.4f}  device "
            f"{statistics.median(res_dev) / statistics.median(nat_dev):.4f}; native spread (max - min) / median "
            f"{(max(nat) - min(nat)) / statistics.median(nat):.4f}")
    say("  with profiling on (every launch bracketed by events):")
    eng.profile_enable(True)
    for rate in RATES:
        eng.set_output_rate(rate)
        ms, pcm = [], []
        for _ in range(reps):
            eng.profile_reset()
            out = eng.run(ids, lens, sc, forced_durations=forced, seed=1, want_float=False, want_pcm16=True)
            rep = eng.profile_report()
            ms.append(rep["resample"]["ms"]); pcm.append(rep["pcm16"]["ms"])
            nbytes = rep["resample"]["bytes"]
            del out
        med = statistics.median(ms)
        say(f"    {rate} Hz: resample {_fmt(ms)}; {nbytes / 1e6:.1f} MB -> {nbytes / (med * 1e-3) / 1e12:.3f} TB/s = "
            f"{nbytes / (med * 1e-3) / HBM_ROOF:.3f} of the 8 TB/s roof; pcm16 {statistics.median(pcm):.4f}")
    eng.set_output_rate(0)
    pcm = []
    for _ in range(reps):
        eng.profile_reset()
        out = eng.run(ids, lens, sc, forced_durations=forced, seed=1, want_float=False, want_pcm16=True)
        pcm.append(eng.profile_report()["pcm16"]["ms"])
        del out
    say(f"    native: pcm16 {statistics.median(pcm):.4f}")
    eng.profile_enable(False)


def ragged(eng, cfg, reps, say):
    B = 48
    rng = np.random.default_rng(141)
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    sc = [0.667, 1.0, 0.8]

    def step(rate):
        eng.set_output_rate(rate)
        hz = rate or cfg.sample_rate
        lead = [0] + [int(250.0 / 1000.0 * hz)] * (B - 1)
        t0 = time.perf_counter()
        pk = eng.run_packed(ids, lens, sc, seed=1, lead_samples=lead, wav=True)
        view = pk.wav
        t1 = time.perf_counter()
        n = len(view)
        del pk, view
        return (t1 - t0) * 1e3, eng.last_run_ms(), n

    for rate in (0,) + RATES:
        step(rate)
        step(rate)
    say(f"ragged: {B} rows of 20 .. 128 ids to one WAV with 250 ms breaks (run_packed, host to host)")
    for rate in RATES:
        nat, res, nat_dev, res_dev = [], [], [], []
        for _ in range(reps):
            a = step(0)
            b = step(rate)
            nat.append(a[0]); nat_dev.append(a[1]); res.append(b[0]); res_dev.append(b[1])
        say(f"  {rate} Hz: file {b[2]} B (native {a[2]} B)")
        say(f"    native    host {_fmt(nat)}   device {_fmt(nat_dev)}")
        say(f"    resampled host {_fmt(res)}   device {_fmt(res_dev)}")
    # accuracy on the same batch
    eng.set_output_rate(0)
    native = eng.run(ids, lens, sc, seed=1, want_float=True)
    nat_audio, nat_len = native["audio"].copy(), native["lengths"].copy()
    say("accuracy on the ragged batch (worst row, relative RMS against the fp64 yardstick on the engine's own native audio):")
    for rate in (8000, 11025, 16000, 24000, 44100, 48000):
        eng.set_output_rate(rate)
        out = eng.run(ids, lens, sc, seed=1, want_float=True)
        L, M = R.ratio(cfg.sample_rate, rate)
        we = wf = 0.0
        for b in range(0, B, 4):
            e, f = R.errors(out["audio"][b, : int(out["lengths"][b])], nat_audio[b, : int(nat_len[b])], L, M)
            we, wf = max(we, e), max(wf, f)
        say(f"  {rate} Hz ({L} / {M}): engine {we:.3e}  plain f32 {wf:.3e}  ratio {we / wf:.2f}")
    eng.set_output_rate(0)


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
    say(f"resample_ab: {eng.native.version()}, math {eng.math}, reps {args.reps}")
    headline(eng, cfg, args.reps, say)
    ragged(eng, cfg, args.reps, say)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
