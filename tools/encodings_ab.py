"""The encoded packed streams against the int16 one, the sides alternating in ONE process on one device (the numbers of
DESIGN.md's packed-results section).

  python tools/encodings_ab.py [--reps 7] [--out FILE]

1. Headline shape (256 rows x 128 ids x 6 forced frames, apope_low shapes, synthetic weights): one synthesis per round, then
   mi355vits_fetch_packed in each encoding — the forms of the one kernel k_pack (csrc/kernels_pack.cpp): int16 (profile label `pcm16.pack`,
   6 B per sample) against G.711 / f32 (`pack.ulaw` / `pack.alaw`, 5 B per sample; `pack.f32`, 8 B per sample) from mi355vits_profile_report, with the bytes each
   copies from the device beside them.
2. 48 ragged rows (20 .. 128 ids, natural durations) at 8000 Hz to one mu-law WAV with 250 ms breaks, host-to-host:
   run_packed(encoding="ulaw", wav=True) against run_packed(wav=True) + mu-law on the host (audioop.lin2ulaw where the interpreter
   has it, else postprocess.lin2ulaw) + postprocess.wav_bytes.
Two untimed warm-up rounds; prints min / median / max over the repetitions; nothing is asserted."""
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

try:
    import audioop
except ImportError:
    audioop = None

LABELS = {"s16le": "pcm16.pack", "ulaw": "pack.ulaw", "alaw": "pack.alaw", "f32le": "pack.f32"}


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def headline(eng, cfg, reps, say):
    B, Tx = 256, 128
    rng = np.random.default_rng(1)
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    lens = np.full(B, Tx, np.int64)
    forced = np.full((B, Tx), 6, np.int32)
    t = {LABELS[e]: [] for e in LABELS}
    eng.set_output_encoding("s16le")
    for rep in range(reps + 2):  # two untimed warm-up rounds
        res = eng.run(ids, lens, [0.667, 1.0, 0.8], forced_durations=forced, seed=1, device_only=True, want_float=False)
        eng.profile_enable(True)
        ms = {}
        for enc in LABELS:  # the sides alternate inside a round
            eng.set_output_encoding(enc)
            eng.profile_reset()
            pk = eng.fetch_packed()
            ms[LABELS[enc]] = eng.profile_report()[LABELS[enc]]["ms"]
            if rep == 0:
                say(f"  {LABELS[enc]:11s} {pk.total_samples} samples, D2H {pk.data.nbytes} B")
            del pk
        eng.profile_enable(False)
        if rep == 0:
            say(f"headline shape: {B} rows x {int(res['lengths'][0])} samples")
        if rep >= 2:
            for k, v in ms.items():
                t[k].append(v)
    eng.set_output_encoding("s16le")
    say("  kernel times (ms, HIP events around the launch):")
    for k, v in t.items():
        say(f"  {k:11s} {_fmt(v)}")
    ref, mu = t["pcm16.pack"], t["pack.ulaw"]
    say(f"  gate: median pack.ulaw {statistics.median(mu):.4f} <= median pcm16.pack {statistics.median(ref):.4f} + its spread "
        f"{max(ref) - min(ref):.4f} = {statistics.median(ref) + max(ref) - min(ref):.4f}: "
        f"{'met' if statistics.median(mu) <= statistics.median(ref) + max(ref) - min(ref) else 'MISSED'}")


def ragged(eng, cfg, reps, say):
    B, hz = 48, 8000
    rng = np.random.default_rng(141)
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    sc = [0.667, 1.0, 0.8]
    lead = [0] + [int(250.0 / 1000.0 * hz)] * (B - 1)
    eng.set_output_rate(hz)
    t = {k: [] for k in ("s16_then_host_ulaw_ms", "ulaw_stream_ms", "s16_dev_ms", "ulaw_dev_ms")}
    for rep in range(reps + 2):
        eng.set_output_encoding("s16le")
        t0 = time.perf_counter()
        pk = eng.run_packed(ids, lens, sc, seed=1, lead_samples=lead, wav=True)
        codes = np.frombuffer(audioop.lin2ulaw(pk.pcm.tobytes(), 2), np.uint8) if audioop else PP.lin2ulaw(pk.pcm)
        wav_a = PP.wav_bytes([codes], hz, "ulaw")
        t1 = time.perf_counter()
        da, bytes_a = eng.last_run_ms(), pk.pcm.nbytes
        del pk
        eng.set_output_encoding("ulaw")
        t2 = time.perf_counter()
        pk = eng.run_packed(ids, lens, sc, seed=1, lead_samples=lead, wav=True)
        wav_b = bytes(pk.wav)
        t3 = time.perf_counter()
        db = eng.last_run_ms()
        if rep == 0:
            say(f"ragged at {hz} Hz: {B} rows, {pk.total_samples} samples with the breaks; the two files are "
                f"{'identical' if wav_a == wav_b else 'DIFFERENT'}; D2H int16 {bytes_a} B, mu-law {pk.data.nbytes} B; "
                f"host mu-law by {'audioop' if audioop else 'numpy'}")
        del pk
        if rep >= 2:
            for k, v in zip(t, ((t1 - t0) * 1e3, (t3 - t2) * 1e3, da, db)):
                t[k].append(v)
    eng.set_output_encoding("s16le")
    eng.set_output_rate(None)
    say("  host-to-host and device times (ms):")
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
    say(f"encodings_ab: {eng.native.version()}, math {eng.math}, reps {args.reps} (times in ms)")
    headline(eng, cfg, args.reps, say)
    ragged(eng, cfg, args.reps, say)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
