"""The packed stream as FLAC against the S16LE stream it compresses, the sides alternating on ONE handle in one process on one device
(the numbers of DESIGN.md §4.15).

  python tools/flac_ab.py [--reps 7] [--out profiles/flac_ab.txt]

For each of three requests — the headline shape (256 rows x 128 ids x 6 forced frames), and 48 ragged rows (20 .. 128 ids, natural
durations, 250 ms breaks) at the voice's rate and at 8000 Hz — one synthesis per round (apope_low shapes, synthetic weights), then
mi355vits_fetch_packed as S16LE and as FLAC of that same run:
  * the `pack.flac` kernel time (k_flac_frames + k_flac_scan + k_flac_gather) and the `pcm16.pack` time in front of it, from
    mi355vits_profile_report (HIP events around the launches);
  * n_bytes / (2 * total_samples);
  * host-to-host time of fetch_packed as FLAC against fetch_packed as S16LE (profiler off).
The synthetic voices are NOT speech: their waveform is close to noise, so the ratio here says how the encoder treats noise and digital
silence, not what a trained voice compresses to.  Two untimed warm-up rounds; min / median / max over the repetitions; nothing is
asserted — the record is the deliverable."""
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


def measure(eng, name, synthesize, pack, reps, say):
    t = {k: [] for k in ("pack.flac_ms", "pcm16.pack_ms", "fetch_flac_host_ms", "fetch_s16le_host_ms")}
    for rep in range(reps + 2):  # two untimed warm-up rounds
        synthesize()
        row = {}
        eng.profile_enable(True)  # the kernel times: one fetch each, the sides alternating inside a round
        eng.profile_reset()
        fl = eng.fetch_packed(compression="flac", **pack)
        r = eng.profile_report()
        row["pack.flac_ms"], row["pcm16.pack_ms"] = r["pack.flac"]["ms"], r["pcm16.pack"]["ms"]
        eng.profile_enable(False)
        n_flac, total = len(fl.flac), fl.total_samples
        del fl
        for key, comp in (("fetch_s16le_host_ms", None), ("fetch_flac_host_ms", "flac")):  # host to host, profiler off
            t0 = time.perf_counter()
            pk = eng.fetch_packed(compression=comp, **pack)
            row[key] = (time.perf_counter() - t0) * 1e3
            del pk
        if rep == 0:
            say(f"{name}: {total} samples at {eng.output_rate} Hz, {-(-total // 4096)} frames; S16LE {2 * total} B, FLAC {n_flac} B, "
                f"n_bytes / (2 * total_samples) = {n_flac / (2 * total):.4f}  (synthetic voice: not speech)")
        if rep >= 2:
            for k, v in row.items():
                t[k].append(v)
    for k, v in t.items():
        say(f"  {k:20s} {_fmt(v)}")


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
    say(f"flac_ab: {eng.native.version()}, math {eng.math}, reps {args.reps} (times in ms)")
    sc = [0.667, 1.0, 0.8]
    B, Tx = 256, 128
    rng = np.random.default_rng(1)
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    lens = np.full(B, Tx, np.int64)
    forced = np.full((B, Tx), 6, np.int32)
    measure(eng, "headline shape (256 rows x 128 ids x 6 frames)",
            lambda: eng.run(ids, lens, sc, forced_durations=forced, seed=1, device_only=True, want_float=False), {}, args.reps, say)
    rb = 48
    rng = np.random.default_rng(141)
    rlens = rng.integers(20, 129, rb).astype(np.int64)
    rlens[0], rlens[rb // 2] = 128, 20
    rids = np.zeros((rb, 128), np.int64)
    for b in range(rb):
        rids[b, : rlens[b]] = rng.integers(1, cfg.num_symbols, size=int(rlens[b]))
    for hz in (None, 8000):
        eng.set_output_rate(hz)
        lead = [0] + [int(250.0 / 1000.0 * eng.output_rate)] * (rb - 1)
        measure(eng, f"48 ragged rows with 250 ms breaks at {'the native rate' if hz is None else '8000 Hz'}",
                lambda: eng.run(rids, rlens, sc, seed=1, device_only=True, want_float=False), dict(lead_samples=lead), args.reps, say)
    eng.set_output_rate(None)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
