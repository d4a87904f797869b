"""What a loudness target of the packed streams costs, the sides alternating in ONE process on one device (the numbers of
DESIGN.md §4.11 and §6).

  python tools/loudness_ab.py [--reps 7] [--out FILE]

On the headline shape (256 rows x 128 ids x 6 forced frames, apope_low shapes, synthetic weights) and on 48 ragged rows (20 .. 128
ids, natural durations):
1. the `loudness` launches (k_loud + k_loud_gate) from mi355vits_profile_report beside `edges`, `align` with levels and `pcm16.pack`
   (k_pack<S16>, csrc/kernels_pack.cpp) of the same run, and `pcm16.pack` with the scale row (k_pack<S16, .., NORM>) against
   without from one synthesis; `loudness` also as bytes / s and as a
   share of mi355vits_last_run_ms;
2. host to host, 250 ms breaks, ids in -> file bytes out: run_packed(wav=True) with the target off (bit for bit what it was before
   the setting existed) against loudness = -23 LUFS, and against the host route — run_packed, the float audio fetched, the
   measurement of tests/loudness_ref.py in numpy, the gain rule, re-quantise, re-join, postprocess.wav_bytes — with the two files
   compared for equality; and fetch_alignment (timing only) on such a run, the project's own measured price of one more
   synchronisation and small copy.
Two untimed warm-up rounds; prints min / median / max over the repetitions.  The two conditions it checks and prints, on the
48-sentence leg: median(normalised) <= median(un-normalised) + (max - min of that side) + 2 x median(fetch_alignment), and
median(normalised) < median(host route)."""
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
from tests import loudness_ref as R  # noqa: E402

TARGET, CEILING = -23.0, -1.0


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def host_normalise(eng, ids, lens, lead, kw):
    """The same file made on the host: one un-normalised run_packed, the float audio of that run, numpy for the measure and the rule."""
    eng.run_packed(ids, lens, [0.667, 1.0, 0.8], seed=1, **kw)
    res = eng.fetch(want_float=True)
    hz = eng.last_rate
    chunks = []
    for b in range(len(lens)):
        x = res["audio"][b, : int(res["lengths"][b])]
        gain, _ = R.gain_rule(R.measure(x, hz)[0], res["peaks"][b], TARGET, CEILING)
        chunks += [np.zeros(lead[b], np.int16), R.pcm16_quant(x, np.float32(32767.0 * gain))]
    return PP.wav_bytes(chunks, hz)


def measure(eng, name, ids, lens, reps, say, check, **kw):
    lead = [0] + [int(0.25 * eng.config.sample_rate)] * (len(lens) - 1)  # a 250 ms break between sentences
    pack = dict(lead_samples=lead, wav=True)
    keys = ("loudness_ms", "edges_ms", "align.levels_ms", "pack_ms", "pack.scaled_ms")
    h2h_keys = ("run_packed_ms", "run_packed.loudness_ms", "run_packed+host_ms", "fetch_alignment_ms")
    t = {k: [] for k in keys + h2h_keys}
    share, rate_gbs = [], []
    for rep in range(reps + 2):  # two untimed warm-up rounds
        # (1) the kernels of ONE synthesis: the plain pack, align with levels, edges, then loudness + the scaled pack
        eng.set_loudness_target(None)
        eng.set_edge_trim(0.0)
        eng.profile_enable(True)
        eng.profile_reset()
        plain = eng.run_packed(ids, lens, [0.667, 1.0, 0.8], seed=1, **pack, **kw)
        run_ms = eng.last_run_ms()
        ms = {"pack_ms": eng.profile_report()["pcm16.pack"]["ms"]}
        eng.profile_reset()
        eng.fetch_alignment(levels=True)
        ms["align.levels_ms"] = eng.profile_report()["align"]["ms"]
        eng.set_edge_trim(float(np.float32(0.01)), 0)
        eng.profile_reset()
        eng.fetch_edges()
        ms["edges_ms"] = eng.profile_report()["edges"]["ms"]
        eng.set_edge_trim(0.0)
        eng.set_loudness_target(TARGET, CEILING)
        eng.profile_reset()
        scaled = eng.fetch_packed(**pack)
        rep_ = eng.profile_report()
        ms["loudness_ms"] = rep_["loudness"]["ms"]
        ms["pack.scaled_ms"] = rep_["pcm16.pack"]["ms"]
        eng.profile_enable(False)
        if rep == 0:
            say(f"{name}: {len(lens)} rows, {int(np.sum(plain.lengths))} samples, {int(rep_['loudness']['bytes'])} B moved by loudness; "
                f"lufs {np.min(scaled.lufs):.2f} .. {np.max(scaled.lufs):.2f}, gain {np.min(scaled.gain):.3f} .. {np.max(scaled.gain):.3f}, "
                f"{int(np.sum(scaled.limited))} rows limited")
        nbytes = rep_["loudness"]["bytes"]
        del plain, scaled
        # (2) host to host, the sides alternating inside a round
        h2h = {k: [] for k in h2h_keys}
        last_on = None
        for side in ("off", "on", "host", "on", "off") if check else ("off", "on", "on", "off"):  # the host route on the 48 sentences only
            eng.set_loudness_target(TARGET if side == "on" else None, CEILING)
            t0 = time.perf_counter()
            if side == "host":
                wav = host_normalise(eng, ids, lens, lead, kw)
                h2h["run_packed+host_ms"].append((time.perf_counter() - t0) * 1e3)
                same = wav == last_on
                if rep == 0:
                    say(f"  the host-made file and the normalised run_packed file are {'equal' if same else 'DIFFERENT'} ({len(wav)} bytes)")
                if not same:
                    raise SystemExit("loudness_ab: the host-made file differs from the engine's")
                t0 = time.perf_counter()
                eng.fetch_alignment()
                h2h["fetch_alignment_ms"].append((time.perf_counter() - t0) * 1e3)
                continue
            out = eng.run_packed(ids, lens, [0.667, 1.0, 0.8], seed=1, **pack, **kw)
            h2h["run_packed.loudness_ms" if side == "on" else "run_packed_ms"].append((time.perf_counter() - t0) * 1e3)
            if side == "on":
                last_on = bytes(out.wav)
            del out
        if rep >= 2:
            for k, v in ms.items():
                t[k].append(v)
            for k, v in h2h.items():
                t[k].extend(v)
            share.append(ms["loudness_ms"] / run_ms)
            rate_gbs.append(nbytes / (ms["loudness_ms"] * 1e-3) / 1e9)
    eng.set_loudness_target(None)
    say("  kernel times (ms, HIP events around the launch):")
    for k in keys:
        say(f"  {k:24s} {_fmt(t[k])}")
    say(f"  loudness: median {statistics.median(rate_gbs):.1f} GB/s, {100.0 * statistics.median(share):.3f} % of last_run_ms")
    say("  host to host (ms):")
    for k in h2h_keys:
        if t[k]:
            say(f"  {k:24s} {_fmt(t[k])}")
    if check:
        off, on, al, host = t["run_packed_ms"], t["run_packed.loudness_ms"], t["fetch_alignment_ms"], t["run_packed+host_ms"]
        bound = statistics.median(off) + (max(off) - min(off)) + 2.0 * statistics.median(al)
        met = statistics.median(on) <= bound
        say(f"  condition 1: normalised median {statistics.median(on):.4f} <= un-normalised median {statistics.median(off):.4f} + spread "
            f"{max(off) - min(off):.4f} + 2 x fetch_alignment median {statistics.median(al):.4f} = {bound:.4f}: {'MET' if met else 'MISSED'}")
        met2 = statistics.median(on) < statistics.median(host)
        say(f"  condition 2: normalised median {statistics.median(on):.4f} < host route median {statistics.median(host):.4f}: "
            f"{'MET' if met2 else 'MISSED'}")


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
    say(f"loudness_ab: {eng.native.version()}, math {eng.math}, reps {args.reps}, target {TARGET} LUFS, ceiling {CEILING} dBFS (times in ms)")
    rng = np.random.default_rng(1)
    B, Tx = 256, 128
    measure(eng, "headline shape", rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64), args.reps, say, False,
            forced_durations=np.full((B, Tx), 6, np.int32))
    rng = np.random.default_rng(141)
    B = 48
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    measure(eng, "48 ragged sentences", ids, lens, args.reps, say, True)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
