"""What edge trimming of the packed streams costs, the sides alternating in ONE process on one device (the numbers of DESIGN.md §4.10).

  python tools/edge_trim_ab.py [--reps 7] [--out FILE]

On the headline shape (256 rows x 128 ids x 6 forced frames, apope_low shapes, synthetic weights) and on 48 ragged rows (20 .. 128
ids, natural durations):
1. the `edges` kernel from mi355vits_profile_report beside `align` with levels and `pcm16.pack` (k_pack<S16>, csrc/kernels_pack.cpp)
   of the same run, and `pcm16.pack` trimmed (k_pack<S16, TRIM>; at -40 dB with 10 ms kept, and at ratio 0.9, which cuts these
   noise-like voices deeply) against untrimmed from one synthesis;
2. host to host: run_packed(wav=True) with trimming off against trimming on at -40 dB with 10 ms kept, and against both the same rule
   on the host — run_packed, the float audio fetched, numpy finds each row's edges, slices and re-joins, postprocess.wav_bytes frames —
   with the two files compared for equality; and fetch_alignment (timing only) on such a run, the project's own measured price of
   one more synchronisation and small copy.
Two untimed warm-up rounds; prints min / median / max over the repetitions.  The condition it checks and prints, on the 48-sentence
leg: median(trimmed run_packed) <= median(untrimmed run_packed) + (max - min of the untrimmed side) + median(fetch_alignment)."""
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

DB, KEEP_MS = -40.0, 10.0


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def host_trim(eng, ids, lens, ratio, keep, lead, kw):
    """The same file made on the host: one untrimmed run_packed, the float audio of that run, numpy for the rule."""
    pk = eng.run_packed(ids, lens, [0.667, 1.0, 0.8], seed=1, **kw)
    res = eng.fetch(want_float=True)
    chunks = []
    for b in range(len(lens)):
        n = int(res["lengths"][b])
        loud = np.flatnonzero(np.abs(res["audio"][b, :n]) >= np.float32(res["peaks"][b]) * np.float32(ratio))
        first, end = max(0, int(loud[0]) - keep), min(n, int(loud[-1]) + 1 + keep)
        chunks += [np.zeros(lead[b], np.int16), pk.rows[b][first:end]]
    return PP.wav_bytes(chunks, eng.last_rate)


def measure(eng, name, ids, lens, reps, say, check, **kw):
    ratio = float(np.float32(10.0 ** (DB / 20.0)))
    keep = int((KEEP_MS / 1000.0) * eng.config.sample_rate)
    lead = [0] + [int(0.25 * eng.config.sample_rate)] * (len(lens) - 1)  # a 250 ms break between sentences
    pack = dict(lead_samples=lead, wav=True)
    keys = ("edges_ms", "align.levels_ms", "pack_ms", "pack.trimmed_ms", "edges@0.9_ms", "pack.trimmed@0.9_ms")
    h2h_keys = ("run_packed_ms", "run_packed.trimmed_ms", "run_packed+host_ms", "fetch_alignment_ms")
    t = {k: [] for k in keys + h2h_keys}
    for rep in range(reps + 2):  # two untimed warm-up rounds
        # (1) the kernels of ONE synthesis: the untrimmed pack, align with levels, then edges + the trimmed pack at two thresholds
        eng.set_edge_trim(0.0)
        eng.profile_enable(True)
        eng.profile_reset()
        plain = eng.run_packed(ids, lens, [0.667, 1.0, 0.8], seed=1, **pack, **kw)
        ms = {"pack_ms": eng.profile_report()["pcm16.pack"]["ms"]}
        eng.profile_reset()
        eng.fetch_alignment(levels=True)
        ms["align.levels_ms"] = eng.profile_report()["align"]["ms"]
        for r, k, suffix in ((ratio, keep, ""), (0.9, 0, "@0.9")):
            eng.set_edge_trim(r, k)
            eng.profile_reset()
            cut = eng.fetch_packed(**pack)
            rep_ = eng.profile_report()
            ms["edges" + suffix + "_ms"] = rep_["edges"]["ms"]
            ms["pack.trimmed" + suffix + "_ms"] = rep_["pcm16.pack"]["ms"]
            if rep == 0:
                say(f"  ratio {r:.6g} keep {k}: {cut.total_samples} of {plain.total_samples} stream samples stay, "
                    f"{int(rep_['edges']['bytes'])} B moved by edges")
        eng.profile_enable(False)
        if rep == 0:
            say(f"{name}: {len(lens)} rows, {int(np.sum(plain.lengths))} samples")
        del plain, cut
        # (2) host to host, the sides alternating inside a round
        h2h = {k: [] for k in h2h_keys}
        last_on = None
        for side in ("off", "on", "host", "on", "off"):
            eng.set_edge_trim(ratio if side == "on" else 0.0, keep if side == "on" else 0)
            t0 = time.perf_counter()
            if side == "host":
                wav = host_trim(eng, ids, lens, ratio, keep, lead, kw)
                h2h["run_packed+host_ms"].append((time.perf_counter() - t0) * 1e3)
                same = wav == last_on
                if rep == 0:
                    say(f"  the host-made file and the trimmed run_packed file are {'equal' if same else 'DIFFERENT'} ({len(wav)} bytes)")
                if not same:
                    raise SystemExit("edge_trim_ab: the host-made file differs from the engine's")
                t0 = time.perf_counter()
                eng.fetch_alignment()
                h2h["fetch_alignment_ms"].append((time.perf_counter() - t0) * 1e3)
                continue
            out = eng.run_packed(ids, lens, [0.667, 1.0, 0.8], seed=1, **pack, **kw)
            h2h["run_packed.trimmed_ms" if side == "on" else "run_packed_ms"].append((time.perf_counter() - t0) * 1e3)
            if side == "on":
                last_on = bytes(out.wav)
            del out
        if rep >= 2:
            for k, v in ms.items():
                t[k].append(v)
            for k, v in h2h.items():
                t[k].extend(v)
    eng.set_edge_trim(0.0)
    say("  kernel times (ms, HIP events around the launch):")
    for k in keys:
        say(f"  {k:24s} {_fmt(t[k])}")
    say("  host to host (ms):")
    for k in h2h_keys:
        say(f"  {k:24s} {_fmt(t[k])}")
    if check:
        off, on, al = t["run_packed_ms"], t["run_packed.trimmed_ms"], t["fetch_alignment_ms"]
        bound = statistics.median(off) + (max(off) - min(off)) + statistics.median(al)
        met = statistics.median(on) <= bound
        say(f"  condition: trimmed median {statistics.median(on):.4f} <= untrimmed median {statistics.median(off):.4f} + spread "
            f"{max(off) - min(off):.4f} + fetch_alignment median {statistics.median(al):.4f} = {bound:.4f}: {'MET' if met else 'MISSED'}")
        if not met:
            say(f"  where the time went: edges {statistics.median(t['edges_ms']):.4f} ms on the device; the rest of "
                f"{statistics.median(on) - statistics.median(off):.4f} ms is the second synchronisation, the 8 B byte copy, the table's own "
                "upload (an untrimmed run_packed sends it with the per-stage lengths) and the edges of the result fetched for PackedAudio.first / .end")


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
    say(f"edge_trim_ab: {eng.native.version()}, math {eng.math}, reps {args.reps}, trim {DB} dB with {KEEP_MS} ms kept (times in ms)")
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
