"""Streams v2 (compression, limiter window and ceiling mode per stream) against what exists, the sides alternating in ONE process on
one handle and one device (the numbers of DESIGN.md §4.16).

  python tools/streams2_ab.py [--reps 7] [--seconds 3] [--rounds 2] [--out profiles/streams2_ab.txt]

(a) A v2 call that uses no new field against the v1 call on the same run — the same launches, so expected equal —, at the headline
    shape (256 rows x 196,608 samples) and on 48 ragged rows: the wall time of the fetch and the device time of `pack.streams`.
    v1 is measured twice per round: "equal" means inside the spread of v1 against itself.
(b) 64 one-row FLAC streams in one block (one `fetch_streams`) against 64 `fetch_packed(compression="flac")` calls on the same run —
    the only way to per-client FLAC before —, wall time; and `pack.flac` of the block against the single pack's `pack.flac` for the
    same total samples (one stream of the same 64 rows), device time.
(c) Serving: 64 closed-loop clients, one ragged sentence per call, each wanting a FLAC file: `run_request` (shared calls) against
    `run_packed(compression="flac")` per client.  Sentences/s and p50 / p99 of a call.
Prints min / median / max over the repetitions; nothing is asserted.  The synthetic voices are near-noise: the sizes say nothing about
speech."""
import argparse
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from mimic3_amd.session import InferenceSession, SessionOptions  # noqa: E402


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def _ragged_ids(cfg, B, seed=141):
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    return ids, lens


def _timed(eng, fn, label):
    eng.profile_reset()
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    rep = eng.profile_report()
    return out, wall, (rep[label]["ms"] if label in rep else 0.0)


def v1_against_v2(eng, name, B, reps, say):
    """(a): one run is on the handle; every side is a fetch of it."""
    v1 = [dict(order=[b], wav=True) for b in range(B)]
    v2 = [dict(st, compression=None, limiter=0, true_peak=False) for st in v1]
    t = {}
    for rep in range(reps + 2):  # two untimed warm-up rounds
        sides = []
        for label, streams in (("v1 (first)", v1), ("v2, no new field", v2), ("v1 (second)", v1)):
            got, wall, dev = _timed(eng, lambda: eng.fetch_streams(streams), "pack.streams")
            sides.append((label, wall, dev, got[0].block.tobytes() if rep == 0 else None))
            del got
        if rep == 0:
            assert sides[0][3] == sides[1][3] == sides[2][3]
            say(f"  {name}: {B} WAV streams of one row, block of {len(sides[0][3])} B")
        if rep >= 2:
            for label, wall, dev, _ in sides:
                t.setdefault(label + " wall ms", []).append(wall)
                t.setdefault(label + " pack.streams ms", []).append(dev)
    for k in sorted(t):
        say(f"    {k:36s} {_fmt(t[k])}")
    for what in ("wall ms", "pack.streams ms"):
        a, b, c = (statistics.median(t[f"{k} {what}"]) for k in ("v1 (first)", "v2, no new field", "v1 (second)"))
        say(f"    {what}: v2 / v1 (medians) {b / a:.3f}; v1 (second) / v1 (first) {c / a:.3f}")


def block_against_calls(eng, name, rows, reps, say):
    """(b): 64 one-row FLAC files of the run on the handle."""
    streams = [dict(order=[b], compression="flac") for b in rows]
    t = {}
    for rep in range(reps + 2):
        block, w_block, d_block = _timed(eng, lambda: eng.fetch_streams(streams), "pack.flac")
        calls, w_calls, _ = _timed(eng, lambda: [eng.fetch_packed(order=[b], compression="flac") for b in rows], "pack.flac")
        one, w_one, d_one = _timed(eng, lambda: eng.fetch_packed(order=list(rows), compression="flac"), "pack.flac")
        if rep == 0:
            assert all(bytes(a.flac) == bytes(b.flac) for a, b in zip(block, calls))
            say(f"  {name}: {len(rows)} files, {sum(a.total_samples for a in block)} samples, {sum(a.frames for a in block)} frames, "
                f"{sum(a.stream_bytes for a in block)} B compressed (one file of the same rows: {len(one.flac)} B)")
        del block, calls, one
        if rep >= 2:
            for k, v in (("one block of 64 streams, wall ms", w_block), ("64 fetch_packed calls, wall ms", w_calls), ("one pack of the 64 rows, wall ms", w_one),
                         ("pack.flac of the block, device ms", d_block), ("pack.flac of the one pack, device ms", d_one)):
                t.setdefault(k, []).append(v)
    for k, v in t.items():
        say(f"    {k:40s} {_fmt(v)}")
    m = {k: statistics.median(v) for k, v in t.items()}
    say(f"    64 calls / one block (wall, medians): {m['64 fetch_packed calls, wall ms'] / m['one block of 64 streams, wall ms']:.2f}x; "
        f"pack.flac block / single pack (device, medians): {m['pack.flac of the block, device ms'] / m['pack.flac of the one pack, device ms']:.3f}")


def kernel(cfg, blob, reps, say):
    eng = Engine(blob, device=0)
    eng.profile_enable(True)
    B, Tx = 256, 128
    rng = np.random.default_rng(1)
    eng.run(rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64), [0.667, 1.0, 0.8], forced_durations=np.full((B, Tx), 6, np.int32),
            seed=1, want_float=False, device_only=True)
    say("(a) a v2 call without a new field against v1, same run, ms")
    v1_against_v2(eng, "headline (256 rows x 196,608 samples)", B, reps, say)
    say("(b) 64 one-row FLAC streams in one block against 64 fetch_packed calls, same run, ms")
    block_against_calls(eng, "headline rows 0 .. 63", range(64), reps, say)
    ids, lens = _ragged_ids(cfg, 64)
    eng.run(ids, lens, [0.667, 1.0, 0.8], seed=1, want_float=False, device_only=True)
    block_against_calls(eng, "64 ragged rows", range(64), reps, say)
    ids, lens = _ragged_ids(cfg, 48)
    eng.run(ids, lens, [0.667, 1.0, 0.8], seed=1, want_float=False, device_only=True)
    say("(a) on 48 ragged rows")
    v1_against_v2(eng, "48 ragged rows", 48, reps, say)
    eng.close()


def serve(sess, route, sentences, seconds, clients=64):
    lat, done = [[] for _ in range(clients)], [0] * clients
    stop = time.perf_counter() + seconds
    scales = np.array([0.667, 1.0, 0.8], np.float32)
    call = sess.run_request if route == "run_request" else sess.run_packed

    def client(c):
        i = c
        while time.perf_counter() < stop:
            ids = sentences[i % len(sentences)]
            feed = {"input": ids[None, :], "input_lengths": np.array([ids.shape[0]], np.int64), "scales": scales}
            t0 = time.perf_counter()
            file = call(feed, compression="flac").flac
            lat[c].append((time.perf_counter() - t0) * 1e3)
            done[c] += 1
            i += clients
            del file

    ts = [threading.Thread(target=client, args=(c,)) for c in range(clients)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return sum(done) / (time.perf_counter() - t0), [x for l in lat for x in l]


def serving(cfg, blob, seconds, rounds, say):
    say("(c) serving: 64 closed-loop clients, one ragged sentence (20 .. 128 ids) per call, a FLAC file per call; 2 lanes")
    so = SessionOptions()
    so.lanes = 2
    so.micro_batch_window_ms = 2.0
    so.micro_batch_max = 64
    so.seed = 1
    sess = InferenceSession(blob, sess_options=so)
    ids, lens = _ragged_ids(cfg, 256, seed=9)
    sentences = [ids[b, : int(lens[b])].copy() for b in range(256)]
    feed = {"input": sentences[0][None, :], "input_lengths": np.array([sentences[0].shape[0]], np.int64), "scales": np.array([0.0, 1.0, 0.0], np.float32)}
    assert bytes(sess.run_request(feed, compression="flac").flac) == bytes(sess.run_packed(feed, compression="flac").flac)
    res = {"run_packed per client": [], "run_request": []}
    for r in range(rounds + 1):  # one untimed warm-up round
        for route in res:
            out = serve(sess, route, sentences, seconds if r else min(seconds, 1.5))
            if r:
                res[route].append(out)
    for route, outs in res.items():
        lat = np.concatenate([np.asarray(o[1]) for o in outs])
        say(f"    {route:22s} sentences/s {_fmt([o[0] for o in outs])}   p50 {np.percentile(lat, 50):.1f} ms  p99 {np.percentile(lat, 99):.1f} ms")
    a, b = [o[0] for o in res["run_packed per client"]], [o[0] for o in res["run_request"]]
    say(f"    run_request / run_packed per client (medians): {statistics.median(b) / statistics.median(a):.3f}; spreads "
        f"{100 * (max(a) - min(a)) / statistics.median(a):.1f} % and {100 * (max(b) - min(b)) / statistics.median(b):.1f} %")
    mb = sess._batcher
    say(f"    micro-batcher: {mb.requests} requests in {mb.batches} calls")
    sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip-serving", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = VitsConfig.apope_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0))
    say(f"streams2_ab: reps {args.reps}, serving {args.rounds} rounds x {args.seconds} s per route")
    kernel(cfg, blob, args.reps, say)
    if not args.skip_serving:
        serving(cfg, blob, args.seconds, args.rounds, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
