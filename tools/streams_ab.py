"""Several streams per run against the single-stream path, both sides alternating in ONE process on one device (the numbers of
DESIGN.md §4.12).

  python tools/streams_ab.py [--reps 7] [--seconds 4] [--rounds 3] [--out FILE]

(a) Kernel, device events (mi355vits_profile_report), after ONE synthesis per shape, every side a fetch of that run:
    `pack.streams` with one stream against `pcm16.pack` / `pack.ulaw` (k_pack, unchanged) at the headline shape (256 rows x
    196,608 samples) and on 48 ragged rows; then 256 streams (the headline shape: one row each; ragged: 48 streams) to show what
    stream boundaries cost.  Both kernels move the same bytes with the same one-writer structure: the expected ratio is 1.
(b) Serving: 64 closed-loop clients, one ragged sentence per call, each wanting a WAV file — s16le at the native rate, and mu-law
    at 8000 Hz.  Today's route: run_pcm16 through the micro-batcher + postprocess.wav_bytes (+ lin2ulaw) on the client thread; the
    new route: run_stream (the file is a view of the batch's block).  Sentences/s, p50 / p99 of a call, device-to-host bytes per batch.
Prints min / median / max over the repetitions; nothing is asserted."""
import argparse
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimic3_amd import postprocess as PP  # noqa: E402
from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from mimic3_amd.session import InferenceSession, SessionOptions  # noqa: E402

LABEL = {"s16le": "pcm16.pack", "ulaw": "pack.ulaw"}


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


def kernel_ab(eng, name, B, reps, say):
    """One run is on the handle; every side below is a fetch of it."""
    t = {}
    for rep in range(reps + 2):  # two untimed warm-up rounds
        for enc in ("s16le", "ulaw"):
            sides = []
            eng.set_output_encoding(enc)
            eng.profile_reset()
            pk = eng.fetch_packed()
            sides.append((f"{LABEL[enc]:12s} k_pack, one stream", eng.profile_report()[LABEL[enc]]))
            eng.profile_reset()
            one = eng.fetch_streams([dict(encoding=enc)])
            sides.append((f"pack.streams {enc}, one stream", eng.profile_report()["pack.streams"]))
            eng.profile_reset()
            many = eng.fetch_streams([dict(order=[b], encoding=enc) for b in range(B)])
            sides.append((f"pack.streams {enc}, {B} streams of one row", eng.profile_report()["pack.streams"]))
            if rep == 0:
                assert one[0].data.tobytes() == pk.data.tobytes()
                assert b"".join(m.data.tobytes() for m in many) == pk.data.tobytes()
                say(f"  {name} {enc}: {pk.data.nbytes} B in one stream, block of {B} streams {many[0].block.nbytes} B; bytes moved per launch {sides[0][1]['bytes']:.0f}")
            del pk, one, many
            if rep >= 2:
                for k, r in sides:
                    t.setdefault(k, []).append(r["ms"])
    eng.set_output_encoding("s16le")
    for k, v in t.items():
        say(f"    {k:44s} {_fmt(v)}")
    for enc in ("s16le", "ulaw"):
        base = t[f"{LABEL[enc]:12s} k_pack, one stream"]
        spread = (max(base) - min(base)) / statistics.median(base)
        for k in (f"pack.streams {enc}, one stream", f"pack.streams {enc}, {B} streams of one row"):
            say(f"    ratio {k} / k_pack (medians): {statistics.median(t[k]) / statistics.median(base):.3f}   (k_pack's own min-max spread {100 * spread:.1f} %)")


def kernel(cfg, blob, reps, say):
    eng = Engine(blob, device=0)
    eng.profile_enable(True)
    say("(a) kernel: device events around the one launch, ms")
    B, Tx = 256, 128
    rng = np.random.default_rng(1)
    eng.run(rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64), [0.667, 1.0, 0.8], forced_durations=np.full((B, Tx), 6, np.int32),
            seed=1, want_float=False, device_only=True)
    kernel_ab(eng, "headline (256 rows x 196,608 samples)", B, reps, say)
    ids, lens = _ragged_ids(cfg, 48)
    eng.run(ids, lens, [0.667, 1.0, 0.8], seed=1, want_float=False, device_only=True)
    kernel_ab(eng, "48 ragged rows", 48, reps, say)
    eng.close()


def serve(sess, route, encoding, rate, sentences, seconds, clients=64):
    """`clients` closed-loop threads for `seconds`: (sentences/s, latencies in ms, D2H bytes per engine call)."""
    d2h = []
    inner = sess._engine_run

    def spy(*a, **kw):
        out = inner(*a, **kw)
        d2h.append(out[0].block.nbytes if isinstance(out, list) else out["pcm"].nbytes)
        return out

    sess._engine_run = spy
    lat, done = [[] for _ in range(clients)], [0] * clients
    stop = time.perf_counter() + seconds
    scales = np.array([0.667, 1.0, 0.8], np.float32)

    def client(c):
        i = c
        while time.perf_counter() < stop:
            ids = sentences[i % len(sentences)]
            feed = {"input": ids[None, :], "input_lengths": np.array([ids.shape[0]], np.int64), "scales": scales}
            t0 = time.perf_counter()
            if route == "run_stream":
                wav = sess.run_stream(feed, wav=True, encoding=encoding, sample_rate=rate).wav
            else:
                rows, _ = sess.run_pcm16(feed, sample_rate=rate)
                row = PP.lin2ulaw(rows[0]) if encoding == "ulaw" else rows[0]
                wav = PP.wav_bytes([row], rate or sess.config.sample_rate, encoding)
            lat[c].append((time.perf_counter() - t0) * 1e3)
            done[c] += 1
            i += clients
            del wav

    ts = [threading.Thread(target=client, args=(c,)) for c in range(clients)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    wall = time.perf_counter() - t0
    sess._engine_run = inner
    return sum(done) / wall, [x for l in lat for x in l], d2h


def serving(cfg, blob, seconds, rounds, say):
    say("(b) serving: 64 closed-loop clients, one ragged sentence (20 .. 128 ids) per call, a WAV file per call; 2 lanes")
    so = SessionOptions()
    so.lanes = 2
    so.micro_batch_window_ms = 2.0
    so.micro_batch_max = 64
    so.seed = 1
    sess = InferenceSession(blob, sess_options=so)
    ids, lens = _ragged_ids(cfg, 256, seed=9)
    sentences = [ids[b, : int(lens[b])].copy() for b in range(256)]
    for form, (enc, rate) in {"s16le at the native rate": ("s16le", None), "mu-law at 8000 Hz": ("ulaw", 8000)}.items():
        feed = {"input": sentences[0][None, :], "input_lengths": np.array([sentences[0].shape[0]], np.int64), "scales": np.array([0.0, 1.0, 0.0], np.float32)}
        rows, _ = sess.run_pcm16(feed, sample_rate=rate)
        row = PP.lin2ulaw(rows[0]) if enc == "ulaw" else rows[0]
        assert PP.wav_bytes([row], rate or cfg.sample_rate, enc) == bytes(sess.run_stream(feed, wav=True, encoding=enc, sample_rate=rate).wav)
        res = {"run_pcm16 + wav_bytes": [], "run_stream": []}
        for r in range(rounds + 1):  # one untimed warm-up round
            for route in res:
                out = serve(sess, route, enc, rate, sentences, seconds if r else min(seconds, 1.5))
                if r:
                    res[route].append(out)
        say(f"  {form}:")
        for route, outs in res.items():
            lat = np.concatenate([np.asarray(o[1]) for o in outs])
            d2h = np.concatenate([np.asarray(o[2], np.float64) for o in outs])
            say(f"    {route:22s} sentences/s {_fmt([o[0] for o in outs])}   p50 {np.percentile(lat, 50):.1f} ms  p99 {np.percentile(lat, 99):.1f} ms   "
                f"D2H per batch {d2h.mean() / 1e6:.3f} MB over {len(d2h)} batches")
        a, b = [o[0] for o in res["run_pcm16 + wav_bytes"]], [o[0] for o in res["run_stream"]]
        say(f"    run_stream / today (medians): {statistics.median(b) / statistics.median(a):.3f}; today's own min-max spread {100 * (max(a) - min(a)) / statistics.median(a):.1f} %, "
            f"run_stream's {100 * (max(b) - min(b)) / statistics.median(b):.1f} %")
    sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-serving", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = VitsConfig.apope_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0))
    say(f"streams_ab: reps {args.reps}, serving {args.rounds} rounds x {args.seconds} s per route")
    kernel(cfg, blob, args.reps, say)
    if not args.skip_serving:
        serving(cfg, blob, args.seconds, args.rounds, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
