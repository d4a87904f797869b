"""What the true-peak ceiling of the loudness chain costs and does, the sides alternating in ONE process on one device (the numbers
of DESIGN.md §4.14).

  python tools/true_peak_ab.py [--reps 7] [--out FILE]

1. The 48-ragged-sentence request of tools/loudness_ab.py (20 .. 128 ids, natural durations, 250 ms breaks) to ONE WAV at 8 kHz, ids
   in -> file bytes out, with limiter_ms = 5, three ways alternating inside a round: the sample-peak ceiling, the true-peak ceiling,
   and the host route — the float audio of a padded run fetched, tests/loudness_ref.py and tests/true_peak_ref.py in numpy (the
   oversampling, the gain rule, the envelope's curve), re-quantised and re-joined by postprocess.wav_bytes — whose file is compared
   with the true-peak one for equality.  At two settings: loudness = -16 LUFS / ceiling = -1 dB (the synthetic voice is far
   flatter and louder than speech: whether any row of it is over there is printed, not assumed) and a DERIVED target under the same
   ceiling at which it binds on about half the rows in true-peak mode.
   Checked and printed: median(true peak) < median(host route); median(true peak) <= median(sample) + the medians of the
   `truepeak` and `truepeak.env` launches + 2 x (max - min of the sample side).
2. Per over row of the derived setting: the yardstick's true peak of the limited F32LE entry relative to the ceiling, in dB, beside
   what sample mode leaves there — consequence 3 of include/mi355vits.h, a number and not a pass mark.
3. The headline shape (256 rows x 128 ids x 6 forced frames, native rate): the `truepeak` launch and, at the derived setting, the
   `truepeak.env` and `limit` launches from mi355vits_profile_report, as times and as achieved bytes / s and double operations / s
   (126 per sample and oversampled row).
Two untimed warm-up rounds; prints min / median / max over the repetitions.  (The sample-mode numbers against the parent commit's:
tools/ab_prev.py.)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimic3_amd import postprocess as PP  # noqa: E402
from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine, hooks_library, limiter_window  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from tests import limiter_ref as M  # noqa: E402
from tests import loudness_ref as R  # noqa: E402
from tests import true_peak_ref as TP  # noqa: E402

CEILING = -1.0
SPEECH_TARGET = -16.0
WINDOW_MS = 5.0
FLOP_PER_SAMPLE = 126.0  # 63 products and 63 sums


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def derived_target(eng, say):
    """The target at which CEILING binds on half the rows of the last run in true-peak mode: a row is over iff its true peak in dB lies
    more than ceiling - target above its loudness."""
    eng.set_loudness_target(-23.0, CEILING)
    ld, tp = eng.fetch_loudness(), eng.fetch_true_peak()
    ok = np.isfinite(ld.lufs) & (tp.true_peak > 0)
    crest = (tp.dbtp - ld.lufs)[ok]
    excess = (tp.dbtp - 20.0 * np.log10(tp.peak.astype(np.float64)))[ok]
    say(f"  this run's rows: lufs {np.min(ld.lufs):.2f} .. {np.max(ld.lufs):.2f}, true peak over sample peak {excess.min():.2f} .. {excess.max():.2f} dB "
        f"(median {np.median(excess):.2f}), crest factor (dBTP - lufs) {crest.min():.2f} .. {crest.max():.2f} dB, median {np.median(crest):.2f}")
    return max(-69.0, min(-0.5, round(2.0 * (CEILING - float(np.median(crest)))) / 2.0))


def host_route(eng, ids, lens, lead, target, L, h, kw):
    """The true-peak file made on the host: one padded run, its float audio fetched, numpy for the measure, the oversampling, the rule
    and the curve."""
    res = eng.run(ids, lens, [0.667, 1.0, 0.8], want_float=True, seed=1, **kw)
    hz = eng.last_rate
    c = M.ceiling_linear(CEILING)
    chunks = []
    for b in range(len(lens)):
        x = res["audio"][b, : int(res["lengths"][b])]
        lufs = R.measure(x, hz)[0]
        g = 1.0 if np.isinf(lufs) else 10.0 ** ((target - lufs) / 20.0)
        tp = TP.true_peak(x, h)
        over = tp > 0 and c / tp < g
        scale = TP.curve(x, g, c, 32767.0, L, h)[0] if over else np.float32(32767.0 * g)
        chunks += [np.zeros(lead[b], np.int16), R.pcm16_quant(x, scale)]
    return PP.wav_bytes(chunks, hz)


def request(eng, h, ids, lens, reps, say):
    rate = 8000
    eng.set_output_rate(rate)
    L = limiter_window(WINDOW_MS, rate)
    lead = [0] + [int(0.25 * rate)] * (len(lens) - 1)
    pack = dict(lead_samples=lead, wav=True)
    eng.set_loudness_limiter(L)
    eng.run(ids, lens, [0.667, 1.0, 0.8], want_float=False, seed=1)
    say(f"48 ragged sentences to one WAV at {rate} Hz, ceiling {CEILING} dB, limiter window {L} samples ({WINDOW_MS} ms)")
    settings = ((SPEECH_TARGET, ""), (derived_target(eng, say), " (derived)"))
    for target, tag in settings:
        eng.set_loudness_target(target, CEILING)
        over = {}
        for mode in ("sample", "true_peak"):
            eng.set_loudness_ceiling_mode(mode)
            over[mode] = eng.fetch_limiter().engaged
        say(f"  target {target} LUFS{tag}: {int(over['sample'].sum())} of {len(lens)} rows over in sample mode, {int(over['true_peak'].sum())} in true-peak mode")
        t = {k: [] for k in ("sample_ms", "true_peak_ms", "host_ms", "truepeak_kernel_ms", "truepeak.env_kernel_ms")}
        files = {}
        for rep in range(reps + 2):
            for side in ("sample", "true_peak", "host", "true_peak", "sample"):
                if side == "host" and rep not in (0, 1, 2, reps + 1):  # numpy over 48 rows takes seconds: the warm-ups and two timed rounds
                    continue
                eng.set_loudness_ceiling_mode("sample" if side == "host" else side)
                eng.profile_enable(side == "true_peak" and rep % 2 == 1)  # the kernel times from every other round: profiling adds events
                eng.profile_reset()
                t0 = time.perf_counter()
                if side == "host":
                    files[side] = host_route(eng, ids, lens, lead, target, L, h, {})
                else:
                    files[side] = bytes(eng.run_packed(ids, lens, [0.667, 1.0, 0.8], seed=1, **pack).wav)
                ms = (time.perf_counter() - t0) * 1e3
                r = eng.profile_report() if side == "true_peak" and rep % 2 == 1 else {}
                eng.profile_enable(False)
                if rep < 2:
                    continue
                if r:
                    t["truepeak_kernel_ms"].append(r["truepeak"]["ms"])
                    if "truepeak.env" in r:
                        t["truepeak.env_kernel_ms"].append(r["truepeak.env"]["ms"])
                else:
                    t[side + "_ms"].append(ms)
        for k, v in t.items():
            if v:
                say(f"    {k:24s} {_fmt(v)}")
        same = files["host"] == files["true_peak"]
        say(f"    the host-made file and the true-peak run_packed file are {'equal' if same else 'DIFFERENT'} ({len(files['true_peak'])} bytes); "
            f"the sample-mode file is {'equal to' if files['sample'] == files['true_peak'] else 'different from'} the true-peak one")
        if not same:
            raise SystemExit("true_peak_ab: the host-made file differs from the engine's")
        med = {k: statistics.median(v) for k, v in t.items() if v}
        spread = max(t["sample_ms"]) - min(t["sample_ms"])
        kernels = med["truepeak_kernel_ms"] + med.get("truepeak.env_kernel_ms", 0.0)
        say(f"    condition 1: true peak median {med['true_peak_ms']:.4f} < host route median {med['host_ms']:.4f}: "
            f"{'met' if med['true_peak_ms'] < med['host_ms'] else 'NOT met'}")
        bound = med["sample_ms"] + kernels + 2.0 * spread
        say(f"    condition 2: true peak median {med['true_peak_ms']:.4f} <= sample median {med['sample_ms']:.4f} + kernels {kernels:.4f} + 2 x spread "
            f"{spread:.4f} = {bound:.4f}: {'met' if med['true_peak_ms'] <= bound else 'NOT met'}")
    # consequence 3: the true peak of the limited output, per over row of the derived setting
    target = settings[1][0]
    c = M.ceiling_linear(CEILING)
    eng.set_output_encoding("f32le")
    packs = {}
    for mode in ("sample", "true_peak"):
        eng.set_loudness_ceiling_mode(mode)
        packs[mode] = eng.fetch_packed()
    eng.set_output_encoding("s16le")
    say(f"  true peak of the limited F32LE entries over the ceiling, target {target} LUFS (dB; rows over in true-peak mode):")
    worst = {"sample": -np.inf, "true_peak": -np.inf}
    for b in np.nonzero(packs["true_peak"].limited)[0]:
        d = {m: 20.0 * np.log10(TP.true_peak(packs[m].rows[b], h) / c) for m in packs}
        worst = {m: max(worst[m], d[m]) for m in d}
        say(f"    row {int(b):2d}: true-peak mode {d['true_peak']:+.4f}, sample mode {d['sample']:+.4f}{'' if packs['sample'].limited[b] else ' (not over there: uncapped)'}")
    say(f"    worst: true-peak mode {worst['true_peak']:+.4f} dB, sample mode {worst['sample']:+.4f} dB")
    eng.set_loudness_ceiling_mode("sample")
    eng.set_loudness_limiter(0)
    eng.set_loudness_target(None)
    eng.set_output_rate(0)


def headline(eng, ids, lens, reps, say, **kw):
    eng.run(ids, lens, [0.667, 1.0, 0.8], want_float=False, seed=1, **kw)
    hz = eng.last_rate
    lengths = eng.fetch(want_float=False)["lengths"]
    say(f"headline shape: {len(lens)} rows, {int(np.sum(lengths))} samples at {hz} Hz")
    L = limiter_window(WINDOW_MS, hz)
    eng.set_loudness_limiter(L)
    eng.set_loudness_target(derived_target(eng, say), CEILING)
    eng.set_loudness_ceiling_mode("true_peak")
    over = eng.fetch_limiter().engaged
    say(f"  {int(over.sum())} of {len(lens)} rows over in true-peak mode, window {L}")
    t = {k: [] for k in ("truepeak", "truepeak.env", "limit")}
    nbytes = {}
    eng.profile_enable(True)
    for rep in range(reps + 2):
        eng.run(ids, lens, [0.667, 1.0, 0.8], want_float=False, seed=1, **kw)  # a run drops the measurement the host holds
        eng.profile_reset()
        out = eng.fetch_packed(wav=True)
        r = eng.profile_report()
        del out
        if rep < 2:
            continue
        for k in t:
            if k in r:
                t[k].append(r[k]["ms"])
                nbytes[k] = r[k]["bytes"]
    eng.profile_enable(False)
    for k, v in t.items():
        if not v:
            continue
        s = statistics.median(v) * 1e-3
        samples = float(np.sum(lengths)) if k == "truepeak" else float(np.sum(lengths[over]))
        extra = f"  {FLOP_PER_SAMPLE * samples / s / 1e12:.2f} T double op/s" if k != "limit" else ""
        say(f"    {k + '_ms':16s} {_fmt(v)}  {nbytes[k] / s / 1e9:.1f} GB/s of {int(nbytes[k])} B{extra}")
    eng.set_loudness_ceiling_mode("sample")
    eng.set_loudness_limiter(0)
    eng.set_loudness_target(None)


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
    h = hooks_library().lab_true_peak_plan()[0]
    say(f"true_peak_ab: {eng.native.version()}, math {eng.math}, reps {args.reps} (host-to-host times: a host clock around calls that end in a "
        "synchronise; kernel times: HIP events around the launch; ms)")
    say("No real voice is measured here: synthetic weights only.")
    rng = np.random.default_rng(141)
    B = 48
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    request(eng, h, ids, lens, args.reps, say)
    rng = np.random.default_rng(1)
    B, Tx = 256, 128
    headline(eng, rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64), args.reps, say,
             forced_durations=np.full((B, Tx), 6, np.int32))
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
