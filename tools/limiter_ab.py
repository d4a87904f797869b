"""What the look-ahead peak limiter of the packed streams costs and does, the sides alternating in ONE process on one device (the
numbers of DESIGN.md §4.13).

  python tools/limiter_ab.py [--reps 7] [--out FILE] [--parent-root DIR]

On the headline shape (256 rows x 128 ids x 6 forced frames, apope_low shapes, synthetic weights) and on 48 ragged rows (20 .. 128
ids, natural durations), from ONE synthesis each:
1. per setting — the speech targets -16 LUFS / -1 dBFS and -14 LUFS / -2 dBFS, and a DERIVED one (the ceiling of -1 dBFS under the
   target at which it binds on half the rows of this run: the synthetic voice is far flatter and louder than speech, so at the speech
   targets no row of it is over and the limiter has nothing to do) — and per window (5 ms and the largest, 4,096 samples): how many
   rows are over, the sum of reduced_samples and the smallest min_scale (mi355vits_fetch_limiter), the `limit` launch (k_limit) and
   the int16 pack with the curve (k_pack_curve) against the pack with the limiter off (k_pack<.., NORM>) from
   mi355vits_profile_report, and — as a number, not a pass mark — the loudness of the limited F32LE stream's entries re-measured by
   the loudness kernels alone (mi355vits_lab_loudness, hooks library) against the target;
2. with --parent-root (a checkout of the parent commit with its library built): the normalised int16 pack with the limiter OFF on this
   build against the parent's, the two handles alternating in this process, and whether the difference of the medians lies within the
   run-to-run spread (max - min) of either side IN THIS RUN, and — where profiles/loudness_ab.txt is present — within the spread that
   file shows for `pack.scaled_ms` at the same shape (another run, another day: the first judgment is the stricter like-for-like one).
The loudness and crest factor of the synthetic voice are printed from this run's own fetch_loudness and peaks.
Two untimed warm-up rounds; prints min / median / max over the repetitions."""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine, hooks_library  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402

SPEECH_SETTINGS = ((-16.0, -1.0), (-14.0, -2.0))
DERIVED_CEILING = -1.0
WINDOW_MS = 5.0


def _fmt(xs):
    return f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}  (n={len(xs)})"


def parent_engine_class(root):
    """The parent commit's own binding (its package imported under another name) over its own library."""
    pkg = os.path.join(os.path.abspath(root), "mimic3_amd")
    spec = importlib.util.spec_from_file_location("mimic3_amd_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mimic3_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module("mimic3_amd_parent._native").Engine


def derived_target(eng, say):
    """The target at which DERIVED_CEILING binds on half the rows of the last run: a row is over iff its peak in dBFS lies more than
    ceiling - target above its loudness.  Prints the run's own loudness and crest factor (peak in dBFS - lufs)."""
    eng.set_loudness_target(-23.0, DERIVED_CEILING)
    ld = eng.fetch_loudness()
    peaks = eng.fetch(want_float=False)["peaks"].astype(np.float64)
    crest = (20.0 * np.log10(peaks) - ld.lufs)[np.isfinite(ld.lufs) & (peaks > 0)]
    say(f"  this run's rows: lufs {np.min(ld.lufs):.2f} .. {np.max(ld.lufs):.2f}, peak {20.0 * np.log10(peaks.min()):.2f} .. "
        f"{20.0 * np.log10(peaks.max()):.2f} dBFS, crest factor (peak - lufs) {crest.min():.2f} .. {crest.max():.2f} dB, median {np.median(crest):.2f}")
    return max(-69.0, min(-0.5, round(2.0 * (DERIVED_CEILING - float(np.median(crest)))) / 2.0))


def recorded_pack_spread(index):
    """max - min of `pack.scaled_ms` of the index-th shape in profiles/loudness_ab.txt, or None when the file is not there."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loudness_ab.txt")
    if not os.path.exists(path):
        return None
    rows = [ln.split() for ln in open(path) if ln.strip().startswith("pack.scaled_ms")]
    if index >= len(rows):
        return None
    return float(rows[index][6]) - float(rows[index][2])  # "pack.scaled_ms min A median B max C (n=7)"


def measure(eng, hooks, name, ids, lens, reps, say, parent, shape_index, **kw):
    run = dict(seed=1, **kw)
    eng.set_loudness_target(None)
    eng.set_loudness_limiter(0)
    eng.run(ids, lens, [0.667, 1.0, 0.8], want_float=False, **run)
    hz = eng.last_rate
    lengths = eng.fetch(want_float=False)["lengths"]
    say(f"{name}: {len(lens)} rows, {int(np.sum(lengths))} samples at {hz} Hz")
    settings = SPEECH_SETTINGS + ((derived_target(eng, say), DERIVED_CEILING),)
    windows = (int(round(WINDOW_MS * hz / 1000.0)), 4096)
    for target, ceiling in settings:
        eng.set_loudness_target(target, ceiling)
        for L in windows:
            eng.set_loudness_limiter(L)
            lim = eng.fetch_limiter()
            over = int(lim.engaged.sum())
            tag = f"target {target} LUFS, ceiling {ceiling} dBFS{' (derived)' if (target, ceiling) == settings[-1] else ''}, window {L}"
            say(f"  {tag}: {over} of {len(lens)} rows over, reduced_samples {int(lim.reduced_samples.sum())} "
                f"({100.0 * float(lim.reduced_samples.sum()) / max(1.0, float(np.sum(lengths[lim.engaged]))):.2f} % of the over rows' samples), "
                f"min_scale {float(lim.min_scale.min()):.4f}")
            t = {k: [] for k in ("limit_ms", "pack.curve_ms", "pack.scaled_ms")}
            nbytes = 0.0
            for rep in range(reps + 2):
                eng.profile_enable(True)
                for side in ("off", "on", "on", "off"):
                    eng.set_loudness_limiter(L if side == "on" else 0)
                    eng.profile_reset()
                    out = eng.fetch_packed(wav=True)
                    r = eng.profile_report()
                    del out
                    if rep < 2:
                        continue
                    if side == "on":
                        t["pack.curve_ms"].append(r["pcm16.pack"]["ms"])
                        if "limit" in r:
                            t["limit_ms"].append(r["limit"]["ms"])
                            nbytes = r["limit"]["bytes"]
                    else:
                        t["pack.scaled_ms"].append(r["pcm16.pack"]["ms"])
                eng.profile_enable(False)
            for k, v in t.items():
                if v:
                    say(f"    {k:16s} {_fmt(v)}" + (f"  {nbytes / (statistics.median(v) * 1e-3) / 1e9:.1f} GB/s of {int(nbytes)} B" if k == "limit_ms" else ""))
            if not t["limit_ms"]:
                say("    no row is over: k_limit is not launched and the pack is the limiter-off kernel's")
            # the loudness the limited F32LE entries really have (a number, not a pass mark)
            eng.set_loudness_limiter(L)
            eng.set_output_encoding("f32le")
            f32 = eng.fetch_packed()
            eng.set_loudness_limiter(0)
            capped = eng.fetch_packed()
            eng.set_output_encoding("s16le")
            stride = int(max(f32.lengths))
            for label, p in (("limited", f32), ("gain capped (limiter off)", capped)):
                audio = np.zeros((len(lens), stride), np.float32)
                for i, row in enumerate(p.rows):
                    audio[i, : len(row)] = row
                lufs = hooks.lab_loudness(audio, np.asarray(p.lengths, np.int32), hz)[0]
                d = lufs - target
                sel = lim.engaged & np.isfinite(lufs)
                if sel.any():
                    say(f"    re-measured, {label}: over rows {np.min(d[sel]):+.2f} .. {np.max(d[sel]):+.2f} LU from target"
                        + (f"; other rows {np.min(d[~sel]):+.3f} .. {np.max(d[~sel]):+.3f} LU" if (~sel).any() else ""))
                else:
                    say(f"    re-measured, {label}: all rows {np.min(d):+.3f} .. {np.max(d):+.3f} LU from target")
            del f32, capped
    eng.set_loudness_limiter(0)
    if parent is not None:
        target, ceiling = settings[0]
        parent.run(ids, lens, [0.667, 1.0, 0.8], want_float=False, **run)
        t = {"this build": [], "parent": []}
        for e in (eng, parent):
            e.set_loudness_target(target, ceiling)
            e.profile_enable(True)
        same = bytes(eng.fetch_packed(wav=True).wav) == bytes(parent.fetch_packed(wav=True).wav)
        say(f"  limiter off, target {target}: this build's file and the parent's are {'equal' if same else 'DIFFERENT'}")
        for rep in range(reps + 2):
            for side in ("this build", "parent", "parent", "this build"):
                e = eng if side == "this build" else parent
                e.profile_reset()
                out = e.fetch_packed(wav=True)
                ms = e.profile_report()["pcm16.pack"]["ms"]
                del out
                if rep >= 2:
                    t[side].append(ms)
        for e in (eng, parent):
            e.profile_enable(False)
            e.set_loudness_target(None)
        for k, v in t.items():
            say(f"    pcm16.pack, limiter off, {k:10s} {_fmt(v)}")
        diff = abs(statistics.median(t["this build"]) - statistics.median(t["parent"]))
        spread = max(max(v) - min(v) for v in t.values())
        say(f"    difference of the medians {diff:.4f} ms, run-to-run spread (max - min) of this run {spread:.4f} ms: "
            f"{'within' if diff <= spread else 'OUTSIDE'} the spread")
        rec = recorded_pack_spread(shape_index)
        if rec is not None:
            say(f"    spread of pack.scaled_ms at this shape in profiles/loudness_ab.txt {rec:.4f} ms: "
                f"the difference is {'within' if diff <= rec else 'OUTSIDE'} it")
    eng.set_loudness_target(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-root", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = VitsConfig.apope_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0))
    eng = Engine(blob, device=0)
    parent = parent_engine_class(args.parent_root)(blob, device=0) if args.parent_root else None
    hooks = hooks_library()
    say(f"limiter_ab: {eng.native.version()}, math {eng.math}, reps {args.reps} (times in ms, HIP events around the launch)")
    say("No real voice is measured here: synthetic weights only.  How many rows of real speech are over at the speech targets is not claimed.")
    rng = np.random.default_rng(1)
    B, Tx = 256, 128
    measure(eng, hooks, "headline shape", rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64), args.reps, say, parent, 0,
            forced_durations=np.full((B, Tx), 6, np.int32))
    rng = np.random.default_rng(141)
    B = 48
    lens = rng.integers(20, 129, B).astype(np.int64)
    lens[0], lens[B // 2] = 128, 20
    ids = np.zeros((B, 128), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    measure(eng, hooks, "48 ragged sentences", ids, lens, args.reps, say, parent, 1)
    eng.close()
    if parent is not None:
        parent.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
