"""A/B of two builds of the PRODUCT library on one MI355X lease: bit identity first, then alternating bench runs.

    python tools/ab_prev.py bits  PREV.so NEW.so          # the same ragged batch through both: waveforms, lengths, PCM compared bitwise
    python tools/ab_prev.py bench PREV.so NEW.so [--batch 256 --steps 20 --rounds 2]
    python tools/ab_prev.py digest [--root TREE] [--emu]  # sha256 of a tree's own results: `bits` across an ABI change

`bits` opens both files with THIS tree's binding, so PREV must export every entry point the binding knows.  When the ABI has grown
since PREV, run `digest` once in each tree (or with --root on a checkout that holds its built library) and compare the lines: the
ragged batch of `bits`, and the headline shape (256 rows x 128 ids x 6 forced frames) as padded int16 and as the default packed stream.
Then the result paths on that ragged batch (`digest pack ...` / `digest streams ...` / `digest fail ...`): every packed-form call —
run and fetch, each encoding, header, trim, target, limiter, true peak, FLAC, v1 and v2 streams — as the sha256 of its block and of
every result array, with the profiler's (label, calls, bytes) of the call: the labels outside the synthesis graph spelled out, the
graph's own as one hash.  `--emu` runs the result-path lines alone on the CPU model's library (tests/emu) with the tiny voice: the
host code is the same, and the model is too slow for the full voices.  Last the input forms (`digest inputs ...`) on a multi-speaker
voice: per-row settings, forced durations, injected noise, each timing input, a speaker mix, speaker vectors, their combinations and
every class of refused input, as the sha256 of each result array with every profiler label of the call.

`bench` swaps the file bench.py opens (mimic3_amd/csrc/libmi355vits.so) — the product reads no library switch — and always puts NEW
back at the end.  Output: one line per run with ms/step, the host side of a call (wall time minus device time, one handle) and the
kernel table rows named in --rows; a run without a result line ends the A/B.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PRODUCT = os.path.join(ROOT, "mimic3_amd", "csrc", "libmi355vits.so")


def run_bits(lib_path, math=None):
    import numpy as np

    from mimic3_amd import weights as W
    from mimic3_amd._native import Engine, NativeLibrary
    from mimic3_amd.config import VitsConfig

    out = {}
    for voice in ("apope_low", "vctk_low"):
        cfg = getattr(VitsConfig, voice)()
        w = W.synthetic_weights(cfg, seed=11, frames_per_id=4.0)
        eng = Engine(W.pack(cfg, w), device=0, library=NativeLibrary(lib_path))
        if math is not None:
            eng.set_math(math)
        rng = np.random.default_rng(5)
        lens = [97, 128, 33, 5, 64, 120, 1, 77]
        ids = np.zeros((len(lens), 128), np.int64)
        for b, n in enumerate(lens):
            ids[b, :n] = rng.integers(1, cfg.num_symbols, size=n)
        sid = (np.arange(len(lens)) % max(cfg.n_speakers, 1)).astype(np.int64) if cfg.n_speakers > 1 else None
        r = eng.run(ids, lens, [0.667, 1.0, 0.8], sid=sid, seed=1234, want_pcm16=True)
        out[voice] = (r["audio"].copy(), r["lengths"].copy(), r["pcm"].copy())
        eng.close()
    return out


RAGGED = [97, 128, 33, 5, 64, 120, 1, 77]  # the eight rows of `bits`
TRIM = (0.03, 3)
TARGET = (-6.0, -6.0)
HUGE = (1 << 31) - 100  # a silence that fits on its own and not with any audio behind it


def digest_results(sha, emu_root=None):
    """The result-path lines: one synthesis of the ragged batch per run line, every fetch line served from the run before it."""
    import numpy as np

    from mimic3_amd import weights as W
    from mimic3_amd._native import Engine, NativeError, NativeLibrary
    from mimic3_amd.config import VitsConfig

    cfg = VitsConfig.tiny() if emu_root else VitsConfig.apope_low()
    lib = NativeLibrary(os.path.join(emu_root, "tests", "emu", "libmi355vits_emu.so")) if emu_root else None
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=11, frames_per_id=4.0)), device=0, library=lib)
    Tx = 16 if emu_root else 128
    lens = [max(1, n * Tx // 128) for n in RAGGED]
    rng = np.random.default_rng(5)
    ids = np.zeros((len(lens), Tx), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(1, cfg.num_symbols, size=n)
    run_args = (ids, lens, [0.667, 1.0, 0.8])
    run_kw = dict(seed=1234, pcm_volume=np.linspace(0.5, 3.0, len(lens)))
    eng.profile_enable(True)
    eng.profile_reset()
    eng.run(*run_args, seed=1234)
    graph = set(eng.profile_report())  # the labels of the synthesis itself

    def prof(full=False):
        rep = sorted((k, v["calls"], v["bytes"]) for k, v in eng.profile_report().items())
        if full:  # the graph itself differs between the forms: every label spelled out
            return "prof [" + " ".join(f"{k}:{c}:{b:.0f}" for k, c, b in rep) + "]"
        own = " ".join(f"{k}:{c}:{b:.0f}" for k, c, b in rep if k not in graph)
        return f"prof [{own}] graph {sha(np.frombuffer(repr([r for r in rep if r[0] in graph]).encode(), np.uint8))}"

    def arrays(pa):
        block = pa.flac if pa.compression else (pa.wav if pa.wav is not None else pa.data)
        out = [np.frombuffer(bytes(block), np.uint8), np.int64(pa.total_samples)]
        for k in ("offsets", "lengths", "peaks", "first", "end", "lufs", "gain", "limited"):
            v = getattr(pa, k)
            out.append(np.zeros(0) if v is None else np.asarray(v))
        for k in ("stream_offset", "data_offset", "stream_bytes", "frames", "uncompressed_bytes"):
            out.append(np.int64(-1 if getattr(pa, k, None) is None else getattr(pa, k)))
        return out

    def line(kind, name, call):
        eng.profile_reset()
        try:
            got = call()
        except NativeError as e:
            print(f"digest {kind} {name}: error {e.code} {e}", flush=True)
            return
        if isinstance(got, dict):  # a padded run (the `inputs` lines): its arrays by name
            named = " ".join(f"{k} {sha(got[k])}" for k in ("audio", "lengths", "pcm", "peaks", "timing_factor") if k in got)
            print(f"digest {kind} {name}: {named} {prof(full=True)}", flush=True)
            return
        got = got if isinstance(got, list) else [got]
        whole = [np.asarray(got[0].block)] if getattr(got[0], "block", None) is not None else []
        print(f"digest {kind} {name}: " + " ".join(sha(*arrays(pa)) for pa in got) + (f" block {sha(*whole)} " if whole else " ") + prof(), flush=True)

    order = [5, 0, 7, 2, 6, 1]
    pack = dict(order=order, lead_samples=[0, 9000, 1, 100, 7, 4097], tail_samples=33)
    settings = {
        "plain": {},
        "trim": dict(trim=TRIM),
        "target": dict(loudness=TARGET),
        "target+limiter": dict(loudness=TARGET, limiter=32),
        "target+truepeak": dict(loudness=TARGET, true_peak=True),
        "flac": dict(compression="flac"),
    }

    def setup(encoding="s16le", trim=(0.0, 0), loudness=(None, -1.0), limiter=0, true_peak=False, compression=None):
        eng.set_output_encoding(encoding)
        eng.set_edge_trim(*trim)
        eng.set_loudness_target(*loudness)
        eng.set_loudness_limiter(limiter)
        eng.set_loudness_ceiling_mode("true_peak" if true_peak else "sample")
        eng.set_output_compression(compression)

    for sname, st in settings.items():
        for enc in ("s16le",) if sname == "flac" else ("s16le", "ulaw", "alaw", "f32le"):
            for wav in (False,) if sname == "flac" else (False, True):
                setup(encoding=enc, **st)
                tag = f"{sname} {enc}{' wav' if wav else ''}"
                line("pack", "run " + tag, lambda: eng.run_packed(*run_args, wav=wav, **pack, **run_kw))
                line("pack", "fetch " + tag, lambda: eng.fetch_packed(wav=wav, **pack))
    setup()
    # v1: four streams that share rows, mixed encodings, a header, a trimmed and normalised one; then the same measured from a fetch
    four = [
        dict(order=[3], lead_samples=[1], wav=True, encoding="ulaw"),
        dict(order=[0, 4, 3], lead_samples=[0, 777, 2], tail_samples=5, wav=True, encoding="f32le"),
        dict(order=[1, 0], encoding="s16le", trim=TRIM, loudness=TARGET),
        dict(order=[2, 3], lead_samples=[4096 + 453, 0], encoding="alaw"),
        dict(order=[3, 6], wav=True, encoding="s16le"),
    ]
    plain4 = [dict(st) for st in four if "trim" not in st]
    eng.set_loudness_limiter(16)  # the one pair of handle settings a v1 call reads
    line("streams", "run v1 plain", lambda: eng.run_streams(*run_args, streams=plain4, **run_kw))
    line("streams", "fetch v1 plain", lambda: eng.fetch_streams(plain4))
    line("streams", "run v1 measured", lambda: eng.run_streams(*run_args, streams=four, **run_kw))
    line("streams", "fetch v1 measured", lambda: eng.fetch_streams(four))
    setup()
    # v2: two FLAC streams, two windows, both modes (tests/streams2_cases.py: SEVEN)
    seven = [
        dict(order=[3], wav=True, encoding="s16le", compression=None),
        dict(order=[2, 0, 1], lead_samples=[0, 9000, 100], tail_samples=33, compression="flac"),
        dict(order=[3], lead_samples=[1], wav=True, encoding="ulaw"),
        dict(order=[2, 0, 1], lead_samples=[0, 9000, 100], tail_samples=33, compression="flac", trim=TRIM, loudness=TARGET, limiter=32, true_peak=True),
        dict(order=[1, 4], encoding="s16le", loudness=TARGET, limiter=8, true_peak=False),
        dict(order=[1, 4], encoding="s16le", loudness=TARGET, limiter=0),
        dict(order=[0, 4], lead_samples=[0, 777], tail_samples=5, encoding="f32le"),
    ]
    line("streams", "run v2 seven", lambda: eng.run_streams(*run_args, streams=seven, **run_kw))
    line("streams", "fetch v2 seven", lambda: eng.fetch_streams(seven))
    line("streams", "run v2 flac only", lambda: eng.run_streams(*run_args, streams=seven[1:2], **run_kw))
    # failing calls: the code and the text; a failing late path serves nothing afterwards
    line("fail", "run_packed duplicate row", lambda: eng.run_packed(*run_args, order=[1, 2, 1], **run_kw))
    line("fail", "fetch_packed negative silence", lambda: eng.fetch_packed(order=[1, 2], lead_samples=[0, -4]))
    line("fail", "run_packed early over the limit", lambda: eng.run_packed(*run_args, order=[1], lead_samples=[HUGE], **run_kw))
    line("fail", "fetch_packed after it", lambda: eng.fetch_packed())
    eng.run(*run_args, seed=1234)
    setup(trim=TRIM)
    line("fail", "run_packed trimmed over the limit", lambda: eng.run_packed(*run_args, order=[1], lead_samples=[HUGE], **run_kw))
    line("fail", "fetch_packed after it", lambda: eng.fetch_packed())
    setup()
    eng.run(*run_args, seed=1234)
    line("fail", "run_streams duplicate row", lambda: eng.run_streams(*run_args, streams=[dict(order=[0]), dict(order=[2, 2])], **run_kw))
    line("fail", "fetch_streams negative tail", lambda: eng.fetch_streams([dict(order=[0]), dict(order=[2], tail_samples=-1)]))
    line("fail", "fetch_streams flac with wav", lambda: eng.fetch_streams([dict(order=[0], compression="flac", wav=True)]))
    line("fail", "run_streams trimmed over the limit",
         lambda: eng.run_streams(*run_args, streams=[dict(order=[0]), dict(order=[1], lead_samples=[HUGE], trim=TRIM)], **run_kw))
    line("fail", "fetch_packed after it", lambda: eng.fetch_packed())
    line("fail", "run_streams block over the limit",
         lambda: eng.run_streams(*run_args, streams=[dict(order=[0], lead_samples=[HUGE // 2]), dict(order=[1], lead_samples=[HUGE // 2])], **run_kw))

    # ---- the input forms (`digest inputs ...`): every optional input of a run on the same ragged batch, on a multi-speaker voice;
    # each line the sha256 of every result array and the profiler's (label, calls, bytes) of the whole call
    from mimic3_amd._native import SpeakerArgs

    def speaker_args(n_terms=0, sid=None, weight=None, vectors=None, reserved=0):  # the struct as given, unchecked by the binding
        s = SpeakerArgs()
        s.n_terms, s.reserved[3] = n_terms, reserved
        s.keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((sid, np.int64), (weight, np.float32), (vectors, np.float32))]
        if sid is not None:
            s.mix_sid = s.keep[0].ctypes.data_as(type(s.mix_sid))
        if weight is not None:
            s.mix_weight = s.keep[1].ctypes.data_as(type(s.mix_weight))
        if vectors is not None:
            s.vectors = s.keep[2].ctypes.data_as(type(s.vectors))
        return s

    line("inputs", "fail speakers on a single-speaker voice", lambda: eng.run(*run_args, speakers=[0] * len(lens)))
    eng.close()
    cfg = VitsConfig.tiny(n_speakers=4) if emu_root else VitsConfig.vctk_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=11, frames_per_id=4.0))
    eng = Engine(blob, device=0, library=lib)
    eng.profile_enable(True)
    B, S, gin = len(lens), cfg.n_speakers, cfg.gin_channels
    sid = np.arange(B) % S
    kw = dict(seed=1234, want_pcm16=True)
    rows = dict(pcm_volume=np.linspace(0.5, 3.0, B), utterance_keys=[7, 7, 1 << 40, 3, 2, 1, 0, 99])
    row_scales = np.stack([np.linspace(0.0, 0.9, B), np.linspace(0.7, 1.6, B), np.linspace(0.9, 0.0, B)], axis=1)
    base = eng.run(ids, lens, run_args[2], sid, **kw)
    frames = base["lengths"] // cfg.hop_length
    stretch = rng.uniform(0.5, 2.0, (B, Tx)).astype(np.float32)
    stretch[1, 0] = 0.0
    min_frames = rng.integers(0, 6, (B, Tx)).astype(np.int32)
    target = (frames * 5 // 4 + min_frames.sum(axis=1)).astype(np.int32)
    target[2] = 0
    noise_w = rng.standard_normal((B, 2, Tx)).astype(np.float32)
    ty = int(eng.run(ids, lens, run_args[2], sid, noise_w=noise_w, **kw)["ty_max"])
    noise_z = rng.standard_normal((B, cfg.inter_channels, ty + 3)).astype(np.float32)
    mix = [{b % S: 0.7, (b + 1) % S: 0.0, (b + 2) % S: 0.3 + 0.1 * b} for b in range(B)]  # K = 3, a zero-weight term in every row
    vectors = [eng.speaker_embedding(b % S) * np.float32(0.5 + 0.1 * b) for b in range(B)]
    wide_z = rng.standard_normal((B, cfg.inter_channels, 4 * ty + int(min_frames.sum(axis=1).max()))).astype(np.float32)  # frames for the timed rows
    everything = dict(noise_w=noise_w, noise_z=wide_z, stretch=stretch, min_frames=min_frames, target_frames=target, speakers=mix, **rows)

    def run(*a, **k):
        return lambda: eng.run(ids, lens, *a, **{**kw, **k})

    line("inputs", "plain sid", run(run_args[2], sid))
    line("inputs", "rows", run(row_scales, sid, **rows))
    line("inputs", "forced_durations", run(run_args[2], sid, forced_durations=rng.integers(1, 7, (B, Tx))))
    line("inputs", "noise_w noise_z", run(run_args[2], sid, noise_w=noise_w, noise_z=noise_z))
    line("inputs", "timing stretch", run(run_args[2], sid, stretch=stretch))
    line("inputs", "timing min_frames", run(run_args[2], sid, min_frames=min_frames))
    line("inputs", "timing target_frames", run(run_args[2], sid, target_frames=target))
    line("inputs", "timing all three", run(run_args[2], sid, stretch=stretch, min_frames=min_frames, target_frames=target))
    line("inputs", "speakers mix K=3", run(run_args[2], speakers=mix))
    line("inputs", "speakers vectors", run(run_args[2], speakers=vectors))
    line("inputs", "rows timing mix", run(row_scales, stretch=stretch, target_frames=target, speakers=mix, **rows))
    eng.close()
    eng = Engine(blob, device=0, library=lib)  # a fresh handle: its first call sizes the text side, the second brings every input
    eng.profile_enable(True)
    line("inputs", "fresh handle: no optional input", run(run_args[2], sid))
    line("inputs", "fresh handle: every compatible input", run(row_scales, **everything))
    # failing calls, one per class of check, with code and text
    bad_scales = row_scales.copy()
    bad_scales[3, 1] = 0.0
    bad_ids = ids.copy()
    bad_ids[2, 0] = cfg.num_symbols
    bad_stretch = stretch.copy()
    bad_stretch[2, 1] = np.nan
    w3 = np.full((B, 3), 0.5, np.float32)
    s3 = np.tile(np.arange(3), (B, 1))

    def edit(a, at, v, dtype=None):
        a = np.array(a, dtype)
        a[at] = v
        return a

    line("inputs", "fail row scales", run(bad_scales, sid))
    line("inputs", "fail length", lambda: eng.run(ids, edit(lens, 4, Tx + 1), run_args[2], sid, **kw))
    line("inputs", "fail phoneme id", lambda: eng.run(bad_ids, lens, run_args[2], sid, **kw))
    line("inputs", "fail sid", run(run_args[2], edit(sid, 5, S)))
    line("inputs", "fail noise_z_frames", run(run_args[2], sid, noise_z=noise_z[:, :, :0]))
    line("inputs", "fail timing with forced_durations", run(run_args[2], sid, stretch=stretch, forced_durations=np.ones((B, Tx), np.int32)))
    line("inputs", "fail stretch", run(run_args[2], sid, stretch=bad_stretch))
    line("inputs", "fail min_frames", run(run_args[2], sid, min_frames=edit(min_frames, (6, 0), -1)))
    line("inputs", "fail target_frames", run(run_args[2], sid, target_frames=edit(target, 7, -1)))
    line("inputs", "fail speakers reserved", run(run_args[2], speakers=speaker_args(3, s3, w3, reserved=1)))
    line("inputs", "fail speakers mix and vectors", run(run_args[2], speakers=speaker_args(3, s3, w3, np.zeros((B, gin)))))
    line("inputs", "fail speakers neither", run(run_args[2], speakers=speaker_args()))
    line("inputs", "fail speakers n_terms with vectors", run(run_args[2], speakers=speaker_args(2, vectors=np.zeros((B, gin)))))
    line("inputs", "fail speakers vector not finite", run(run_args[2], speakers=speaker_args(vectors=edit(np.zeros((B, gin)), (1, 2), np.inf))))
    line("inputs", "fail speakers mix_sid alone", run(run_args[2], speakers=speaker_args(3, sid=s3)))
    line("inputs", "fail speakers n_terms 0", run(run_args[2], speakers=speaker_args(0, s3, w3)))
    line("inputs", "fail speakers n_terms 9", run(run_args[2], speakers=speaker_args(9, s3, w3)))
    line("inputs", "fail speakers weight not finite", run(run_args[2], speakers=speaker_args(3, s3, edit(w3, (4, 1), np.nan))))
    line("inputs", "fail speakers weight beyond 1024", run(run_args[2], speakers=speaker_args(3, s3, edit(w3, (4, 2), -1025.0))))
    line("inputs", "fail speakers sid", run(run_args[2], speakers=speaker_args(3, edit(s3, (0, 2), S), w3)))
    line("inputs", "fail speakers every weight 0", run(run_args[2], speakers=speaker_args(3, s3, edit(w3, 5, 0.0))))
    line("inputs", "fetch_packed after the refused calls", lambda: eng.fetch_packed())  # the last completed run is still served
    line("inputs", "fail target below the floor", run(run_args[2], sid, min_frames=np.full((B, Tx), 50, np.int32), target_frames=edit(target, 0, 1)))
    line("inputs", "fetch_packed after it", lambda: eng.fetch_packed())
    # wrong in two ways at once: the order of the checks decides which error the caller sees
    line("inputs", "fail scales and id", lambda: eng.run(bad_ids, lens, bad_scales, sid, **kw))
    line("inputs", "fail stretch and speaker weight", run(run_args[2], stretch=bad_stretch, speakers=speaker_args(3, s3, edit(w3, (0, 0), np.nan))))
    line("inputs", "fail missing sid and length", lambda: eng.run(ids, edit(lens, 0, -1), run_args[2], **kw))
    eng.close()


def run_digest(root, emu=False):
    """One line per result of the tree at `root`, through that tree's own package and product library (emu: the CPU model's)."""
    import hashlib

    sys.path.insert(0, root)
    import numpy as np

    def sha(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()[:32]

    if emu:
        digest_results(sha, root)
        return
    from mimic3_amd import weights as W
    from mimic3_amd._native import Engine
    from mimic3_amd.config import VitsConfig

    for voice, (audio, lengths, pcm) in run_bits(os.path.join(root, "mimic3_amd", "csrc", "libmi355vits.so")).items():
        print(f"digest ragged {voice}: audio {sha(audio)} lengths {sha(lengths)} pcm {sha(pcm)}")
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0)), device=0)
    B, Tx = 256, 128
    ids = np.random.default_rng(1).integers(1, cfg.num_symbols, (B, Tx))
    lens, forced = np.full(B, Tx, np.int64), np.full((B, Tx), 6, np.int32)
    r = eng.run(ids, lens, [0.667, 1.0, 0.8], forced_durations=forced, seed=1, want_float=True, want_pcm16=True)
    print(f"digest headline padded: audio {sha(r['audio'])} lengths {sha(r['lengths'])} pcm {sha(r['pcm'])} peaks {sha(r['peaks'])}")
    del r
    pk = eng.run_packed(ids, lens, [0.667, 1.0, 0.8], forced_durations=forced, seed=1, lead_samples=[7] * B, tail_samples=11, wav=True,
                        pcm_volume=np.linspace(0.5, 3.0, B))
    print(f"digest headline packed wav: bytes {sha(np.frombuffer(bytes(pk.wav), np.uint8))} offsets {sha(pk.offsets)} peaks {sha(pk.peaks)}")
    eng.close()
    digest_results(sha)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bits", "bench", "digest"])
    ap.add_argument("prev", nargs="?")
    ap.add_argument("new", nargs="?")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--emu", action="store_true", help="digest: the result-path lines on the CPU model's library of the tree")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--rows", default="flow.wn_layer_b3,dec.mrf_p.s2,dec.mrf_s.s1,dec.rb.s0,enc.ffn1,enc.ffn2,dec.conv_pre")
    a = ap.parse_args()
    if a.mode == "digest":
        run_digest(os.path.abspath(a.root), a.emu)
        return
    if not a.prev or not a.new:
        ap.error("bits / bench need PREV.so and NEW.so")
    if a.mode == "bits":
        import numpy as np

        ok = True
        for math in (None,):
            p, n = run_bits(a.prev, math), run_bits(a.new, math)
            for v in p:
                same = all(np.array_equal(x, y) for x, y in zip(p[v], n[v]))
                print(f"bits {v}: {'IDENTICAL' if same else 'DIFFERENT'} ({int(p[v][1].sum())} samples)")
                if not same:
                    d = np.abs(p[v][0].astype(np.float64) - n[v][0].astype(np.float64))
                    print("   max abs diff", d.max(), "lengths equal", np.array_equal(p[v][1], n[v][1]))
                ok = ok and same
        sys.exit(0 if ok else 1)
    keep = PRODUCT + ".ab_keep"
    shutil.copy2(a.new, keep)
    try:
        for r in range(a.rounds):
            for tag, lib in (("prev", a.prev), ("new", keep)):
                shutil.copy2(lib, PRODUCT)
                cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--batch", str(a.batch), "--steps", str(a.steps), "--warmup", "5",
                       "--full", "--no-extra", "--no-cpu-baseline", "--no-traffic", "--no-b1"]
                pr = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                try:
                    d = json.loads(pr.stdout.strip().splitlines()[-1])
                    rf = d.get("roofline", {})
                    rows = "  ".join(f"{k}={rf.get('ms:' + k)}" for k in a.rows.split(","))
                    host = d.get("host_ms_per_step", {})  # one handle driven sequentially: the call's wall time minus its device time
                    print(f"{tag} b{a.batch} round {r}: ms/step {d['ms_per_step']:.3f} host_side {host.get('host_side_ms', float('nan')):.3f} "
                          f"(call {host.get('one_handle_call_ms', float('nan')):.3f} device {host.get('device_ms', float('nan')):.3f}) | {rows}", flush=True)
                except Exception as ex:  # noqa: BLE001
                    print(f"{tag}: no bench line ({ex}); stderr tail: {pr.stderr[-400:]}", flush=True)
                    sys.exit(1)  # nothing more is started on a device a run may have left in trouble (NEW is put back below)
    finally:
        shutil.copy2(keep, PRODUCT)
        os.remove(keep)


if __name__ == "__main__":
    main()
