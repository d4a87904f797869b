"""A/B of two builds of the PRODUCT library on one MI355X lease: bit identity first, then alternating bench runs.

    python tools/ab_prev.py bits  PREV.so NEW.so          # the same ragged batch through both: waveforms, lengths, PCM compared bitwise
    python tools/ab_prev.py bench PREV.so NEW.so [--batch 256 --steps 20 --rounds 2]
    python tools/ab_prev.py digest [--root TREE]          # sha256 of a tree's own results: `bits` across an ABI change

`bits` opens both files with THIS tree's binding, so PREV must export every entry point the binding knows.  When the ABI has grown
since PREV, run `digest` once in each tree (or with --root on a checkout that holds its built library) and compare the lines: the
ragged batch of `bits`, and the headline shape (256 rows x 128 ids x 6 forced frames) as padded int16 and as the default packed stream.

`bench` swaps the file bench.py opens (mimic3_amd/csrc/libmi355vits.so) — the product reads no library switch — and always puts NEW
back at the end.  Output: one line per run with ms/step and the kernel table rows named in --rows.
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


def run_digest(root):
    """One line per result of the tree at `root`, through that tree's own package and product library."""
    import hashlib

    sys.path.insert(0, root)
    import numpy as np

    from mimic3_amd import weights as W
    from mimic3_amd._native import Engine
    from mimic3_amd.config import VitsConfig

    def sha(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()[:32]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bits", "bench", "digest"])
    ap.add_argument("prev", nargs="?")
    ap.add_argument("new", nargs="?")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--rows", default="flow.wn_layer_b3,dec.mrf_p.s2,dec.mrf_s.s1,dec.rb.s0,enc.ffn1,enc.ffn2,dec.conv_pre")
    a = ap.parse_args()
    if a.mode == "digest":
        run_digest(os.path.abspath(a.root))
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
                    print(f"{tag} b{a.batch} round {r}: ms/step {d['ms_per_step']:.3f} | {rows}", flush=True)
                except Exception as ex:  # noqa: BLE001
                    print(f"{tag}: no bench line ({ex}); stderr tail: {pr.stderr[-400:]}", flush=True)
    finally:
        shutil.copy2(keep, PRODUCT)
        os.remove(keep)


if __name__ == "__main__":
    main()
