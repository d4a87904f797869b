#!/usr/bin/env python3
"""A/B of k_wn_layer_b3's MFMA shape inside ONE process of the lab library: v_mfma_f32_16x16x32_bf16 (the default) against
v_mfma_f32_32x32x16_bf16 (MI355VITS_WN_SHAPE=32), on the bench workload's own data (apope_low, synthetic weights seed 1234, bench.py's
seeded ids, 128 ids x 6 frames = 768 frames per row) at batch 256 and batch 32.

    python -m mimic3_amd.build lab && python tools/wn_shape_ab.py > profiles/wn_shape_ab.txt

One device, one handle.  After at least two seconds of warm-up steps the two forms alternate for ROUNDS rounds (the order flips every
round); a round of a form is STEPS whole steps with the engine's profiler on — in BOTH arms — and its figure is the mean HIP-event
time of one flow.wn_layer_b3 launch in that round (16 launches per step).  Printed per form: median, min and max over the rounds.
The gate: the new form's median below the 32x32x16 form's median by more than max(its max - min, 3 % of its median).

The shader clock each form holds comes from a counters-only pass of this same script (both forms profiled alike, never compared with
the un-profiled figures above): GRBM_GUI_ACTIVE / 8 / kernel time per launch,

    rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_INSTS_VALU SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES \
        SQ_BUSY_CYCLES GRBM_GUI_ACTIVE -d DIR -o p -- python tools/wn_shape_ab.py --batches 256 --rounds 2
    python tools/rocprof_summary.py pmc DIR"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from bench import make_batch  # noqa: E402
from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine, NativeLibrary  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402

NAME = "flow.wn_layer_b3"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    lab = NativeLibrary(os.path.join(ROOT, "mimic3_amd", "csrc", "libmi355vits_lab.so"))
    cfg = VitsConfig.apope_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=1234))
    scales = np.array([0.667, 1.0, 0.8], np.float32)
    ok_all = []
    for B in (int(b) for b in args.batches.split(",")):
        eng = Engine(blob, device=args.device, library=lab)
        ids, lengths = make_batch(B, 128, 0)
        forced = np.full((B, 128), 6, np.int32)
        steps = max(2, 512 // B)

        def step(i):
            eng.run(ids, lengths, scales, None, forced_durations=forced, seed=1, utterance_base=i * B, want_float=False, want_pcm16=True,
                    device_only=True)

        eng.profile_enable(True)
        t0, i = time.time(), 0
        while time.time() - t0 < 2.5:  # warm-up: both forms
            os.environ["MI355VITS_WN_SHAPE"] = "32" if i & 1 else "16"
            step(i)
            i += 1
        per = {16: [], 32: []}
        for r in range(args.rounds):
            for shape in ((16, 32) if r % 2 == 0 else (32, 16)):
                os.environ["MI355VITS_WN_SHAPE"] = str(shape)
                step(i)  # one un-timed step after the switch
                eng.profile_reset()
                for _ in range(steps):
                    i += 1
                    step(i)
                rep = eng.profile_report()[NAME]
                per[shape].append(rep["ms"] / rep["calls"])
        eng.close()
        print(f"batch {B} x 768 frames, {args.rounds} rounds x {steps} steps per form, ms per {NAME} launch (mean of a round's launches):")
        for shape in (32, 16):
            v = per[shape]
            print(f"  {'32x32x16' if shape == 32 else '16x16x32'}: median {statistics.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}   rounds "
                  + " ".join(f"{x:.4f}" for x in v))
        m32, m16 = statistics.median(per[32]), statistics.median(per[16])
        margin = max(max(per[32]) - min(per[32]), 0.03 * m32)
        ok = m16 < m32 - margin
        ok_all.append(ok)
        print(f"  gate: 16x16x32 median {m16:.4f} vs 32x32x16 median {m32:.4f} - margin {margin:.4f} = {m32 - margin:.4f}: "
              f"{'PASS' if ok else 'MISS'} ({100 * (m32 - m16) / m32:+.1f} % of the 32x32x16 median)")
    print("gate at every batch:", "PASS" if all(ok_all) else "MISS")


if __name__ == "__main__":
    main()
