"""The workload behind the per-kernel figures of DESIGN.md §4.16 (b): after one run of the headline shape, ten times 64 one-row FLAC
streams in one block (`fetch_streams`) and ten times one FLAC pack of the same 64 rows (`fetch_packed`).  Run it under a kernel tracer
and keep the lines of the FLAC and pack kernels:

  rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/streams2_trace.py
  grep -i "flac\\|pack" DIR/p_kernel_stats.csv > profiles/streams2_kernel_stats.txt

(columns: name, calls, total ns, average ns, percent, min ns, max ns, standard deviation).  Nothing is asserted."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402


def main():
    cfg = VitsConfig.apope_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0)), device=0)
    B, Tx = 256, 128
    rng = np.random.default_rng(1)
    eng.run(rng.integers(1, cfg.num_symbols, (B, Tx)), np.full(B, Tx, np.int64), [0.667, 1.0, 0.8], forced_durations=np.full((B, Tx), 6, np.int32),
            seed=1, want_float=False, device_only=True)
    streams = [dict(order=[b], compression="flac") for b in range(64)]
    for _ in range(10):
        eng.fetch_streams(streams)
        eng.fetch_packed(order=list(range(64)), compression="flac")
    eng.close()


if __name__ == "__main__":
    main()
