"""The yardstick of the alignment tests (mi355vits_fetch_alignment, k_align), in Python ints and fp64 numpy.

    c[t] = frames[0] + .. + frames[t], c[-1] = 0
    start[t]   = ceil(hop c[t-1] L / M)
    samples[t] = ceil(hop c[t] L / M) - start[t]
    positions at or past the row's phoneme count: frames = samples = 0, start = the end of the covered part
    peak = max |y|, rms = sqrt(mean(y^2)) over the span in fp64, both 0 for an empty span

``L / M`` and ``ceil(n L / M)`` are ``tests/resample_ref.ratio`` / ``out_len``.  Never the code under test: nothing here is
imported by the package.
"""
from __future__ import annotations

import numpy as np

from tests import resample_ref as R


def spans(frames, n_ids: int, hop: int, L: int = 1, M: int = 1):
    """One row: (frames, start, samples) as lists of Python ints over all ``len(frames)`` positions."""
    fr, st, sm = [], [], []
    c = 0
    for t in range(len(frames)):
        f = int(frames[t]) if t < int(n_ids) else 0
        s0 = R.out_len(int(hop) * c, L, M)
        c += f
        s1 = R.out_len(int(hop) * c, L, M)
        fr.append(f)
        st.append(s0)
        sm.append(s1 - s0)
    return fr, st, sm


def timing(frames, lens, hop: int, L: int = 1, M: int = 1):
    """A batch: three int64 arrays [B, Tx]."""
    rows = [spans(frames[b], int(lens[b]), hop, L, M) for b in range(len(lens))]
    return tuple(np.array([r[i] for r in rows], np.int64) for i in range(3))


def levels(audio_row, start, samples):
    """One row: (peak, rms) float32 [Tx] — fp64 over the f32 samples ``audio_row[start[t] : start[t] + samples[t]]``, cast once."""
    peak = np.zeros(len(start), np.float32)
    rms = np.zeros(len(start), np.float32)
    y = np.asarray(audio_row, np.float32)
    for t, (s, n) in enumerate(zip(start, samples)):
        s, n = int(s), int(n)
        if n > 0:
            v = y[s: s + n].astype(np.float64)
            assert v.shape[0] == n, "span outside the row"
            peak[t] = np.float32(np.max(np.abs(v)))
            rms[t] = np.float32(np.sqrt(np.sum(v * v) / n))
    return peak, rms
