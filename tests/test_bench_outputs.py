"""bench.py --dump-outputs on the CPU: what the dump holds (dtypes, the seeded column sample, row sums exact for int16), its
size at the shapes bench.py runs (one rank and the batch of 256 spread over 2 / 4 / 8 ranks), how the calls of one step are
merged, and that Workload.run_steps hands back the last steps' results whichever engine handle ran them."""
import os
import random
import threading
import time

import numpy as np
import pytest

import bench

L = 196608  # samples per utterance of the benchmark workload (128 ids x 6 frames x hop 256)
LIMIT = 64 * 10 ** 6


def _outputs(B, width=L, seed=0):
    rng = np.random.default_rng(seed)
    return {"lengths": np.full(B, width, np.int64), "peaks": rng.random(B).astype(np.float32), "l_max": np.int64(width),
            "ty_max": np.int64(768), "pcm": rng.integers(-32768, 32768, (B, width)).astype(np.int16)}


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_of_the_batch_of_256(tmp_path):
    out = _outputs(256)
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["l_max.npy", "lengths.npy", "pcm.npy", "pcm_columns.npy", "pcm_row_sum.npy", "pcm_row_sumsq.npy",
                     "peaks.npy", "ty_max.npy"]
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:  # the same outputs give the same files: the column sample is fixed
        assert np.array_equal(got[n[:-4]], np.load(tmp_path / "b" / n)), n
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["pcm"].dtype == np.float32 and got["peaks"].dtype == np.float32 and got["lengths"].dtype == np.float64
    assert np.array_equal(got["lengths"], out["lengths"]) and np.array_equal(got["peaks"], out["peaks"])
    assert got["l_max"] == L and got["ty_max"] == 768
    cols = got["pcm_columns"].astype(np.int64)
    assert np.all(np.diff(cols) > 0) and 0 <= cols[0] and cols[-1] < L
    assert got["pcm"].shape == (256, cols.size) and np.array_equal(got["pcm"], out["pcm"][:, cols].astype(np.float32))
    p = out["pcm"].astype(np.int64)
    assert np.array_equal(got["pcm_row_sum"], p.sum(1).astype(np.float64))
    assert np.array_equal(got["pcm_row_sumsq"], (p * p).sum(1).astype(np.float64))
    assert _dir_bytes(tmp_path / "a") <= LIMIT


@pytest.mark.parametrize("world", [2, 4, 8])
def test_dump_of_every_rank_together_stays_within_the_limit(tmp_path, world):
    B = 256 // world
    out = _outputs(B)
    for rank in range(world):
        bench.dump_outputs(out, str(tmp_path), prefix=f"rank{rank}_", budget=bench.DUMP_SAMPLE_BYTES // world)
    assert len(os.listdir(tmp_path)) == 8 * world
    assert _dir_bytes(tmp_path) <= LIMIT


def test_small_output_is_written_whole(tmp_path):
    out = _outputs(2, width=1000)
    bench.dump_outputs(out, str(tmp_path))
    assert "pcm_columns.npy" not in os.listdir(tmp_path)
    assert np.array_equal(np.load(tmp_path / "pcm.npy"), out["pcm"].astype(np.float32))


def test_calls_of_one_step_are_merged_in_call_order():
    a, b = _outputs(2, width=10, seed=1), _outputs(3, width=12, seed=2)
    m = bench.merge_calls([a, b])
    assert m["pcm"].shape == (5, 12)
    assert np.array_equal(m["pcm"][:2, :10], a["pcm"]) and not m["pcm"][:2, 10:].any()
    assert np.array_equal(m["pcm"][2:], b["pcm"])
    assert np.array_equal(m["lengths"], np.r_[a["lengths"], b["lengths"]])
    assert np.array_equal(m["peaks"], np.r_[a["peaks"], b["peaks"]])
    assert m["l_max"] == 12 and m["ty_max"] == 768
    assert bench.merge_calls([a]) is a


class _Handle:
    """Stands in for an engine handle: returns the utterance number it was given, after a random delay."""

    def __init__(self, rng, lock):
        self.rng, self.lock = rng, lock

    def run(self, ids, lengths, scales, sid, *, utterance_base, **kw):
        with self.lock:
            delay = self.rng.random() * 2e-3
        time.sleep(delay)
        return {"utterance_base": utterance_base}


def _workload(n_handles, B=4):
    w = object.__new__(bench.Workload)
    rng, lock = random.Random(3), threading.Lock()
    w.engines = [_Handle(rng, lock) for _ in range(n_handles)]
    w.B, w.rank, w.world = B, 0, 1
    w.ids, w.lengths = np.zeros((B, 3), np.int64), np.full(B, 3, np.int64)
    w.scales, w.sid, w.forced = np.zeros(3, np.float32), None, np.ones((B, 3), np.int32)
    return w


@pytest.mark.parametrize("handles", [1, 3])
def test_run_steps_returns_the_last_steps_in_step_order(handles):
    w = _workload(handles)
    n = 40
    assert [o["utterance_base"] for o in w.run_steps(n)] == [(n - 1) * w.B]
    assert [o["utterance_base"] for o in w.run_steps(n, keep=4)] == [i * w.B for i in range(n - 4, n)]
    assert [o["utterance_base"] for o in w.run_steps(2, keep=4)] == [0, w.B]
