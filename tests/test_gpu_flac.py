"""Device twin of tests/test_flac.py (pytest -m gpu): mi355vits_set_output_compression and the FLAC kernels on the MI355X.  The
yardsticks are tests/flac_ref.py (a numpy encoder of DESIGN.md §4.15's rules and a decoder written separately from it) and the
device's own int16 packed stream, which is older than the setting.  Every hook input is at most 3 * 4096 + 777 samples — four
frames, one per workgroup —, so the second trip of a workgroup through k_flac_frames' persistent loop is reached through the engine:
the 48-row request carries enough silence for more frames than the grid has workgroups, and its file is decoded."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_cases as C  # noqa: E402
import flac_ref as F  # noqa: E402

from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from tests.test_flac import KEYS, SCALES, SEED, VECTORS, VOLUMES, _inputs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(VECTORS)))
def test_fixed_vectors(gpu_hooks, i):
    x, rate, hexed = VECTORS[i]
    assert gpu_hooks.lab_flac(x, rate)[0].hex() == hexed


@pytest.mark.parametrize("name", sorted(C.CONTENTS))
def test_kernel_files_are_the_yardsticks(gpu_hooks, name):
    for n in C.LENGTHS:
        C.check_hook(gpu_hooks, name, n)


@pytest.mark.parametrize("rate", C.RATES)
def test_kernel_rate_forms(gpu_hooks, rate):
    for name, n in (("speech", 4097), ("constant", 5), ("noise", 257)):
        C.check_hook(gpu_hooks, name, n, rate)


@pytest.mark.parametrize("first_frame", C.FIRST_FRAMES)
def test_kernel_frame_number_widths(gpu_hooks, first_frame):
    C.check_hook(gpu_hooks, "speech", 4096 + 100, 22050, first_frame)


@pytest.mark.parametrize("offset", [1, 3, 4, 7])
def test_kernel_input_at_an_odd_offset(gpu_hooks, offset):
    C.check_hook(gpu_hooks, "speech", C.LONGEST, offset=offset)
    C.check_hook(gpu_hooks, "full_scale_alternating", 4097, offset=offset)


def test_empty_stream_is_its_header(gpu_hooks):
    file, sizes = gpu_hooks.lab_flac(np.zeros(0, np.int16), 22050)
    assert file == F.encode(np.zeros(0, np.int16), 22050) and sizes.shape == (0,)


@pytest.mark.parametrize("setting", C.SETTINGS)
def test_flac_pack_decodes_to_the_s16_pack(gpu_lib, setting):
    """The tiny voice, 3 ragged rows, a reordered pack with silences of 0 / 9000 / 100 samples and a tail."""
    cfg = VitsConfig.tiny()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=31)), device=0, library=gpu_lib)
    C.apply_settings(eng, setting)
    ids, lens = _inputs(cfg)
    rate = eng.output_rate
    ran = eng.run_packed(ids, lens, SCALES, None, seed=SEED, utterance_keys=KEYS, pcm_volume=VOLUMES, compression="flac", **C.PACK)
    s16, fl = C.check_flac_pack(eng, rate)
    assert bytes(ran.flac) == bytes(fl.flac)  # run_packed is fetch_packed
    assert s16.total_samples > 2 * F.BLOCK and s16.total_samples % F.BLOCK
    if setting == "trim_loudness_limiter_true_peak":
        assert fl.first is not None and fl.limited is not None and fl.limited.any()
    # off after on: the raw stream is the raw stream
    assert eng.output_compression is None
    assert np.array_equal(eng.fetch_packed(**C.PACK).pcm, s16.pcm)
    eng.close()


def test_48_ragged_rows_at_8000_hz(gpu_lib):
    """48 ragged rows of 20 .. 64 ids with natural durations, noise on, per-row scales, volumes and keys at 8000 Hz, a permutation with
    silences: the FLAC file decodes to the S16LE twin of the same run, and the profile names the launches with their bytes.  The
    silences (up to 25 s each) make more than 1,536 frames — the grid is three workgroups per CU, 768 on an MI355X —, so every workgroup
    encodes several frames in a row, frames of audio and constant frames of silence in turn."""
    cfg = VitsConfig.vctk_low()
    eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=141, frames_per_id=3.0)), device=0, library=gpu_lib)
    eng.set_output_rate(8000)
    B = 48
    rng = np.random.default_rng(141)
    lens = rng.integers(20, 65, B).astype(np.int64)
    lens[0], lens[B // 2] = 64, 20
    ids = np.zeros((B, 64), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    sid = (np.arange(B) % cfg.n_speakers).astype(np.int64) if cfg.is_multispeaker else None
    scales = np.stack([rng.uniform(0.3, 0.9, B), rng.uniform(0.8, 1.3, B), rng.uniform(0.2, 1.0, B)], axis=1).astype(np.float32)
    vol = rng.choice([0.5, 1.0, 1.5, 3.0, 0.075], B)
    keys = [int(k) for k in rng.integers(0, 1 << 40, B)]
    order = [int(b) for b in rng.permutation(B) if b != 17]
    lead = [int(v) for v in rng.integers(160000, 200001, len(order))]
    lead[:3] = [0, 1, 777]
    pack = dict(order=order, lead_samples=lead, tail_samples=801)
    eng.run_packed(ids, lens, scales, sid, seed=SEED, utterance_keys=keys, pcm_volume=vol, **pack)
    eng.profile_enable(True)
    eng.profile_reset()
    s16, fl = C.check_flac_pack(eng, 8000, pack, encode_too=False)
    rep = eng.profile_report()
    assert rep["pack.flac"]["calls"] == 1 and rep["pcm16.pack"]["calls"] == 2
    assert rep["pack.flac"]["bytes"] == 2 * fl.total_samples + (len(fl.flac) - 42)
    assert len({int(v) for v in s16.lengths}) > B // 2 and any(int(o) % 8 for o in s16.offsets)
    kinds = [f[2] for f in F.decode_frames(bytes(fl.flac))[2]]
    assert len(kinds) > 1536 and 400 > sum(k != 0 for k in kinds) > 80  # constant frames of silence with the frames of audio among them
    print(f"pack.flac, 48 ragged rows at 8000 Hz: {rep['pack.flac']['ms']:.4f} ms, {len(fl.flac)} bytes for {s16.total_samples} samples "
          f"(ratio {len(fl.flac) / (2 * s16.total_samples):.4f}; synthetic voice, not speech)")
    eng.profile_enable(False)
    eng.close()
