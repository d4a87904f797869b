"""Device twin of tests/test_speaker_mix.py (pytest -m gpu): mi355vits_run_speakers and k_speaker_cond_mix on the MI355X.  The same
checks against the same yardstick (tests/speaker_ref.py), bit for bit, and once the released multi-speaker shape (vctk_low: 109
speakers, gin 512) with two-term mixes."""
import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from tests import speaker_ref as SR
from tests.test_speaker_mix import (KERNEL_CASES, KERNEL_CASES_WIDE, MIXES, augmented, check_composes, check_errors, check_identities,
                                    check_kernel_alone, check_whole_run, oracle_for, voice)
from tests.test_timing import SCALES, SEED, feed

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", KERNEL_CASES + KERNEL_CASES_WIDE, ids=lambda c: "gin%d-B%d-K%d-%djobs" % (c["gin"], c["B"], c["K"], len(c["couts"])))
def test_kernel_alone_matches_the_yardstick_and_k_speaker_cond(gpu_hooks, c):
    check_kernel_alone(gpu_hooks, c)


@pytest.mark.parametrize("kind", ["tiny", "h192", "det"])
def test_a_mixed_run_identities_rows_alone_and_permutation(gpu_lib, kind):
    cfg, w = voice(kind)
    a = feed(cfg)
    make = lambda blob: Engine(blob, device=0, library=gpu_lib)  # noqa: E731
    eng, mixed, g = check_whole_run(make, cfg, w, a, MIXES, oracle_row=2 if kind != "h192" else None, oracle=oracle_for(kind))
    blob = W.pack(cfg, w)
    check_identities(eng, lambda: make(blob), a, MIXES, mixed, g)
    eng.close()


def test_composes_with_timing_output_forms_and_the_launch_list(gpu_lib):
    cfg, w = voice("tiny")
    a = feed(cfg)
    g = SR.mix(w["emb_g.weight"], *SR.tables(MIXES))
    eng = Engine(W.pack(cfg, w), device=0, library=gpu_lib)
    eng_aug = Engine(augmented(cfg, w, g)[1], device=0, library=gpu_lib)
    check_composes(eng, eng_aug, cfg, a, MIXES)
    eng.close()
    eng_aug.close()


def test_errors(gpu_lib):
    cfg, w = voice("tiny")
    c1 = VitsConfig.tiny()
    eng = Engine(W.pack(cfg, w), device=0, library=gpu_lib)
    single = Engine(W.pack(c1, W.synthetic_weights(c1, seed=31, frames_per_id=3.0)), device=0, library=gpu_lib)
    check_errors(eng, single, feed(cfg))
    eng.close()
    single.close()


def test_the_released_multi_speaker_shape(gpu_lib):
    """vctk_low (109 speakers, gin 512) with synthetic weights, B = 8 x Tx = 16, two-term mixes: the run is bitwise the plain run on
    the voice whose emb_g carries the blended vectors as further rows, and two rows of the batch are bitwise the rows alone."""
    cfg = VitsConfig.vctk_low()
    w = W.synthetic_weights(cfg, seed=151, frames_per_id=3.0)
    rng = np.random.default_rng(8)
    B, Tx = 8, 16
    lens = rng.integers(1, Tx + 1, B).astype(np.int64)
    lens[0], lens[1] = Tx, 1
    ids = rng.integers(1, cfg.num_symbols, (B, Tx)).astype(np.int64)
    keys = [int(k) for k in rng.integers(0, 1 << 40, B)]
    mixes = [{int(s0): float(x), int(s1): float(1.0 - x)} for s0, s1, x in
             zip(rng.integers(0, 54, B), rng.integers(54, cfg.n_speakers, B), rng.uniform(-0.5, 1.5, B))]
    g = SR.mix(w["emb_g.weight"], *SR.tables(mixes))
    kw = dict(seed=SEED, utterance_keys=keys, want_float=True, want_pcm16=True)
    eng = Engine(W.pack(cfg, w), device=0, library=gpu_lib)
    out = eng.run(ids, lens, SCALES, None, speakers=mixes, debug_taps=True, **kw)
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}
    assert eng.tap("g")[:, :, 0].tobytes() == g.tobytes()
    eng2 = Engine(augmented(cfg, w, g)[1], device=0, library=gpu_lib)
    plain = eng2.run(ids, lens, SCALES, cfg.n_speakers + np.arange(B), **kw)
    for k in ("audio", "pcm", "lengths", "peaks"):
        assert out[k].tobytes() == plain[k].tobytes(), k
    eng2.close()
    for b in (0, 5):
        one = eng.run(ids[b:b + 1], lens[b:b + 1], SCALES, None, speakers=[mixes[b]], seed=SEED, utterance_keys=keys[b:b + 1],
                      want_float=True, want_pcm16=True)
        n = int(out["lengths"][b])
        assert int(one["lengths"][0]) == n and one["audio"][0, :n].tobytes() == out["audio"][b, :n].tobytes()
        assert one["pcm"][0, :n].tobytes() == out["pcm"][b, :n].tobytes() and one["peaks"].tobytes() == out["peaks"][b:b + 1].tobytes()
    eng.close()
