#!/usr/bin/env python3
"""Pin voices with the deterministic duration predictor (use_sdp = false) against HuggingFace ``VitsModel``.

TEST INFRASTRUCTURE, CPU only (needs ``transformers``).  ``VitsModel(use_stochastic_duration_prediction=False)`` is an
independent implementation of upstream VITS with ``DurationPredictor``.  For a tiny ResBlock1 graph, single- and
multi-speaker, this script copies one set of seeded synthetic weights into it (everything but the duration predictor
through ``oracle/hf_crosscheck.build_hf``), runs zero-noise inference and writes

    tests/golden/hf_tiny_detdp.npz
    tests/golden/hf_tiny_detdp_multispeaker.npz

with the ids, lengths, weights and HF's logw, durations and audio (of the batch, and of every row run alone).  The test suite reads only these files.

Run from the repo root:  ``python tools/make_detdp_golden.py``
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from oracle.hf_crosscheck import build_hf, hf_resblock1_config  # noqa: E402
from tests.detdp_util import DetOracle, det_config  # noqa: E402


def build_hf_det(cfg: VitsConfig, weights):
    """HF VitsModel with the deterministic predictor: the rest of the graph loaded by build_hf (through an SDP twin of the
    config with placeholder SDP tensors), the predictor's tensors copied by name."""
    from transformers import VitsModel

    sdp = VitsConfig(**{**cfg.__dict__})
    sdp.use_sdp = True
    filler = W.synthetic_weights(sdp, seed=0)
    twin = build_hf(sdp, {**filler, **{k: v for k, v in weights.items() if not k.startswith("dp.")}})
    hf_cfg = twin.config
    hf_cfg.use_stochastic_duration_prediction = False
    hf_cfg.duration_predictor_filter_channels = cfg.dp_filter_channels
    hf_cfg.duration_predictor_kernel_size = cfg.dp_kernel_size
    hf_cfg.duration_predictor_dropout = 0.0
    torch.manual_seed(0)
    model = VitsModel(hf_cfg).eval()
    sd = {k: v for k, v in twin.state_dict().items() if not k.startswith("duration_predictor.")}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    for hf, ours in (("conv_1", "dp.conv_1"), ("conv_2", "dp.conv_2"), ("proj", "dp.proj"), ("cond", "dp.cond")):
        if ours + ".weight" in weights:
            sd[f"duration_predictor.{hf}.weight"] = t(weights[ours + ".weight"])
            sd[f"duration_predictor.{hf}.bias"] = t(weights[ours + ".bias"])
    for n in ("norm_1", "norm_2"):
        sd[f"duration_predictor.{n}.weight"] = t(weights[f"dp.{n}.gamma"])
        sd[f"duration_predictor.{n}.bias"] = t(weights[f"dp.{n}.beta"])
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith("posterior_encoder.") for k in missing), [k for k in missing if not k.startswith("posterior_encoder.")]
    return model


def run(cfg: VitsConfig, seed: int, ids: np.ndarray, lengths: np.ndarray, sid, path: str, tag: str):
    weights = W.synthetic_weights(cfg, seed=seed, frames_per_id=3.0)
    model = build_hf_det(cfg, weights)
    logw = {}

    def keep(module, inputs, output):
        logw["v"] = output.detach().numpy().copy()

    model.duration_predictor.register_forward_hook(keep)
    am = (np.arange(ids.shape[1])[None, :] < lengths[:, None]).astype(np.int64)
    with torch.no_grad():
        out = model(torch.from_numpy(ids), attention_mask=torch.from_numpy(am),
                    speaker_id=None if sid is None else int(sid[0]))  # HF takes one speaker per call
    wave, hf_len, hf_logw = out.waveform.numpy(), out.sequence_lengths.numpy(), logw["v"]
    w_ceil = np.ceil(np.exp(hf_logw) * am[:, None, :]).astype(np.int64)[:, 0]
    # sanity: the oracle with this predictor agrees with HF (same durations, audio well inside the suite's HF tolerance)
    ref = DetOracle(cfg, weights).infer(ids, lengths, [0.0, 1.0, 0.0], sid=sid, batch_semantics="upstream")
    assert np.array_equal(ref["w_ceil"][:, 0].astype(np.int64), w_ceil), (ref["w_ceil"], w_ceil)
    assert np.array_equal(ref["audio_lengths"], hf_len), (ref["audio_lengths"], hf_len)
    for b in range(ids.shape[0]):
        L = int(hf_len[b])
        a, r = ref["audio"][b, 0, :L], wave[b, :L]
        rel = float(np.sqrt(np.mean((a - r) ** 2)) / np.sqrt(np.mean(r ** 2)))
        print(f"[{tag}] utt {b}: L={L} frames={int(w_ceil[b].sum())} rel_rms(oracle vs HF)={rel:.3e} "
              f"max|dlogw|={np.abs(ref['logw'][b] - hf_logw[b]).max():.2e}")
        assert rel < 2e-5, rel
    # every row alone as well: HF decodes a padded batch unmasked, the engine (like the reference, one utterance per call) does not
    solo = np.zeros_like(wave)
    for b in range(ids.shape[0]):
        n = int(lengths[b])
        with torch.no_grad():
            o1 = model(torch.from_numpy(ids[b:b + 1, :n]), speaker_id=None if sid is None else int(sid[b]))
        assert int(o1.sequence_lengths[0]) == int(hf_len[b])
        solo[b, : int(hf_len[b])] = o1.waveform.numpy()[0, : int(hf_len[b])]
    extra = {} if sid is None else {"sid": sid}
    np.savez_compressed(path, config_json=np.array(cfg.to_json()), ids=ids, lengths=lengths, hf_logw=hf_logw,
                        hf_w_ceil=w_ceil, hf_waveform=wave, hf_waveform_rows=solo, hf_lengths=hf_len, **extra,
                        **{"w:" + k: v for k, v in weights.items()})
    print(tag, "->", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    rng = np.random.default_rng(17)
    cfg = det_config(hf_resblock1_config(VitsConfig.tiny()), 64)
    ids = rng.integers(1, cfg.num_symbols, size=(3, 12)).astype(np.int64)
    lengths = np.array([12, 7, 9], dtype=np.int64)
    for b in range(3):
        ids[b, lengths[b]:] = 0
    run(cfg, 21, ids, lengths, None, os.path.join(gold, "hf_tiny_detdp.npz"), "tiny-detdp")

    cfg_ms = det_config(hf_resblock1_config(VitsConfig.tiny(n_speakers=5)), 64)
    ids1 = rng.integers(1, cfg_ms.num_symbols, size=(1, 10)).astype(np.int64)
    len1 = np.array([10], dtype=np.int64)
    run(cfg_ms, 22, ids1, len1, np.array([3]), os.path.join(gold, "hf_tiny_detdp_multispeaker.npz"), "tiny-detdp-ms")


if __name__ == "__main__":
    main()
