"""Test-only helpers for voices with the deterministic duration predictor (``use_sdp = false``).

``oracle/vits_oracle.py`` has no such predictor, so the reference here restates upstream ``models.DurationPredictor``
(inference) in torch, in the oracle's own precision (float64 for the ``logw`` reference), and ``DetOracle`` swaps it in
for the stochastic one; everything else in the graph is the oracle's.  ``export_detdp_onnx`` traces that graph into a
``generator.onnx`` the way ``tests/onnx_fixture.py`` does for stochastic voices."""
from __future__ import annotations

import io
import warnings

import numpy as np
import torch
import torch.nn.functional as Fn

from mimic3_amd import weights as W
from mimic3_amd.config import VitsConfig
from oracle.vits_oracle import VitsOracle


def det_config(base: VitsConfig, filter_channels: int = 256) -> VitsConfig:
    c = VitsConfig(**{**base.__dict__})
    c.use_sdp = False
    c.dp_filter_channels = filter_channels
    c.validate()
    return c


def det_weights(cfg: VitsConfig, seed: int, frames_per_id: float = 3.0):
    return W.synthetic_weights(cfg, seed=seed, frames_per_id=frames_per_id)


def det_logw(w, x, x_mask, g=None, cond=None):
    """upstream DurationPredictor.forward at inference (dropout off): the restatement every test compares against.
    ``w``: tensors by name (torch); ``g`` [B, gin, 1] or None; ``cond(name, g)`` applies a 1x1 conv."""
    K = w["dp.conv_1.weight"].shape[2]

    def ln(name, h):
        mean = h.mean(1, keepdim=True)
        var = ((h - mean) ** 2).mean(1, keepdim=True)
        return (h - mean) * torch.rsqrt(var + 1e-5) * w[name + ".gamma"].view(1, -1, 1) + w[name + ".beta"].view(1, -1, 1)

    if g is not None:
        x = x + Fn.conv1d(g, w["dp.cond.weight"], w["dp.cond.bias"])
    h = ln("dp.norm_1", torch.relu(Fn.conv1d(x * x_mask, w["dp.conv_1.weight"], w["dp.conv_1.bias"], padding=K // 2)))
    h = ln("dp.norm_2", torch.relu(Fn.conv1d(h * x_mask, w["dp.conv_2.weight"], w["dp.conv_2.bias"], padding=K // 2)))
    return Fn.conv1d(h * x_mask, w["dp.proj.weight"], w["dp.proj.bias"]) * x_mask


class DetOracle(VitsOracle):
    """VitsOracle with the deterministic predictor in place of the stochastic one (noise_w is not used, as upstream)."""

    def duration_predictor(self, x, x_mask, g, noise_w, noise):
        return det_logw(self.w, x, x_mask, g)


def logw_ref(cfg: VitsConfig, w, ids, lengths, sid=None) -> np.ndarray:
    """float64 logw [B, 1, Tx] of the whole text side (encoder + predictor)."""
    o = DetOracle(cfg, w, dtype=torch.float64)
    ids_t = torch.as_tensor(np.asarray(ids), dtype=torch.long)
    x, _, _, x_mask = o.text_encoder(ids_t, torch.as_tensor(np.asarray(lengths), dtype=torch.long))
    g = None
    if cfg.is_multispeaker:
        g = o.w["emb_g.weight"][torch.as_tensor(np.asarray(sid), dtype=torch.long)].unsqueeze(-1)
    return o.duration_predictor(x, x_mask, g, None, None).numpy()


def check_durations(w_ceil, logw64, lengths, length_scale=1.0, max_excluded=0.001):
    """w_ceil [B, (1,) Tx] of the engine against ceil(exp(logw64) * length_scale): equal at every valid phoneme whose float64
    w is more than 1e-5 w from an integer (a different summation order may move ceil at a knife edge).  At most
    ``max_excluded`` of the phonemes may be excluded.  length_scale: scalar or [B].  Returns the number excluded."""
    w_ceil = np.asarray(w_ceil).reshape(len(lengths), -1)
    lw = np.asarray(logw64, np.float64).reshape(len(lengths), -1)
    ls = np.broadcast_to(np.asarray(length_scale, np.float64).reshape(-1, 1), lw.shape)
    wv = np.exp(lw) * ls
    valid = np.arange(lw.shape[1])[None, :] < np.asarray(lengths)[:, None]
    edge = np.abs(wv - np.round(wv)) <= 1e-5 * wv
    keep = valid & ~edge
    want = np.ceil(wv)
    bad = np.argwhere(keep & (w_ceil != want))
    assert bad.size == 0, f"durations differ at {bad[:5].tolist()}: {w_ceil[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    assert np.all(w_ceil[~valid] == 0)
    n_ex = int((valid & edge).sum())
    assert n_ex <= max_excluded * max(1, int(valid.sum())), (n_ex, int(valid.sum()))
    return n_ex


def export_detdp_onnx(cfg: VitsConfig, weights, weight_norm_prefixes=("flow.",), opset: int = 13) -> bytes:
    """Bytes of a ``generator.onnx`` of a deterministic-predictor voice (TorchScript exporter, constant folding on)."""
    from torch.onnx._internal.torchscript_exporter import onnx_proto_utils

    from tests.onnx_fixture import TraceableGenerator

    model = TraceableGenerator(cfg, weights, weight_norm_prefixes).eval()
    tree = model.oracle.w
    model.oracle.duration_predictor = lambda x, x_mask, g, noise_w, noise: det_logw(tree, x, x_mask, g)
    Tx = 7
    args = [torch.randint(1, cfg.num_symbols, (1, Tx)), torch.tensor([Tx]), torch.tensor([0.667, 1.0, 0.8])]
    names = ["input", "input_lengths", "scales"]
    if cfg.is_multispeaker:
        args.append(torch.tensor([0]))
        names.append("sid")
    saved = onnx_proto_utils._add_onnxscript_fn
    onnx_proto_utils._add_onnxscript_fn = lambda proto, custom_opsets: proto
    buf = io.BytesIO()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.onnx.export(model, tuple(args), buf, dynamo=False, input_names=names, output_names=["output"],
                              opset_version=opset, do_constant_folding=True,
                              dynamic_axes={"input": {0: "batch", 1: "phonemes"}, "input_lengths": {0: "batch"},
                                            "output": {0: "batch", 2: "time"}})
    finally:
        onnx_proto_utils._add_onnxscript_fn = saved
    return buf.getvalue()
