"""Voices with the deterministic duration predictor (use_sdp = false; upstream models.DurationPredictor): config and
container, ONNX import, and the engine on the CPU model of the kernels (tests/emu).  test_gpu_det_dp.py runs the engine
side on the MI355X.

References: logw = the float64 restatement in tests/detdp_util.py; the waveform = the oracle with the engine's durations
forced (the predictor is the only part of the graph that differs from a stochastic voice); and HF VitsModel's outputs frozen
in tests/golden/hf_tiny_detdp*.npz by tools/make_detdp_golden.py."""
import hashlib
import json
import os

import numpy as np
import pytest

from mimic3_amd import onnx_import as OI
from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError
from mimic3_amd.config import VitsConfig
from tests import onnx_writer as OW
from tests.detdp_util import DetOracle, check_durations, det_config, det_weights, export_detdp_onnx, logw_ref
from tests.util import TIGHT_REL_RMS_TOL, make_inputs, rel_rms

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DET_TENSORS = {"dp.conv_1.weight", "dp.conv_1.bias", "dp.norm_1.gamma", "dp.norm_1.beta", "dp.conv_2.weight", "dp.conv_2.bias",
               "dp.norm_2.gamma", "dp.norm_2.beta", "dp.proj.weight", "dp.proj.bias"}
# sha256 of W.pack(apope_low, synthetic_weights(seed 7, 3 frames per id)) as the stochastic-only code wrote it
APOPE_LOW_CONTAINER_SHA256 = "fd5ef2c9dd8117e1d38c6086d273748e02015feafca5be75abad111d380717e2"


# ------------------------------------------------------------------------------------------------ config and container
def test_config_validates_and_lists_the_predictor_tensors():
    cfg = det_config(VitsConfig.apope_low())
    specs = W.tensor_specs(cfg)
    dp = {k for k in specs if k.startswith("dp.")}
    assert dp == DET_TENSORS
    H, F, K = cfg.hidden_channels, cfg.dp_filter_channels, cfg.dp_kernel_size
    assert specs["dp.conv_1.weight"] == (F, H, K) and specs["dp.conv_2.weight"] == (F, F, K)
    assert specs["dp.proj.weight"] == (1, F, 1) and specs["dp.proj.bias"] == (1,) and specs["dp.norm_2.beta"] == (F,)
    ms = W.tensor_specs(det_config(VitsConfig.vctk_low()))
    assert {k for k in ms if k.startswith("dp.")} == DET_TENSORS | {"dp.cond.weight", "dp.cond.bias"}
    assert ms["dp.cond.weight"] == (H, 512, 1)
    with pytest.raises(ValueError):
        det_config(VitsConfig.tiny(), 0)


@pytest.mark.parametrize("F,n_speakers", [(256, 1), (96, 3)])
def test_pack_unpack_and_c_struct_round_trip(F, n_speakers):
    cfg = det_config(VitsConfig.tiny(n_speakers=n_speakers), F)
    w = det_weights(cfg, seed=4)
    c = cfg.to_c()
    assert (c.dp_n_flows, c.dp_dds_layers, c.dp_num_bins) == (0, 0, 0)
    assert VitsConfig.from_c(c).use_sdp is False
    cfg2, w2 = W.unpack(W.pack(cfg, w))
    assert cfg2 == cfg and cfg2.dp_filter_channels == F
    assert set(w2) == set(w)
    for k in w:
        assert np.array_equal(w2[k], w[k]), k
    # natural durations land near frames_per_id
    assert abs(float(w["dp.proj.bias"][0]) - np.log(3.0)) < 1e-6


def test_trainer_config_json_with_use_sdp_false_loads():
    d = json.loads(VitsConfig.apope_low().to_json())
    trainer = {"model": {k: v for k, v in d["model"].items()}, "audio": d["audio"], "inference": d["inference"]}
    trainer["model"]["use_sdp"] = False
    cfg = VitsConfig.from_json(json.dumps(trainer))
    assert cfg.use_sdp is False and cfg.dp_filter_channels == 256
    assert VitsConfig.from_json(cfg.to_json()) == cfg


def test_stochastic_voice_containers_are_unchanged():
    cfg = VitsConfig.apope_low()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=7, frames_per_id=3.0))
    assert hashlib.sha256(blob).hexdigest() == APOPE_LOW_CONTAINER_SHA256
    assert W.unpack(blob)[0].use_sdp is True


# ------------------------------------------------------------------------------------------------ ONNX import
def _det_voice(n_speakers):
    cfg = det_config(VitsConfig.tiny(n_speakers=n_speakers), 64)
    return cfg, det_weights(cfg, seed=30 + n_speakers)


@pytest.mark.parametrize("n_speakers", [1, 3])
def test_onnx_import_named(n_speakers):
    cfg, w = _det_voice(n_speakers)
    blob = export_detdp_onnx(cfg, w)
    cfg2, t = OI.import_onnx_bytes(blob)
    assert cfg2.use_sdp is False and cfg2.dp_filter_channels == 64 and cfg2.dp_kernel_size == 3
    assert cfg2.n_speakers == cfg.n_speakers
    assert set(t) == set(w)
    for k in w:
        if k.startswith("dp."):
            assert np.array_equal(t[k], w[k]), k
    cfg3, _ = W.unpack(OI.onnx_to_m355_bytes(blob))
    assert cfg3.use_sdp is False and cfg3.dp_filter_channels == 64


@pytest.mark.parametrize("n_speakers", [1, 3])
def test_onnx_import_without_predictor_names(n_speakers):
    """Every tensor of the predictor anonymous: the traced export already folds the LayerNorm parameters into anonymous
    constants (placed by first-use order); here the conv weights and biases lose their names too (placed by the conv
    execution order), and the kernel size comes from the Conv node."""
    cfg, w = _det_voice(n_speakers)
    m = OI.parse_model(export_detdp_onnx(cfg, w))
    assert not [n for n in m.initializers if ".dp.norm_" in n]
    rename = {n: f"onnx::Anon_{9000 + i}" for i, n in enumerate(m.initializers) if ".dp." in n and not n.endswith("dp.conv_1.bias")}
    assert len(rename) == 5 + (2 if n_speakers > 1 else 0)
    cfg2, t = OI.import_onnx_bytes(OW.rewrite(m, rename=rename))
    assert cfg2.use_sdp is False and cfg2.dp_filter_channels == 64 and cfg2.dp_kernel_size == 3
    for k in w:
        if k.startswith("dp."):
            assert np.array_equal(t[k], w[k]), k
    # and with the conv_1 bias anonymous too, config.json supplies use_sdp / F
    rename.update({n: "onnx::Anon_8999" for n in m.initializers if n.endswith("dp.conv_1.bias")})
    cfg3, t3 = OI.import_onnx_bytes(OW.rewrite(m, rename=rename), declared=VitsConfig.from_json(cfg.to_json()))
    assert cfg3.use_sdp is False
    for k in w:
        if k.startswith("dp."):
            assert np.array_equal(t3[k], w[k]), k


def test_execution_orders_cover_the_inventory():
    for cfg in (det_config(VitsConfig.apope_low()), det_config(VitsConfig.vctk_low())):
        specs = W.tensor_specs(cfg)
        convs = OI.conv_execution_order(cfg)
        points = OI.pointwise_execution_order(cfg)
        assert [c for c in convs if c.startswith("dp.")] == (["dp.cond"] if cfg.is_multispeaker else []) + ["dp.conv_1", "dp.conv_2", "dp.proj"]
        assert [p for p in points if p.startswith("dp.")] == ["dp.norm_1.gamma", "dp.norm_1.beta", "dp.norm_2.gamma", "dp.norm_2.beta"]
        biases = {n for n in specs if n.endswith(".bias")}
        assert {c + ".weight" for c in convs} | set(points) | biases == set(specs)


def test_describe_and_convert_name_the_predictor(tmp_path, capsys):
    cfg, w = _det_voice(1)
    p = tmp_path / "generator.onnx"
    p.write_bytes(export_detdp_onnx(cfg, w))
    assert "deterministic" in OI.describe(str(p))
    assert OI.main([str(p)]) == 0
    assert "deterministic" in capsys.readouterr().err
    assert W.load(str(tmp_path / "generator.m355"))[0].use_sdp is False


# ------------------------------------------------------------------------------------------------ engine (CPU model)
def _run_and_check(eng, cfg, w, ids, lens, sid, scales=(0.0, 1.0, 0.0)):
    out = eng.run(ids, lens, scales, sid, want_pcm16=True, debug_taps=True)
    lw = eng.tap("logw")
    ref = logw_ref(cfg, w, ids, lens, sid)
    assert lw.shape == ref.shape
    assert np.abs(lw - ref).max() <= 1e-5, np.abs(lw - ref).max()
    excluded = check_durations(eng.tap("w_ceil"), ref, lens, scales[1])
    wc = eng.tap("w_ceil").reshape(len(lens), -1).astype(np.int64)
    o = DetOracle(cfg, w).infer(ids, lens, scales, sid=sid, forced_durations=wc)
    assert np.array_equal(out["lengths"], o["audio_lengths"])
    for b in range(len(lens)):
        L = int(out["lengths"][b])
        assert rel_rms(out["audio"][b, :L], o["audio"][b, 0, :L]) < TIGHT_REL_RMS_TOL
    return out, excluded


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("n_speakers,resblock,F", [(1, "2", 64), (3, "2", 96), (1, "1", 256), (4, "1", 64)])
def test_engine_matches_the_restated_predictor(emu_lib, math, n_speakers, resblock, F):
    cfg = det_config(VitsConfig.tiny(n_speakers=n_speakers, resblock=resblock), F)
    w = det_weights(cfg, seed=40 + F)
    eng = Engine(W.pack(cfg, w), library=emu_lib)
    eng.set_math(math)
    ids, lens, sid = make_inputs(cfg, 3, 13, seed=F)  # ragged B = 3
    out, excluded = _run_and_check(eng, cfg, w, ids, lens, sid)
    print(f"{math} F={F}: {excluded} knife-edge phonemes excluded")
    eng.close()


def test_long_rows_cross_tiles_and_a_wide_encoder(emu_lib):
    """Rows longer than one workgroup's tile (62 columns) and the real hidden width (192)."""
    cfg = det_config(VitsConfig.tiny_h192(), 64)
    w = det_weights(cfg, seed=5)
    eng = Engine(W.pack(cfg, w), library=emu_lib)
    ids, lens, sid = make_inputs(cfg, 2, 130, seed=3)
    lens[1] = 63
    ids[1, 63:] = 0
    _run_and_check(eng, cfg, w, ids, lens, sid, scales=(0.0, 0.8, 0.0))
    eng.close()


def test_noise_w_is_ignored_and_noise_scale_is_not(emu_lib):
    cfg = det_config(VitsConfig.tiny(), 64)
    eng = Engine(W.pack(cfg, det_weights(cfg, seed=6)), library=emu_lib)
    ids, lens, _ = make_inputs(cfg, 2, 11, seed=6)
    a = eng.run(ids, lens, [0.667, 1.0, 0.8], seed=9)
    b = eng.run(ids, lens, [0.667, 1.0, 0.0], seed=9)
    c = eng.run(ids, lens, [0.667, 1.0, 2.5], seed=9)
    for r in (b, c):
        assert np.array_equal(a["lengths"], r["lengths"]) and np.array_equal(a["audio"], r["audio"])
    d = eng.run(ids, lens, [0.3, 1.0, 0.8], seed=9)
    assert not np.array_equal(a["audio"], d["audio"])
    with pytest.raises((NativeError, ValueError)):
        eng.run(ids, lens, [0.667, 1.0, -0.1])
    eng.close()


@pytest.mark.parametrize("n_speakers", [1, 3])
def test_batched_rows_equal_their_solo_runs(emu_lib, n_speakers):
    cfg = det_config(VitsConfig.tiny(n_speakers=n_speakers), 64)
    w = det_weights(cfg, seed=8)
    eng = Engine(W.pack(cfg, w), library=emu_lib)
    ids, lens, sid = make_inputs(cfg, 4, 70, seed=8)
    scales = np.array([[0.0, 1.0, 0.0], [0.5, 0.7, 0.8], [0.0, 1.3, 0.0], [0.2, 1.0, 0.3]], np.float32)
    keys = [5, 11, 2, 40]
    full = eng.run(ids, lens, scales, sid, seed=3, utterance_keys=keys, debug_taps=True)
    wfull = eng.tap("w_ceil").reshape(4, -1)
    check_durations(wfull, logw_ref(cfg, w, ids, lens, sid), lens, scales[:, 1])
    for b in range(4):
        n = int(lens[b])
        one = eng.run(ids[b:b + 1, :n], [n], scales[b], None if sid is None else sid[b:b + 1], seed=3, utterance_base=keys[b],
                      debug_taps=True)
        L = int(one["lengths"][0])
        assert L == int(full["lengths"][b])
        assert np.array_equal(one["audio"][0, :L], full["audio"][b, :L]), b
        assert np.array_equal(eng.tap("w_ceil").reshape(-1)[:n], wfull[b, :n]), b
    eng.close()


def test_forced_durations_still_override(emu_lib):
    cfg = det_config(VitsConfig.tiny(), 64)
    w = det_weights(cfg, seed=9)
    eng = Engine(W.pack(cfg, w), library=emu_lib)
    ids, lens, _ = make_inputs(cfg, 2, 9, seed=9)
    forced = np.full((2, 9), 2, np.int32)
    out = eng.run(ids, lens, [0.0, 1.0, 0.0], forced_durations=forced)
    assert list(out["lengths"]) == [2 * int(n) * cfg.hop_length for n in lens]
    o = DetOracle(cfg, w).infer(ids, lens, [0, 1, 0], forced_durations=forced)
    for b in range(2):
        L = int(out["lengths"][b])
        assert rel_rms(out["audio"][b, :L], o["audio"][b, 0, :L]) < TIGHT_REL_RMS_TOL
    eng.close()


def test_unsupported_filter_width_is_a_clean_error(emu_lib):
    cfg = det_config(VitsConfig.tiny(), 48)  # not a multiple of 32
    with pytest.raises(NativeError, match="deterministic duration predictor"):
        Engine(W.pack(cfg, det_weights(cfg, seed=1)), library=emu_lib)


@pytest.mark.parametrize("name", ["hf_tiny_detdp.npz", "hf_tiny_detdp_multispeaker.npz"])
def test_engine_against_hf_vits_fixture(emu_lib, name):
    g = np.load(os.path.join(GOLDEN, name))
    cfg = VitsConfig.from_json(str(g["config_json"]))
    assert cfg.use_sdp is False
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    sid = g["sid"] if "sid" in g.files else None
    eng = Engine(W.pack(cfg, w), library=emu_lib)
    out = eng.run(g["ids"], g["lengths"], [0.0, 1.0, 0.0], sid, debug_taps=True)
    assert np.array_equal(eng.tap("w_ceil").reshape(len(g["lengths"]), -1), g["hf_w_ceil"])
    assert np.abs(eng.tap("logw") - g["hf_logw"]).max() < 1e-5
    assert np.array_equal(out["lengths"], g["hf_lengths"])
    for b in range(len(g["lengths"])):
        L = int(g["hf_lengths"][b])
        assert rel_rms(out["audio"][b, :L], g["hf_waveform_rows"][b, :L]) < 2e-5  # rows of a batch are their solo runs
    eng.close()
