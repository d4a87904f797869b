"""Voices with the deterministic duration predictor (use_sdp = false) on the MI355X: k_dp_det in every math mode, against the
float64 restatement of the predictor (tests/detdp_util.py), the oracle with the engine's durations forced, HF VitsModel's
frozen outputs, and the rows' solo runs.  test_det_dp.py covers the same ground on the CPU model."""
import os

import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from oracle.vits_oracle import audio_float_to_int16
from tests.detdp_util import DetOracle, check_durations, det_config, det_weights, export_detdp_onnx, logw_ref
from tests.util import REL_RMS_TOL, TIGHT_REL_RMS_TOL, make_inputs, rel_rms

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BF16W_REL_RMS_TOL = 2e-2
SDP_KERNELS = ("dp.stack", "convflow.stack", "convflow.pre", "sdp.noise", "spline", "dds.layer")


def _check_rows(out, o, rows, tol, check_pcm=True):
    for b in rows:
        L = int(out["lengths"][b])
        assert L == int(o["audio_lengths"][b]), b
        a, r = out["audio"][b, :L], o["audio"][b, 0, :L]
        assert rel_rms(a, r) < tol, (b, rel_rms(a, r), tol)
        if check_pcm:
            assert np.array_equal(out["pcm"][b, :L], audio_float_to_int16(a))
            d = np.abs(out["pcm"][b, :L].astype(np.int32) - audio_float_to_int16(r).astype(np.int32))
            assert d.max() <= 1, (b, d.max())


@pytest.mark.parametrize("shape", ["tiny", "apope_low"])
def test_parity_in_every_math_mode(gpu_lib, shape):
    base = VitsConfig.tiny() if shape == "tiny" else VitsConfig.apope_low()
    cfg = det_config(base, 64 if shape == "tiny" else 256)
    w = det_weights(cfg, seed=51)
    ids, lens, sid = make_inputs(cfg, 2, 40, seed=51)  # ragged B = 2
    ref = logw_ref(cfg, w, ids, lens, sid)
    eng = Engine(W.pack(cfg, w), library=gpu_lib)
    lengths = {}
    for math in ("bf16x3", "f32", "f16x2", "bf16w"):
        eng.set_math(math)
        out = eng.run(ids, lens, [0.0, 1.0, 0.0], sid, want_pcm16=True, debug_taps=True)
        assert np.abs(eng.tap("logw") - ref).max() <= 1e-5, (math, np.abs(eng.tap("logw") - ref).max())
        n_ex = check_durations(eng.tap("w_ceil"), ref, lens)
        wc = eng.tap("w_ceil").reshape(2, -1).astype(np.int64)
        o = DetOracle(cfg, w).infer(ids, lens, [0, 1, 0], sid=sid, forced_durations=wc)
        lengths[math] = out["lengths"].copy()
        if math == "bf16w":
            _check_rows(out, o, range(2), BF16W_REL_RMS_TOL, check_pcm=False)
        else:
            _check_rows(out, o, range(2), TIGHT_REL_RMS_TOL if math != "f16x2" else REL_RMS_TOL, check_pcm=math != "f16x2")
        print(f"{shape} {math}: {n_ex} knife-edge phonemes excluded")
    assert np.array_equal(lengths["bf16w"], lengths["bf16x3"])  # the text side never rounds its weights
    eng.close()


def test_multispeaker_vctk_low_shape(gpu_lib):
    cfg = det_config(VitsConfig.vctk_low())
    w = det_weights(cfg, seed=52)
    ids, lens, _ = make_inputs(cfg, 32, 48, seed=52)
    sid = (np.arange(32) % 109).astype(np.int64)
    eng = Engine(W.pack(cfg, w), library=gpu_lib)
    out = eng.run(ids, lens, [0.0, 1.0, 0.0], sid, want_pcm16=True, debug_taps=True)
    ref = logw_ref(cfg, w, ids, lens, sid)
    assert np.abs(eng.tap("logw") - ref).max() <= 1e-5
    check_durations(eng.tap("w_ceil"), ref, lens)
    rows = [0, 7, 31]
    wc = eng.tap("w_ceil").reshape(32, -1).astype(np.int64)
    o = DetOracle(cfg, w).infer(ids[rows], lens[rows], [0, 1, 0], sid=sid[rows], forced_durations=wc[rows])
    sub = {k: out[k][rows] for k in ("audio", "pcm", "lengths")}
    _check_rows(sub, o, range(len(rows)), TIGHT_REL_RMS_TOL)
    eng.close()


def test_batch_256_by_128_natural_durations(gpu_lib):
    cfg = det_config(VitsConfig.apope_low())
    w = det_weights(cfg, seed=53)
    rng = np.random.default_rng(53)
    ids = rng.integers(1, cfg.num_symbols, size=(256, 128)).astype(np.int64)
    lens = np.full(256, 128, np.int64)
    lens[1::3] = rng.integers(20, 128, size=len(lens[1::3]))
    for b in range(256):
        ids[b, lens[b]:] = 0
    eng = Engine(W.pack(cfg, w), library=gpu_lib)
    out = eng.run(ids, lens, [0.0, 1.0, 0.0], want_pcm16=True, debug_taps=True)
    lw, wc = eng.tap("logw"), eng.tap("w_ceil").reshape(256, -1).astype(np.int64)
    ref = np.concatenate([logw_ref(cfg, w, ids[i:i + 32], lens[i:i + 32]) for i in range(0, 256, 32)])
    assert np.abs(lw - ref).max() <= 1e-5, np.abs(lw - ref).max()
    n_ex = check_durations(wc, ref, lens)
    print(f"256 x 128: {n_ex} of {int(lens.sum())} phonemes at a knife edge")
    rows = [0, 1, 128, 255]
    o = DetOracle(cfg, w).infer(ids[rows], lens[rows], [0, 1, 0], forced_durations=wc[rows])
    _check_rows({k: out[k][rows] for k in ("audio", "pcm", "lengths")}, o, range(4), TIGHT_REL_RMS_TOL)
    for b in rows:
        n = int(lens[b])
        one = eng.run(ids[b:b + 1, :n], [n], [0.0, 1.0, 0.0], want_pcm16=True)
        L = int(one["lengths"][0])
        assert L == int(out["lengths"][b])
        assert np.array_equal(one["audio"][0, :L], out["audio"][b, :L]), b
        assert np.array_equal(one["pcm"][0, :L], out["pcm"][b, :L]), b
    eng.close()


@pytest.mark.parametrize("name", ["hf_tiny_detdp.npz", "hf_tiny_detdp_multispeaker.npz"])
def test_hf_goldens_on_the_device(gpu_lib, name):
    g = np.load(os.path.join(GOLDEN, name))
    cfg = VitsConfig.from_json(str(g["config_json"]))
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    eng = Engine(W.pack(cfg, w), library=gpu_lib)
    out = eng.run(g["ids"], g["lengths"], [0.0, 1.0, 0.0], g["sid"] if "sid" in g.files else None, debug_taps=True)
    assert np.array_equal(eng.tap("w_ceil").reshape(len(g["lengths"]), -1), g["hf_w_ceil"])
    assert np.array_equal(out["lengths"], g["hf_lengths"])
    for b in range(len(g["lengths"])):
        L = int(g["hf_lengths"][b])
        assert rel_rms(out["audio"][b, :L], g["hf_waveform_rows"][b, :L]) < 2e-5
    eng.close()


def test_the_new_kernel_ran(gpu_lib):
    ids = np.random.default_rng(5).integers(1, 50, size=(4, 32)).astype(np.int64)
    for cfg, det in ((det_config(VitsConfig.apope_low()), True), (VitsConfig.apope_low(), False)):
        eng = Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=5, frames_per_id=3.0)), library=gpu_lib)
        eng.profile_enable(True)
        eng.run(ids, [32] * 4, [0.667, 1.0, 0.8])
        rep = eng.profile_report()
        eng.close()
        if det:
            assert "dp.det" in rep and not any(k.startswith(SDP_KERNELS) for k in rep), sorted(rep)
        else:
            assert "dp.det" not in rep and "dp.stack" in rep and "sdp.noise" in rep and "convflow.stack" in rep, sorted(rep)


def test_session_runs_a_deterministic_generator_onnx(gpu_lib, tmp_path):
    from mimic3_amd.session import InferenceSession

    cfg = det_config(VitsConfig.apope_low())
    w = det_weights(cfg, seed=54)
    (tmp_path / "generator.onnx").write_bytes(export_detdp_onnx(cfg, w, weight_norm_prefixes=("flow.", "dec.")))
    sess = InferenceSession(str(tmp_path / "generator.onnx"))
    assert sess.config.use_sdp is False
    ids = np.expand_dims(np.random.default_rng(6).integers(1, 50, 24).astype(np.int64), 0)
    feed = {"input": ids, "input_lengths": np.array([24], np.int64), "scales": np.array([0.0, 1.0, 0.8], np.float32)}
    audio = sess.run(None, feed)[0].squeeze()
    o = DetOracle(cfg, w).infer(ids, feed["input_lengths"], [0.0, 1.0, 0.0])
    r = o["audio"][0, 0]
    assert audio.shape == r.shape
    assert rel_rms(audio, r) < REL_RMS_TOL
