"""Ragged batches at any compute-unit count, and on a poisoned workspace (CPU model of the kernels, tests/emu).

The persistent decoder kernels walk only the (row, column block) items that have work, each workgroup with a cursor that moves
forward only; which items a workgroup takes depends on the grid, and the grid on the device's compute units.  The CPU model
reports the count a test sets (mi355vits_emu_set_cu_count), so these tests run the same work on grids of other sizes than the
device's 256 and the model's default 8: odd counts, counts below 8, counts above the item count.

Columns past a row's end are never computed: they keep what the workspace held before.  Every consumer must mask them by select,
never by multiply, so the tests put quiet NaNs and infinities there — in the kernels' inputs directly, and in the engine's whole
workspace through mi355vits_test_fill_workspace — and demand bitwise the solo runs of the rows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from tests.util import TIGHT_REL_RMS_TOL, check_parity

DEFAULT_CUS = 8  # what the CPU model reports unless a test sets another count


@pytest.fixture
def cu_count(emu_lib):
    """Sets the compute units the CPU model reports (create engine handles after setting it); restores the default afterwards."""
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(DEFAULT_CUS)


def _ragged_lens(T, N, halo, extra=0):
    """Row lengths at a kernel's edges: empty, one column, shorter than the halo, item width - 1 / exact / + 1, T - 1, T, two
    items; then rows at full length until the item count (a row of len columns: ceil((len + extra) / N) items of N positions)
    exceeds 26 — enough for a 13-workgroup grid to walk three items — and is no multiple of 3, 8 or 13."""
    lens = [0, 1, min(5, max(1, halo - 1)), N - 1, N, N + 1, T - 1, T, 2 * N]
    items = lambda: sum((n + extra + N - 1) // N for n in lens if n > 0)
    while items() < 27 or any(items() % c == 0 for c in (3, 8, 13)):
        lens.append(T)
    return np.array(lens, np.int32)


def _poison(x, lens, inf_row):
    """x with the columns past each row's length set to qNaN, and those of row `inf_row` to +Inf."""
    xp = x.copy()
    for b, n in enumerate(lens):
        xp[b, :, n:] = np.inf if b == inf_row else np.nan
    return xp


def _check_rows(y, ref, lens, stride, err1, maxabs1):
    """Valid columns finite; RMS over every row's own columns within the existing bound against fp64 (1e-6, and 1.25 x the
    f32-MFMA kernel's error + 2e-8); per row, the largest error within 4 x the f32-MFMA kernel's largest + 1e-7 (a column
    that was skipped or read a poisoned neighbour is off by O(1): it cannot hide inside the RMS)."""
    sq, cnt = 0.0, 0
    for b, n in enumerate(lens):
        L = int(n) * stride
        if L == 0:
            continue
        yb = y[b, :, :L].astype(np.float64)
        assert np.isfinite(yb).all(), (b, int(n))
        d = yb - ref[b][:, :L]
        sq += float(np.sum(d * d))
        cnt += d.size
        assert np.abs(d).max() <= 4 * maxabs1 + 1e-7, (b, int(n), float(np.abs(d).max()), maxabs1)
    err = float(np.sqrt(sq / cnt))
    assert err < 1e-6 and err <= 1.25 * err1 + 2e-8, (err, err1)


# grids: one workgroup, fewer than the eight XCDs, the model's default, odd, and as many workgroups as items (100, 256: one item
# each); the 128-column form is the expensive one on the CPU model, it takes the counts that differ in kind
ALL_CUS, FEW_CUS = [1, 3, 8, 13, 100, 256], [1, 13, 100]
RBC_CUS = {"0": ALL_CUS, "1": FEW_CUS}


@pytest.mark.parametrize("kd", [(7, 12), (3, 1), (5, 6)])
@pytest.mark.parametrize("wide", ["1", "0"])
def test_resident_input_resblock_conv_ragged_at_any_grid(emu_lib, cu_count, kd, wide, monkeypatch):
    """k_rb_conv_pw (128-column items) / k_rb_conv (32-column items) through mi355vits_test_conv1d impl 4: ragged rows at their
    edges, the inputs past every row's end poisoned (qNaN; one row +Inf), on grids of 1 .. 256 workgroups — each row against an
    fp64 conv of that row alone.  A grid that is not a multiple of 8 (and smaller than the item count) once took the XCD-major item
    order, under which a workgroup's items do not grow: the forward-only cursor skipped whole blocks of valid rows."""
    K, dil = kd
    monkeypatch.setenv("MI355VITS_RBC_WIDE", wide)
    N = 128 if wide == "1" else 32
    C, T = 128, 260
    lens = _ragged_lens(T, N, (K - 1) // 2 * dil)
    B = len(lens)
    rng = np.random.default_rng(1000 * K + dil + N)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    w = (rng.standard_normal((C, C, K)) / np.sqrt(C * K)).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    res = rng.standard_normal((B, C, T)).astype(np.float32)
    x0 = np.where(np.arange(T)[None, None, :] < lens[:, None, None], x, 0).astype(np.float32)
    # a row alone = its own columns with zeros around them: leaky-relu keeps the zeros, so the batched fp64 conv of the clean input
    # restricted to [0, len_b) is each row's solo result
    conv = F.conv1d(F.leaky_relu(torch.from_numpy(x0).double(), 0.1), torch.from_numpy(w).double(), torch.from_numpy(bias).double(),
                    dilation=dil, padding=(K * dil - dil) // 2)
    full = ((conv + torch.from_numpy(res).double()) * 0.5).numpy()
    ref = [full[b, :, :n] for b, n in enumerate(lens)]
    y1 = emu_lib.test_conv1d(x0, w, bias, res, dilation=dil, impl=1, in_len=lens, in_slope=0.1, out_scale=0.5)
    e1 = [y1[b, :, :n].astype(np.float64) - ref[b] for b, n in enumerate(lens) if n]
    err1 = float(np.sqrt(sum(float(np.sum(d * d)) for d in e1) / sum(d.size for d in e1)))
    maxabs1 = max(float(np.abs(d).max()) for d in e1)
    xp = _poison(x, lens, inf_row=3)
    for cus in RBC_CUS[wide]:
        cu_count(cus)
        y = emu_lib.test_conv1d(xp, w, bias, res, dilation=dil, impl=4, in_len=lens, in_slope=0.1, out_scale=0.5)
        _check_rows(y, ref, lens, 1, err1, maxabs1)


# (Cin, Cout, stride, K) of the "_low" voices' upsamplers -> {MI355VITS_RBC_WIDE: (positions per work item, grids)}; the 256- and
# 128-channel forms are the expensive ones on the CPU model
UPS_CASES = {(256, 128, 8, 16): {"1": (64, [1, 13]), "0": (32, [13, 100])}, (128, 64, 8, 16): {"1": (128, FEW_CUS), "0": (32, ALL_CUS)},
             (64, 32, 4, 8): {"1": (127, ALL_CUS), "0": (31, ALL_CUS)}}


@pytest.mark.parametrize("case", list(UPS_CASES))
@pytest.mark.parametrize("wide", ["1", "0"])
def test_resident_input_upsamplers_ragged_at_any_grid(emu_lib, cu_count, case, wide, monkeypatch):
    """k_ups_pl (256 -> 128, 128 -> 64) and k_ups64 (64 -> 32) through mi355vits_test_conv_transpose1d impl 3 with per-row input
    lengths: rows at their edges (a row of len inputs has len + 1 polyphase output positions), the inputs past every row's end
    poisoned, grids of 1 .. 256 workgroups.  Per row the fp64 reference is ConvTranspose1d(leaky(x[b, :, :len_b])) on
    [0, len_b x stride): what the row computes alone."""
    Cin, Cout, stride, K = case
    monkeypatch.setenv("MI355VITS_RBC_WIDE", wide)
    N, counts = UPS_CASES[case][wide]
    Tin = max(150, 2 * N + 24)
    lens = _ragged_lens(Tin, N, 1, extra=1)
    B = len(lens)
    rng = np.random.default_rng(Cin + N)
    x = rng.standard_normal((B, Cin, Tin)).astype(np.float32)
    w = (rng.standard_normal((Cin, Cout, K)) / np.sqrt(Cin * K / stride)).astype(np.float32)
    bias = rng.standard_normal(Cout).astype(np.float32)
    x0 = np.where(np.arange(Tin)[None, None, :] < lens[:, None, None], x, 0).astype(np.float32)
    # zeros past a row's end are what its solo run sees there (leaky-relu keeps them): the batched transpose conv of the clean
    # input, cut at len_b x stride, is every row's solo result
    full = F.conv_transpose1d(F.leaky_relu(torch.from_numpy(x0).double(), 0.1), torch.from_numpy(w).double(), torch.from_numpy(bias).double(),
                              stride=stride, padding=(K - stride) // 2).numpy()
    ref = [full[b] for b in range(B)]
    y1 = emu_lib.test_conv_transpose1d(x0, w, bias, stride, in_slope=0.1, impl=1)
    e1 = [y1[b, :, :n * stride].astype(np.float64) - full[b, :, :n * stride] for b, n in enumerate(lens) if n]
    err1 = float(np.sqrt(sum(float(np.sum(d * d)) for d in e1) / sum(d.size for d in e1)))
    maxabs1 = max(float(np.abs(d).max()) for d in e1)
    xp = _poison(x, lens, inf_row=4)
    for cus in counts:
        cu_count(cus)
        y = emu_lib.test_conv_transpose1d(xp, w, bias, stride, in_slope=0.1, impl=3, in_len=lens)
        _check_rows(y, ref, lens, stride, err1, maxabs1)


SCALES = [0.667, 1.0, 0.8]


def _voice():
    """tiny_wide at 256 initial channels: the 128-channel stage runs on the k_rb_conv family, the 64- and 32-channel ones on k_mrf_p /
    k_mrf_s, the upsamplers on k_ups_pl / k_ups64 / the staged polyphase kernel."""
    cfg = VitsConfig.tiny_wide(initial_channel=256)
    w = W.synthetic_weights(cfg, seed=91, frames_per_id=2.0)
    return cfg, w, W.pack(cfg, w)


def _batch(cfg, lengths, Tx=40, frames=3, seed=12):
    """A ragged batch with forced durations and explicit noise (the same tensors serve the solo runs)."""
    lengths = np.asarray(lengths)
    B = len(lengths)
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, cfg.num_symbols, (B, Tx))
    forced = np.full((B, Tx), frames, np.int32)
    nw = rng.standard_normal((B, 2, Tx)).astype(np.float32)
    nz = rng.standard_normal((B, cfg.inter_channels, Tx * frames)).astype(np.float32)
    return dict(ids=ids, lengths=lengths, forced=forced, nw=nw, nz=nz)


def _run(eng, bt, rows=None, taps=False):
    """The batch (or its rows `rows` alone, each at its own length) with its noise."""
    if rows is None:
        return eng.run(bt["ids"], bt["lengths"], SCALES, forced_durations=bt["forced"], noise_w=bt["nw"], noise_z=bt["nz"],
                       want_pcm16=True, debug_taps=taps)
    n = int(bt["lengths"][rows])
    f = int(bt["forced"][rows, 0])
    return eng.run(bt["ids"][rows:rows + 1, :n], [n], SCALES, forced_durations=bt["forced"][rows:rows + 1, :n],
                   noise_w=bt["nw"][rows:rows + 1, :, :n], noise_z=bt["nz"][rows:rows + 1, :, :n * f], want_pcm16=True)


def _assert_rows_equal(out, solo, b):
    L = int(solo["lengths"][0])
    assert L == int(out["lengths"][b]), b
    assert np.array_equal(solo["audio"][0, :L], out["audio"][b, :L]), b
    assert np.array_equal(solo["pcm"][0, :L], out["pcm"][b, :L]), b


ENGINE_ROWS = [40, 3, 22, 1, 0, 31, 9, 14]  # 1 .. 40 ids and an empty row


@pytest.mark.parametrize("math,counts", [("bf16x3", [1, 7, 13, 32, 256]), ("f32", [1, 13])])
def test_engine_output_does_not_depend_on_the_cu_count(emu_lib, cu_count, math, counts):
    """Every form the code picks by compute-unit count — rb_conv 128- / 32-column items, the WaveNet layer's 128- / 64-column tile,
    the encoder's wide form and its resblock loop, the persistent form of the staged conv, the attention's high-occupancy form, the
    mrf_s row sweep and k_mrf_p's item groups — gives the same bits: every tap, the waveform and the int16 output of a
    ragged batch with noise on grids of 1 .. 256 compute units are bitwise those of the model's 8."""
    cfg, _, blob = _voice()
    bt = _batch(cfg, ENGINE_ROWS)

    def run_at(cus):
        cu_count(cus)
        eng = Engine(blob, library=emu_lib)
        eng.set_math(math)
        out = _run(eng, bt, taps=True)
        taps = {k: eng.tap(k) for k in eng.taps()}
        eng.close()
        return out, taps

    base, btaps = run_at(DEFAULT_CUS)
    assert np.isfinite(base["audio"]).all() and len(btaps) > 8, list(btaps)
    for cus in counts:
        out, taps = run_at(cus)
        assert set(taps) == set(btaps), (cus, set(taps) ^ set(btaps))
        for k in btaps:
            assert np.array_equal(taps[k], btaps[k]), (cus, k)
        assert np.array_equal(out["lengths"], base["lengths"]), cus
        assert np.array_equal(out["audio"], base["audio"]), cus
        assert np.array_equal(out["pcm"], base["pcm"]), cus


def test_engine_at_an_odd_cu_count_matches_the_oracle_and_the_solo_runs(emu_lib, cu_count):
    """13 compute units (no multiple of 8, fewer than the decoder's items): check_parity's tight bound at every tap and the
    waveform, and every row bitwise its solo run on the same grid."""
    cu_count(13)
    cfg, w, blob = _voice()
    rows = [n for n in ENGINE_ROWS if n > 0]
    Tx = max(rows)
    rng = np.random.default_rng(12)
    ids = rng.integers(1, cfg.num_symbols, (len(rows), Tx))
    forced = np.full(ids.shape, 3, np.int32)
    eng = Engine(blob, library=emu_lib)
    eng.set_math("bf16x3")
    out, _ = check_parity(emu_lib, cfg, ids=ids, lengths=rows, forced=forced, noise=True, seed=12, weights=w, engine=eng)
    assert out["audio_error"] < TIGHT_REL_RMS_TOL
    rng2 = np.random.default_rng(12 + 7)  # check_parity's noise draws (tests/util.py): the same tensors for the solo runs
    bt = dict(ids=ids, lengths=np.array(rows), forced=forced, nw=rng2.standard_normal((len(rows), 2, Tx)).astype(np.float32),
              nz=rng2.standard_normal((len(rows), cfg.inter_channels, Tx * 3)).astype(np.float32))
    for b in range(len(rows)):
        _assert_rows_equal(out, _run(eng, bt, rows=b), b)
    eng.close()


def test_det_dp_voice_at_an_odd_cu_count(emu_lib, cu_count):
    """A voice with the deterministic duration predictor (k_dp_det) on 13 compute units: logw against the float64 restatement of
    upstream's predictor, and the output bitwise the 8-unit run's."""
    from tests.detdp_util import det_config, det_weights, logw_ref
    from tests.util import make_inputs

    cfg = det_config(VitsConfig.tiny(), 64)
    w = det_weights(cfg, seed=31)
    ids, lens, sid = make_inputs(cfg, 5, 70, seed=31)
    outs = {}
    for cus in (DEFAULT_CUS, 13):
        cu_count(cus)
        eng = Engine(W.pack(cfg, w), library=emu_lib)
        outs[cus] = eng.run(ids, lens, [0.0, 1.0, 0.0], sid, want_pcm16=True, debug_taps=True)
        lw = eng.tap("logw")
        assert np.abs(lw - logw_ref(cfg, w, ids, lens, sid)).max() <= 1e-5
        eng.close()
    for k in ("lengths", "audio", "pcm"):
        assert np.array_equal(outs[13][k], outs[DEFAULT_CUS][k]), k


POISON = [0x7FC00000, 0xFFFFFFFF, 0x7F800000, 0x7F7FFFFF]  # qNaN, a negative NaN with every mantissa bit, +Inf, the largest float
POISON_ROWS = [24, 3, 13, 1, 0, 17, 9]


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("cus", [DEFAULT_CUS, 13])
def test_poisoned_workspace_never_reaches_a_valid_sample(emu_lib, cu_count, math, cus):
    """Columns past a row's end are never computed: they hold what the workspace held.  Consumers must mask them by select, never
    by multiply (NaN x 0 = NaN): with the whole workspace filled with NaN, Inf or the largest float before a ragged batch, every
    row is still bitwise its solo run on a fresh handle, the audio finite and the int16 output equal.  A larger batch sizes the
    workspace first, so the ragged run cannot reallocate (and zero) it."""
    cfg, _, blob = _voice()
    bt = _batch(cfg, POISON_ROWS, Tx=24, frames=2)
    big = _batch(cfg, [24] * len(POISON_ROWS), Tx=24, frames=2, seed=5)
    fresh = Engine(blob, library=emu_lib)
    fresh.set_math(math)
    solo = {b: _run(fresh, bt, rows=b) for b, n in enumerate(POISON_ROWS) if n}
    clean = _run(fresh, bt)  # (an empty row has one silent frame: as on a clean workspace)
    fresh.close()
    cu_count(cus)
    eng = Engine(blob, library=emu_lib)
    eng.set_math(math)
    assert np.isfinite(_run(eng, big)["audio"]).all()
    for pattern in POISON:
        eng.fill_workspace(pattern)
        out = _run(eng, bt)
        assert np.isfinite(out["audio"]).all(), hex(pattern)
        for b, n in enumerate(POISON_ROWS):
            if n:
                _assert_rows_equal(out, solo[b], b)
            else:
                L = int(clean["lengths"][b])
                assert int(out["lengths"][b]) == L and np.array_equal(out["audio"][b, :L], clean["audio"][b, :L]), b
    eng.close()
