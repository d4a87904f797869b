"""k_wn_layer_b3 on v_mfma_f32_16x16x32_bf16, on the CPU model of the kernels: the weight fragments of pack_conv_weights_w16 unpacked
against the weights they came from, and the layer against fp64 per element with the criterion of tests/wn_ref.py (the one
tests/test_wn_layer.py and tests/test_gpu_wn_layer.py use) at lengths around the 16-column tiles.  tests/test_gpu_wn_shape.py runs the
same cases on the MI355X.  The hook serves MATH_BF16X3; the MATH_BF16W forms (the same loop without the three products of the weights'
lower terms) run through a whole engine on the 192-channel tiny voice, read at the flow's output (the `z` tap): the two MFMA shapes
against each other, the 32- / 96- / 128-column forms bit for bit, and against the oracle."""
import numpy as np
import pytest

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from oracle.vits_oracle import VitsOracle
from tests import wn_ref as Wn
from tests.util import TIGHT_REL_RMS_TOL, rel_rms

H = 192
SHAPE_LENGTHS = [1, 15, 16, 17, 33, 127, 129]  # around one and two 16-column tiles, a 32-column tile, a 128-column tile
# (Crs == 2H, cond given): a two-output layer and a flow's last layer, with and without speaker conditioning
SHAPE_OPTIONS = [(True, True), (True, False), (False, True), (False, False)]


def shape_lengths(T):
    """Three rows: full, one ending inside a 16-column tile (7 columns short: T - 7 is no multiple of 16 at any T of the table),
    and one of about half."""
    inside = max(T - 7, 1)
    assert T < 16 or inside % 16 != 0
    return (T, inside, T // 2 + 1)


def shape_case(lib, T, two, cond, skip_init=False):
    return Wn.check_vs_fp64(lib, 2, H, T, 5, 1, 2 * H if two else H, shape_lengths(T), with_cond=cond, skip_init=skip_init)


def _bf16_rne(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_value(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def w16_indices(Cout, Cin, gate):
    """(output channel [tile, lane], input channel [group, lane, slot]) of a fragment element, as csrc/kernels.h states them."""
    tile, lane = np.arange(Cout // 16)[:, None], np.arange(64)[None, :]
    n = tile >> 1 if gate else tile
    row = lane & 15
    co = np.where(gate & (tile & 1) == 1, Cout // 2, 0) + 32 * (n >> 1) + 8 * (row >> 2) + 4 * (n & 1) + (row & 3)
    g, ln, e = np.arange(Cin // 32)[:, None, None], np.arange(64)[None, :, None], np.arange(8)[None, None, :]
    ci = 32 * g + 16 * (ln >> 5) + 8 * (e >> 2) + 4 * ((ln >> 4) & 1) + (e & 3)
    return co, ci


@pytest.mark.parametrize("gate,Cout,K", [(True, 2 * H, 5), (True, 2 * H, 1), (False, 2 * H, 1), (False, H, 1), (False, 2 * H, 5)])
def test_packed_fragments_unpack_to_the_weights(emu_lib, gate, Cout, K):
    """Every (tile, tap, group, lane, slot) holds the three-term bf16 split of the weight the layout names: the leading term is the
    weight rounded to nearest even, the three terms sum to it within 2^-24 of its size, and every weight appears exactly once."""
    rng = np.random.default_rng([Cout, K, int(gate)])
    w = (rng.standard_normal((Cout, H, K)) / np.sqrt(H * K)).astype(np.float32)
    p = emu_lib.lab_pack_w16(w, gate=gate)  # [tile, tap, group, plane, lane, slot]
    assert p.shape == (Cout // 16, K, H // 32, 3, 64, 8)
    co, ci = w16_indices(Cout, H, gate)
    seen = np.zeros((Cout, H), np.int32)
    np.add.at(seen, (co[:, None, :, None], ci[None, :, :, :]), 1)
    assert (seen == 1).all()
    want = w[co[:, None, :, None], ci[None, :, :, :], :]            # [tile, group, lane, slot, tap]
    want = np.moveaxis(want, 4, 1)                                  # [tile, tap, group, lane, slot]
    assert np.array_equal(p[:, :, :, 0], _bf16_rne(want))
    total = sum(_bf16_value(p[:, :, :, k]).astype(np.float64) for k in range(3))
    assert np.all(np.abs(total - want) <= 2.0 ** -24 * np.abs(want))
    r1 = want - _bf16_value(p[:, :, :, 0])
    assert np.array_equal(p[:, :, :, 1], _bf16_rne(r1))
    assert np.array_equal(p[:, :, :, 2], _bf16_rne(r1 - _bf16_value(p[:, :, :, 1])))


@pytest.mark.parametrize("two,cond", SHAPE_OPTIONS)
@pytest.mark.parametrize("T", SHAPE_LENGTHS)
def test_layer_vs_fp64_around_the_16_column_tiles(emu_lib, T, two, cond):
    assert emu_lib.lab_wn_plan(3, T)[0] == 32  # the grid rule's form for three short rows
    shape_case(emu_lib, T, two, cond)


@pytest.mark.parametrize("T", [33, 129])
def test_forms_agree_bitwise_and_meet_the_criterion(emu_lib, T):
    """32-, 96- and 128-column tiles and both epilogues of the 96-column form: one arithmetic, the same bits in every valid column."""
    outs = []
    for env in Wn.B3_FORMS:
        with Wn.Env(**env):
            outs.append(shape_case(emu_lib, T, True, True))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            for r, L in enumerate(shape_lengths(T)):
                assert np.array_equal(a[r, :, :L], b[r, :, :L])


def test_the_32x32x16_form_behind_the_lab_switch(emu_lib):
    """MI355VITS_WN_SHAPE=32 runs the earlier body and packing: within the criterion too, and not the same bits (the sum inside an
    MFMA runs over other channels) — which shows that the switch switches."""
    new = shape_case(emu_lib, 129, True, True)
    with Wn.Env(MI355VITS_WN_SHAPE=32):
        old = shape_case(emu_lib, 129, True, True)
        last = shape_case(emu_lib, 33, False, False, skip_init=True)
    assert np.isfinite(last[1]).all()
    assert not np.array_equal(new[1], old[1])


# ---------------------------------------------------------------------------------------------------- MATH_BF16W through the engine
# Two rows of 24 and 17 ids at six frames each: 144 and 102 frames — two 128- or 96-column tiles and five 32-column ones, the second
# row ending inside a 16-column tile (102 = 6 x 16 + 6).  Two coupling layers x two WaveNet layers (a two-output layer and a last one).
BF16W_FRAMES = (144, 102)
# bf16 round-to-nearest leaves each weight within 2^-9 of its size, uniformly: 2^-9 / sqrt(3) = 1.13e-3 rms.  Independent errors add like
# the terms they sit on, so a conv's output carries that fraction of its own rms; z has passed at most 12 such convs (2 couplings x
# (pre, 2 in-layer, 2 res/skip, post)), and were every one to reach z in full: sqrt(12) x 1.13e-3.
BF16W_Z_TOL = 12 ** 0.5 * 2.0 ** -9 / 3 ** 0.5


@pytest.fixture(scope="module")
def bf16w_voice():
    cfg = VitsConfig.tiny_h192()
    w = W.synthetic_weights(cfg, seed=83, frames_per_id=2.0)
    rng = np.random.default_rng(83)
    return dict(cfg=cfg, w=w, blob=W.pack(cfg, w), ids=rng.integers(1, cfg.num_symbols, (2, 24)), lengths=np.array([24, 17]),
                forced=np.full((2, 24), 6, np.int32))


def bf16w_flow_run(lib, v, math="bf16w", device=None, **env):
    """(z over each row's own frames, zero elsewhere; audio; audio lengths) of the voice in `math` with the lab switches `env` set."""
    with Wn.Env(**env):
        eng = Engine(v["blob"], library=lib) if device is None else Engine(v["blob"], device=device, library=lib)
        eng.set_math(math)
        eng.profile_enable(True)
        out = eng.run(v["ids"], v["lengths"], (0.0, 1.0, 0.0), forced_durations=v["forced"], debug_taps=True)
        assert "flow.wn_layer_b3" in eng.profile_report()  # the fused layer kernel ran
        z = eng.tap("z")
        eng.close()
    assert z.shape[2] == BF16W_FRAMES[0]
    live = (np.arange(z.shape[2])[None, :] < np.array(BF16W_FRAMES)[:, None])[:, None, :]
    return z * live, out["audio"], out["lengths"]


def bf16w_shapes_case(lib, v, device=None):
    """The two MFMA shapes form the same exact products of the bf16-rounded weights and differ in the order of the f32 sums alone: each
    is within the f32-grade bound of the exactly summed result, the two within twice that — at the flow's output and in the waveform."""
    new = bf16w_flow_run(lib, v, device=device)
    old = bf16w_flow_run(lib, v, device=device, MI355VITS_WN_SHAPE=32)
    e = rel_rms(new[0], old[0])
    print(f"bf16w z: 16x16x32 vs 32x32x16 rel rms {e:.3e}")
    assert e < 2 * TIGHT_REL_RMS_TOL, e
    assert not np.array_equal(new[0], old[0])  # the switch switched
    assert np.array_equal(new[2], old[2])
    for b, L in enumerate(int(n) for n in new[2]):
        assert rel_rms(new[1][b, :L], old[1][b, :L]) < 2 * TIGHT_REL_RMS_TOL, b
    return new


def bf16w_forms_case(lib, v, device=None):
    """k_wn_layer_b3<16, true, NT> with 32-, 96- and 128-column tiles (and either epilogue switch at 96): the same bits at the flow's
    output and in the waveform; and not the bits of MATH_BF16X3, so the mode under test is the one that ran."""
    runs = [bf16w_flow_run(lib, v, device=device, **env) for env in Wn.B3_FORMS]
    for env, r in zip(Wn.B3_FORMS[1:], runs[1:]):
        assert np.array_equal(runs[0][0], r[0]), ("z", env)
        assert np.array_equal(runs[0][1], r[1]) and np.array_equal(runs[0][2], r[2]), ("audio", env)
    x3 = bf16w_flow_run(lib, v, math="bf16x3", device=device)
    assert not np.array_equal(x3[0], runs[0][0])
    return runs[0]


def test_bf16w_the_two_shapes_agree_at_the_f32_level(emu_lib, bf16w_voice):
    bf16w_shapes_case(emu_lib, bf16w_voice)


def test_bf16w_forms_agree_bitwise(emu_lib, bf16w_voice):
    bf16w_forms_case(emu_lib, bf16w_voice)


def test_bf16w_flow_output_vs_the_oracle(emu_lib, bf16w_voice):
    """z against the oracle (exact weights) within what bf16 weights can cost (BF16W_Z_TOL), and not at the f32 level: the rounded
    weights are really in use.  MATH_BF16X3 on the same input is at the f32 level."""
    v = bf16w_voice
    o = VitsOracle(v["cfg"], v["w"]).infer(v["ids"], v["lengths"], (0.0, 1.0, 0.0), forced_durations=v["forced"])
    assert tuple(int(n) for n in o["y_lengths"]) == BF16W_FRAMES
    live = (np.arange(BF16W_FRAMES[0])[None, :] < o["y_lengths"][:, None])[:, None, :]
    ew = rel_rms(bf16w_flow_run(emu_lib, v)[0], o["z"] * live)
    e3 = rel_rms(bf16w_flow_run(emu_lib, v, math="bf16x3")[0], o["z"] * live)
    print(f"z vs oracle: bf16w {ew:.3e} (bound {BF16W_Z_TOL:.3e}), bf16x3 {e3:.3e}")
    assert TIGHT_REL_RMS_TOL < ew < BF16W_Z_TOL and e3 < TIGHT_REL_RMS_TOL, (ew, e3)
