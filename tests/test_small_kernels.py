"""The text side's small kernels and the Philox noise on the CPU model of the kernels: every form run alone through the lab hooks,
against an fp64 restatement of its rule per element (tests/small_ref.py holds the rules, the calibrations and the case tables; the
same tables run on the MI355X in tests/test_gpu_small_kernels.py).

form -> test
  k_embed (64 columns x 4 channel groups, clamp, zeros)        test_embed
  k_layernorm<cached>, every option alone, the engine's four
  combinations, the three in-place uses                        test_layernorm_cached
  k_layernorm<cached>: variance 0, mean 100 / spread 1         test_layernorm_constant_and_offset_columns
  k_layernorm<cached> at and past premask_len / out_len        test_layernorm_padding
  k_layernorm<uncached> (C > 256)                              test_layernorm_uncached
  launch_layernorm's refusal                                   test_layernorm_refusals
  k_dp_det<F32>, k_dp_det<split-bf16>, K 1 / 3 / 5 / 7         test_dp_det, test_dp_det_plan_and_refusals
  k_sdp_noise (Philox, tensor id 0)                            test_sdp_noise
  k_expand_prior, keyed branch (Philox, tensor id 1)           test_expand_prior_keyed
  seed / utterance_base / tensor ids at the engine's calls     test_engine_draws_are_the_reference_tensors
the reference itself (no kernel runs)                          test_philox_known_answers, test_reference_draws_are_normal,
                                                               test_reference_draws_depend_on_every_key_word, test_edge_uniforms,
                                                               test_dp_det_rule_is_the_restated_predictor, test_dp_case_table_holds_every_seam
and test_wrong_variants_fail_the_criterion_and_pass_the_older_checks is the proof that the criterion bites."""
import numpy as np
import pytest
import torch

from mimic3_amd import weights as W
from mimic3_amd._native import Engine
from mimic3_amd.config import VitsConfig
from tests import small_ref as S
from tests.detdp_util import det_logw
from tests.small_ref import NativeError
from tests.util import TIGHT_REL_RMS_TOL, make_inputs, rel_rms

WHERE = "CPU model"


@pytest.fixture(scope="module")
def lib(emu_lib):
    S.ratios_into(WHERE)
    return emu_lib


# ------------------------------------------------------------------------------------------------ the reference itself
def test_philox_known_answers():
    for ctr, key, want in S.KNOWN_ANSWERS:
        got = tuple(int(v) for v in S.philox4x32(*ctr, *key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    # arrays go through the same arithmetic as scalars
    c0 = np.asarray([k[0][0] for k in S.KNOWN_ANSWERS], np.uint64)
    rest = [np.asarray([k[0][i] for k in S.KNOWN_ANSWERS], np.uint64) for i in (1, 2, 3)]
    keys = [np.asarray([k[1][i] for k in S.KNOWN_ANSWERS], np.uint64) for i in (0, 1)]
    out = S.philox4x32(c0, *rest, *keys)
    assert [tuple(int(o[i]) for o in out) for i in range(3)] == [k[2] for k in S.KNOWN_ANSWERS]


def test_reference_draws_are_normal():
    """2^17 draws of one key (256 channels x 512 steps): mean, variance, skew, excess kurtosis and the lag-one correlations along t
    and along c, each within five standard errors of N(0, 1)'s."""
    for tensor, utt in ((0, 7), (1, 2 ** 32 + 7)):
        m = S.moments(S.normals(S.SEED, utt, tensor, 256, 512, np.float64))
        print("moments / standard error (mean, var, skew, kurtosis, corr t, corr c):", np.round(m, 2))
        assert np.all(np.abs(m) < 5.0), m


def test_reference_draws_depend_on_every_key_word():
    """Each word of the key and the counter, changed alone, changes more than 99 % of the draws."""
    C, T = 64, 256
    base = S.normals(S.SEED, 2 ** 32 + 7, 0, C, T, np.float32)
    others = {
        "tensor id": S.normals(S.SEED, 2 ** 32 + 7, 1, C, T, np.float32),
        "c and t swapped": S.normals(S.SEED, 2 ** 32 + 7, 0, T, C, np.float32).T,  # element (c, t) drawn at (t, c)
        "low word of utt": S.normals(S.SEED, 2 ** 32 + 8, 0, C, T, np.float32),
        "high word of utt": S.normals(S.SEED, 2 ** 33 + 7, 0, C, T, np.float32),
        "low word of the seed": S.normals(S.SEED ^ 1, 2 ** 32 + 7, 0, C, T, np.float32),
        "high word of the seed": S.normals(S.SEED ^ (1 << 32), 2 ** 32 + 7, 0, C, T, np.float32),
    }
    for what, o in others.items():
        changed = float(np.mean(o != base))
        assert changed > 0.99, (what, changed)
    assert np.array_equal(base, S.normals(S.SEED, 2 ** 32 + 7, 0, C, T, np.float32))


def test_edge_uniforms():
    """r >> 8 = 0 gives u = 2^-25 and the largest draw, sqrt(50 ln 2) = 5.887...; r >> 8 = 2^24 - 1 gives u = 1.0 exactly (the + 0.5f
    rounds up), hence -/+ 0: finite both, in the rule and in the calibration."""
    lo, hi = np.asarray([0], np.uint64), np.asarray([0xFFFFFFFF], np.uint64)
    assert S.uniform_of(lo)[0] == np.float32(2.0 ** -25) and S.uniform_of(hi)[0] == np.float32(1.0)
    assert S.uniform_of(np.asarray([(2 ** 23) << 8], np.uint64))[0] == np.float32(0.5)  # 2^23 + 0.5 rounds to even
    for dt in (np.float64, np.float32):
        big = S.normal_of(lo, lo, dt)[0]
        assert abs(float(big) - np.sqrt(50.0 * np.log(2.0))) < 1e-6 and 5.887 < big < 5.888
        for r1 in (lo, hi, np.asarray([1 << 31], np.uint64)):
            z = S.normal_of(hi, r1, dt)[0]
            assert z == 0.0 and np.isfinite(z)


def _torch_weights(w):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    return {"dp.conv_1.weight": t(w["w1"]), "dp.conv_1.bias": t(w["b1"]), "dp.norm_1.gamma": t(w["g1"]), "dp.norm_1.beta": t(w["be1"]),
            "dp.conv_2.weight": t(w["w2"]), "dp.conv_2.bias": t(w["b2"]), "dp.norm_2.gamma": t(w["g2"]), "dp.norm_2.beta": t(w["be2"]),
            "dp.proj.weight": t(w["proj_w"]).reshape(1, -1, 1), "dp.proj.bias": t(w["proj_b"])}


def test_dp_det_rule_is_the_restated_predictor():
    """small_ref.dp_det_rule in fp64 is tests/detdp_util.py's det_logw (upstream DurationPredictor in torch, double), row by row."""
    for (H, F, K), cond in (((64, 32, 3), True), ((32, 256, 5), False)):
        c = S.dp_case(H, F, K, 64 - 2 * (K // 2), 2 * (K // 2), cond)
        x = c["x"].astype(np.float64) + (c["cond"].astype(np.float64)[:, :, None] if cond else 0.0)
        for b, L in enumerate(int(n) for n in c["lens"]):
            if L:
                got = det_logw(_torch_weights(c["w"]), torch.from_numpy(x[b:b + 1, :, :L]), torch.ones(1, 1, L, dtype=torch.float64)).numpy()
                assert np.abs(got[0, 0] - c["ref"][b, :L]).max() < 1e-12 and np.all(c["ref"][b, L:] == 0), b


def test_dp_case_table_holds_every_seam():
    for K in (1, 3, 5, 7):
        cols, halo = 64 - 2 * (K // 2), 2 * (K // 2)
        T = 2 * cols + 3
        lens = S.class_lengths(T, cols, halo)
        assert lens[0] == T and {0, 1} <= set(lens)
        for m in (cols, 2 * cols):
            assert {n for n in (m - 1, m, m + 1, m - halo, m + halo) if n <= T} <= set(lens), (K, m)
        assert len(lens) * 256 * T < 1_000_000


# ------------------------------------------------------------------------------------------------ embed
@pytest.mark.parametrize("H", S.EMBED_H)
def test_embed(lib, H):
    for T in S.EMBED_T:
        S.check_embed(lib, H, T)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("C", S.LN_C)
def test_layernorm_cached(lib, C):
    for T in S.LN_T:
        for name, opts in S.LN_OPTIONS:
            S.check_ln(lib, S.ln_case(C, T, tuple(opts.items())), "k_layernorm<cached>", f"C={C} T={T} {name}")


def test_layernorm_constant_and_offset_columns(lib):
    """A column constant over the channels: variance 0, the output exactly beta.  Mean 100 with spread 1: the kernel's two passes
    meet the criterion that one-pass arithmetic (E[v^2] - mean^2 in float32) fails."""
    for C, T in ((17, 17), (192, 33)):
        c = S.ln_case(C, T, kind="constant")
        got = S.check_ln(lib, c, "k_layernorm<cached>", f"C={C} T={T} constant columns")
        assert np.array_equal(got.view(np.uint32), np.broadcast_to(c["beta"][None, :, None], got.shape).view(np.uint32)), (C, T, "variance 0: exactly beta")
        c = S.ln_case(C, T, kind="offset")
        S.check_ln(lib, c, "k_layernorm<cached>", f"C={C} T={T} mean 100, spread 1", ill_conditioned=True)
        ref, f32 = S.layernorm_rule(c, np.float64), S.layernorm_rule(c, np.float32)
        assert not S.passes_vs_fp64(S.layernorm_rule(c, np.float32, one_pass=True), ref, f32, c["cmp_len"]), (C, T, "one pass would pass")


@pytest.mark.parametrize("C,T", [(17, 17), (192, 33), (256, 15), (5, 33)])
def test_layernorm_padding(lib, C, T):
    """NaN bits in x or the partial sums at t >= premask_len, and in x, res and add_to at t >= out_len: no bit moves and no NaN
    comes out; exact zeros under out_len (check_ln); every row equals its solo run."""
    for name, opts in S.LN_OPTIONS[-4:] + [("premask_len", dict(premask=True)), ("res + add_to + gelu + out_len", dict(res=True, add_to=True, gelu=True, out_len=True))]:
        c = S.ln_case(C, T, tuple(opts.items()), seed=1)
        S.check_ln(lib, c, "k_layernorm<cached>", f"C={C} T={T} {name} (padding case)")
        S.ln_padding_case(lib, c, "k_layernorm<cached>", f"C={C} T={T} {name}")


@pytest.mark.parametrize("C", S.LN_C_UNCACHED)
def test_layernorm_uncached(lib, C):
    for T in S.LN_T_UNCACHED:
        for name, opts in S.LN_OPTIONS_UNCACHED:
            c = S.ln_case(C, T, tuple(opts.items()))
            S.check_ln(lib, c, "k_layernorm<uncached>", f"C={C} T={T} {name}")
            if c["out_len"] is not None:
                S.ln_padding_case(lib, c, "k_layernorm<uncached>", f"C={C} T={T} {name}")


def test_layernorm_refusals(lib):
    """The split-conv input at C > 256 is the launcher's refusal, MI355VITS_ERR_INVALID; the same options are served at C = 256."""
    for opts in S.LN_REFUSED:
        c = S.ln_case(257, 17, tuple(opts.items()))
        with pytest.raises(NativeError) as e:
            S.run_ln(lib, c)
        assert e.value.code == -1, (opts, e.value)  # MI355VITS_ERR_INVALID
        S.check_ln(lib, S.ln_case(256, 17, tuple(opts.items())), "k_layernorm<cached>", f"C=256 T=17 {opts}: served")


# ------------------------------------------------------------------------------------------------ k_dp_det
@pytest.mark.parametrize("with_cond", [True, False], ids=["cond", "no cond"])
@pytest.mark.parametrize("shape", S.DP_SHAPES, ids=lambda s: "H%d-F%d-K%d" % s)
def test_dp_det(lib, shape, with_cond):
    for math in S.MATHS:
        S.check_dp_det(lib, shape, math, with_cond, alone=with_cond)


def test_dp_det_plan_and_refusals(lib):
    """The plan call reports the library's own seam (64 - 2 (K / 2) columns) and LDS request — (256, 256, 7) is the largest of the
    table — and refuses what dp_det_supported refuses, as the hook does before any launch."""
    lds = {(s, m): lib.lab_dp_det_plan(*s, m)[2] for s in S.DP_SHAPES for m in S.MATHS}
    assert max(lds, key=lds.get)[0] == (256, 256, 7) and max(lds.values()) <= 160 * 1024, lds
    assert [lib.lab_dp_det_plan(32, 32, K)[:2] for K in (1, 3, 5, 7)] == [(64, 0), (62, 2), (60, 4), (58, 6)]
    rng = np.random.default_rng(0)
    for H, F, K in S.DP_REFUSED:
        w = dict(w1=rng.standard_normal((F, H, K)), w2=rng.standard_normal((F, F, K)), proj_w=np.ones(F), proj_b=np.zeros(1),
                 **{k: np.ones(F) for k in ("b1", "g1", "be1", "b2", "g2", "be2")})
        for math in S.MATHS:
            with pytest.raises(NativeError) as e:
                lib.lab_dp_det_plan(H, F, K, math)
            assert e.value.code == -1
            with pytest.raises(NativeError) as e:
                lib.test_dp_det(rng.standard_normal((1, H, 9)), [9], w, None, math)
            assert e.value.code == -1, (H, F, K, e.value)
    with pytest.raises(NativeError) as e:
        lib.lab_dp_det_plan(32, 32, 3, 2)  # MATH_BF16W: the engine maps it to BF16X3 before this kernel
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------ the noise
@pytest.mark.parametrize("T", S.NOISE_T)
def test_sdp_noise(lib, T):
    S.check_sdp_noise(lib, T)


@pytest.mark.parametrize("I,Ty", S.EXPAND_KEYED)
def test_expand_prior_keyed(lib, I, Ty):
    S.check_expand_keyed(lib, I, Ty)


def test_engine_draws_are_the_reference_tensors(lib):
    """A run under (seed, utterance_base) against the same run fed the reference's tensor 0 as noise_w and tensor 1 as noise_z (and
    the first run's durations): utt = utterance_base + b, the seed's way through the run's inputs, and the tensor ids at the engine's
    own call sites.  logw within the 1e-5 of tests/test_det_dp.py, the audio within TIGHT_REL_RMS_TOL."""
    cfg = VitsConfig.tiny()
    assert cfg.use_sdp
    w = W.synthetic_weights(cfg, seed=21, frames_per_id=3.0)
    eng = Engine(W.pack(cfg, w), library=S.native_of(lib))
    ids, lens, sid = make_inputs(cfg, 3, 13, seed=4)
    B, Tx = ids.shape
    scales, base = [0.667, 1.0, 0.8], 2 ** 32 - 1  # (row 1 onwards: a non-zero high word of utt)
    a = eng.run(ids, lens, scales, sid, seed=S.SEED, utterance_base=base, debug_taps=True)
    logw_a, wc = eng.tap("logw").copy(), eng.tap("w_ceil").reshape(B, -1).astype(np.int32)
    Ty = int(wc.sum(axis=1).max())
    nw = np.stack([S.normals(S.SEED, base + b, 0, 2, Tx, np.float64) for b in range(B)]).astype(np.float32)
    nz = np.stack([S.normals(S.SEED, base + b, 1, cfg.inter_channels, Ty, np.float64) for b in range(B)]).astype(np.float32)
    r = eng.run(ids, lens, scales, sid, noise_w=nw, noise_z=nz, forced_durations=wc, debug_taps=True)
    d = float(np.abs(eng.tap("logw") - logw_a).max())
    print(f"engine mapping: max |logw - logw| = {d:.3e}")
    assert d <= 1e-5, d
    assert np.array_equal(a["lengths"], r["lengths"])
    for b in range(B):
        L = int(a["lengths"][b])
        e = rel_rms(a["audio"][b, :L], r["audio"][b, :L])
        print(f"engine mapping: row {b}: {L} samples, rel rms {e:.3e}")
        assert e < TIGHT_REL_RMS_TOL, (b, e)
    # the draws are used: another base moves the audio
    o = eng.run(ids, lens, scales, sid, seed=S.SEED, utterance_base=base + 1, forced_durations=wc)
    assert not np.array_equal(o["audio"], a["audio"])
    eng.close()


# ------------------------------------------------------------------------------------------------ the proof that the tests bite
def test_wrong_variants_fail_the_criterion_and_pass_the_older_checks():
    """Python-side wrong variants of the rules (no kernel is altered): each fails the per-element criterion, and passes what the
    suite checked before — repeatable draws that do not depend on the batch and move with the seed (and are still normal); a
    LayerNorm at C = 192, the one width the A/B tests run; max |logw - ref| <= 1e-5."""
    T = 65
    lens = [T if v != 0 else 0 for v in S.NOISE_W]
    ref, f32 = S.sdp_noise_rule(T, np.float64), S.sdp_noise_rule(T, np.float32)
    assert S.passes_vs_fp64(f32, ref, f32, lens)
    for variant in (dict(rounds=9), dict(swap_ct=True)):
        bad = S.sdp_noise_rule(T, np.float32, **variant)
        assert not S.passes_vs_fp64(bad, ref, f32, lens), variant
        assert np.array_equal(bad, S.sdp_noise_rule(T, np.float32, **variant))
        assert np.array_equal(bad[2], S.sdp_noise_rule(T, np.float32, utts=S.UTTS[2:3], noise_w=S.NOISE_W[2:3], **variant)[0])
        assert not np.array_equal(bad, S.sdp_noise_rule(T, np.float32, seed=S.SEED + 1, **variant))
        assert np.all(np.abs(S.moments(S.normals(S.SEED, 7, 0, 256, 512, np.float64, **variant))) < 5.0), variant
    # the variance over the padded channel count: 32 for C = 17; at C = 192 the count is C itself
    c = S.ln_case(17, 17)
    ref, f32 = S.layernorm_rule(c, np.float64), S.layernorm_rule(c, np.float32)
    assert not S.passes_vs_fp64(S.layernorm_rule(c, np.float32, var_count=32), ref, f32, c["cmp_len"])
    c = S.ln_case(192, 17)
    assert np.array_equal(S.layernorm_rule(c, np.float32, var_count=-(-192 // 16) * 16), S.layernorm_rule(c, np.float32))
    # k_dp_det's convs without the third term of the operands' bf16 splits
    c = S.dp_case(192, 64, 3, 62, 2, True)
    bad = S.dp_det_rule(c, np.float64, 0, drop_third=True).astype(np.float32)
    e, e32 = (S.norm_err(a[:, None, :], c["ref"][:, None, :], c["lens"]) for a in (bad, c["f32"]))
    old = float(np.abs(bad - c["ref"]).max())
    print(f"dropped third split term: e = {e:.3e}  e32 = {e32:.3e}  e/e32 = {e / e32:.1f}  max abs = {old:.3e} (old bound {S.DP_OLD_MAX_ABS_TOL})")
    assert not S.passes_vs_fp64(bad, c["ref"], c["f32"], c["lens"]), (e, e32)
    assert old <= S.DP_OLD_MAX_ABS_TOL, old


def test_zz_worst_ratios_of_this_run(lib):
    """Prints the worst e / e32 per kernel over the tests of this module that ran before it (DESIGN.md quotes the figures)."""
    S.print_ratios(WHERE)
