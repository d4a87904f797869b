"""One WaveNet layer of the coupling flow (csrc/kernels.h "fused WaveNet layer"): the fp64 reference, its float32
calibration, the per-element criterion and the case tables that tests/test_wn_layer.py (CPU model of the kernels) and
tests/test_gpu_wn_layer.py (MI355X) share.

The paths behind ``test_wn_layer(..., impl=)``: 0 = the two launches the engine falls back to (gate conv + res/skip conv), 1 =
launch_wn_layer (k_wn_layer<1> at H = 32; k_wn_layer<6>, k_wn_layer_h192<4>, <12> at H = 192), 2 = launch_wn_layer_b3
(k_wn_layer_b3 with 32-, 96- or 128-column tiles and two epilogue forms).

The rule, per row on its own [:, :L] with zero padding:  a = in(h) + cond,  u = tanh(a[:H]) * sigmoid(a[H:]),  rs = res_skip(u);
Crs = 2H: h' = h + rs[:H], skip (+)= rs[H:];  Crs = H: skip (+)= rs and h' is not written.

Criterion (assert_vs_fp64), the one of tests/attention_ref.py (norm_err and f32_bound are imported from there): for each output,
e = norm_err(kernel) and e32 = norm_err(wn_layer_f32), both against wn_layer_fp64 on the same inputs, per row over its own columns;
the kernel passes when e <= max(3 * e32, 2**-23), and its rel. RMS per row stays below the engine-level tests' 5e-6
(tests/util.py).  wn_layer_f32 is the calibration and is never under test: the rule in numpy float32 with the products summed tap by
tap, as many input channels per float32 addition as the path's matrix instruction takes per rounding of an accumulator (GROUP).
With whole taps summed by BLAS the calibration's error at T = 1 — one tap of five meets data — falls to 6e-8 and the intact
launch_wn_layer measured 3.7 x that."""
import functools
import os

import numpy as np

from tests.attention_ref import f32_bound, norm_err
from tests.util import TIGHT_REL_RMS_TOL, rel_rms

IMPL_NAMES = {0: "gate conv + res/skip conv", 1: "launch_wn_layer", 2: "launch_wn_layer_b3"}
JUNK = np.float32(-7.5e29)  # what the padding tests put at and past a row's length: large, finite, an unmistakable bit pattern


def _conv(x, w, bias, dil, dt, group=0):
    """'same' Conv1d of one row x [Cin, L] (zero padding) in dtype dt: the accumulator starts from the bias and takes the products tap
    by tap, `group` input channels per addition (0: a whole tap's)."""
    Cout, Cin, K = w.shape
    L = x.shape[1]
    pad = (K - 1) // 2 * dil
    xp = np.zeros((Cin, L + 2 * pad), dt)
    xp[:, pad:pad + L] = x
    acc = np.repeat(bias.astype(dt)[:, None], L, axis=1)
    g = group or Cin
    for k in range(K):
        for c0 in range(0, Cin, g):
            acc = acc + w[:, c0:c0 + g, k].astype(dt) @ xp[c0:c0 + g, k * dil:k * dil + L]
        assert acc.dtype == dt
    return acc


def _layer(h, skip, w_in, b_in, w_rs, b_rs, lens, dil, cond, skip_init, dt, group=0):
    h = np.asarray(h, dt)
    skip = np.asarray(skip, dt)
    B, H, T = h.shape
    two = w_rs.shape[0] == 2 * H
    h2 = np.zeros((B, H, T), dt)
    s2 = np.zeros((B, H, T), dt)
    one = dt(1.0)
    for b in range(B):
        L = int(lens[b])
        if L == 0:
            continue
        bc = np.asarray(b_in, dt) if cond is None else np.asarray(b_in, dt) + np.asarray(cond[b], dt)
        a = _conv(h[b, :, :L], w_in, bc, dil, dt, group)
        u = np.tanh(a[:H]) * (one / (one + np.exp(-a[H:])))
        rs = _conv(u, w_rs, b_rs, 1, dt, group)
        assert rs.dtype == dt
        if two:
            h2[b, :, :L] = h[b, :, :L] + rs[:H]
            s2[b, :, :L] = rs[H:] if skip_init else skip[b, :, :L] + rs[H:]
        else:
            s2[b, :, :L] = rs if skip_init else skip[b, :, :L] + rs
    return (h2 if two else None), s2


def wn_layer_fp64(h, skip, w_in, b_in, w_rs, b_rs, lens, dil=1, cond=None, skip_init=False):
    """The rule of this module's docstring in float64.  Returns (h' or None, skip'), zero at and past a row's length."""
    return _layer(h, skip, w_in, b_in, w_rs, b_rs, lens, dil, cond, skip_init, np.float64)


def wn_layer_f32(h, skip, w_in, b_in, w_rs, b_rs, lens, dil=1, cond=None, skip_init=False, group=2):
    """The same rule in numpy float32 throughout, as a float32 matrix instruction evaluates it: the products summed tap by tap, `group`
    input channels per float32 addition (the k of the instruction: see GROUP); tanh, exp and the divide are numpy's.  The calibration."""
    return _layer(h, skip, w_in, b_in, w_rs, b_rs, lens, dil, cond, skip_init, np.float32, group)


# input channels per float32 accumulation on an accumulator of the matrix instructions a path runs on: impl -> channels.  The
# two-launch path and launch_wn_layer: v_mfma_f32_32x32x2_f32, two channels per instruction.  launch_wn_layer_b3:
# v_mfma_f32_32x32x16_bf16 takes 16 channels, and a product of split operands takes six instructions (six roundings at the
# accumulator's size): 2.7 channels per accumulation.
GROUP = {0: 2, 1: 2, 2: 2}


def calibration(c, impl):
    """The float32 calibration (h' or None, skip') of case c for a path, computed once per instruction width."""
    g = GROUP[impl]
    if g not in c["f32"]:
        c["f32"][g] = wn_layer_f32(c["h"], c["skip"], c["w_in"], c["b_in"], c["w_rs"], c["b_rs"], c["lens"], c["dil"], c["cond"], c["skip_init"], g)
    return c["f32"][g]


@functools.lru_cache(maxsize=6)
def reference_case(H, T, K, dil, Crs, lens, with_cond=True, skip_init=False, seed=0):
    """The inputs of a case and its fp64 / float32 results, computed once and read-only: a dict.  h is zero at and past a row's
    length (impl 0 reads it there, as the engine's two-launch path does); the padding tests put JUNK there themselves."""
    rng = np.random.default_rng([seed, H, T, K, dil, Crs, int(with_cond), int(skip_init)])
    B = len(lens)
    ln = np.asarray(lens, np.int32)
    live = (np.arange(T)[None, :] < ln[:, None])[:, None, :]
    c = dict(
        h=(rng.standard_normal((B, H, T)) * live).astype(np.float32),
        skip=rng.standard_normal((B, H, T)).astype(np.float32),
        w_in=(rng.standard_normal((2 * H, H, K)) / np.sqrt(H * K)).astype(np.float32),
        b_in=(0.3 * rng.standard_normal(2 * H)).astype(np.float32),
        w_rs=(rng.standard_normal((Crs, H, 1)) / np.sqrt(H)).astype(np.float32),
        b_rs=(0.3 * rng.standard_normal(Crs)).astype(np.float32),
        cond=(0.5 * rng.standard_normal((B, 2 * H))).astype(np.float32) if with_cond else None,
        lens=ln, dil=dil, skip_init=skip_init)
    args = (c["h"], c["skip"], c["w_in"], c["b_in"], c["w_rs"], c["b_rs"], ln, dil, c["cond"], skip_init)
    c["ref"] = wn_layer_fp64(*args)
    c["f32"] = {}  # per instruction width: calibration()
    for v in list(c.values()) + list(c["ref"]):
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def run_case(lib, impl, c, h=None, skip=None, h_out_prior=None):
    return lib.test_wn_layer(c["h"] if h is None else h, c["skip"] if skip is None else skip, c["w_in"], c["b_in"], c["w_rs"], c["b_rs"],
                             c["lens"], dilation=c["dil"], cond=c["cond"], skip_init=c["skip_init"], impl=impl, h_out_prior=h_out_prior)


RATIOS = {}  # worst e / e32 seen per impl in this process (printed by the tests; DESIGN.md quotes them)


def assert_vs_fp64(got, c, impl, tag):
    """The criterion of this module's docstring on (h', skip') of a case.  Prints e, e32 and their ratio per output."""
    lens = c["lens"]
    for name, g, ref, f32 in zip(("h'", "skip"), got, c["ref"], calibration(c, impl)):
        if ref is None:
            continue
        assert g.shape == ref.shape and g.dtype == np.float32
        for b, L in enumerate(lens):
            assert np.isfinite(g[b][:, :int(L)]).all(), (tag, IMPL_NAMES[impl], name, b, "a valid element is not finite")
        e, e32 = norm_err(g, ref, lens), norm_err(f32, ref, lens)
        rms = max([rel_rms(g[b][:, :int(L)], ref[b][:, :int(L)]) for b, L in enumerate(lens) if L] or [0.0])
        ratio = e / max(e32, 1e-30)
        RATIOS[impl] = max(RATIOS.get(impl, 0.0), ratio if e > 2.0 ** -23 else 0.0)
        print(f"wn {IMPL_NAMES[impl]} {tag} {name}: e = {e:.3e}  e32 = {e32:.3e}  e/e32 = {ratio:.3f}  rel rms = {rms:.3e}")
        assert e <= f32_bound(e32), (tag, IMPL_NAMES[impl], name, e, e32, f32_bound(e32), worst_element(g, ref, lens))
        assert rms < TIGHT_REL_RMS_TOL, (tag, IMPL_NAMES[impl], name, rms)


def worst_element(got, ref, lens):
    """(row, channel, column, got, ref) of the largest difference over the rows' own columns: where a failure sits."""
    best = (0.0, None)
    for b, L in enumerate(lens):
        L = int(L)
        if L:
            d = np.abs(np.asarray(got[b][:, :L], np.float64) - ref[b][:, :L])
            d = np.where(np.isfinite(d), d, np.inf)
            i = np.unravel_index(int(np.argmax(d)), d.shape)
            if d[i] >= best[0]:
                best = (float(d[i]), (b, int(i[0]), int(i[1]), float(got[b][i]), float(ref[b][i])))
    return best[1]


def check_vs_fp64(lib, impl, H, T, K, dil, Crs, lens, with_cond=True, skip_init=False):
    c = reference_case(H, T, K, dil, Crs, tuple(int(n) for n in lens), with_cond, skip_init)
    got = run_case(lib, impl, c)
    assert_vs_fp64(got, c, impl, f"H={H} T={T} K={K} d={dil} Crs={Crs} cond={int(with_cond)} init={int(skip_init)}")
    return got


# ---------------------------------------------------------------------------------------------------- the case tables
TILE_WIDTHS = (32, 96, 128)  # what mi355vits_lab_wn_plan may report; k_wn_layer's workgroups are 32 columns wide
LENGTH_CLASSES = [1, 31, 32, 33, 95, 96, 97, 127, 128, 129]  # around every tile width; odd T: rows not 16-byte aligned (scalar staging)


def ragged_lengths(T, pad=2):
    """One batch row each: full, empty, column 1, and around every tile seam below T — one short of it, on it, one past it, and `pad`
    columns to either side (the end of the row inside the halo of the next / of its own last tile)."""
    s = {T, 0, 1}
    for w in TILE_WIDTHS:
        for m in range(w, T + 1, w):
            s |= {m - 1, m, m + 1, m - pad, m + pad}
    return sorted(n for n in s if 0 <= n <= T)


def case_lengths(T):
    """The rows of a length-class case: ragged_lengths(T), and full rows up to 8 in all (the criterion's float32 calibration is a
    maximum over the case's elements: a single column of 192 is a small sample)."""
    r = ragged_lengths(T)
    return r + [T] * max(0, 8 - len(r))


# (K, dilation): the shipped one, the small ones, the 24-column halo limit twice, the 8-column limit of the 128-column form
KD_CASES = [(5, 1), (1, 1), (3, 1), (5, 2), (5, 6), (7, 4), (3, 4)]
KD_T = 141  # a 128-column tile and a 13-column one, odd


def kd_lengths(K, dil):
    """Rows ending `pad` columns to either side of every tile seam (inside the halo of the next tile / of their own last one)."""
    pad = max(1, (K - 1) // 2 * dil)
    return sorted({KD_T, 128 + pad, 128, 128 - pad, 96 + pad, 96 - pad, 32 + pad, 33, 32 - pad, 1, 0})


KD_REFUSED = [(5, 7), (7, 5)]        # one past the 24-column limit: refused by impl 1 (LDS) and impl 2
KD_PAST_128 = [(3, 5), (5, 3)]       # one past the 8-column limit: the launcher serves them with the 96-column form
# (skip_init, Crs == 2H, cond given)
OPTION_CASES = [(si, two, cd) for si in (False, True) for two in (True, False) for cd in (True, False)]
FORMS_T = 300  # three 128-column, four 96-column and ten 32-column tiles, the last one ragged in every form
FORMS_LENS = (300, 258, 257, 256, 193, 129, 127, 97, 94, 33, 1, 0)  # ends on, before and past seams of all three widths


PATHS = [(1, 192), (2, 192), (1, 32)]  # (impl, H) of the fused layers


class Twice:
    """A library with every kernel-hook call repeated: the two results must be the same bits (a producer / consumer race is
    invisible to the CPU model; the device tests wrap their library in this)."""

    def __init__(self, lib):
        self.lib = lib

    def __getattr__(self, name):
        return getattr(self.lib, name)

    def _twice(self, fn, *a, **k):
        r1, r2 = fn(*a, **k), fn(*a, **k)
        for u, v in zip(r1 if isinstance(r1, tuple) else (r1,), r2 if isinstance(r2, tuple) else (r2,)):
            assert np.array_equal(u, v, equal_nan=True), (fn.__name__, "two runs of one case differ")
        return r1

    def test_mrf_stage(self, *a, **k):
        return self._twice(self.lib.test_mrf_stage, *a, **k)

    def test_wn_layer(self, *a, **k):
        return self._twice(self.lib.test_wn_layer, *a, **k)

    def test_conv1d(self, *a, **k):
        return self._twice(self.lib.test_conv1d, *a, **k)

    def test_conv_transpose1d(self, *a, **k):
        return self._twice(self.lib.test_conv_transpose1d, *a, **k)

    def test_enc_o_ln(self, *a, **k):
        return self._twice(self.lib.test_enc_o_ln, *a, **k)

    def test_conv_post(self, *a, **k):
        return self._twice(self.lib.test_conv_post, *a, **k)


class Env:
    """Sets the lab switches the launchers read at every launch (lab build and CPU model) and puts the old values back."""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


B3_FORMS = [dict(MI355VITS_WN_B3_NT=1), dict(MI355VITS_WN_B3_NT=3, MI355VITS_WN_EPI=0), dict(MI355VITS_WN_B3_NT=3, MI355VITS_WN_EPI=1),
            dict(MI355VITS_WN_B3_NT=4)]
B3_FORM_TILES = [32, 96, 96, 128]
F32_FORMS = [dict(MI355VITS_WN_SIX_WAVES=g) for g in (0, 1, 2)]


def forms_case(lib, impl, K=5, dil=1):
    """Every form of impl 1 / 2 through the lab switches on one ragged batch: the plan call reports the forced form, each form meets
    the criterion, and all forms of the impl give the same bits.  Returns the common result."""
    T = FORMS_T
    lens = FORMS_LENS
    c = reference_case(192, T, K, dil, 384, tuple(lens))
    outs = []
    for i, env in enumerate(B3_FORMS if impl == 2 else F32_FORMS):
        with Env(**env):
            tile, geom = lib.lab_wn_plan(len(lens), T, K, dil)
            if impl == 2:
                want = B3_FORM_TILES[i] if (K - 1) * dil <= 8 or B3_FORM_TILES[i] != 128 else 96
                assert tile == want, (env, tile, want)
            else:
                assert geom == i, (env, geom)
            got = run_case(lib, impl, c)
        assert_vs_fp64(got, c, impl, f"form {env}")
        outs.append(got)
    for i, o in enumerate(outs[1:], 1):  # (past a row's end the forms write different extents: the hook's comment)
        for name, a, b in zip(("h'", "skip"), outs[0], o):
            for r, L in enumerate(lens):
                assert np.array_equal(a[r, :, :L], b[r, :, :L]), (IMPL_NAMES[impl], name, "form", i, "differs from form 0 in row", r)
    return outs[0]


FORM_LENGTH_CLASSES = [1, 31, 95, 96, 97, 127, 128, 129]  # narrower than a wide tile, a tile + / - 1 (a one-column last tile), odd pitch


def forms_at_length(lib, impl, T):
    """Every form of impl 1 / 2 through the lab switches on a SMALL tensor: T columns, narrower than a 96- / 128-column tile or one
    column past it, odd T with rows that are not 16-byte aligned (the scalar staging branches of every geometry, the buffer-addressed
    epilogue of the 128-column form on an odd pitch).  Each form against fp64, and bit for bit the form the grid rule picks."""
    lens = sorted({T, T - 1, max(T - 33, 0), min(T, 33), 1, 0})
    lens += [T] * max(0, 6 - len(lens))
    c = reference_case(192, T, 5, 1, 384, tuple(lens))
    base = run_case(lib, impl, c)
    assert_vs_fp64(base, c, impl, f"T={T}, the grid rule's form")
    for i, env in enumerate(B3_FORMS if impl == 2 else F32_FORMS):
        with Env(**env):
            tile, geom = lib.lab_wn_plan(len(lens), T, 5, 1)
            assert (tile == B3_FORM_TILES[i]) if impl == 2 else (geom == i), (env, tile, geom)
            got = run_case(lib, impl, c)
        assert_vs_fp64(got, c, impl, f"T={T} form {env}")
        for name, a, b in zip(("h'", "skip"), base, got):
            for r, L in enumerate(lens):
                assert np.array_equal(a[r, :, :L], b[r, :, :L]), (IMPL_NAMES[impl], name, T, env, "differs from the default form in row", r)


def agree_case(lib, T=129, K=5, dil=1):
    """impl 0, 1 and 2 on one input: each within the criterion, pairwise within the sum of their bounds."""
    lens = ragged_lengths(T)
    c = reference_case(192, T, K, dil, 384, tuple(lens))
    outs = [run_case(lib, impl, c) for impl in (0, 1, 2)]
    for impl, o in enumerate(outs):
        assert_vs_fp64(o, c, impl, f"agree T={T}")
    for k, name in enumerate(("h'", "skip")):
        bounds = [f32_bound(norm_err(calibration(c, impl)[k], c["ref"][k], c["lens"])) for impl in (0, 1, 2)]
        for a, b in ((0, 1), (0, 2), (1, 2)):
            e, bound = norm_err(outs[a][k], outs[b][k], c["lens"]), bounds[a] + bounds[b]
            print(f"wn {name}: impl {a} vs impl {b}: {e:.3e} (bound {bound:.3e})")
            assert e <= bound, (name, a, b, e, bound)


def written_end(impl, L, T, tile):
    """First column of a row that the path leaves untouched (include/mi355vits_lab.h, mi355vits_test_wn_layer)."""
    if impl != 2:
        return T
    return min(T, -(-L // tile) * tile)


def padding_case(lib, impl, T=FORMS_T, K=5, dil=1, two=True, skip_init=False):
    """Everything at and past each row's length — h, the prior skip, the prior contents of h' — replaced by JUNK: every valid column
    keeps its bits, h' is zero up to the end of what the path writes, and every column the hook's comment calls untouched still holds
    JUNK.  impl 0 reads h past the length, as the engine's two-launch path does: its h stays zero there, the JUNK goes to the prior
    skip and h' only, and it is held to what the hook's comment says it writes (zeros in h', the update in skip, at every column)."""
    H = 192
    lens = FORMS_LENS
    c = reference_case(H, T, K, dil, 2 * H if two else H, tuple(lens), True, skip_init)
    plain_h, plain_s = run_case(lib, impl, c)
    past = (np.arange(T)[None, :] >= c["lens"][:, None])[:, None, :] & np.ones((1, H, 1), bool)
    h = c["h"] if impl == 0 else np.where(past, JUNK, c["h"])
    skip = np.where(past, JUNK, c["skip"])
    prior = np.full_like(c["h"], JUNK)
    got_h, got_s = run_case(lib, impl, c, h=h, skip=skip, h_out_prior=prior)
    tile, _ = lib.lab_wn_plan(len(lens), T, K, dil)
    for b, L in enumerate(int(n) for n in c["lens"]):
        end = written_end(impl, L, T, tile)
        assert np.array_equal(got_s[b, :, :L], plain_s[b, :, :L]), (IMPL_NAMES[impl], "skip", b, L)
        assert np.all(got_s[b, :, end:] == JUNK), (IMPL_NAMES[impl], "skip past the last computed tile", b, L, end)
        assert np.isfinite(got_s[b]).all()
        if impl == 0 and skip_init:  # every column written: no JUNK left (skip += on JUNK stays JUNK-sized, so only `=` can show it)
            assert np.all(np.abs(got_s[b]) < 1e6), (IMPL_NAMES[impl], "skip is written at every column", b)
        if two:
            assert np.array_equal(got_h[b, :, :L], plain_h[b, :, :L]), (IMPL_NAMES[impl], "h'", b, L)
            assert np.all(got_h[b, :, L:end] == 0.0), (IMPL_NAMES[impl], "h' is masked inside the last tile", b, L, end)
            assert np.all(got_h[b, :, end:] == JUNK), (IMPL_NAMES[impl], "h' past the last computed tile", b, L, end)
        elif impl != 0:  # (the hook reads the device's h' buffer back for impl 1 and 2; impl 0 works in place and reports nothing)
            assert np.all(got_h[b] == JUNK), (IMPL_NAMES[impl], "the last layer leaves h' alone", b)
    return tile


GRID_T = 3200


def grid_case(lib, impl, want):
    """The product's own grid rule: the smallest batch of 3,200-column rows for which the plan call reports the wanted form on this
    device (impl 2: `want` = the tile width 96 / 128; impl 1: the geometry 1 / 0) — every row bit for bit its single-row run (the
    32-column form / geometry 2), three rows against fp64.  Returns the batch size."""
    T = GRID_T
    assert lib.lab_wn_plan(1, T) == (32, 2)
    for B in range(2, 17):
        if lib.lab_wn_plan(B, T)[0 if impl == 2 else 1] == want:
            break
    else:
        raise AssertionError(f"no batch of up to 16 rows x {T} columns reaches form {want} on this device")
    lens = tuple(T - (37 * b) % 300 for b in range(B))
    c = reference_case(192, T, 5, 1, 384, lens)
    h2, s2 = run_case(lib, impl, c)
    assert_vs_fp64((h2, s2), c, impl, f"{B} rows x {T}: form {want}")
    for b, L in enumerate(lens):
        o_h, o_s = lib.test_wn_layer(c["h"][b:b + 1], c["skip"][b:b + 1], c["w_in"], c["b_in"], c["w_rs"], c["b_rs"], c["lens"][b:b + 1],
                                     dilation=1, cond=c["cond"][b:b + 1], skip_init=False, impl=impl)
        assert np.array_equal(o_h[0, :, :L], h2[b, :, :L]) and np.array_equal(o_s[0, :, :L], s2[b, :, :L]), (impl, want, b, "differs from its single-row bits")
    return B
