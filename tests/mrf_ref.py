"""One multi-receptive-field stage of the decoder (csrc/kernels.h "fused multi-receptive-field stage"): the fp64
reference, its float32 calibration, the per-element criterion and the case tables that tests/test_mrf_stage.py (CPU model of the
kernels) and tests/test_gpu_mrf_stage.py (MI355X) share.

The kernels behind ``test_mrf_stage(..., impl=)``: 0 = k_mrf_fused (f32 tiles in LDS; MATH_F32 or MATH_BF16X3), 1 = k_mrf_p<32>,
<64> ((row, column block) items of a persistent grid), 2 = k_mrf_s<64> (the row sweep over segments; the bits of k_mrf_p).

The rule, every row alone on its own [:, :L] with zero padding ("a row is synthesised as if it were alone"):
  y = s * sum_j RB_j(x),  RB_j: x1 = x + conv_{k_j,d1_j}(lrelu_0.1 x),  x2 = x1 + conv_{k_j,d2_j}(lrelu_0.1 x1),
  s = out_scale when out_scale > 0, else 1 / n.  The zero padding of the second conv is x1's own: x1 counts as zero outside [0, L).

Criterion (assert_vs_fp64), the one of tests/attention_ref.py (norm_err and f32_bound are imported from there): e =
norm_err(kernel) and e32 = norm_err(mrf_stage_f32), both against mrf_stage_fp64 on the same inputs, per row over its own columns;
the kernel passes when e <= max(3 * e32, 2**-23), and its rel. RMS per row stays below the engine-level tests' 5e-6
(tests/util.py).  mrf_stage_f32 is the calibration and is never under test: the rule in numpy float32 as a float32 matrix
instruction has to evaluate it — the accumulator starts from the residual (conv2: from the running sum over the resblocks), the
products join it tap by tap, as many input channels per float32 addition as the kernel's instruction takes per rounding of an
accumulator (GROUP).  With every conv summed apart and added afterwards (_stage with group = 0) the intact kernels measured 3.6
(k_mrf_p / k_mrf_s) to 10.4 (k_mrf_fused in f32) x the calibration's error, evenly over all columns: each of their additions
rounds at the size of the running sum."""
import functools

import numpy as np

from tests.attention_ref import f32_bound, norm_err
from tests.util import TIGHT_REL_RMS_TOL, rel_rms
from tests.wn_ref import JUNK, Twice, _conv, worst_element  # noqa: F401 (Twice: the device tests wrap their library in it)

IMPL_NAMES = {0: "k_mrf_fused", 1: "k_mrf_p", 2: "k_mrf_s"}
LOW_KS = (3, 5, 7)
LOW_DILS = ((1, 2), (2, 6), (3, 12))  # the "_low" voices': the one set k_mrf_p / k_mrf_s serve on the device
OTHER_DILS = [((1, 3), (1, 3), (1, 3)), ((3, 1), (2, 1), (1, 2))]  # the CPU model's k_mrf_p / k_mrf_s run them too (tests/test_emu_engine.py)


def _stage(x, ks, dils, weights, biases, lens, out_scale, dt, group=0):
    """group = 0: every conv summed on its own (from its bias, tap by tap) and then added to its residual — the rule as written.
    group > 0: the accumulator starts from the residual (conv1: x + bias; conv2: the running sum over the resblocks + x1 + bias) and
    takes the products `group` input channels at a time, tap by tap."""
    x = np.asarray(x, dt)
    B, C, T = x.shape
    y = np.zeros((B, C, T), dt)
    slope = dt(0.1)
    lrelu = lambda v: np.where(v >= 0, v, v * slope)
    scale = dt(out_scale) if out_scale > 0 else dt(1.0) / dt(len(ks))

    def onto(seed, v, w, dil):
        K = w.shape[2]
        L = v.shape[1]
        pad = (K - 1) // 2 * dil
        vp = np.zeros((C, L + 2 * pad), dt)
        vp[:, pad:pad + L] = v
        acc = seed
        for k in range(K):
            for c0 in range(0, C, group):
                acc = acc + w[:, c0:c0 + group, k].astype(dt) @ vp[c0:c0 + group, k * dil:k * dil + L]
        assert acc.dtype == dt
        return acc

    for b in range(B):
        L = int(lens[b])
        if L == 0:
            continue
        xb = x[b, :, :L]
        acc = np.zeros((C, L), dt)
        for j in range(len(ks)):
            if group:
                x1 = onto(xb + biases[j][0].astype(dt)[:, None], lrelu(xb), weights[j][0], dils[j][0])
                acc = onto(acc + (x1 + biases[j][1].astype(dt)[:, None]), lrelu(x1), weights[j][1], dils[j][1])
            else:
                x1 = xb + _conv(lrelu(xb), weights[j][0], biases[j][0], dils[j][0], dt)
                x2 = x1 + _conv(lrelu(x1), weights[j][1], biases[j][1], dils[j][1], dt)
                acc = acc + x2
            assert acc.dtype == dt
        y[b, :, :L] = acc * scale
    return y


def mrf_stage_fp64(x, ks, dils, weights, biases, lens, out_scale=0.0):
    """The rule of this module's docstring in float64; zero at and past a row's length."""
    return _stage(x, ks, dils, weights, biases, lens, out_scale, np.float64)


def mrf_stage_f32(x, ks, dils, weights, biases, lens, out_scale=0.0, group=2):
    """The same rule in numpy float32 throughout, as a float32 matrix instruction evaluates it: x2 = x1 + conv(..) and y = sum_j
    accumulate, so the accumulator starts from the residual / the running sum and takes the products tap by tap, `group` input
    channels per float32 addition (the k of the instruction: see GROUP).  The calibration."""
    return _stage(x, ks, dils, weights, biases, lens, out_scale, np.float32, group)


# input channels per float32 accumulation on an accumulator of the matrix instructions a kernel form runs on: (impl, math) -> channels.
#   k_mrf_fused MATH_F32: v_mfma_f32_32x32x2_f32, two channels per instruction.  MATH_BF16X3: v_mfma_f32_32x32x16_bf16 takes 16
#   channels, and a product of split operands takes six instructions (six roundings at the accumulator's size): 2.7 per accumulation.
#   k_mrf_p / k_mrf_s: v_mfma_f32_16x16x32_bf16 takes 32 channels; the six instructions of a split product go to two accumulator
#   chains of three, joined once per 32 channels: 10.7 channels per accumulation of a chain, rounded down to a divisor of 32.
GROUP = {(0, 0): 2, (0, 1): 2, (1, 1): 8, (2, 1): 8}


def calibration(c, impl, math=None):
    """The float32 calibration of case c for a kernel form, computed once per instruction width."""
    g = GROUP[(impl, (0 if impl == 0 else 1) if math is None else int(math))]
    if g not in c["f32"]:
        c["f32"][g] = mrf_stage_f32(c["x"], c["ks"], c["dils"], c["w"], c["b"], c["lens"], c["out_scale"], g)
        c["f32"][g].flags.writeable = False
    return c["f32"][g]


@functools.lru_cache(maxsize=4)
def reference_case(C, T, ks, dils, lens, out_scale=0.0, seed=0):
    """The inputs of a case and its fp64 / float32 results, computed once and read-only: a dict."""
    rng = np.random.default_rng([seed, C, T, len(ks)] + [d for p in dils for d in p])
    B = len(lens)
    c = dict(x=rng.standard_normal((B, C, T)).astype(np.float32), ks=ks, dils=dils, d1=[p[0] for p in dils], d2=[p[1] for p in dils],
             w=[[(rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32) for _ in range(2)] for k in ks],
             b=[[(0.1 * rng.standard_normal(C)).astype(np.float32) for _ in range(2)] for _ in ks],
             lens=np.asarray(lens, np.int32), out_scale=out_scale)
    c["ref"] = mrf_stage_fp64(c["x"], ks, dils, c["w"], c["b"], c["lens"], out_scale)
    c["f32"] = {}  # per instruction width: calibration()
    for v in [c["x"], c["lens"], c["ref"]] + [a for p in c["w"] + c["b"] for a in p]:
        v.flags.writeable = False
    return c


def run_case(lib, impl, c, math=None, seg=0, x=None, y_prior=None, rows=None):
    """The hook on the case (rows: a subset of its batch, as a batch of its own)."""
    xx = c["x"] if x is None else x
    lens = c["lens"]
    if rows is not None:
        xx, lens = xx[rows], lens[rows]
        y_prior = None if y_prior is None else y_prior[rows]
    return lib.test_mrf_stage(xx, c["ks"], c["d1"], c["d2"], c["w"], c["b"], lens, impl=impl, math=math, out_scale=c["out_scale"], seg=seg,
                              y_prior=y_prior)


RATIOS = {}  # worst e / e32 seen per impl in this process (printed by the tests; DESIGN.md quotes them)


def assert_vs_fp64(got, c, impl, tag, rows=None, math=None):
    """The criterion of this module's docstring.  Prints e, e32 and their ratio."""
    rows = list(range(len(c["lens"]))) if rows is None else list(rows)
    lens, ref, f32 = c["lens"][rows], c["ref"][rows], calibration(c, impl, math)[rows]
    assert got.shape == ref.shape and got.dtype == np.float32
    for b, L in enumerate(lens):
        assert np.isfinite(got[b][:, :int(L)]).all(), (tag, IMPL_NAMES[impl], b, "a valid element is not finite")
    e, e32 = norm_err(got, ref, lens), norm_err(f32, ref, lens)
    rms = max([rel_rms(got[b][:, :int(L)], ref[b][:, :int(L)]) for b, L in enumerate(lens) if L] or [0.0])
    ratio = e / max(e32, 1e-30)
    key = (impl, (0 if impl == 0 else 1) if math is None else int(math))
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio if e > 2.0 ** -23 else 0.0)
    print(f"mrf {IMPL_NAMES[impl]} {tag}: e = {e:.3e}  e32 = {e32:.3e}  e/e32 = {ratio:.3f}  rel rms = {rms:.3e}")
    assert e <= f32_bound(e32), (tag, IMPL_NAMES[impl], e, e32, f32_bound(e32), worst_element(got, ref, lens))
    assert rms < TIGHT_REL_RMS_TOL, (tag, IMPL_NAMES[impl], rms)


def check_vs_fp64(lib, impl, C, T, ks, dils, lens, out_scale=0.0, math=None, seg=0):
    c = reference_case(C, T, tuple(ks), tuple(tuple(p) for p in dils), tuple(int(n) for n in lens), out_scale)
    got = run_case(lib, impl, c, math=math, seg=seg)
    assert_vs_fp64(got, c, impl, f"C={C} T={T} ks={tuple(ks)} dils={tuple(dils)} scale={out_scale} math={math} seg={seg}", math=math)
    return got


# ---------------------------------------------------------------------------------------------------- the case tables
def edge_lengths(W, R):
    """Row ends (and tensor widths) around a work item of W columns with a halo of R: 1, 2, R, R + 1, W - 1, W, W + 1, W + R,
    W + R + 1, 2 W + 1."""
    return sorted({1, 2, R, R + 1, W - 1, W, W + 1, W + R, W + R + 1, 2 * W + 1})


def ragged_batch(W, R):
    """One batch of width 2 W + 1: a row per edge length, an empty row, a one-column row."""
    return [0] + edge_lengths(W, R)


def written_end(impl, L, T, W, seg=0):
    """First column of a row that the kernel leaves untouched (include/mi355vits_lab.h, mi355vits_test_mrf_stage); W = the plan
    call's width (k_mrf_p: the item, k_mrf_s: the step)."""
    if impl == 0:
        return T
    if L == 0:
        return 0
    if impl == 1:
        return min(T, -(-L // W) * W)
    c0 = (L - 1) // seg * seg
    return min(T, c0 + seg, c0 + -(-(L - c0) // W) * W)


def padding_case(lib, impl, c, W, plain, math=None, seg=0):
    """Everything at and past each row's length — x and the prior contents of y — replaced by JUNK: every valid column keeps the
    bits of `plain` (the same case run on clean buffers), every written column is finite, and every column the hook's comment calls
    untouched still holds JUNK."""
    B, C, T = c["x"].shape
    past = (np.arange(T)[None, :] >= c["lens"][:, None])[:, None, :] & np.ones((1, C, 1), bool)
    x = np.where(past, JUNK, c["x"])
    got = run_case(lib, impl, c, math=math, seg=seg, x=x, y_prior=np.full_like(c["x"], JUNK))
    for b, L in enumerate(int(n) for n in c["lens"]):
        end = written_end(impl, L, T, W, seg)
        assert np.array_equal(got[b, :, :L], plain[b, :, :L]), (IMPL_NAMES[impl], "valid columns changed with the padding", b, L)
        assert np.isfinite(got[b, :, :end]).all() and np.all(np.abs(got[b, :, L:end]) < 1e6), (IMPL_NAMES[impl], "junk reached a written column", b, L, end)
        assert np.all(got[b, :, end:] == JUNK), (IMPL_NAMES[impl], "a column past the last computed item was written", b, L, end)


def plan(lib, impl, C, ks=LOW_KS, dils=LOW_DILS):
    return lib.lab_mrf_plan(impl, C, ks, [p[0] for p in dils], [p[1] for p in dils])


def block_case(lib, C, dils=LOW_DILS, out_scale=0.0):
    """k_mrf_p on the ragged batch around its work item (width 2 W + 1, odd: rows not 16-byte aligned): against fp64, and
    independent of the padding.  Returns (case, output)."""
    W, R, _, _ = plan(lib, 1, C, LOW_KS, dils)
    c = reference_case(C, 2 * W + 1, LOW_KS, tuple(dils), tuple(ragged_batch(W, R)), out_scale)
    got = run_case(lib, 1, c)
    assert_vs_fp64(got, c, 1, f"C={C} dils={dils} ragged batch")
    padding_case(lib, 1, c, W, got)
    return c, got


def width_case(lib, C, T, dils=LOW_DILS):
    """A tensor T columns wide (rows: full, one short, one column, empty): k_mrf_p against fp64; at 64 channels k_mrf_s with one-step
    segments and with one segment for the row gives the same bits."""
    c = reference_case(C, T, LOW_KS, tuple(dils), tuple(sorted({T, max(T - 1, 0), 1, 0})))
    got = run_case(lib, 1, c)
    assert_vs_fp64(got, c, 1, f"C={C} T={T}")
    if C == 64:
        S = plan(lib, 2, C, LOW_KS, dils)[0]
        for seg in (S, -(-T // S) * S):
            s = run_case(lib, 2, c, seg=seg)
            for b, L in enumerate(int(n) for n in c["lens"]):
                assert np.array_equal(s[b, :, :L], got[b, :, :L]), ("k_mrf_s differs from k_mrf_p", T, seg, b)
    return got


SWEEP_T = 1205  # 1152 + one step + 5: the planner's shortest segment (24 steps) and a short, ragged second one
SWEEP_ROWS = (0, 30, 1147, 1152, 1157, 1205)  # empty, shorter than the pipeline fill, in the last step of the first 1152-column
# segment, on the seam, in the first step of the second segment, full (the last, partial step of the second)


def sweep_case(lib, segs, dils=LOW_DILS, T=SWEEP_T, rows=SWEEP_ROWS, padding_segs=()):
    """k_mrf_s on one batch for every segment length of `segs`: bit for bit k_mrf_p (as the engine relies on), against fp64, and
    (padding_segs) independent of the padding.  The default batch is long enough for both rings (128 / 176 columns) to wrap more
    than six times."""
    S, R, xr, x1r = plan(lib, 2, 64, LOW_KS, dils)
    assert T != SWEEP_T or T > 3 * max(xr, x1r) + 2 * S
    c = reference_case(64, T, LOW_KS, tuple(dils), tuple(rows))
    p = run_case(lib, 1, c)
    assert_vs_fp64(p, c, 1, f"sweep case T={T}, k_mrf_p dils={dils}")
    for seg in segs:
        assert seg % S == 0
        s = run_case(lib, 2, c, seg=seg)
        for b, L in enumerate(int(n) for n in c["lens"]):
            assert np.array_equal(s[b, :, :L], p[b, :, :L]), ("k_mrf_s differs from k_mrf_p", seg, b, L)
        assert_vs_fp64(s, c, 2, f"sweep T={T} seg={seg} dils={dils}")
        if seg in padding_segs:
            padding_case(lib, 2, c, S, s, seg=seg)


# k_mrf_fused: (C, taps, dilations, math, out_scale)
FUSED_CASES = [
    (32, LOW_KS, LOW_DILS, 0, 0.0), (32, LOW_KS, LOW_DILS, 1, 0.5), (32, (3,), ((1, 3),), 1, 0.0), (32, (3, 5), ((3, 1), (2, 1)), 0, 0.25),
    (64, LOW_KS, LOW_DILS, 0, 0.37), (64, LOW_KS, LOW_DILS, 1, 0.0), (64, (3, 5), ((3, 1), (2, 1)), 1, 0.5), (64, (3,), ((1, 2),), 0, 0.0),
    (128, (3, 5), ((1, 2), (2, 6)), 0, 0.0), (128, (3, 5), ((1, 2), (2, 6)), 1, 1.0 / 3.0), (128, (3,), ((1, 3),), 1, 0.0),
    (128, (3, 3, 3), ((1, 3), (1, 3), (1, 3)), 0, 0.5),
]


def fused_width_case(lib, C, math, T):
    """k_mrf_fused on a tensor T columns wide (rows: full, one short, one column, empty): T below the halo, a one-column last item,
    small and odd row pitches."""
    c = reference_case(C, T, LOW_KS, LOW_DILS, tuple(sorted({T, max(T - 1, 0), 1, 0})))
    got = run_case(lib, 0, c, math=math)
    assert_vs_fp64(got, c, 0, f"C={C} T={T} math={math}", math=math)
    return got


def fused_case(lib, C, ks, dils, math, out_scale):
    W, R, _, _ = plan(lib, 0, C, ks, dils)
    c = reference_case(C, 2 * W + 1, tuple(ks), tuple(dils), tuple(ragged_batch(W, R)), out_scale)
    got = run_case(lib, 0, c, math=math)
    assert_vs_fp64(got, c, 0, f"C={C} ks={ks} dils={dils} math={math} scale={out_scale}", math=math)
    padding_case(lib, 0, c, W, got, math=math)
    return got


def many_items_case(lib, C, cus, items_per_row=30):
    """More work items than compute units (several items per persistent workgroup; at 32 channels the next item's x is staged under
    the running one): rows of `items_per_row` items, ragged, as one batch — every row bit for bit its single-row run (one item per
    workgroup), three rows against fp64."""
    W, R, _, _ = plan(lib, 1, C)
    T = items_per_row * W
    B = cus // items_per_row + 2
    lens = [T - (b * (W // 3 + 1)) % (2 * W) for b in range(B)]
    lens[1] = T - W - 1
    assert sum(-(-n // W) for n in lens) > cus
    c = reference_case(C, T, LOW_KS, LOW_DILS, tuple(lens))
    got = run_case(lib, 1, c)
    for b in range(B):
        one = run_case(lib, 1, c, rows=[b])
        assert np.array_equal(one[0, :, :lens[b]], got[b, :, :lens[b]]), (C, b, "a row of the full grid differs from its single-row bits")
    rows = [0, 1, B - 1]
    assert_vs_fp64(got[rows], c, 1, f"C={C} {B} rows x {items_per_row} items on {cus} compute units", rows=rows)
    return got
