/* mi355vits_lab.h — test / benchmark / probe hooks around the kernels of libmi355vits (NOT the product ABI: that is
 * include/mi355vits.h, which mirrors the reference's onnxruntime boundary, mimic3_tts/voice.py:230,403-405).
 *
 * Exported by
 *   mimic3_amd/csrc/libmi355vits_hooks.so  — the product library's own object files + csrc/lab_api.cpp: the kernel-level tests
 *                                            (tests/test_gpu_parity.py ...) and bench.py's box probe run the PRODUCT's kernels through it;
 *   mimic3_amd/csrc/libmi355vits_lab.so    — the -DMI355_LAB build (kernel-choice switches for A/B runs, tools/);
 *   tests/emu/libmi355vits_emu.so          — the CPU model of the kernels.
 * libmi355vits.so itself exports none of these symbols. */
#ifndef MI355VITS_LAB_H
#define MI355VITS_LAB_H

#include "mi355vits.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel unit-test hook: ONE Conv1d ("same" padding, odd or even K) through a chosen implementation on host buffers, with the standard
 * epilogue of csrc/kernels_conv.cpp (epi_std), in this order:
 *   v = conv(lrelu_{in_slope}(x * [t < in_len[b]])); v += bias; v += cond[b]; relu; (mask_before_res: v = 0 at t >= out_len[b]);
 *   v = res + v (res_sub: res - v); v *= out_scale; (not mask_before_res: v = 0 at t >= out_len[b]); accumulate: v += y;  y = v.
 * The hook packs the weights with the library's own pack functions, as the engine does for the chosen kernel.
 * impl: 0 = launch_conv1d_generic (k_conv1d_generic: any shape), math MI355VITS_MATH_F32;
 *       1 = launch_conv1d_mfma in MATH_F32 (k_conv1d_mfma staged, k_conv_direct_mfma, k_conv_direct_splitk — the launcher's rule; even Cin);
 *       2 = launch_conv1d_mfma on the split-bf16 staged kernel (k_conv1d_b3), math MATH_BF16X3 or MATH_BF16W (the weights count with
 *           their leading bf16 term only): Cin % 32 == 0 and T > 512, or any T with fixed_rule (the flow's and decoder's convs: the
 *           kernel follows the layer, never T);
 *       3 = launch_enc_conv_b3 (k_enc_b3, k_enc_b3w), math MATH_BF16X3 or MATH_BF16W: Cin = 96 or Cin % 192 == 0, K in {1, 3}, dilation 1;
 *           Cin > 192: the raw sums of the 192-channel slices added up in slice order by the hook — no bias, cond, res, relu, scale,
 *           out_len or accumulate;
 *       4 = launch_rb_conv (k_rb_conv, k_rb_conv_pw: every input channel resident in LDS), math MATH_BF16X3: Cin = Cout = 128, (K,
 *           dilation) in {(3,1), (3,2), (5,2), (5,6), (7,3), (7,12)}; needs res and in_len; no cond, relu, res_sub, mask_before_res, out_len.
 * fixed_rule (impl 1 and 2 only) = ConvArgs.fixed_rule.  A shape, math mode or option the chosen kernel does not serve is
 * MI355VITS_ERR_INVALID before any launch.  Which form of an impl runs is the launcher's business: mi355vits_lab_conv_plan reports it.
 * The caller's y goes to the device first (it is the accumulate source, and a column no kernel writes keeps it).
 * At and past in_len[b] / out_len[b] (0 <= len <= T; NULL = T), per row:
 *   x       no kernel uses it at t >= in_len[b], and every one masks by SELECT: impl 0, 1 do not load it there (impl 1's staged form
 *           does not even with 16-byte loads: a quad that straddles in_len[b] is loaded element by element); impl 2, 3, 4 clamp every
 *           load to column max(in_len[b] - 1, 0) and discard by select.  Any finite or non-finite bits may lie there.
 *   y       impl 0 - 3 write every column t < T of every row.  At out_len[b] <= t < T the epilogue above gives, and the kernels
 *           write: exact zeros without accumulate and without mask_before_res (res is then discarded by select: any bits);
 *           res * out_scale with mask_before_res (res or res - 0); plus the prior y with accumulate (the prior y and, with
 *           mask_before_res, res are then READ there and enter by arithmetic).  Without out_len nothing is masked: a column
 *           in_len[b] <= t < T holds the conv of the zero-extended row (its taps that reach below in_len[b], else bias + cond ...).
 *           impl 4 never computes an item that starts at or past in_len[b]: it writes up to the end of the item that holds column
 *           in_len[b] - 1 (item = the plan call's cols) and masks nothing (it has no out_len): at in_len[b] <= t inside that item
 *           the same epilogue on the zero-extended row — res and, accumulating, the prior y are READ there and enter by arithmetic,
 *           the consumer masks —, every later column keeps what y held; a row with in_len[b] = 0 is not touched.
 *   res     impl 0 - 3: discarded by select at t >= out_len[b], except with mask_before_res (above); impl 4: above.
 *   cond    [B, Cout], one value per row and channel: no padding.
 * Columns below the lengths depend on nothing at or past them and on no other row. */
typedef struct mi355vits_conv_test {
    int32_t impl, B, Cin, Cout, T, K, dilation;
    const float* x;       /* [B,Cin,T] */
    const float* w;       /* [Cout,Cin,K] */
    const float* bias;    /* [Cout] or NULL */
    const float* res;     /* [B,Cout,T] or NULL */
    const int32_t* in_len;  /* [B] or NULL */
    const int32_t* out_len; /* [B] or NULL */
    float in_slope;       /* leaky-relu slope on the input, 1 = identity */
    int32_t relu;         /* relu on the output */
    float out_scale;
    int32_t res_sub;      /* y = res - conv instead of res + conv */
    float* y;             /* [B,Cout,T]: its prior contents go to the device first; the accumulate source when accumulate != 0 */
    int32_t accumulate;
    int32_t math;         /* MI355VITS_MATH_F32 for impl 0 / 1; _BF16X3 or _BF16W for impl 2 / 3; _BF16X3 for impl 4 */
    const float* cond;    /* [B,Cout] or NULL */
    int32_t mask_before_res;
    int32_t fixed_rule;
} mi355vits_conv_test;
int mi355vits_test_conv1d(int device, const mi355vits_conv_test* t);
/* Kernel unit-test hook: ONE ConvTranspose1d (padding (K - stride) / 2) of lrelu_{in_slope}(x): x [B,Cin,Tin], w [Cin,Cout,K], y [B,Cout,
 * Tin * stride].  impl: 0 = launch_conv_transpose1d (k_conv_transpose1d: any shape), 1 = the polyphase filters (convt_to_polyphase) on
 * launch_conv1d_mfma in MATH_F32, 2 = on its split-bf16 staged kernels in MATH_BF16X3 (Cin % 32 == 0; 64-channel chunks run the
 * persistent producer / consumer form), 3 = launch_ups_pl (k_ups_pl: 256 -> 128 and 128 -> 64 with stride 8 / K 16; k_ups64: 64 -> 32
 * with stride 4 / K 8), MATH_BF16X3.  K >= stride with K - stride even (the output is then exactly Tin * stride samples); anything else,
 * or a shape the chosen kernel does not serve, is MI355VITS_ERR_INVALID before any launch.
 * in_len [B] (0 <= in_len[b] <= Tin) or NULL = every row at full length: impl 3 only (anything else: MI355VITS_ERR_INVALID).
 * The caller's y goes to the device first.  impl 0 - 2 write every output position n < Tin * stride of every row.  impl 3 writes the
 * positions of the items it computes: at least every n < in_len[b] * stride, computed from x * [t < in_len[b]] (x is not used at or
 * past in_len[b]: clamped loads, select); positions at or past in_len[b] * stride are left undefined (written or not, by the item
 * width the plan call reports), and a row with in_len[b] = 0 is not touched. */
int mi355vits_test_conv_transpose1d(int device, int impl, int B, int Cin, int Cout, int Tin, int K, int stride,
                                    const float* x, const float* w, const float* bias, float in_slope, const int32_t* in_len, float* y);
/* What the conv launchers would run for a hook call of this shape on the current device, every base pointer 16-byte aligned as the
 * hooks' buffers are: stride = 0: mi355vits_test_conv1d(impl) on [B,Cin,T]; stride > 0: mi355vits_test_conv_transpose1d(impl) with
 * Tin = T (dilation ignored).  has_res / has_cond: whether the call passes res / cond (they enter the choice of the epilogue path and
 * of the encoder kernel's wide form); len = in_len [B] or NULL (the persistent kernels size their grid by the rows' items).
 * The launchers' own functions (with the lab switches where they are read).  Host arithmetic only: no kernel runs.
 * MI355VITS_ERR_INVALID where the hook would refuse the call. */
enum {
    MI355VITS_CONVK_GENERIC = 0, MI355VITS_CONVK_F32_STAGED = 1, MI355VITS_CONVK_F32_DIRECT = 2, MI355VITS_CONVK_F32_SPLITK = 3,
    MI355VITS_CONVK_B3_STAGED32 = 4, MI355VITS_CONVK_B3_STAGED64 = 5, MI355VITS_CONVK_B3_PC = 6, MI355VITS_CONVK_ENC_B3 = 7,
    MI355VITS_CONVK_ENC_B3W8 = 8, MI355VITS_CONVK_ENC_B3W6 = 9, MI355VITS_CONVK_RB_CONV = 10, MI355VITS_CONVK_RB_CONV_PW = 11,
    MI355VITS_CONVK_UPS_PL = 12, MI355VITS_CONVK_UPS64 = 13, MI355VITS_CONVK_CONVT_GENERIC = 14
};
typedef struct mi355vits_conv_plan {
    int32_t kernel;          /* MI355VITS_CONVK_* */
    int32_t cols, rows;      /* a work item: conv positions (transposed: input positions; the generic transposed kernel: output samples) x output rows */
    int32_t MT, NT, WM, WN;  /* tile shape of the staged / direct MFMA kernels; 0 where the kernel has one shape */
    int32_t chunk;           /* input channels staged at a time (0: none) */
    int32_t ring;            /* k_conv1d_mfma: 32 = 64-channel chunks (a tap's pairs unrolled), 0 = ring pipeline, -1 = plain loop */
    int32_t rb_loop;         /* k_enc_b3 / k_enc_b3w: row blocks per workgroup */
    int32_t vec, yvec, ovec; /* 16-byte staging loads / vector stores / the row-major epilogue through LDS */
    int32_t grid[3];         /* persistent kernels: grid[0] workgroups */
    int32_t lds_bytes;
} mi355vits_conv_plan;
int mi355vits_lab_conv_plan(int impl, int B, int Cin, int Cout, int T, int K, int dilation, int stride, int math, int fixed_rule,
                            int has_res, int has_cond, const int32_t* len, mi355vits_conv_plan* out);
/* Kernel unit-test hook: launch_enc_o_ln (k_enc_o_ln) alone, the attention block's tail of the text encoder:
 *   y = LN_c(res + conv1x1(x * [t < in_len[b]]) + bias) * [t < ln_out_len[b]],  192 -> 192 channels, LayerNorm over the channels with
 * gamma / beta [192] and eps, math MI355VITS_MATH_BF16X3 or _BF16W.  x, res [B,192,T]; in_len, ln_out_len [B] or NULL.  in_place = 0:
 * y is a buffer of its own (the caller's y goes to the device first); in_place != 0: the kernel runs with y == res on the device (y's
 * prior contents are not used) and the result is returned in y.  Anything else than 192 channels or these math modes:
 * MI355VITS_ERR_INVALID.  At and past the lengths: x is not used at t >= in_len[b] (clamped loads, select); res IS read at every
 * t < T (it enters the statistics of its own column only) and discarded by select at t >= ln_out_len[b]: any bits; y is written at
 * every t < T, exact zeros at t >= ln_out_len[b]. */
int mi355vits_test_enc_o_ln(int device, int math, int B, int T, const float* x, const float* w, const float* bias, const float* res,
                            const float* gamma, const float* beta, float eps, const int32_t* in_len, const int32_t* ln_out_len,
                            int in_place, float* y);
/* Kernel unit-test hook: the decoder's tail, launch_conv_post_tanh then launch_pcm16, on host buffers:
 *   audio[b, t] = tanh(sum_{c,k} w[c, k] * lrelu_0.01(x[b, c, t - (K - 1) / 2 + k] * [. < valid_len[b]])),  no bias, K odd;
 *   peaks[b] = max_{t < valid_len[b]} |audio[b, t]| (0 for an empty row);
 *   pcm[b, t] = audio_float_to_int16 of the row with its own peak (scale 32767 / max(0.01, peak), clip, truncate), then audioop.mul by
 *   volumes[b] when volumes is given and != 1 (double product, clip, floor); 0 at t >= valid_len[b].
 * x [B,Cin,L], w [1,Cin,K], valid_len [B] (0 <= valid_len[b] <= L), volumes [B] doubles or NULL.  audio [B,L], peaks [B], pcm [B,L]:
 * their prior contents go to the device first (peaks is then zeroed, as the engine does before the launch).  *kernel (or NULL) = the
 * kernel launch_conv_post_tanh picked: 0 = k_conv_post_tanh_dpp (K = 7, Cin % 4 == 0, L % 4 == 0), 1 = k_conv_post_tanh_vec (odd K <= 9,
 * L % 4 == 0), 2 = k_conv_post_tanh (any); in the lab build and the CPU model MI355VITS_CONV_POST_V1 takes the first away,
 * MI355VITS_CONV_POST_STAGED the first two.  All three give the same bits.
 * At and past valid_len[b]: x is not used (select; the dpp kernel switches whole 16-byte loads off); audio is written at every
 * t < L — the conv of the zero-extended row: non-zero within (K - 1) / 2 samples of valid_len[b], exact zeros behind; pcm is written
 * at every t < L, zero there. */
int mi355vits_test_conv_post(int device, int B, int Cin, int K, int L, const float* x, const float* w, const int32_t* valid_len,
                             const double* volumes, float* audio, float* peaks, int16_t* pcm, int32_t* kernel);
/* Test hook: fills the whole capacity of the handle's two workspace arenas with a 32-bit pattern (on the engine stream, then
 * synchronises).  A later run on the same handle that does not outgrow the workspace finds the pattern in every column it does
 * not write: the columns past a row's end must reach no valid sample (consumers mask by select, never by multiply). */
int mi355vits_test_fill_workspace(mi355vits_handle h, uint32_t pattern);
/* Kernel unit-test hook: relative-position attention on host buffers.  qkv [B, 3H, T], emb_rel_k / emb_rel_v
 * [2W+1, H/n_heads], len [B] (0 <= len <= T), out [B, H, T].  impl: 0 = VALU kernel (T <= rel_attention_valu_cap), 1 = the
 * f32-MFMA kernel (T <= 512, even head width, W <= 15), 2 = the streamed kernel (any T; even head width <= 128, W <= 15).  A shape
 * the chosen kernel does not serve is MI355VITS_ERR_INVALID before any launch.  Every element of out is written.  Query rows at or
 * past len[b]: impl 0 and 1 write what the reference's -1e4 fill gives there — every logit equal, so the plain mean of v over all T
 * columns of the batch, padding included (plus the band's E_v rows over T): finite for finite input, dependent on T and on what lies
 * past len[b], never read by a valid frame; impl 2 writes exact zeros.  Columns below len[b] depend on neither T nor the padding. */
int mi355vits_test_rel_attention(int device, int impl, int B, int T, int H, int n_heads, int W, const float* qkv,
                                 const float* emb_rel_k, const float* emb_rel_v, const int32_t* len, float* out);
/* Kernel unit-test hook: ONE WaveNet layer of the coupling flow (csrc/kernels_wn.cpp) on host buffers:
 *   u = tanh(in(h)[:H] + cond[:H]) * sigmoid(in(h)[H:] + cond[H:]),  rs = res_skip(u),
 *   Crs = 2H: h' = (h + rs[:H]) * mask, skip (+)= rs[H:];   Crs = H (a stack's last layer): skip (+)= rs, h' is not written.
 * in = a "same" conv with K taps (odd) at `dilation`, res_skip a 1x1 conv; skip_init != 0: skip = instead of skip +=.  The hook packs
 * the weights with the library's own pack functions, as the engine does for the chosen path.
 * impl: 0 = the two launches the engine falls back to (gate conv, then res/skip conv in place: the f32-MFMA conv kernel, the
 *           generic one for odd H, decided per conv as the engine does), math MI355VITS_MATH_F32;
 *       1 = launch_wn_layer (k_wn_layer<1> at H = 32; k_wn_layer<6>, k_wn_layer_h192<4 | 12> at H = 192, chosen by the grid),
 *           math MI355VITS_MATH_F32;
 *       2 = launch_wn_layer_b3 (k_wn_layer_b3: H = 192, (K - 1) * dilation <= 24; 32-, 96- or 128-column tiles chosen by the grid,
 *           the 128-column form only for (K - 1) * dilation <= 8), math MI355VITS_MATH_BF16X3.
 * A shape or math mode the chosen path does not serve is MI355VITS_ERR_INVALID before any launch.  Which form of an impl runs is
 * the launcher's business (its grid rule; in the lab build and the CPU model also MI355VITS_WN_B3_NT, MI355VITS_WN_EPI,
 * MI355VITS_WN_SIX_WAVES, read at every launch); all forms of one impl give the same bits.  (MI355VITS_WN_SHAPE=32, lab build and CPU
 * model, is no form in that sense: it runs impl 2 on v_mfma_f32_32x32x16_bf16 with the packing of that form — other sums, other bits.)
 * At and past len[b] (0 <= len[b] <= T), per row:
 *   h_in    impl 1 and 2 never use it there: every staged column is masked at len[b] (impl 2 does load h_in there for the residual of
 *           the last tile it computes, and discards it by select: any finite or non-finite bits may lie there).  impl 0 READS it, as the
 *           engine's two-launch path does (its h is zero there because every layer masks h'): the caller keeps it zero.
 *   h_out   (Crs = 2H) impl 0 and 1 write zeros at every column len[b] <= t < T.  impl 2 never computes a tile that starts at or
 *           past len[b]: zeros from len[b] to the end of the tile that holds column len[b] - 1 (tile = mi355vits_lab_wn_plan's
 *           width), every later column keeps what h_out held; a row with len[b] = 0 is not touched at all.  Crs = H: no path writes
 *           h_out; for impl 1 and 2 the hook still reads the device's buffer back, so a stray write shows (impl 0 works in place on
 *           its copy of h_in and returns the caller's h_out as it came).
 *   skip    is NOT masked (its consumer masks): impl 0 and 1 apply the update at every column t < T, with u computed from a zero input
 *           there; impl 2 does so inside the last computed tile, and every later column keeps what skip held.
 * Columns below len[b] depend on nothing at or past len[b] and on no other row. */
typedef struct mi355vits_wn_test {
    int32_t impl, B, H, T, K, dilation, Crs, skip_init, math;
    const float* h_in;   /* [B,H,T] */
    const float* w_in;   /* [2H,H,K]: tanh rows, then sigmoid rows */
    const float* b_in;   /* [2H] */
    const float* w_rs;   /* [Crs,H,1] */
    const float* b_rs;   /* [Crs] */
    const float* cond;   /* [B,2H] or NULL */
    const int32_t* len;  /* [B] */
    float* h_out;        /* [B,H,T]: its prior contents go to the device first */
    float* skip;         /* [B,H,T], in / out */
} mi355vits_wn_test;
int mi355vits_test_wn_layer(int device, const mi355vits_wn_test* t);
/* What the launchers would pick for a [B, 192, T] layer with (K, dilation) on the current device: *b3_tile = the columns of a
 * k_wn_layer_b3 workgroup (32, 96 or 128), *f32_geometry = launch_wn_layer's wave geometry (0: 4 waves x 3 tiles, 1: 6 x 2, 2: 12 x 1).
 * The launchers' own functions (with the lab switches where they are read).  No kernel runs. */
int mi355vits_lab_wn_plan(int B, int T, int K, int dilation, int32_t* b3_tile, int32_t* f32_geometry);
/* The weight fragments k_wn_layer_b3 reads in the split-bf16 modes (csrc/kernels.h, pack_conv_weights_w16): w [Cout, Cin, K] ->
 * out [Cout / 16][K][Cin / 32][3 planes][64 lanes][4] 32-bit words, two bf16 each (the even k-slot in the low half).  gate != 0: Cout = 2 H,
 * tanh rows then sigmoid rows, paired per 16 channels.  Cin % 32 == 0, Cout % 32 == 0 (gate: Cout % 64 == 0).  Host only: no device is touched.
 * MI355VITS_WN_SHAPE=32 (lab build and CPU model) makes the WaveNet hooks and the engine use the earlier 32x32x16 form and packing instead. */
int mi355vits_lab_pack_w16(const float* w, int Cout, int Cin, int K, int gate, uint32_t* out);
/* Kernel unit-test hook: ONE multi-receptive-field stage of the decoder (csrc/kernels_mrf.cpp, kernels_mrfp.cpp,
 * kernels_mrfs.cpp) on host buffers:  y = s * sum_j RB_j(x), s = out_scale when out_scale > 0, else 1 / nrb;
 *   RB_j: x1 = x + conv_{k_j, d1_j}(lrelu_0.1(x)) + b;  x2 = x1 + conv_{k_j, d2_j}(lrelu_0.1(x1)) + b   ("same" convs),
 * every row evaluated alone on its own [:, :len[b]] with zero padding (x1 counts as zero at and past len[b] too).  The hook packs
 * w[j][q] [C, C, k_j] with the library's own pack functions, as the engine does for the chosen kernel, and passes len_host.
 * impl: 0 = launch_mrf_fused (k_mrf_fused: C in {32, 64, 128}, nrb 1 .. 4, what fits LDS), math MI355VITS_MATH_F32 or _BF16X3;
 *       1 = launch_mrf_p (k_mrf_p<32 | 64>: C in {32, 64}, taps (3, 5, 7); on the device dilations (1,2), (2,6), (3,12) only),
 *           math MI355VITS_MATH_BF16X3, out_scale as above;
 *       2 = launch_mrf_s (k_mrf_s<64>: as impl 1 with C = 64) with segments of `seg` columns: any positive multiple of the step
 *           (mi355vits_lab_mrf_plan's width) is served — a segment is an independent work item with its own pipeline fill, so
 *           segments shorter than mrf_s_segment would ever return are right, only slow; anything else is refused.
 * A shape, math mode or seg the chosen kernel does not serve is MI355VITS_ERR_INVALID before any launch.  impl 1 and 2 give the same bits.
 * At and past len[b] (0 <= len[b] <= T), per row:
 *   x       no kernel uses it there: every load is clamped to column len[b] - 1 and masked by select.
 *   y       impl 0 writes every column t < T (past len[b]: what the rule gives for a zero input, finite).  impl 1 never computes a
 *           work item that starts at or past len[b]: it writes up to the end of the item that holds column len[b] - 1 (finite values),
 *           every later column keeps what y held.  impl 2 likewise with the step inside a segment: within the segment that holds
 *           column len[b] - 1 it writes up to the end of that column's step (and never past the segment), later columns keep
 *           what y held.  A row with len[b] = 0 is not touched by impl 1 and 2.
 * Columns below len[b] depend on nothing at or past len[b] and on no other row. */
typedef struct mi355vits_mrf_test {
    int32_t impl, B, C, T, nrb, math, seg;
    int32_t k[4], d1[4], d2[4];
    const float* x;           /* [B,C,T] */
    const float* w[4][2];     /* [C,C,k[j]] */
    const float* bias[4][2];  /* [C] */
    const int32_t* len;       /* [B] */
    float out_scale;
    float* y;                 /* [B,C,T]: its prior contents go to the device first */
} mi355vits_mrf_test;
int mi355vits_test_mrf_stage(int device, const mi355vits_mrf_test* t);
/* How kernel `impl` (as above) cuts a row of a C-channel stage: *width = the columns of a work item (T_B of k_mrf_fused / k_mrf_p, the
 * step of k_mrf_s), *halo = max_j (k_j - 1) / 2 * (d1_j + d2_j), the columns an output looks to either side, *x_ring / *x1_ring = the
 * sweep's LDS ring lengths in columns (0 for impl 0 and 1).  MI355VITS_ERR_INVALID where the kernel does not serve the stage.
 * Host arithmetic only: no kernel runs. */
int mi355vits_lab_mrf_plan(int impl, int C, int nrb, const int32_t* k, const int32_t* d1, const int32_t* d2, int32_t* width,
                           int32_t* halo, int32_t* x_ring, int32_t* x1_ring);
/* Kernel unit-test hook: ONE DDS stack of the stochastic duration predictor (csrc/kernels_misc.cpp) with what
 * surrounds it, on host buffers:
 *   pre     pre_mode 0: x = conv1x1(src) + pre_b (+ cond[b])      (StochasticDurationPredictor.pre + cond; pre_w [C, C, 1])
 *           pre_mode 1: x = pre_w[c] * z[b, zch, t] + pre_b[c] + src[b, c, t]   (ConvFlow.pre on one channel + g; pre_w [C])
 *   layers  x += gelu(LN2(conv1x1(gelu(LN1(dwconv_{K, K^i}(x * mask))))))   i = 0 .. n_layers - 1, LayerNorm over channels, eps 1e-5,
 *           erf GELU; dw_w[i] [C, 1, K], w1x1[i] [C, C, 1]
 *   proj    out = (conv1x1(x * mask) + proj_b) * mask     (proj_w [proj_cout, C, 1], or NULL: no proj, x_out only)
 *   spline  (spline != 0; needs proj, z and proj_cout = 3 nb - 1, nb <= 16)  z[b, 1 - zch] <- RQS^-1(z[b, 1 - zch]; theta = out)
 *           inside [-tail, tail], then z *= mask, as mi355vits_test_spline_inverse.
 * The hook packs the 1x1 weights with the library's own pack functions, as the engine does for the chosen path.
 * impl: 0 = one launch per piece (launch_convflow_pre or the pre conv; per layer launch_dds_dwconv_ln_gelu, the 1x1 conv, launch_layernorm
 *           with add_to / gelu; the proj conv with in_len / out_len; launch_spline_inverse).  The convs run the f32-MFMA kernel, the
 *           generic one where it does not take the shape (odd C), decided per conv as the engine does.  Any C >= 1, any odd K.
 *       1 = the same pieces with launch_dds_layer per layer (k_dds_layer): C in {32, 64, 128, 192, 256}.
 *       2 = launch_dds_stack in MATH_F32 (k_dds_stack<6>): C = 192, K = 3, n_layers <= 3 (the taps' reach <= 16 columns).
 *       3 = launch_dds_stack in MATH_BF16X3 (k_dds_stack_b3<false>) or MATH_BF16W (k_dds_stack_b3<true>: the 1x1 / pre / proj weights
 *           count with their leading bf16 term only).  The engine never launches the MATH_BF16W form — its tmath() maps BF16W to
 *           BF16X3, durations must not move with the math mode — so this hook is the only way to reach k_dds_stack_b3<true>.
 *     math: MATH_F32 for impl 0, 1, 2; MATH_BF16X3 or MATH_BF16W for impl 3.  impl 1 and 2 give the same bits below len[b], on the CPU
 *           model and on the device (both form a LayerNorm's variance through dds_sq_sum).
 * A shape or math mode the chosen path does not serve is MI355VITS_ERR_INVALID before any launch.
 * At and past len[b] (0 <= len[b] <= T), per row; the prior contents of out, x_out and z go to the device first:
 *   src, z  are READ there by every impl (clamped, unconditional loads), and every use is masked by select at len[b]: any finite or
 *           non-finite bits may lie there.  Nothing below len[b] depends on them, on T or on another row.
 *   x_out   is written at every column t < T.  Past len[b] it holds the same column arithmetic with every tap at or past len[b]
 *           counted as zero — finite for finite src / z, a function of src and z THERE, never masked (the proj masks its input).
 *   out     is written at every column t < T: exact zeros at len[b] <= t < T.
 *   z       spline != 0: z[b, 1 - zch] is rewritten below len[b]; BOTH channels are exact zeros at len[b] <= t < T; z[b, zch] keeps
 *           its contents below len[b].  spline == 0: no path writes z (the hook still reads the device's buffer back). */
typedef struct mi355vits_dds_stack_test {
    int32_t impl, math, B, C, T, K, n_layers, pre_mode, zch, proj_cout, spline, nb;
    float tail, inv_sqrt_fc;
    const float* src;         /* [B,C,T] */
    const float* pre_w;       /* pre_mode 0: [C,C,1]; pre_mode 1: [C] */
    const float* pre_b;       /* [C] */
    const float* cond;        /* [B,C] or NULL; pre_mode 0 only */
    const float* dw_w[4];     /* [C,1,K] */
    const float* dw_b[4];     /* [C] */
    const float* g1[4];       /* LN1 gamma, beta [C] */
    const float* b1[4];
    const float* w1x1[4];     /* [C,C,1] */
    const float* bias1x1[4];  /* [C] */
    const float* g2[4];       /* LN2 gamma, beta [C] */
    const float* b2[4];
    const float* proj_w;      /* [proj_cout,C,1] or NULL */
    const float* proj_b;      /* [proj_cout] */
    const int32_t* len;       /* [B] */
    float* z;                 /* [B,2,T] in / out; NULL allowed with pre_mode 0 and no spline */
    float* out;               /* [B,proj_cout,T]; NULL allowed without proj */
    float* x_out;             /* [B,C,T] */
} mi355vits_dds_stack_test;
int mi355vits_test_dds_stack(int device, const mi355vits_dds_stack_test* t);
/* Kernel unit-test hook: launch_spline_inverse (k_spline_inverse) alone: the rational-quadratic spline inverse with linear tails (HF
 * modeling_vits.py: min width / height / derivative 1e-3, end derivatives from the constant) of x1 = z[b, 1 - ch_x0, t] with the
 * parameters theta[b, :, t] ([B, 3 nb - 1, T]: nb widths and nb heights, both scaled by inv_sqrt_fc, nb - 1 interior derivatives),
 * 2 <= nb <= 16 (anything else: MI355VITS_ERR_INVALID).  |x1| > tail, NaN: passed through.  z [B, 2, T] in / out.
 * At and past len[b] (0 <= len[b] <= T): theta and z are read (any bits may lie there), both channels of z are written as exact
 * zeros at len[b] <= t < T.  Below len[b], z[b, ch_x0] keeps its contents. */
int mi355vits_test_spline_inverse(int device, int B, int T, int nb, int ch_x0, float tail, float inv_sqrt_fc, const float* theta,
                                  const int32_t* len, float* z);
/* Kernel unit-test hook: launch_durations (k_durations) alone.  z [B, 2, T], ch the channel read, ea_m / ea_logs the
 * ElementwiseAffine's parameters, len [B], forced [B, T] or NULL, scales [B, 3] = noise_scale, length_scale, noise_w (length_scale
 * is the one read) -> logw [B, T] = (z - ea_m) * exp(-ea_logs) * mask, w_ceil [B, T] = ceil(exp(logw) * mask * length_scale) (forced:
 * forced[b, t] below len[b]); a w that is not below the frame cap 2^22 (+inf and NaN included), a forced count that is negative or above
 * the cap: cap + 1.  cum [B, T] = the inclusive scan of w_ceil, saturating at 2 cap; ylen [B] = max(1, cum[b, T - 1]).
 * At and past len[b] (0 <= len[b] <= T): every output is written at every t < T: logw and w_ceil are zero there, cum stays at its
 * value.  z IS READ there and masked by a multiply: the caller keeps it finite (the engine's z is zero there: the spline writes it);
 * forced is not read there. */
int mi355vits_test_durations(int device, int B, int T, int ch, float ea_m, float ea_logs, const float* z, const int32_t* len,
                             const int32_t* forced, const float* scales, float* logw, int32_t* w_ceil, int32_t* cum, int32_t* ylen);
/* Kernel unit-test hook: the fit stage of launch_durations_timed (k_durations_timed; include/mi355vits.h, timing control) alone on
 * a given u [B, T] (what the kernel otherwise makes from logw, length_scale and stretch).  len [B], min_frames [B, T] or NULL (= 0),
 * target [B] or NULL (= none; 0 = none for that row, else 1 .. cap) -> frames [B, T], cum [B, T] (inclusive scan, saturating at
 * 2 cap), ylen [B] = max(1, sum), factor [B] = s* (1.0f without a target), status [B]: 0 ok; 1 the target is below the floor
 * F(2^-30): frames = f(2^-30), factor = 2^-30; 2 the target is above F(2^30): frames = f(2^30), factor = 2^30.
 * Every output is written at every t < T (frames 0 and cum flat at and past len[b]); the caller's contents of the outputs are
 * uploaded first, so a missing write shows.  u and min_frames are not read at and past len[b]. */
int mi355vits_test_fit_durations(int device, int B, int T, const float* u, const int32_t* len, const int32_t* min_frames,
                                 const int32_t* target, int32_t* frames, int32_t* cum, int32_t* ylen, float* factor, int32_t* status);
/* Kernel unit-test hook: launch_expand_prior (k_expand_prior; the length regulator + the prior's sample) with injected noise.
 * stats [B, 2 I, Tx] = m_p | logs_p, cum [B, Tx] (non-decreasing, >= 0), ylen [B] (0 <= ylen[b] <= Ty), scales [B, 3] (noise_scale is
 * the one read), injected [B, I, injected_frames] with injected_frames >= Ty, or NULL where every row's noise_scale is 0 (anything
 * else would run the Philox generator: that is mi355vits_test_expand_prior_keyed below, whose draws tests/small_ref.py restates from
 * the published Philox4x32-10; here it is MI355VITS_ERR_INVALID).
 * z [B, I, Ty]: frame t of row b takes phoneme j = #{j : cum[b, j] <= t}: z = m_p[j] + injected * exp(logs_p[j]) * noise_scale (m_p[j]
 * alone, bit for bit, at noise_scale = 0).  Every element of z is written: exact zeros at t >= ylen[b] and where j = Tx; injected is
 * not read there, nor in a row whose noise_scale is 0. */
int mi355vits_test_expand_prior(int device, int B, int I, int Tx, int Ty, const float* stats, const int32_t* cum, const int32_t* ylen,
                                const float* injected, int injected_frames, const float* scales, float* z);
/* Kernel unit-test hook: launch_expand_prior (k_expand_prior) with the kernel's OWN noise (injected = NULL): as the hook above, with
 * n = the Philox draw of csrc/kernels_misc.cpp (philox_normal) under key `seed`, utterance utt[b], tensor id 1, channel c, frame t:
 *   Philox4x32-10 of counter (t, c, low32(utt), 1 ^ high32(utt) * 0x9E3779B9 mod 2^32) under key (low32(seed), high32(seed)) -> r;
 *   u_i = ((float)(r_i >> 8) + 0.5f) * 2^-24 in float32 (from 2^23 on the sum rounds; the last value gives u = 1);
 *   n = sqrtf(-2 logf(u_0)) * cosf(6.2831855f * u_1).
 * scales [B, 3] (noise_scale is the one read), utt [B].  Every element of z [B, I, Ty] is written (its prior contents go to the device
 * first): exact zeros at t >= ylen[b] and where no phoneme holds the frame; m_p[j] alone, bit for bit, in a row whose noise_scale is 0
 * (no draw is made there). */
int mi355vits_test_expand_prior_keyed(int device, int B, int I, int Tx, int Ty, const float* stats, const int32_t* cum, const int32_t* ylen,
                                      const float* scales, uint64_t seed, const uint64_t* utt, float* z);
/* Kernel unit-test hook: launch_sdp_noise (k_sdp_noise) alone with the kernel's own noise (injected = NULL): z [B, 2, T],
 * z[b, c, t] = n * noise_w[b] with n the draw above under tensor id 0, channel c, time t; scales [B, 3] (noise_w = scales[b, 2] is the one
 * read), utt [B].  The kernel knows no length: every element of z is written (its prior contents go to the device first), a row whose
 * noise_w is 0 as exact +0 (no draw is made there). */
int mi355vits_test_sdp_noise(int device, int B, int T, uint64_t seed, const uint64_t* utt, const float* scales, float* z);
/* Kernel unit-test hook: launch_embed (k_embed) alone, ONE launch: ids [B, T] int64, len [B] (0 <= len[b] <= T), emb [num_symbols, H]
 * -> y [B, H, T] = emb[ids[b, t]][c] * scale (one float32 product) at t < len[b].  The caller's y goes to the device first; every element
 * of it is written.  At len[b] <= t < T: exact zeros; ids ARE read there (an id outside 0 .. num_symbols - 1 reads row 0 — anywhere: the
 * product's callers validate below the lengths, the kernel clamps as a second line) and the value is discarded by select. */
int mi355vits_test_embed(int device, int B, int T, int H, int num_symbols, const int64_t* ids, const int32_t* len, const float* emb,
                         float scale, float* y);
/* Kernel unit-test hook: launch_layernorm (k_layernorm<cached> for C <= 256, k_layernorm<uncached> above) alone, ONE launch, the fields
 * of LNArgs (csrc/kernels.h):
 *   v = x  (nparts > 1: x[0] + x[1] + ... in slice order, slice p at x + p * part_stride floats, part_stride >= B C T);  v += bias[c];
 *   v = 0 at t >= premask_len[b];  v += res;  y = (v - mean_c v) / sqrt(var_c v + eps) * gamma[c] + beta[c]  (two passes: the mean,
 *   then the biased variance of the centred values);  gelu: y = erf-GELU(y);  y += add_to;  y = 0 at t >= out_len[b].
 * alias: 0 = y is a buffer of its own (the caller's y goes to the device first); 1, 2, 3 = the kernel runs with y == x (slice 0),
 * y == res, y == add_to on the device — the engine's three in-place uses — and the result is returned in y, whose prior contents are not
 * used.  nparts > 1, bias or premask_len at C > 256 is the launcher's refusal: MI355VITS_ERR_INVALID before any launch.
 * At and past the lengths (0 <= len <= T; NULL = T), per row: y is written at every t < T.  x (every slice), res and add_to are READ at
 * every t < T; at t >= premask_len[b] x's slices and bias are discarded by select (any bits), at t >= out_len[b] the whole column is
 * (x, res and add_to may hold any bits there: exact zeros come out).  A column's result depends on that column alone: on no other
 * column, no other row, and not on T. */
typedef struct mi355vits_layernorm_test {
    int32_t B, C, T, nparts, gelu, alias;
    float eps;
    int64_t part_stride;         /* floats between the slices of x (nparts > 1) */
    const float* x;              /* [B,C,T], or nparts slices of it */
    const float* bias;           /* [C] or NULL */
    const int32_t* premask_len;  /* [B] or NULL */
    const float* res;            /* [B,C,T] or NULL */
    const float* add_to;         /* [B,C,T] or NULL */
    const float* gamma;          /* [C] */
    const float* beta;           /* [C] */
    const int32_t* out_len;      /* [B] or NULL */
    float* y;                    /* [B,C,T] */
} mi355vits_layernorm_test;
int mi355vits_test_layernorm(int device, const mi355vits_layernorm_test* t);
/* Kernel unit-test hook: launch_dp_det (k_dp_det<F32> in MI355VITS_MATH_F32, k_dp_det<split-bf16> in MATH_BF16X3) alone, ONE launch: the
 * deterministic duration predictor (csrc/kernels_dp.cpp),
 *   h1 = LN_1(relu(conv_1((x + cond[b]) * m)));  h2 = LN_2(relu(conv_2(h1 * m)));  logw = (proj_w . h2 + proj_b) * m,   m = [t < len[b]],
 * "same" convs with K taps, LayerNorm over the F channels with eps 1e-5.  The hook packs w1 [F,H,K] and w2 [F,F,K] with the library's
 * own pack functions, as Engine::duration_predictor_det does for the mode.  H, F multiples of 32 up to 256, K odd up to 7
 * (dp_det_supported); anything else, or another math mode: MI355VITS_ERR_INVALID before any launch.
 * At and past len[b] (0 <= len[b] <= T): x is not used there (MATH_F32 does not load it; the split-bf16 form clamps the load and
 * discards by select): any bits.  logw (the caller's contents go to the device first) is written at every t < T: exact zeros at
 * len[b] <= t < T.  Columns below len[b] depend on nothing at or past it, on no other row and not on where the tile seams fall. */
typedef struct mi355vits_dp_det_test {
    int32_t B, H, F, K, T, math;
    const float* x;        /* [B,H,T] */
    const float* cond;     /* [B,H] or NULL */
    const int32_t* len;    /* [B] */
    const float* w1; const float* b1; const float* g1; const float* be1;  /* conv_1 [F,H,K], its bias, norm_1's gamma / beta [F] */
    const float* w2; const float* b2; const float* g2; const float* be2;  /* conv_2 [F,F,K], ... */
    const float* proj_w;   /* [F] */
    const float* proj_b;   /* [1] */
    float* logw;           /* [B,T] */
} mi355vits_dp_det_test;
int mi355vits_test_dp_det(int device, const mi355vits_dp_det_test* t);
/* How k_dp_det cuts a row: *cols = the output columns of a work item (the 64-column window less *halo), *halo = 2 (K / 2), the columns
 * the two convs look to either side, *lds_bytes = dp_det_lds_bytes, the launch's dynamic LDS.  The library's own functions; host
 * arithmetic only: no kernel runs.  MI355VITS_ERR_INVALID where the hook would refuse the shape or the math mode. */
int mi355vits_lab_dp_det_plan(int H, int F, int K, int math, int32_t* cols, int32_t* halo, int32_t* lds_bytes);
/* Kernel unit-test hook: launch_speaker_cond (k_speaker_cond, the plain run's conditioning) alone on host buffers: emb_g
 * [n_speakers, gin], sid [B] (checked against the table), w [Cout, gin], bias [Cout] or NULL -> out [B, Cout].  out holds out_floats >=
 * B * Cout floats: all of them go to the device first and come back, so a missing or a stray write shows. */
int mi355vits_test_speaker_cond(int device, int B, int gin, int n_speakers, int Cout, const float* emb_g, const int64_t* sid,
                                const float* w, const float* bias, float* out, size_t out_floats);
/* Kernel unit-test hook: launch_speaker_cond_mix (k_speaker_cond_mix; include/mi355vits.h, blended and caller-supplied speakers)
 * alone, ONE launch: the table emb_g [n_speakers, gin] with mix_sid / mix_weight [B, n_terms] (n_terms 1 .. 8; a sid at a non-zero
 * weight is checked against the table, one at a zero weight may hold anything), or vectors [B, gin] with n_terms 0 and the other
 * three NULL; n_jobs consumers (1 .. 10): w[q] [Cout[q], gin], bias[q] [Cout[q]] or NULL -> out[q] [B, Cout[q]], and g [B, gin].
 * out[q] holds out_floats[q] >= B * Cout[q] floats and g holds g_floats >= B * gin: all of them go to the device first and come
 * back, so a missing or a stray write shows.  A row whose every weight is 0 is served with g = 0 (the product refuses it earlier). */
typedef struct mi355vits_speaker_mix_test {
    int32_t B, gin, n_speakers, n_terms, n_jobs;
    const float* emb_g;
    const int64_t* mix_sid;
    const float* mix_weight;
    const float* vectors;
    const float* w[10];
    const float* bias[10];
    int32_t Cout[10];
    float* out[10];
    size_t out_floats[10];
    float* g;
    size_t g_floats;
} mi355vits_speaker_mix_test;
int mi355vits_test_speaker_cond_mix(int device, const mi355vits_speaker_mix_test* t);
/* Kernel unit-test hook: launch_levels (k_levels; include/mi355vits.h, level control in one run) alone, ONE launch, on host buffers:
 * cum [B, T] (the inclusive scan of the frames; read below len[b] only, where it must not decrease), len [B] (0 .. T), gain [B, T]
 * (0 .. 1024 below len[b]; anything behind), ramp [B] (0 .. 4096) or NULL (= 0), hop >= 1, alen [B] = hop * max(1, c[len - 1])
 * (checked), audio [B] rows of audio_bs >= alen[b] floats, shaped in place.  audio holds audio_floats >= B * audio_bs floats: all of
 * them go to the device first and come back, so a stray write behind a row or behind the last row shows.  Row b starts audio_bs * b
 * floats behind a 256-byte aligned address: an odd audio_bs gives every alignment.  peaks [B]: max |y| of every row. */
int mi355vits_test_levels(int device, int B, int T, int hop, const int32_t* cum, const int32_t* len, const float* gain,
                          const int32_t* ramp, const int32_t* alen, int64_t audio_bs, float* audio, size_t audio_floats, float* peaks);
/* Kernel unit-test hooks of pitch control (include/mi355vits.h, mi355vits_run_pitch; kernels_pitch.cpp).
 * mi355vits_test_pitch_table: the filter table h the handles use, Z P + 2 = 1,538 floats (capacity: floats `out` can take).
 * mi355vits_test_pitch_plan: launch_pitch_plan (k_pitch_plan) alone, ONE launch: cum [B, T] (read below len[b] only, where it must
 * not decrease), len [B] (0 .. T), ratio [B, T] (0.5 .. 2 below len[b]) or NULL (= 1), hop >= 1 -> tq [B, T] (int64), wc [B, T],
 * wlen [B] (wc and wlen saturate at 2^31 - 1).
 * mi355vits_test_pitch: the plan, then launch_pitch (k_pitch), one launch each, on host buffers: x [B] rows of x_bs floats, of which
 * hop * max(1, c[len - 1]) are the row (must fit x_bs); y [B] rows of y_bs floats, y_ld <= y_bs of each written (the warped row, then
 * zeros), y_ld >= every wlen[b] (checked; a saturated row is refused).  x holds x_floats >= B * x_bs and y y_floats >= B * y_bs
 * floats: all of y goes to the device first and comes back, so a stray write behind a row's y_ld or behind the last row shows.  Row b
 * of x and of y starts x_bs * b / y_bs * b floats behind a 256-byte aligned address: odd strides give every alignment.
 * peaks [B]: max |y| of every row; wlen [B]: the warped lengths. */
int mi355vits_test_pitch_table(float* out, size_t capacity);
int mi355vits_test_pitch_plan(int device, int B, int T, int hop, const int32_t* cum, const int32_t* len, const float* ratio,
                              int64_t* tq, int32_t* wc, int32_t* wlen);
int mi355vits_test_pitch(int device, int B, int T, int hop, const int32_t* cum, const int32_t* len, const float* ratio,
                         const float* x, int64_t x_bs, size_t x_floats, float* y, int64_t y_bs, int32_t y_ld, size_t y_floats,
                         float* peaks, int32_t* wlen);
/* Kernel unit-test hook: the product's resampler launch (k_resample, mi355vits_set_output_rate) on host buffers.  x [B] rows of
 * row_stride floats, lengths [B] (0 <= lengths[b] <= row_stride) valid samples of each; what lies past a row's length is never
 * looked at.  y [B] rows of y_stride floats, y_stride >= max_b ceil(lengths[b] * L / M): every sample of it is written (zeros
 * past a row's output length); y_lengths [B], peaks [B] = max |y| over the valid samples.  MI355VITS_ERR_INVALID for a rate pair
 * the engine would refuse. */
int mi355vits_test_resample(int device, int B, int64_t row_stride, const float* x, const int32_t* lengths, int32_t in_hz,
                            int32_t out_hz, int64_t y_stride, float* y, int32_t* y_lengths, float* peaks);
/* Kernel unit-test hook: the product's alignment launch (k_align, mi355vits_fetch_alignment) alone on host buffers.  frames [B, T]
 * (read at t < len[b] only; 0 <= frames, a row's sum within the duration cap), len [B] (0 <= len[b] <= T) phonemes of a row,
 * audio [B] rows of row_stride floats with alen [B] (0 <= alen[b] <= row_stride) valid samples each: what lies past them is never
 * looked at (a span's levels stop at alen[b]).  hop samples per frame, L / M the rate ratio (1 <= L, M <= 640).  Writes
 * out_frames / out_start / out_samples [B, T] and, when both are given, out_peak / out_rms [B, T]; with both NULL the timing-only
 * form of the kernel runs and the audio is not read. */
int mi355vits_test_alignment(int device, int B, int T, const int32_t* frames, const int32_t* len, int64_t row_stride, const float* audio,
                             const int32_t* alen, int32_t hop, int32_t L, int32_t M, int32_t* out_frames, int32_t* out_start,
                             int32_t* out_samples, float* out_peak, float* out_rms);
/* Kernel unit-test hook: the edge kernel (k_edges, mi355vits_set_edge_trim) alone over host arrays on the current device.  audio [B]
 * rows of `stride` floats, lens [B] (0 <= lens[b] <= stride) valid samples, peaks [B], 0 < ratio <= 1.  Writes s_first[b] = the first
 * sample with fabsf(y) >= peaks[b] * ratio (lens[b] when there is none) and s_last[b] = the last (-1).  What lies behind a row is
 * never looked at. */
int mi355vits_lab_edges(const float* audio, long stride, const int32_t* lens, const float* peaks, int B, float ratio, int32_t* s_first,
                        int32_t* s_last);
/* Kernel unit-test hook: the loudness kernels (k_loud, k_loud_gate; mi355vits_set_loudness_target) alone over host arrays on the
 * current device.  audio [B] rows of `stride` floats, lens [B] (0 <= lens[b] <= stride) valid samples at `rate` Hz (>= 4000).  Writes
 * lufs / blocks / gated [B] as mi355vits_fetch_loudness defines them.  What lies behind a row is never looked at. */
int mi355vits_lab_loudness(const float* audio, long stride, const int32_t* lens, int B, int32_t rate, double* lufs, int32_t* blocks,
                           int32_t* gated);
/* Kernel unit-test hook: the limiter kernel (k_limit; mi355vits_set_loudness_limiter) alone over host arrays on the current device:
 * audio [B] rows of `stride` floats with lens [B] valid samples each, g [B] the rows' gains, c the linear ceiling, U the encoding's
 * unit (32767.0 or 1.0), 1 <= L <= 4096 the window -> scale_out [B][stride] (scale[k] of include/mi355vits.h's rule at a row's valid
 * samples, 0 behind them), sq_min [B] = min sq[k] and reduced [B] = the count of sq[k] < (L + 1) 2^30 ((L + 1) 2^30 and 0 for an
 * empty row).  Every row is a job, over the ceiling or not.  What lies behind a row is never looked at. */
int mi355vits_lab_limit(const float* audio, long stride, const int32_t* lens, int B, const double* g, double c, double U, int32_t L,
                        float* scale_out, int64_t* sq_min, int32_t* reduced);
/* The same with an envelope (the true-peak ceiling mode, k_limit<true>): env [B][stride] doubles, env[b][t] in place of
 * fabs((double) audio[b][t]) at a row's valid samples (finite, >= 0; what lies behind them is never looked at).  env = NULL: the
 * call above. */
int mi355vits_lab_limit_env(const float* audio, long stride, const int32_t* lens, int B, const double* g, double c, double U, int32_t L,
                            const double* env, float* scale_out, int64_t* sq_min, int32_t* reduced);
/* Kernel unit-test hook: the true-peak kernels (k_true_peak, k_true_peak_env; mi355vits_set_loudness_ceiling_mode) alone over host
 * arrays on the current device.  audio [B] rows of `stride` floats with lens [B] (0 <= lens[b] <= stride) valid samples -> tp [B] and
 * env_out [B][stride] (e[t] at a row's valid samples, 0 behind them; NULL: the measurement only) as include/mi355vits.h defines them.
 * On the device the rows start `offset_floats` (0 .. 3) floats behind a 16-byte boundary plus whatever their stride adds.  What lies
 * behind a row is never looked at. */
int mi355vits_lab_true_peak(const float* audio, long stride, const int32_t* lens, int B, int32_t offset_floats, double* tp, double* env_out);
/* The library's tap table h[0..80] (taps: room for 81 doubles, or NULL) and the samples of a k_true_peak work item.  No kernel runs. */
int mi355vits_lab_true_peak_plan(double* taps, int32_t* tile);
/* How k_loud cuts a row at `rate`: *step = S, the 100 ms step; *warmup = W(rate), the samples an item that starts inside a row runs
 * before it counts; *steps_per_item = K (a work item is K * S samples of one row).  Host arithmetic only: no kernel runs. */
int mi355vits_lab_loudness_plan(int32_t rate, int32_t* step, int32_t* warmup, int32_t* steps_per_item);
/* Kernel unit-test hook: the G.711 encoders of the encoded packed streams (mi355vits_set_output_encoding) over an array on the
 * current device.  law = MI355VITS_ENC_ULAW or MI355VITS_ENC_ALAW; out[i] = the code of in[i].  65,536 inputs cover the function. */
int mi355vits_lab_g711_encode(int law, const int16_t* in, long n, uint8_t* out);
/* Kernel unit-test hook: the FLAC kernels (k_flac_frames, k_flac_scan, k_flac_gather; mi355vits_set_output_compression) alone over an
 * arbitrary int16 stream on the current device: pcm [n] (n >= 0) at `rate` Hz (1 .. 1,048,575) -> out[0, *n_bytes) = the complete
 * file (42 header bytes, then the frames), frame_sizes [ceil(n / 4096)] (or NULL) = the bytes of every frame.  The frames carry the
 * numbers first_frame, first_frame + 1, ... (all below 2^21; STREAMINFO is that of a stream that starts here), so a test reaches the
 * multi-byte frame numbers with two frames.  On the device the samples start as many bytes behind a 16-byte boundary as pcm does on
 * the host (pcm & 15).  cap < the file's size: MI355VITS_ERR_INVALID, with *n_bytes = the size needed. */
int mi355vits_lab_flac(const int16_t* pcm, long n, int32_t rate, int32_t first_frame, uint8_t* out, size_t cap, size_t* n_bytes,
                       int32_t* frame_sizes);
/* Kernel unit-test hook: SEVERAL files in one block by the three kernels of the streams calls alone (k_flac_frames once over a job per
 * array, k_flac_place, k_flac_gather_streams; mi355vits_run_streams2): pcm[j] [n[j]] (n[j] >= 0; n_jobs >= 1) at `rate` Hz ->
 * out[0, *n_bytes) = the block, file j at out[offsets[j], + sizes[j]) with offsets[j] a multiple of 16 (offsets[0] = 0) and every
 * byte between the files zero.  Every job's frames are numbered from 0.  On the device array j starts as many bytes behind a 16-byte
 * boundary as pcm[j] does on the host, as in mi355vits_lab_flac.  cap < the block's size: MI355VITS_ERR_INVALID, *n_bytes = the size. */
int mi355vits_lab_flac_jobs(const int16_t* const* pcm, const long* n, int32_t n_jobs, int32_t rate, uint8_t* out, size_t cap,
                            size_t* n_bytes, int64_t* offsets, int64_t* sizes);
/* Kernel micro-benchmark hook (tools/convbench.py): times `reps` launches of one MFMA Conv1d on random device data.
 * epi: 0 = standard epilogue (bias + residual), 1 = WaveNet gate (Cout = 2*H), 2 = res/skip.  (The tile-shape overrides
 * MI355VITS_CONV_CFG / MI355VITS_CONV_CHUNK exist in the lab build of the library only, csrc/hipx.h lab_getenv.) */
int mi355vits_bench_conv1d(int device, int B, int Cin, int Cout, int T, int K, int dilation, int epi, int reps,
                           float* ms_per_launch);
/* MFMA fragment-layout self test: returns 0 when the 32x32x2 and 16x16x4 f32 MFMA lane maps
 * assumed by the kernels hold on this device; max abs error in *err. */
int mi355vits_test_mfma_layout(int device, float* err);
/* Box probe (bench.py: the numbers ride in the JSON line so that a slow lease can be told from a slow kernel; ~30 ms, 1 GiB of
 * scratch): out[0] = GB/s all CUs together reach streaming ONE 2.6 MB table out of the L2 with 16-byte buffer loads (the
 * weight-fragment pattern of the WaveNet / resident-input kernels), out[1] = ns per dependent vector load over 2 MB (L2 hits),
 * out[2] = GB/s (read + written) of a 256 MiB HBM copy, out[3] = compute units, out[4] = the table stream of out[0] again while
 * every workgroup also copies its slice of 256 MiB through the same L2 (8 bytes of table per byte of copy: what the cache sees of a
 * weight-streaming kernel), out[5] = GB/s streaming a 24 MB table (fits the memory-side cache, not an XCD's L2), out[6] / out[7] =
 * ns per dependent load over 32 MB (memory-side cache) / 1 GiB (HBM, mostly TLB misses). */
int mi355vits_probe_device(int device, double out[8]);
/* The same L2 stream over 2.6 MB windows of THIS handle's weight arena (the bytes the kernels actually stream): out[0..2] = min /
 * median / max GB/s over the windows with eight 16-byte loads in flight per lane, out[3..5] = with one (the latency a kernel sees
 * that fetches its fragments a step ahead), out[6] = windows measured, out[7] = low 36 bits of the arena's device address. */
int mi355vits_probe_weights(mi355vits_handle h, double out[8]);

#ifdef __cplusplus
}
#endif
#endif /* MI355VITS_LAB_H */
