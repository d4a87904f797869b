// kernels.h — launch wrappers of every HIP kernel on the path (definitions in kernels_*.cpp).
// Activations are channels-first fp32 [B, C, T] (the reference graph's layout);
// a tensor "view" is (pointer, batch stride, row stride) so channel halves need no copies.
#pragma once
#include "hipx.h"

#include <vector>

namespace m355 {

struct Profiler;  // engine.h

// ---------------------------------------------------------------- Conv1d
enum ConvEpilogue { EPI_STD = 0, EPI_GATE = 1, EPI_RESSKIP = 2 };

struct ConvArgs {
    const float* x = nullptr; long x_bs = 0; int x_ld = 0;   // input  [B,Cin,T]
    float* y = nullptr;       long y_bs = 0; int y_ld = 0;   // output [B,Cout,T] (GATE: [B,H,T]; RESSKIP: h, in place)
    const float* w = nullptr;      // generic kernel: [Cout,Cin,K]; MFMA kernel: packed fragments (pack_conv_weights_mfma)
    const float* wb3 = nullptr;    // the same weights as three bf16 planes (pack_conv_weights_bf16x3_mode, layout 1) or null
    int math = 0;                  // MATH_BF16X3 + wb3: split-operand path on the bf16 matrix cores (k_conv1d_b3)
    const float* bias = nullptr;   // [Cout] or null
    const float* cond = nullptr; long cond_bs = 0;  // per-(b,co) additive term (speaker conditioning) or null
    const float* res = nullptr; long res_bs = 0; int res_ld = 0;  // residual [B,Cout,T] or null
    float* y2 = nullptr; long y2_bs = 0; int y2_ld = 0;           // RESSKIP: skip accumulator [B,H,T]
    const int* in_len = nullptr;   // [B] valid length of the input (x * mask) or null
    const int* in_len_host = nullptr;  // kernels_rbc.cpp: the host's copy of in_len (launcher: counts the items with work; null: read back; items.h)
    int nvalid = 0;                // kernels_rbc.cpp: (row, column block) items with work, filled by the launcher (items.h)
    int rb_loop = 0;               // k_enc_b3: 64-row output blocks a workgroup walks over one staged slice (launcher: 3 on large grids)
    const int* out_len = nullptr;  // [B] valid length of the output (y * mask) or null
    int B = 1, Cin = 0, Cout = 0, T = 0, K = 1, dil = 1;
    int pad = -1;            // left zero padding; -1 = "same" ((K*dil - dil) / 2), filled in by Engine::conv
    int Tin = -1;            // input extent when it differs from the number of output positions T (-1: = T)
    float in_slope = 1.0f;   // leaky-relu slope applied to the input while staging (1 = identity)
    int relu = 0;            // relu on the output
    float out_scale = 1.0f;  // y = (...) * out_scale
    int accumulate = 0;      // y += instead of y =
    int res_sub = 0;         // v = res - v instead of res + v   (coupling: x1 = (x1 - mean) * mask)
    int mask_before_res = 0; // apply the output mask to the conv result before the residual add (FFN: x + conv(..)*mask)
    int skip_init = 0;       // RESSKIP: first WN layer writes skip instead of accumulating
    int H = 0;               // GATE / RESSKIP: hidden channels
    int epi = EPI_STD;
    // ConvTranspose1d run as a stride-1 conv over `stride` polyphase filters: output channel
    // co' = r * shuf_cout + co of position i lands at y[co][i * shuf_s + r - shuf_p]  (0 <= n < shuf_T)
    int shuf_s = 0, shuf_p = 0, shuf_cout = 0, shuf_T = 0;
    int vec = 0;   // set by the launcher: input rows are 16-byte aligned -> 16-byte staging loads
    int yvec = 0;  // set by the launcher: output rows are 16-byte aligned -> vector stores (polyphase epilogue)
    int ovec = 0;  // set by the launcher: row-major epilogue through LDS (16-byte loads / stores of y, res)
    int ablate = 0;  // timing experiments only (MI355VITS_CONV_ABLATE): 1 no MFMA loop, 2 no staging, 4 no epilogue
    int fixed_rule = 0;  // kernel choice from the layer shape alone, never from T (flow / decoder convs: T = frames depends on
                         // what a row is batched with, and a row's bits must not)
    // launch_enc_conv_b3 only: the input channels in `ksplit` slices of 192, slice s of row b -> raw sums in
    // part[((s * B + b) * Cout + co) * T + t] (no epilogue; launch_layernorm adds them up); ksplit = 1: y with the epilogue
    int ksplit = 1;
    float* part = nullptr;
    int item_order = 0;  // kernels_rbc.cpp (set by its launchers): 1 = the persistent workgroups walk their items XCD-major where the grid allows it (items.h)
};

// What a conv launcher runs for its arguments on the current device: the launchers' whole choice as a pure function (host arithmetic,
// with the lab switches where they are read — at every call).  Each launcher below launches what its plan function returns and keeps
// no rule of its own; mi355vits_lab_conv_plan (include/mi355vits_lab.h) reports the same values to the tests.
enum ConvKernelForm {
    CONVK_GENERIC = 0,        // k_conv1d_generic
    CONVK_F32_STAGED = 1,     // k_conv1d_mfma (LDS-staged input chunks)
    CONVK_F32_DIRECT = 2,     // k_conv_direct_mfma
    CONVK_F32_SPLITK = 3,     // k_conv_direct_splitk
    CONVK_B3_STAGED32 = 4,    // k_conv1d_b3, 32-channel chunks
    CONVK_B3_STAGED64 = 5,    // k_conv1d_b3, 64-channel chunks (K <= 2)
    CONVK_B3_PC = 6,          // k_conv1d_b3_pc (persistent producer / consumer form, 64-channel chunks)
    CONVK_ENC_B3 = 7,         // k_enc_b3
    CONVK_ENC_B3W8 = 8,       // k_enc_b3w, row blocks of eight 32-row tiles
    CONVK_ENC_B3W6 = 9,       // k_enc_b3w, row blocks of six
    CONVK_RB_CONV = 10,       // k_rb_conv (32-column items)
    CONVK_RB_CONV_PW = 11,    // k_rb_conv_pw (128-column items)
    CONVK_UPS_PL = 12,        // k_ups_pl
    CONVK_UPS64 = 13,         // k_ups64
    CONVK_CONVT_GENERIC = 14  // k_conv_transpose1d
};
struct ConvPlan {
    int kernel = CONVK_GENERIC;
    int MT = 0, NT = 0, WM = 0, WN = 0;  // tile shape of the staged / direct MFMA kernels (0: the kernel has one fixed shape)
    int cols = 0, rows = 0;              // a work item: columns (output positions of the conv) x output rows
    int chunk = 0;                       // input channels staged at a time (0: not staged by chunks)
    int ring = 0;                        // k_conv1d_mfma's weight ring: 32 = a 64-channel chunk's pairs unrolled, 0 = ring, -1 = plain loop
    int rb_loop = 0;                     // k_enc_b3 / k_enc_b3w: row blocks a workgroup walks over one staged slice
    int vec = 0, yvec = 0, ovec = 0;     // ConvArgs.vec / yvec / ovec as the launcher sets them
    unsigned gx = 0, gy = 0, gz = 0;     // the grid (persistent kernels: gx workgroups, 0 = nothing to do)
    size_t shmem = 0;                    // dynamic LDS bytes
    int nvalid = 0, item_order = 0;      // kernels_rbc.cpp: ConvArgs.nvalid / item_order as the launcher sets them (items.h)
};
ConvPlan conv1d_generic_plan(const ConvArgs& a);
ConvPlan conv1d_mfma_plan(const ConvArgs& a);    // throws std::runtime_error where launch_conv1d_mfma would
ConvPlan enc_conv_b3_plan(const ConvArgs& a);    // a.ksplit set; the launcher checks the shape
ConvPlan rb_conv_plan(const ConvArgs& a);        // kernel, cols, rows; gx from a.in_len_host (null: the lengths are read back)
ConvPlan ups_pl_plan(const ConvArgs& a);

// Short-sequence dense conv of the text encoder (q/k/v, o, FFN: T = phonemes) in MATH_BF16X3 / BF16W: 64 x 64 output tiles, a
// 192-channel slice of the input staged ONCE per workgroup as three bf16 planes (k_enc_b3, kernels_conv.cpp).  Cin % 192 == 0
// (or Cin = 96: the pointwise conv in front of a coupling layer's WaveNet), K in {1, 3}, dil 1, EPI_STD, wb3 = layout-1 planes.
bool enc_conv_b3_supported(int Cin, int Cout, int K, int dil);
int enc_conv_b3_slices(int Cin);  // workgroups along the input channels = ConvArgs.ksplit (Cin / 192; 1 for the 96-channel form)
void launch_enc_conv_b3(const ConvArgs& a, hipStream_t s);
// y = LN_c(res + conv1x1(x) + bias) in one launch (the attention block's o-proj + residual + LayerNorm; 192 -> 192 channels):
// `c` as for launch_enc_conv_b3 (x, wb3, bias, res, y, in_len, math; no output mask on the conv), then the LayerNorm's
// gamma / beta / eps and its output mask.  y may be the residual buffer.
bool enc_o_ln_supported(int Cin, int Cout, int K);
void launch_enc_o_ln(const ConvArgs& c, const float* gamma, const float* beta, const int* ln_out_len, float eps, hipStream_t s);
// Generic VALU/LDS-tiled Conv1d (any shape; reference implementation + fallback).
void launch_conv1d_generic(const ConvArgs& a, hipStream_t s);
// fp32-MFMA implicit-GEMM Conv1d (v_mfma_f32_32x32x2_f32).  Needs Cin even and packed weights.
void launch_conv1d_mfma(const ConvArgs& a, hipStream_t s);
bool conv1d_mfma_supported(int Cin, int Cout, int K, int dil);
// Host-side weight repack for the MFMA kernel: [Cout,Cin,K] -> [ceil(Cout/32)][K][Cin/2][64].
size_t mfma_packed_floats(int Cout, int Cin, int K);
void pack_conv_weights_mfma(const float* w, int Cout, int Cin, int K, float* out);
void regroup_packed_x4(const float* packed, size_t n_floats, float* out);  // fused MRF stage weights (Cin % 8 == 0)
// f32 weights split into three bf16 planes (w = h + m + l exactly, each rounded to nearest) in the A-fragment order of
// v_mfma_f32_32x32x16_bf16: [Cout/32][K][Cin/16][plane h,m,l][64 lanes][8 bf16]; lane l = (half l >> 5, row l & 31)
// holds the k-slots e < 4: channel 16G + half + 2e, e >= 4: 16G + 8 + half + 2(e - 4) — the channels a lane's two
// ds_read_b128 of a packed activation tile deliver.  Needs Cin % 16 == 0 and Cout % 32 == 0; sizes in 32-bit words.
// BF16W: BF16X3 with the weights' leading bf16 term only.  F16X2 (experimental: every BF16X3 kernel; every other kernel
// runs as in BF16X3): operands split into two fp16 terms (22 significant bits), three products per multiply-add.
enum MathMode { MATH_F32 = 0, MATH_BF16X3 = 1, MATH_BF16W = 2, MATH_F16X2 = 3 };
inline bool math_on_bf16(int m) { return m == MATH_BF16X3 || m == MATH_BF16W; }
// F16X2 scaling (exact powers of two): weights x 2^13 when packed (|w| < 7.99 required), activations x 2^4 when staged
// (saturating at |x| = 4094; both terms are normal halves for |x| >= 2^-7), accumulators therefore x 2^17
constexpr float F16X2_W_SCALE = 8192.0f, F16X2_X_SCALE = 16.0f, F16X2_ACC_SCALE = 131072.0f;
size_t f16x2_packed_words(int Cout, int Cin, int K);
// false (nothing written) when a weight is too large for the fixed scale
bool pack_conv_weights_f16x2(const float* w, int Cout, int Cin, int K, uint32_t* out, int layout = 0);  // layout as for bf16x3
size_t bf16x3_packed_words(int Cout, int Cin, int K);
void pack_conv_weights_bf16x3(const float* w, int Cout, int Cin, int K, uint32_t* out);
// general form: epi selects the tile -> output-channel map (EPI_GATE: tile pairs (c, H + c)), layout the k-slot ->
// channel map (0: packed activation tiles of the fused MRF stage, 1: staged planes of k_conv1d_b3)
size_t bf16x3_packed_words_mode(int Cout, int Cin, int K, int epi);
void pack_conv_weights_bf16x3_mode(const float* w, int Cout, int Cin, int K, int epi, int layout, uint32_t* out);
bool conv1d_b3_supported(int Cin, int Cout, int K, int dil, int T_hint);
// epi = EPI_GATE packs rows as (c, H + c) tile pairs (H = Cout / 2); otherwise identical to the above.
void pack_conv_weights_mfma_mode(const float* w, int Cout, int Cin, int K, int epi, float* out);

// ---------------------------------------------------------------- ConvTranspose1d (K = 2*stride polyphase or general)
struct ConvTArgs {
    const float* x = nullptr; long x_bs = 0; int x_ld = 0;  // [B,Cin,Tin]
    float* y = nullptr; long y_bs = 0; int y_ld = 0;        // [B,Cout,Tin*stride]
    const float* w = nullptr;     // [Cin,Cout,K]
    const float* bias = nullptr;  // [Cout]
    const int* in_len = nullptr;  // [B] valid input frames per row (rows of a batch end at their own length)
    int B = 1, Cin = 0, Cout = 0, Tin = 0, K = 0, stride = 0, pad = 0;
    float in_slope = 1.0f;
};
void launch_conv_transpose1d(const ConvTArgs& a, hipStream_t s);
ConvPlan conv_transpose1d_plan(const ConvTArgs& a);  // k_conv_transpose1d's tile (cols = output samples), grid and LDS
// Polyphase repack: ConvTranspose1d weight [Cin,Cout,K] (+bias [Cout]) -> Conv1d weight
// [stride*Cout, Cin, taps] (+bias [stride*Cout]) with taps = ceil(K/stride); see ConvArgs::shuf_*.
int convt_taps(int K, int stride);
void convt_to_polyphase(const float* w, const float* bias, int Cin, int Cout, int K, int stride, float* w_out,
                        float* bias_out);

// ---------------------------------------------------------------- fused multi-receptive-field stage (K11)
// y = (1/n) * sum_j ResBlock2_j(x),  ResBlock2(k,(d1,d2)): x1 = x + conv_{k,d1}(lrelu(x)); x2 = x1 + conv_{k,d2}(lrelu(x1)).
// One workgroup keeps the x tile (+halo) and the x1 tile in LDS, runs all 2n convolutions on the fp32 matrix
// cores and writes y once: HBM traffic = read x + write y (vs ~7 tensor passes per resblock conv-by-conv).
constexpr int MRF_MAX_RB = 4;
struct MrfArgs {
    const float* x = nullptr; long x_bs = 0; int x_ld = 0;
    float* y = nullptr; long y_bs = 0; int y_ld = 0;
    const float* w[MRF_MAX_RB][2] = {};     // math 0: MFMA-packed x4 [C/32][K][C/8][64][4]; math 1: pack_conv_weights_bf16x3
    int math = 0;                           // MATH_F32 / MATH_BF16X3 (which matrix-core path; the weights must match)
    const float* bias[MRF_MAX_RB][2] = {};
    int k[MRF_MAX_RB] = {}, d1[MRF_MAX_RB] = {}, d2[MRF_MAX_RB] = {};
    int nrb = 0;
    const int* len = nullptr;  // [B] rows end at their own length
    int B = 1, C = 0, T = 0;
    int R = 0, ldx = 0, ld1 = 0, vec = 0;  // filled by the launcher (R = staging halo, rounded up to 4)
    float out_scale = 0.0f;  // 0: y = mean of the nrb resblocks; > 0: y = out_scale * sum (a stage fused only in part:
                             // the remaining resblocks are accumulated onto y by the conv-by-conv path)
    int ablate = 0;  // profiling only (MI355VITS_MRF_ABLATE): 1 = skip MFMA loops, 2 = skip staging, 4 = skip output
    int seg = 0;     // launch_mrf_s: columns per work item (a multiple of the kernel's step), from mrf_s_segment
    unsigned* clk = nullptr;  // -DMRFP_CLOCKS lab builds only: shader-clock stamps (kernels_mrfp.cpp)
    const int* len_host = nullptr;  // the host's copy of `len` (the engine has it: the per-stage lengths are made on the host): lets the
                                    // launcher count the column blocks that have work; nullptr with len != nullptr: read back (tests)
    int nvalid = 0;  // k_mrf_p: work items with work = sum over the rows of ceil(len / T_B), filled by the launcher
    int prio = 0;    // k_mrf_s: wave-priority mode of the conv2 waves (0 none, 1-3 a fixed s_setprio, 4-6 dynamic: see the kernel)
};
bool mrf_fused_supported(int C, int nrb, const int* k, const int* d1, const int* d2);
void launch_mrf_fused(MrfArgs a, hipStream_t s);
// How the three stage kernels cut a row (host arithmetic; the unit-test hooks' plan call): width = the columns of a work item
// (T_B of k_mrf_fused / k_mrf_p, the step TS of k_mrf_s), halo = max_j (r1_j + r2_j), the columns a stage's output looks to either
// side; x_ring / x1_ring = the sweep's LDS ring lengths in columns (0 for the other two).  false (nothing written) where the
// kernel's _supported is false.
inline int mrf_stage_halo(int nrb, const int* k, const int* d1, const int* d2) {  // max_j (r1_j + r2_j): the one definition
    int R = 0;
    for (int j = 0; j < nrb; ++j) {
        const int r = (k[j] - 1) / 2 * d1[j] + (k[j] - 1) / 2 * d2[j];
        R = R > r ? R : r;
    }
    return R;
}
struct MrfPlan { int width = 0, halo = 0, x_ring = 0, x1_ring = 0; };
bool mrf_fused_plan(int C, int nrb, const int* k, const int* d1, const int* d2, MrfPlan* out);
bool mrf_p_plan(int C, int nrb, const int* k, const int* d1, const int* d2, MrfPlan* out);
bool mrf_s_plan(int C, int nrb, const int* k, const int* d1, const int* d2, MrfPlan* out);
// MATH_BF16X3 with every element split once (kernels_mrfp.cpp): bf16 planes in LDS, the running conv's weight fragments in
// registers, v_mfma_f32_16x16x32_bf16 tiles.  w[][] = pack_conv_weights_p16 fragments.  C = 32; taps in {3, 5, 7}.
size_t p16_packed_words(int Cout, int Cin, int K);
void pack_conv_weights_p16(const float* w, int Cout, int Cin, int K, uint32_t* out);
bool mrf_p_supported(int C, int nrb, const int* k, const int* d1, const int* d2);
void launch_mrf_p(MrfArgs a, hipStream_t s);
// The same stage, same bits, as a row sweep (kernels_mrfs.cpp): work item = (row, segment), one pass per resblock with the
// waves specialised by conv, every conv's fragments in registers for the whole segment, no halo recompute; y accumulates the
// resblocks in place.  mrf_s_segment: the segment length for a grid, 0 = the stage is too small for the sweep to pay.
bool mrf_s_supported(int C, int nrb, const int* k, const int* d1, const int* d2);
int mrf_s_segment(int C, int B, int T, int cus, const int* len_host = nullptr);
void launch_mrf_s(MrfArgs a, hipStream_t s);
// One dense conv of a 128-channel ResBlock2 (HiFi-GAN stage 0) in MATH_BF16X3 with all input channels resident in LDS (kernels_rbc.cpp):
// y (+)= (res + bias + conv(lrelu(x * mask))) * out_scale; a.w = pack_conv_weights_p16 fragments; K / dilation pairs of the "_low" voices.
bool rb_conv_supported(const ConvArgs& a);
void launch_rb_conv(ConvArgs a, hipStream_t s);
// The polyphase upsamplers 128 -> 64 (x 8) and 64 -> 32 (x 4) in the same form (k_ups_pl): a = the ConvArgs of the polyphase conv
// (shuf_*, Tin, T = Tin + 1), a.w = pack_conv_weights_p16n fragments of the [stride * Cout, Cin, 2] polyphase filter.
void pack_conv_weights_p16n(const float* w, int Cout, int Cin, int K, uint32_t* out);
bool ups_pl_supported(const ConvArgs& a);
void launch_ups_pl(ConvArgs a, hipStream_t s);
// ---- launch_util.cpp: what the launchers share (the items themselves, their order and the persistent grid: items.h)
// sum over the rows of ceil(min(len, T) / block): the (row, column block) items of a ragged batch that have work.  len_host = the
// host's copy of the device array len (nullptr: copied back, a synchronising call — unit-test hooks only); len == nullptr: every row T
// extra: positions a row has beyond its length (polyphase upsamplers: len input positions -> len + 1 output positions)
int valid_items(const int* len_host, const int* len_dev, int B, int T, int block, int extra = 0);
int current_device_cu_count();  // compute units of the current device (persistent grids): cached per device (CPU model: reread)
// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device attribute: set once per (kernel, current device)
void set_max_dynamic_lds(const void* fn, int bytes);

// ---------------------------------------------------------------- fused WaveNet layer of the coupling flow (K8)
// u = tanh(in(h)[:H] + cond) * sigmoid(in(h)[H:] + cond); rs = res_skip(u); h' = (h + rs[:H]) * mask; skip += rs[H:]
struct WnArgs {
    const float* h_in = nullptr; float* h_out = nullptr; long h_bs = 0; int h_ld = 0;  // [B,H,T], ping-pong
    float* skip = nullptr; long s_bs = 0; int s_ld = 0;                                 // [B,H,T]
    const float* w_in = nullptr;   // MFMA-packed, gate tile map [2*H/32][K][H/2][64]
    const float* b_in = nullptr;   // [2H]
    const float* w_rs = nullptr;   // MFMA-packed [Crs/32][1][H/2][64]
    const float* b_rs = nullptr;   // [Crs]
    const float* cond = nullptr; long cond_bs = 0;  // this layer's [B][2H] conditioning slice or null
    const int* len = nullptr;
    int B = 1, H = 0, T = 0, K = 1, dil = 1, Crs = 0, skip_init = 0;
    int ldx = 0, vec = 0;  // filled by the launcher
    int ablate = 0;        // timing experiments only (MI355VITS_WN_ABLATE): 1 no MFMA loops, 2 no staging, 4 no stores
    int math = 0;          // launch_wn_layer_b3: MATH_BF16X3 or MATH_BF16W
    int shape = 16;        // launch_wn_layer_b3, split-bf16 modes: wn_layer_b3_shape() — which packing w_in / w_rs are in
};
bool wn_layer_fused_supported(int H, int K, int dil);
void launch_wn_layer(WnArgs a, hipStream_t s);
// Split-operand form of the same layer (H = 192); 32, 96 or 128 time columns x all rows per workgroup.  The split-bf16 modes run on
// v_mfma_f32_16x16x32_bf16 (since the shape A/B, profiles/wn_shape_ab.txt) and take pack_conv_weights_w16 fragments (w_in: gate = true);
// MATH_F16X2 runs on 32x32x16 tiles and takes pack_conv_weights_f16x2 fragments (w_in: 32-row tiles of 16 tanh rows and their sigmoid rows).
bool wn_layer_b3_supported(int H, int K, int dil);
void launch_wn_layer_b3(WnArgs a, hipStream_t s);
// 16, or 32 with MI355VITS_WN_SHAPE=32 (lab build and CPU model only: the 32x32x16 form and the layout-1 packing described above, for
// the A/B).  Read at every call; the caller packs / picks the weights for it and passes it on as WnArgs::shape.
int wn_layer_b3_shape();
// Split-bf16 weight fragments of k_wn_layer_b3 on 16x16x32 tiles: [16-row tile][tap][32-channel group][plane][lane] x 16 B.  Row
// 4 q + i of plain tile n is output channel 32 (n >> 1) + 8 q + 4 (n & 1) + i; gate = true (Cout = 2 H: tanh rows, then sigmoid rows):
// tile 2 P is plain tile P of the tanh rows and tile 2 P + 1 the same rows of the sigmoid half.  Lane l holds row l & 15 and the k-slots
// of record 4 g + (l >> 4) of the staged planes: slot e <-> input channel 32 g + 16 (l >> 5) + 8 (e >> 2) + 4 ((l >> 4) & 1) + (e & 3).
// Cin % 32 == 0, Cout % 32 == 0 (gate: Cout % 64 == 0).
size_t w16_packed_words(int Cout, int Cin, int K);
void pack_conv_weights_w16(const float* w, int Cout, int Cin, int K, bool gate, uint32_t* out);

// ---------------------------------------------------------------- one function per packed weight format
// The packed form of a conv's weights w [Cout, Cin, K], sized and filled: what Engine::add_conv_data stages into the weight arena and
// what the hooks of lab_api.cpp hand a kernel.  Which conv gets which form is the caller's decision.
inline std::vector<float> conv_weights_mfma(const float* w, int Cout, int Cin, int K, int epi = EPI_STD) {  // f32 MFMA fragments
    std::vector<float> p(mfma_packed_floats(Cout, Cin, K), 0.0f);
    pack_conv_weights_mfma_mode(w, Cout, Cin, K, epi, p.data());
    return p;
}
inline std::vector<float> conv_weights_mfma_x4(const std::vector<float>& mfma) {  // a lane's fragments of four channel pairs side by side
    std::vector<float> p(mfma.size());
    regroup_packed_x4(mfma.data(), mfma.size(), p.data());
    return p;
}
inline std::vector<uint32_t> conv_weights_bf16x3(const float* w, int Cout, int Cin, int K) {  // three bf16 planes, packed activation tiles
    std::vector<uint32_t> p(bf16x3_packed_words(Cout, Cin, K));
    pack_conv_weights_bf16x3(w, Cout, Cin, K, p.data());
    return p;
}
inline std::vector<uint32_t> conv_weights_bf16x3_staged(const float* w, int Cout, int Cin, int K, int epi = EPI_STD) {  // ... staged planes
    std::vector<uint32_t> p(bf16x3_packed_words_mode(Cout, Cin, K, epi));
    pack_conv_weights_bf16x3_mode(w, Cout, Cin, K, epi, 1, p.data());
    return p;
}
inline std::vector<uint32_t> conv_weights_p16(const float* w, int Cout, int Cin, int K) {  // k_mrf_p / k_rb_conv
    std::vector<uint32_t> p(p16_packed_words(Cout, Cin, K));
    pack_conv_weights_p16(w, Cout, Cin, K, p.data());
    return p;
}
inline std::vector<uint32_t> conv_weights_p16n(const float* w, int Cout, int Cin, int K) {  // k_ups_pl: natural row order
    std::vector<uint32_t> p(p16_packed_words(Cout, Cin, K));
    pack_conv_weights_p16n(w, Cout, Cin, K, p.data());
    return p;
}
inline std::vector<uint32_t> conv_weights_w16(const float* w, int Cout, int Cin, int K, bool gate) {  // k_wn_layer_b3, 16x16x32 tiles
    std::vector<uint32_t> p(w16_packed_words(Cout, Cin, K));
    pack_conv_weights_w16(w, Cout, Cin, K, gate, p.data());
    return p;
}
// two fp16 planes (layout as for bf16x3); empty when a weight is too large for the fixed scale
inline std::vector<uint32_t> conv_weights_f16x2(const float* w, int Cout, int Cin, int K, int layout) {
    std::vector<uint32_t> p(f16x2_packed_words(Cout, Cin, K));
    if (!pack_conv_weights_f16x2(w, Cout, Cin, K, p.data(), layout)) p.clear();
    return p;
}
// The rows of a gate conv [2 H, Cin, K] in the tile order of the kernels that gate in registers: 32-row tile q = the tanh rows of
// channels 16 q .. 16 q + 15, then their sigmoid rows (a lane of the 32 x 32 accumulator tile then holds both halves of its eight
// channels; kernels_wn.cpp).  Cout % 32 == 0.
inline std::vector<float> conv_weights_gate_tiles(const float* w, int Cout, int Cin, int K) {
    const int H = Cout / 2;
    const size_t row = (size_t)Cin * K;
    std::vector<float> p((size_t)Cout * row);
    for (int q = 0; q < Cout / 32; ++q)
        for (int r = 0; r < 32; ++r) {
            const int src = (r < 16 ? 0 : H) + 16 * q + (r & 15);
            memcpy(p.data() + ((size_t)32 * q + r) * row, w + (size_t)src * row, row * sizeof(float));
        }
    return p;
}
// The 32-column tiles per workgroup (1, 3 or 4) launch_wn_layer_b3 takes for this layer on the current device, and the geometry
// (0: 4 waves x 3 tiles, 1: 6 x 2, 2: 12 x 1) launch_wn_layer takes at H = 192: the launchers' own rules (lab build and CPU model:
// with the switches they read), for the launchers and for the unit-test hooks' plan call.
int wn_layer_b3_column_tiles(const WnArgs& a);
int wn_layer_geometry(const WnArgs& a);

// ---------------------------------------------------------------- decoder tail
// y = tanh(conv_post(lrelu_0.01(x * mask))) (Cout = 1, no bias) + per-utterance max|y| over valid samples;
// mask = t < valid_len[b]: every row of a batch is synthesised as if it were alone (zero padding at its own end).
void launch_conv_post_tanh(const float* x, long x_bs, int x_ld, const float* w, int Cin, int K, int B, int L,
                           const int* valid_len, float* audio, long audio_bs, unsigned* peak_bits, hipStream_t s);
// which kernel the launcher above runs (with the lab switches, read at every call): 0 = k_conv_post_tanh_dpp, 1 = k_conv_post_tanh_vec,
// 2 = k_conv_post_tanh.  All three give the same bits.
int conv_post_kernel(const float* x, long x_bs, int x_ld, int Cin, int K, const float* audio, long audio_bs);
// audio_float_to_int16 per utterance (utils.py:237-244) from the peaks found above.
// volumes [B] (device; NULL = 1 for every row): a row's volume != 1 is followed by audioop.mul(pcm, 2, volume) (tts.py:542-543):
// sample * volume in double, clipped to [-32768, 32767], rounded toward minus infinity.
void launch_pcm16(const float* audio, long audio_bs, const unsigned* peak_bits, const int* valid_len, int B, int L,
                  int16_t* pcm, long pcm_bs, hipStream_t s, const double* volumes = nullptr);
// The same conversion into ONE contiguous stream (mi355vits_run_packed / _fetch_packed; k_pack in kernels_pack.cpp), in the sample
// encoding the caller ships (mi355vits_set_output_encoding).  Entry i = row seg[row][i]'s first seg[length][i] samples at
// out[seg[offset][i] ..), entries in ascending order of their offsets; every other sample of out[0, total) is written as the
// encoding's silence (break silences, tail).  One kernel for all encodings — a destination-major walk, one 16-byte store per lane:
//   PACK_ENC_S16            sample for sample k_pcm16's arithmetic, silence 0; a lane owns 8 samples
//   PACK_ENC_ULAW / _ALAW   byte k = the G.711 code of that int16 sample, silence the code of sample 0 (0xFF / 0xD5); a lane owns 16
//   PACK_ENC_F32            the rows' float samples themselves (no normalisation, no volume: peak_bits / volumes are not read),
//                           silence 0.0f; a lane owns 4
// out is 16-byte aligned and holds pack_capacity_bytes(enc, total) bytes (whole 16-byte stores); byte offsets are 64-bit.
enum PackEncoding { PACK_ENC_S16 = 0, PACK_ENC_ULAW = 1, PACK_ENC_ALAW = 2, PACK_ENC_F32 = 3 };
constexpr int pack_bytes_per_sample(int enc) { return enc == PACK_ENC_S16 ? 2 : enc == PACK_ENC_F32 ? 4 : 1; }
inline size_t pack_capacity_bytes(int enc, long total) { return ((size_t)total * pack_bytes_per_sample(enc) + 15) & ~size_t(15); }
// The segment table seg = [pack_seg_rows(trimmed, normalised)][n] int32 on the device — its shape is defined here and nowhere else:
//   PACK_SEG_OFFSET, _ROW, _LENGTH   always: the entry's first sample in the stream, its batch row, its valid samples
//   PACK_SEG_SKIP                    trimmed (packs with edge trimming on) only: the first SOURCE sample of the entry — entry i is
//                                    its row's samples [skip, skip + length)
//   pack_seg_scale_row(trimmed)      normalised (packs with a loudness target) only, behind the others: the bits of the entry's f32
//                                    scale — 32767 * gain, which replaces 32767 / max(0.01, peak) (PACK_ENC_F32: the gain itself,
//                                    one f32 multiply per sample)
enum { PACK_SEG_OFFSET = 0, PACK_SEG_ROW = 1, PACK_SEG_LENGTH = 2, PACK_SEG_SKIP = 3 };
constexpr int pack_seg_scale_row(bool trimmed) { return trimmed ? 4 : 3; }
//   pack_seg_curve_row(trimmed)      curved (normalised packs on some entry of which the limiter engaged: launch_pack with a curve)
//                                    only, behind the scale: the entry's offset into the curves — sample k of its ROW is scaled by
//                                    curve[offset + k] in place of the entry's scale — or -1 for an entry that keeps its scale
constexpr int pack_seg_rows(bool trimmed, bool normalised) { return pack_seg_scale_row(trimmed) + (normalised ? 1 : 0); }
constexpr int pack_seg_curve_row(bool trimmed) { return pack_seg_scale_row(trimmed) + 1; }
constexpr int pack_seg_rows(bool trimmed, bool normalised, bool curved) { return pack_seg_rows(trimmed, normalised) + (curved ? 1 : 0); }
// curve != nullptr (normalised only): k_limit's scales, the table has its curve row
void launch_pack(int enc, const float* audio, long audio_bs, const unsigned* peak_bits, const double* volumes, const int* seg, int n,
                 uint8_t* out, long total, hipStream_t s, bool trimmed, bool normalised, const float* curve = nullptr);
// SEVERAL streams in one block (mi355vits_run_streams / _fetch_streams; k_pack_streams in kernels_pack.cpp): each stream with its own
// order, silences, header, encoding, trim and scale, addressed in BYTES of the block.  The host lays the block out so that every
// stream's first data byte sits at a 16-byte-aligned block offset (a lane's 16-byte store then owns whole samples inside any data
// region) and its RIFF header, if any, ends right in front of it; the kernel writes every byte of [0, n_bytes) and the last store's
// overrun — audio, each stream's own silence code, the header bytes (made on the host, copied from the table), pad bytes and the
// gaps between streams (zero).  Two int32 tables, uploaded as one block tab = [entry table][stream table]; their shape is defined
// here and nowhere else:
//   entry table [PACK_ENT_ROWS][n_entries], the entries of all streams in ascending order of their block offsets:
//     PACK_ENT_OFFSET   block byte offset of the entry's first sample
//     PACK_ENT_ROW      its batch row
//     PACK_ENT_LENGTH   its valid samples
//     PACK_ENT_SKIP     its first source sample (0 untrimmed)
//     PACK_ENT_ENC      its stream's PackEncoding; + PACK_ENT_SCALED when a host-made scale applies (a stream with a loudness target)
//     PACK_ENT_SCALE    then the bits of that f32 scale (as pack_seg_scale_row's)
//     PACK_ENT_CURVE    curved blocks (launch_pack_streams with a curve) only, a seventh row: the offset into the curves of an entry
//                       flagged PACK_ENT_CURVED in its PACK_ENT_ENC word (as pack_seg_curve_row's); the table of any other block
//                       has six rows, as ever
//   stream table [n_streams][PACK_STREAM_WORDS], streams in ascending order:
//     PACK_STREAM_BEGIN block byte offset of the stream's first byte (its header, if it has one)
//     PACK_STREAM_DATA  of its first data byte (16-byte aligned)
//     PACK_STREAM_END   one past its last data byte (the RIFF pad byte and the gap behind it are zero)
//     PACK_STREAM_ENC   its PackEncoding (the silence code)
//     PACK_STREAM_HEADER .. + 15: the header's bytes as little-endian words (44 or 58 of the 64 are used)
// The block is limited to 2^31 - 1 bytes: the offsets fit a word.  out holds pack_streams_capacity(n_bytes) bytes.
enum { PACK_ENT_OFFSET = 0, PACK_ENT_ROW = 1, PACK_ENT_LENGTH = 2, PACK_ENT_SKIP = 3, PACK_ENT_ENC = 4, PACK_ENT_SCALE = 5, PACK_ENT_ROWS = 6 };
enum { PACK_ENT_SCALED = 4, PACK_ENT_CURVED = 8 };  // flags in the PACK_ENT_ENC word, above the encoding's two bits
enum { PACK_ENT_CURVE = 6 };
constexpr int pack_ent_rows(bool curved) { return curved ? PACK_ENT_ROWS + 1 : PACK_ENT_ROWS; }
enum { PACK_STREAM_BEGIN = 0, PACK_STREAM_DATA = 1, PACK_STREAM_END = 2, PACK_STREAM_ENC = 3, PACK_STREAM_HEADER = 4, PACK_STREAM_WORDS = 20 };
constexpr long PACK_STREAMS_ITEM_BYTES = 256L * 16;  // a work item: 256 lanes x one 16-byte store
inline size_t pack_streams_capacity(long n_bytes) { return ((size_t)n_bytes + 15) & ~size_t(15); }
inline size_t pack_streams_table_words(int n_entries, int n_streams, bool curved = false) {
    return (size_t)pack_ent_rows(curved) * n_entries + (size_t)PACK_STREAM_WORDS * n_streams;
}
void launch_pack_streams(const float* audio, long audio_bs, const unsigned* peak_bits, const double* volumes, const int* tab, int n_entries,
                         int n_streams, uint8_t* out, long n_bytes, hipStream_t s, const float* curve = nullptr);
// G.711 of n int16 samples on the device with the stream kernels' own encoders (law: PACK_ENC_ULAW / PACK_ENC_ALAW): the lab hook
void launch_g711_encode(int law, const int16_t* in, long n, uint8_t* out, hipStream_t s);

// ---------------------------------------------------------------- the S16LE stream as FLAC frames (kernels_flac.cpp)
// A job is one int16 stream: frame f of it holds samples [4096 f, min(4096 (f + 1), n)) and carries the number first_frame + f; its
// frames take the slots slot0 .. of the slot and size tables, the jobs in ascending slot0.  k_flac_frames writes frame w to
// slots + w * FLAC_SLOT_BYTES (16-byte aligned) and its byte count to sizes[w]; launch_flac_gather scans the sizes (offsets[w] = the
// bytes in front of frame w, sizes[n_frames] = the low 32 bits of the total) and puts the frames back to back at out.  A frame is
// at most 16 + 2 * block bytes, so out holds flac_out_capacity bytes.  Integer arithmetic only; the bytes depend on nothing but
// (samples, rate, first_frame).
constexpr int FLAC_BLOCK = 4096;
constexpr int FLAC_SLOT_BYTES = 8208;
constexpr int FLAC_HEADER_BYTES = 42;      // "fLaC" + the STREAMINFO block
constexpr int FLAC_MAX_RATE = 0xfffff;     // STREAMINFO's 20 bits
constexpr long FLAC_MAX_FRAME_NUMBER = 0x1fffff;  // four bytes of the header's extended UTF-8
struct FlacJob {
    const int16_t* src;
    long n;
    int first_frame;
    int slot0;
};
inline long flac_frames(long n) { return (n + FLAC_BLOCK - 1) / FLAC_BLOCK; }
inline size_t flac_out_capacity(long n_frames, long total) { return (16 * (size_t)n_frames + 2 * (size_t)total + 15) & ~size_t(15); }
void launch_flac_frames(const FlacJob* jobs, int n_jobs, long n_frames, int rate, uint8_t* slots, int* sizes, hipStream_t s);
void launch_flac_gather(const uint8_t* slots, int* sizes, long long* offsets, long n_frames, uint8_t* out, hipStream_t s);
// the 42 bytes in front of the frames, from the frame sizes the host holds (min / max frame size); the MD5 field stays zero
void flac_stream_header(uint8_t* h, int rate, int64_t total, const int* sizes, long n_frames);
// SEVERAL FLAC files in one block (mi355vits_run_streams2 / _fetch_streams2): one job per compressed stream, every job
// with first_frame = 0 and slot0 = the frames of the jobs in front of it, k_flac_frames launched once over all of them.  File j sits
// at a 16-byte-aligned block offset base[j] (base[0] = base0, base[j + 1] = base[j] + (42 + its frames' bytes rounded up to 16)): its
// 42 header bytes, then its frames back to back.
//   launch_flac_place    one workgroup: the scan of the frame sizes (pre [n_frames + 1]: the bytes of the frames in front, over all
//                        jobs), per job FLAC_INFO_* at sizes[n_frames + 4 j ..], the block's end at sizes[n_frames + 4 n_jobs], per
//                        frame its block offset and job (ftab [n_frames + 1]: .x, .y), per job the 42 header bytes
//                        flac_stream_header makes as 12 little-endian words (hdr), per work item of the gather the last frame that
//                        starts at or before its first byte (item_first [flac_gather_items(bound_bytes)]).  sizes holds
//                        flac_info_words words: what the host copies in one piece.  jtab [FLAC_JTAB_ROWS n_jobs]: the job table of a
//                        launch with more jobs than the LDS holds.
//   launch_flac_gather_streams   destination-major: every 16-byte unit of [base0, end) has one writer lane, which assembles its 16
//                        bytes from the frame(s), header bytes and zero gaps that cover it; persistent over bound_bytes (the host's
//                        bound of end - base0), reading the end from the device.  out[p - base0] = block byte p; out holds
//                        bound_bytes rounded up to 16.
enum { FLAC_INFO_BASE = 0, FLAC_INFO_BYTES = 1, FLAC_INFO_MIN = 2, FLAC_INFO_MAX = 3, FLAC_INFO_WORDS = 4 };
constexpr int FLAC_HDR_WORDS = 12;
constexpr int FLAC_JTAB_ROWS = 5;
constexpr long FLAC_GATHER_ITEM_BYTES = 256L * 16;  // a work item of the gather: 256 lanes x one 16-byte store
inline size_t flac_info_words(long n_frames, int n_jobs) { return (size_t)n_frames + (size_t)FLAC_INFO_WORDS * n_jobs + 1; }
inline size_t flac_gather_items(long bound_bytes) { return (size_t)((bound_bytes + FLAC_GATHER_ITEM_BYTES - 1) / FLAC_GATHER_ITEM_BYTES) + 2; }
// a file's bound: its header, and every frame at its largest, rounded up to the next file's place
inline long flac_file_bound(long total) { return (FLAC_HEADER_BYTES + 16 * flac_frames(total) + 2 * total + 15) & ~15L; }
void launch_flac_place(const FlacJob* jobs, int n_jobs, long n_frames, int rate, long base0, int* sizes, unsigned* pre, int2* ftab,
                       unsigned* hdr, int* item_first, int* jtab, hipStream_t s);
void launch_flac_gather_streams(int n_jobs, long n_frames, const uint8_t* slots, const int* sizes, const int2* ftab, const unsigned* hdr,
                                const int* item_first, long base0, long bound_bytes, uint8_t* out, hipStream_t s);

// ---------------------------------------------------------------- output at a requested sample rate (kernels_resample.cpp)
// y[k] = sum_j h[k M - j L + half] x[j], x zero outside [0, n): what scipy.signal.resample_poly(x, L, M) returns with its default
// filter (Kaiser beta 5, half = 10 max(L, M) taps each side, cut-off 1 / max(L, M), gain L); n_out = ceil(n L / M).
constexpr int RESAMPLE_MAX_RATIO = 640;  // max(L, M) of a supported rate pair: at most 12,801 taps
struct ResampleFilter {
    int in_hz = 0, out_hz = 0;
    int L = 1, M = 1, half = 0;
    int tpp = 0;    // taps of one phase: ceil((2 half + 1) / L)
    int tp = 0;     // a phase's row in the table: tpp rounded up to a multiple of 4 with tp / 4 odd (zero taps behind)
    int tile = 0;   // outputs per work item (what fits the LDS beside the table; 1024 for every common rate)
    std::vector<float> table;  // [L][tp], phase-major; row p holds h[p + (tpp - 1 - i) L] at i: the order the taps are summed in
};
// designs the filter in double; false when out_hz < 1 or max(L, M) > RESAMPLE_MAX_RATIO (f untouched)
bool resample_design(int in_hz, int out_hz, ResampleFilter& f);
inline long long resample_out_len(long long n, int L, int M) { return (n * L + M - 1) / M; }
// the kernel's per-call table: [B] output lengths, then [B + 1] first work item of every row (a row has max(1, ceil(n_out / tile))
// items); n_in = the rows' input lengths on the host.  Returns the number of work items.
inline size_t resample_tab_ints(int B) { return 2 * (size_t)B + 1; }
long resample_fill_tab(const ResampleFilter& f, const int* n_in, int B, int* tab);
// x [B] rows of x_bs floats, x_len [B] (device); coef = f.table on the device; tab = the table above on the device.  Writes every
// sample of y's rows [0, y_ld): zeros at and past a row's output length.  peak_bits [B] must be zero: max |y| over the valid samples
// is added with an atomic max on the float's bits.  Every output sample is one fixed chain of tp fused multiply-adds, whatever the
// tile, the grid or the batch.
void launch_resample(const ResampleFilter& f, const float* coef, const float* x, long x_bs, const int* x_len, int B, const int* tab,
                     long items, float* y, long y_bs, int y_ld, unsigned* peak_bits, hipStream_t s);

// ---------------------------------------------------------------- phoneme timing and levels of a run (kernels_align.cpp)
// w_ceil / cum [B, T] (k_durations' frames and their inclusive scan; read at t < len[b] only), len [B] phonemes of a row, audio [B]
// rows of audio_bs floats with alen [B] valid samples (alen[b] <= audio_bs), hop samples per frame, L / M the reduced rate ratio.
// Writes [B, T] each: frames, start = ceil(hop c[t-1] L / M), samples = ceil(hop c[t] L / M) - start, and with peak and rms both
// given max |y| and (float) sqrt(sum((double) y y) / samples) over the span (0 for an empty one); peak == rms == nullptr: the
// audio is not read.  At t >= len[b]: 0 frames, 0 samples, start = the end of the covered part, levels 0.
void launch_align(const int* w_ceil, const int* cum, const int* len, int B, int T, const float* audio, long audio_bs, const int* alen,
                  int hop, int L, int M, int* frames, int* start, int* samples, float* peak, float* rms, hipStream_t s,
                  const int* wc = nullptr /* a pitch run: k_pitch_plan's warped boundaries take the place of hop * c */);

// ---------------------------------------------------------------- the quiet edges of a run's rows (kernels_edges.cpp)
// audio [B] rows of audio_bs floats with alen [B] valid samples (device), peak_bits [B] the rows' peaks, l_max >= every alen[b].
// thr = peak * ratio (one f32 multiply); a sample is loud iff fabsf(y) >= thr.  Writes first[b] = the first loud sample of row b (or
// max(alen[b], 0) when there is none) and last[b] = the last (or -1); both words are initialised here, on s, whatever they held.
void launch_edges(const float* audio, long audio_bs, const int* alen, const unsigned* peak_bits, int B, long l_max, float ratio,
                  int* first, int* last, hipStream_t s);

// ---------------------------------------------------------------- BS.1770 integrated loudness of a run's rows (kernels_loudness.cpp)
constexpr int LOUD_MIN_HZ = 4000;  // K-weighting's shelf sits at 1,682 Hz: below this rate the measure is not offered
constexpr int LOUD_MAX_K = 16;
// What the host derives from the rate: S = (fs + 5) / 10 the 100 ms step, W the warm-up of an item that starts inside a row (the
// smallest W with sum_{k >= W} |h[k]| <= 2^-40 sum |h|), K steps per work item (K S >= 4 W), c the cascade's coefficients.
struct LoudnessPlan {
    int fs = 0, S = 0, W = 0, K = 0;
    double c[7] = {};
};
bool loudness_plan(int fs, LoudnessPlan& out);  // false below LOUD_MIN_HZ; computed once per rate and process
inline long loudness_steps(long n, int S) { return n > 0 ? (n + S - 1) / S : 0; }  // the steps of a row, its partial last one included
// audio [B] rows of audio_bs floats with alen [B] valid samples (device), l_max >= every alen[b], fs >= LOUD_MIN_HZ.  k_loud writes
// E[b * ldE + j] = the K-weighted energy of step j for j < loudness_steps(alen[b]) (ldE >= loudness_steps(l_max)), k_loud_gate
// lufs / blocks / gated [B]; every word read is written on s before.  What lies behind a row is never looked at.
void launch_loudness(int fs, const float* audio, long audio_bs, const int* alen, int B, long l_max, double* E, long ldE, double* lufs,
                     int* blocks, int* gated, hipStream_t s);

// ---------------------------------------------------------------- look-ahead peak limiter of the packed streams (kernels_limit.cpp)
constexpr int LIMIT_MAX_WINDOW = 4096;  // the largest window L in samples: tile + 2 L staged samples fit 48 KB of LDS
constexpr int LIMIT_TILE = 4096;        // samples of a work item
constexpr long LIMIT_MAX_CURVE = 0x7fffffffL;  // the curves of a launch together: their offsets fit an int
// One row under one (g, c, U): scale[k] of its n >= 1 samples goes to curve[off + k]; tile0 = its first work item.  off and tile0
// are limit_place_jobs': jobs one behind the other, in the order given.
struct LimitJob {
    double g, c, U;
    int row, n, off, tile0;
};
struct LimitStat {
    unsigned long long sq_min;  // min sq[k] over the job's samples ((L + 1) 2^30 when nothing was reduced)
    int reduced, pad;           // samples with sq[k] < (L + 1) 2^30
};
// fills off / tile0 of every job; returns the work items of the launch and *curve_floats = the floats of all curves, or -1 when a
// job is empty or the curves together exceed LIMIT_MAX_CURVE floats
long limit_place_jobs(LimitJob* jobs, int n_jobs, long* curve_floats);
// jobs / stats [n_jobs] and curve on the device; audio rows of audio_bs floats (a job reads its row's [0, n) and nothing behind
// it); 1 <= L <= LIMIT_MAX_WINDOW.  stats are initialised here, on s, whatever they held; curve == nullptr: statistics only.
// env != nullptr (true-peak ceiling mode): rq is made from env[job.off + t] — launch_true_peak_env's e[t] — instead of fabs((double) x[t]).
void launch_limit(const LimitJob* jobs, int n_jobs, long tiles, int L, const float* audio, long audio_bs, LimitStat* stats, float* curve,
                  hipStream_t s, const double* env = nullptr);

// ---------------------------------------------------------------- 4x oversampled peak and its envelope (kernels_truepeak.cpp)
constexpr int TRUE_PEAK_TAPS = 81;          // scipy.signal.resample_poly(., 4, 1)'s default filter: literal doubles in the source
constexpr int TRUE_PEAK_TILE = LIMIT_TILE;  // samples of a work item: the envelope form runs on the limiter's job table
const double* true_peak_taps();             // [TRUE_PEAK_TAPS]
// audio [B] rows of audio_bs floats with alen [B] valid samples (device), l_max >= every alen[b] -> tp [B] doubles (device): the rule
// of include/mi355vits.h.  tp is initialised here, on s, whatever it held.  What lies behind a row is never looked at.
void launch_true_peak(const float* audio, long audio_bs, const int* alen, int B, long l_max, double* tp, hipStream_t s);
// e[t] of every job's row to env[job.off + t] (jobs / tiles: limit_place_jobs'); every element has exactly one writer
void launch_true_peak_env(const LimitJob* jobs, int n_jobs, long tiles, const float* audio, long audio_bs, double* env, hipStream_t s);

// ---------------------------------------------------------------- encoder pieces
void launch_embed(const long long* ids, const int* len, const float* emb, int B, int T, int H, int num_symbols,
                  float scale, float* y, hipStream_t s);
// y = LN_c(x (+ res)) [* gelu] [* mask]; in place allowed (y == x).
struct LNArgs {
    const float* x = nullptr; const float* res = nullptr; float* y = nullptr;
    const float* gamma = nullptr; const float* beta = nullptr;
    const int* out_len = nullptr;
    int B = 1, C = 0, T = 0;
    int gelu = 0;
    const float* add_to = nullptr;  // y = add_to + f(LN(x))   (DDS residual) or null
    float eps = 1e-5f;
    // x as `nparts` raw partial sums of a conv split over its input channels (x + p * part_stride, added in order p = 0, 1, ..),
    // then the conv's epilogue: + bias[c], zero at t >= premask_len[b] (the FFN's mask before the residual); then + res, LN
    int nparts = 1;
    long part_stride = 0;
    const float* bias = nullptr;
    const int* premask_len = nullptr;
};
void launch_layernorm(const LNArgs& a, hipStream_t s);
// relative-position multi-head attention on packed qkv [B, 3H, T] -> out [B, H, T]
void launch_rel_attention(const float* qkv, const float* emb_rel_k, const float* emb_rel_v, const int* len,
                          int B, int T, int H, int n_heads, int window, float* out, hipStream_t s);
// same contract on the fp32 matrix cores (four waves per 32 query rows; T <= 512, window <= 15), see kernels_attn.cpp
bool rel_attention_mfma_supported(int T, int H, int n_heads, int window);
void launch_rel_attention_mfma(const float* qkv, const float* emb_rel_k, const float* emb_rel_v, const int* len,
                               int B, int T, int H, int n_heads, int window, float* out, hipStream_t s);
// same contract for any T: keys streamed through an online softmax (k_rel_attention_stream; even head width <= 128, window <= 15)
bool rel_attention_stream_supported(int H, int n_heads, int window);
void launch_rel_attention_stream(const float* qkv, const float* emb_rel_k, const float* emb_rel_v, const int* len,
                                 int B, int T, int H, int n_heads, int window, float* out, hipStream_t s);
// longest T the VALU kernel k_rel_attention serves: one score row per wave in 64 KiB of LDS
int rel_attention_valu_cap(int H, int n_heads, int window);

// ---------------------------------------------------------------- stochastic duration predictor pieces
// y = gelu(LN(dwconv_k,d(x * mask)))   (first half of a DDS layer, A.6)
void launch_dds_dwconv_ln_gelu(const float* x, const float* w, const float* bias, const float* gamma,
                               const float* beta, const int* len, int B, int C, int T, int K, int dil, float* y,
                               hipStream_t s);
// one whole DDS layer: y = x + gelu(LN2(conv1x1(gelu(LN1(dwconv(x * mask))))))  (x, y different buffers; w1x1 = packed f32
// A fragments of the 1x1 conv).  C in {32, 64, 128, 192, 256}.
bool dds_layer_fused_supported(int C);
void launch_dds_layer(const float* x, float* y, const float* dw_w, const float* dw_b, const float* g1, const float* b1,
                      const float* w1x1_packed, const float* bias1x1, const float* g2, const float* b2, const int* len, int B,
                      int C, int T, int K, int dil, hipStream_t s);
// the whole DDS stack with its pre (1x1 conv + cond, or ConvFlow's affine pre + g), its proj and, for a ConvFlow, the spline:
// one launch (kernels_misc.cpp, k_dds_stack).  C = 192, K = 3, the taps' total reach <= 16 columns.
constexpr int DDS_STACK_MAX_LAYERS = 4, DDS_STACK_W = 64, DDS_STACK_OFF = 16, DDS_STACK_K = 3;
enum { DDS_PRE_CONV = 0, DDS_PRE_AFFINE = 1 };
struct DdsStackArgs {
    const float* src = nullptr;    // PRE_CONV: input of the 1x1 pre conv [B, C, T]; PRE_AFFINE: g [B, C, T]
    int pre_mode = DDS_PRE_CONV;
    const float* pre_w = nullptr;  // PRE_CONV: packed f32 A fragments [C/32][C/2][64]; PRE_AFFINE: [C]
    const float* pre_b = nullptr;  // [C]
    const float* cond = nullptr;   // PRE_CONV: + cond[b * cond_bs + c] (or null)
    long cond_bs = 0;
    float* z = nullptr;            // PRE_AFFINE: z [B, 2, T]; channel zch feeds pre, the spline rewrites channel 1 - zch
    int zch = 0;
    int n_layers = 0, K = 3;       // dilation of layer i = K^i
    const float* dw_w[DDS_STACK_MAX_LAYERS] = {};
    const float* dw_b[DDS_STACK_MAX_LAYERS] = {};
    const float* g1[DDS_STACK_MAX_LAYERS] = {};
    const float* b1[DDS_STACK_MAX_LAYERS] = {};
    const float* w1x1[DDS_STACK_MAX_LAYERS] = {};     // packed f32 A fragments
    const float* bias1x1[DDS_STACK_MAX_LAYERS] = {};
    const float* g2[DDS_STACK_MAX_LAYERS] = {};
    const float* b2[DDS_STACK_MAX_LAYERS] = {};
    float* x_out = nullptr;        // the stack's x before proj [B, C, T] (tests) or null
    const float* proj_w = nullptr; // packed f32 A fragments of proj (rows beyond proj_cout zero) or null: no proj
    const float* proj_b = nullptr;
    int proj_cout = 0;
    float* out = nullptr;          // [B, proj_cout, T] or null (a ConvFlow's theta stays on the CU)
    int spline = 0, nb = 0;
    float tail = 0.0f, inv_sqrt_fc = 0.0f;
    const int* len = nullptr;
    int B = 1, T = 0;
    int math = MATH_F32;  // MATH_BF16X3 / BF16W: pre_w (conv mode), w1x1[], proj_w are layout-1 bf16 planes (k_dds_stack_b3)
    int ablate = 0;  // lab build only
};
bool dds_stack_supported(int C, int K, int n_layers, int proj_cout);
void launch_dds_stack(const DdsStackArgs& a, int C, hipStream_t s);
// ---------------------------------------------------------------- deterministic duration predictor (use_sdp = false)
// logw = proj(LN_2(relu(conv_2(LN_1(relu(conv_1((x + cond) * m))) * m))) * m) * m in one launch (kernels_dp.cpp, k_dp_det).
// w1 / w2: layout-1 bf16 planes (pack_conv_weights_bf16x3_mode) in the split-bf16 modes, packed f32 A fragments in MATH_F32.
struct DpDetArgs {
    const float* x = nullptr;     // text-encoder output [B, H, T]
    const float* cond = nullptr;  // + cond[b * cond_bs + c] before the mask (multi-speaker) or null
    long cond_bs = 0;
    const float* w1 = nullptr; const float* b1 = nullptr; const float* g1 = nullptr; const float* be1 = nullptr;  // conv_1, norm_1
    const float* w2 = nullptr; const float* b2 = nullptr; const float* g2 = nullptr; const float* be2 = nullptr;  // conv_2, norm_2
    const float* pw = nullptr;    // proj weight [F]
    const float* pb = nullptr;    // proj bias [1]
    const int* len = nullptr;
    float* out = nullptr;         // logw at out[b * out_bs + t]; zero at t >= len[b]
    long out_bs = 0;
    int B = 1, T = 0, H = 0, F = 0, K = 3;
    int math = MATH_BF16X3;       // MATH_F32: v_mfma_f32_32x32x2_f32; any other mode: exact split-bf16 products
};
bool dp_det_supported(int H, int F, int K);  // H, F multiples of 32 up to 256; K odd up to 7
int dp_det_tile_cols(int K);  // output columns of a work item: the 64-column window less the two convs' reach, 2 (K / 2)
size_t dp_det_lds_bytes(int H, int F, int K, int math);
void launch_dp_det(const DpDetArgs& a, hipStream_t s);

// h[b,c,t] = w[c] * z[b,ch,t] + bias[c] + g[b,c,t]      (ConvFlow.pre on one channel + conditioning)
void launch_convflow_pre(const float* z, int ch, const float* w, const float* bias, const float* g, int B, int C,
                         int T, float* h, hipStream_t s);
// z[b,1-ch] <- RQS^-1(z[b,1-ch]; theta[b,:,t]) inside the tail bound; then z *= mask     (A.7)
void launch_spline_inverse(float* z, int ch_x0, const float* theta, const int* len, int B, int T, int nbins,
                           float tail, float inv_sqrt_fc, hipStream_t s);
// per-row synthesis settings, device arrays: scales [B,3] = noise_scale, length_scale, noise_w; utt [B] = Philox utterance index
// z init: z[b,c,t] = noise * noise_w[b] (Philox under key utt[b], or injected)
void launch_sdp_noise(float* z, const float* injected, int B, int T, const float* scales, unsigned long long seed,
                      const unsigned long long* utt, hipStream_t s);
// most latent frames one utterance may have (4.2 M frames = 13.5 h of audio); larger / non-finite predictions are an error
constexpr int DURATION_FRAME_CAP = 1 << 22;
// EA^-1 on channel `ch` -> logw; durations: w = ceil(exp(logw)*mask*ls[b]) (or forced); cum = inclusive scan;
// ylen = max(1, sum)
void launch_durations(const float* z, int ch, float ea_m, float ea_logs, const int* len, const int* forced, int B,
                      int T, const float* scales, float* logw, int* w_ceil, int* cum, int* ylen, hipStream_t s);
// the two expressions k_durations and k_durations_timed share, so that a timed run's durations start from the very bits an
// untimed run rounds up: logw out of the flow's channel (EA^-1, es = expf(-ea_logs)), the float duration of a phoneme (m = 1 inside
// the row, 0 behind it) and its guarded frame count
__device__ __forceinline__ float duration_logw(float z, float ea_m, float es, float m) { return (z - ea_m) * es * m; }
__device__ __forceinline__ float duration_float(float lw, float m, float length_scale) { return expf(lw) * m * length_scale; }
// inf / NaN / absurd durations (bad weights, huge length_scale) must not reach the float -> int cast (UB): they become one
// over-the-cap count, which the host turns into ERR_INVALID before sizing anything
__device__ __forceinline__ int duration_count(float w) { return (w < (float)DURATION_FRAME_CAP) ? (int)ceilf(w) : DURATION_FRAME_CAP + 1; }

// ---------------------------------------------------------------- timing control (kernels_timing.cpp; mi355vits_run_timed)
// k_durations_timed in place of k_durations: EA^-1 and logw as there, then per row (L = len[b], t < L)
//   u[t] = fl(w[t] * stretch[b,t]),  f[t](s) = max(c(fl(u[t] * s)), min_frames[b,t]),  F(s) = sum f[t](s)   (c = duration_count)
// without a target frames = f(1.0f); with target N the largest f32 s* in [2^-30, 2^30] with F(s*) <= N by bisection over the bit
// patterns, and the N - F(s*) frames still missing go, in index order, to the phonemes that step at nextafterf(s*): sum frames == N.
// status: 0 ok; 1 F(2^-30) > N (frames = f(2^-30): the floor, factor = 2^-30); 2 F(2^30) < N (frames = f(2^30), factor = 2^30).
// cum / ylen as k_durations.  Integers and single f32 products only: no result depends on the grid, the batch or an address.
constexpr int TIMING_OK = 0, TIMING_BELOW_FLOOR = 1, TIMING_UNREACHABLE = 2;
constexpr int TIMING_LDS_T = 16384;  // rows up to this many phonemes keep u and min_frames in LDS (128 KB); longer ones re-read them
struct DurTimedArgs {
    const float* z = nullptr; int ch = 0; float ea_m = 0, ea_logs = 0;  // as launch_durations ...
    const float* u_in = nullptr;       // ... or (the lab hook: the fit stage alone) u [B, T] given; z, scales, stretch, logw unused
    const int* len = nullptr; int B = 1, T = 0;
    const float* scales = nullptr;
    const float* stretch = nullptr;    // [B, T] or null (= 1)
    const int* min_frames = nullptr;   // [B, T] or null (= 0)
    const int* target = nullptr;       // [B] or null (= none)
    float* logw = nullptr;             // [B, T]
    float* u = nullptr;                // [B, T]: the u[t] the rule ran on, 0 behind the row (the dur_float tap)
    int *w_ceil = nullptr, *cum = nullptr, *ylen = nullptr;
    float* factor = nullptr;           // [B]: s*, 1.0f without a target
    int* status = nullptr;             // [B]: TIMING_*
};
void launch_durations_timed(const DurTimedArgs& a, hipStream_t s);

// ---------------------------------------------------------------- length regulator + prior sampling (K6, K7)
void launch_expand_prior(const float* stats /*[B,2I,Tx]: m_p | logs_p*/, const int* cum, const int* ylen,
                         const float* injected, int injected_frames, int B, int I, int Tx, int Ty,
                         const float* scales, unsigned long long seed, const unsigned long long* utt, float* z,
                         hipStream_t s);

// ---------------------------------------------------------------- speaker conditioning (A.11)
// out[b, co] = W[co, :] . emb_g[sid[b], :] + bias[co]
void launch_speaker_cond(const float* emb_g, const long long* sid, const float* w, const float* bias, int B,
                         int gin, int Cout, float* out, hipStream_t s);

// ---------------------------------------------------------------- blended / caller-supplied speakers (kernels_speaker.cpp;
// mi355vits_run_speakers).  k_speaker_cond_mix: ONE launch makes g [B, gin] of every row and every consumer's projection of it.
//   mix:     over the terms k < K of row b whose weight is not exactly 0, in order of k, per channel i:
//            g[i] = fl(w_0 * e_0[i]), then g[i] = fl(g[i] + fl(w_k * e_k[i])), e_k = emb_g[sid[b,k], :]   (single f32 products and
//            sums, never fused; a skipped term's sid is not read; a row without a term: g = 0, which the engine refuses beforehand)
//   vectors: g[i] = vectors[b, i], bits in, bits out
//   jobs:    out[b, co] = W[co, :] . g + bias[co] with k_speaker_cond's arithmetic per element: lane l of a wave accumulates
//            fmaf(W[co, i], g[i], acc) over i = l, l + 64, .. from 0.0f, then wave_reduce_sum, then + bias
// No result depends on the row block, the grid, the batch or an address.
constexpr int SPEAKER_MIX_MAX_TERMS = 8;   // = MI355VITS_MAX_SPEAKER_TERMS
constexpr int SPEAKER_MIX_MAX_JOBS = 10;   // dp.cond, dec.cond and a cond_layer per flow the kernel serves in one launch (2 + MI355VITS_MAX_STAGES)
constexpr int SPEAKER_MIX_ROWS = 8;        // rows of a workgroup's block (<= 32: a wave stages eight at the most): their g vectors stay in LDS (8 x 512 floats = 16 KiB)
constexpr int SPEAKER_MIX_LDS_FLOATS = 16384;  // the block's LDS budget: a gin above 2048 shrinks the block (gin <= 8192: two rows at least)
constexpr int SPEAKER_MIX_TILE = 16;       // output channels of a workgroup: four per wave, their weight slices in registers
struct SpeakerMixJob {
    const float* w = nullptr;     // [Cout, gin]
    const float* bias = nullptr;  // [Cout] or null (= 0)
    float* out = nullptr;         // [B, Cout]
    int Cout = 0;
    int first_tile = 0;           // the job's first workgroup along grid x (filled in by the launcher)
};
struct SpeakerMixArgs {
    const float* emb_g = nullptr;       // [n_speakers, gin]            (mix)
    const long long* sid = nullptr;     // [B, K]                       (mix)
    const float* weight = nullptr;      // [B, K]                       (mix)
    const float* vectors = nullptr;     // [B, gin]: excludes the three above
    int K = 0, B = 1, gin = 0;
    float* g = nullptr;                 // [B, gin]: written by the workgroups of job 0, tile 0
    int n_jobs = 0;
    SpeakerMixJob jobs[SPEAKER_MIX_MAX_JOBS];
};
void launch_speaker_cond_mix(SpeakerMixArgs a, hipStream_t s);

// ---------------------------------------------------------------- a gain per phoneme with exact ramps (kernels_level.cpp;
// mi355vits_run_levels).  k_levels: ONE launch over the valid samples of every row of the native waveform, in place.  Per row b,
// with c = cum[b, :] (the inclusive scan of the run's frames), L = len[b], n = alen[b] = hop * max(1, c[L - 1]), R = ramp[b]:
//   q[t]  = (int) rintf(gain[b, t] * 2^20)                    0 <= gain <= 1024
//   qs(i) = q[t(i)], t(i) = the smallest t < L with hop * c[t] > i; 2^20 when there is none; edge values repeat outside [0, n)
//   S[k]  = sum of qs(i) over k - R <= i <= k + R              (int64)
//   y[k]  = x[k] * (float) ((double) S[k] / (double) ((2 R + 1) * 2^20)),  0 <= k < n;  peak_bits[b] = the bits of max |y[k]|
// peak_bits [B] must be zero before the launch (same stream); nothing outside [0, n) of a row is read or written; l_max = the
// longest row.  No result depends on the grid, the batch, the row block or an address.
constexpr int LEVELS_TILE = LIMIT_TILE;  // samples of a work item
constexpr int LEVELS_TABLE = 1024;       // non-empty phonemes of a tile's reach staged in LDS at once (16 KiB); more: walked in chunks
constexpr int LEVELS_ONE = 1 << 20;     // the fixed-point unit of a gain
constexpr int LEVELS_MAX_RAMP = 4096;    // R: samples at the native rate
void launch_levels(const int* cum, const int* len, const float* gain, const int* ramp /* null: 0 */, int B, int T, int hop,
                   float* audio, long audio_bs, const int* alen, long l_max, unsigned* peak_bits, hipStream_t s);

// ---------------------------------------------------------------- a pitch ratio per phoneme, duration kept (kernels_pitch.cpp;
// mi355vits_run_pitch: the rule is in include/mi355vits.h).  k_pitch_plan: per row b, with c = cum[b, :], L = len[b],
// fs[t] = c[t] - c[t-1] and inv[t] = (int) rintf(2^20 / ratio[b, t]) (ratio null: 2^20):
//   tq[b, t] = sum over u <= min(t, L - 1) of hop fs[u] inv[u]  (int64)     wc[b, t] = ceil(tq[b, t] / 2^20)
//   wlen[b]  = wc[b, L - 1], or hop for a row without frames (L = 0 or c[L-1] = 0);  wc and wlen saturate at 2^31 - 1
// k_pitch: y[b, k] for 0 <= k < wlen[b] by the rule (the band-limited warp of x[b, 0 .. x_len[b]) along tq), zeros for
// wlen[b] <= k < y_ld; peak_bits[b] = the bits of max |y| (zero before the launch, same stream).  tq / wc / wlen must be
// k_pitch_plan's of the same cum / len / ratio, x_len[b] = hop max(1, c[L-1]) and wlen[b] < 2^31 - 1, y_ld >= max wlen.
// items_tab = pitch_fill_tab's table on the device (pitch_tab_ints(B) ints: [B] wlen, [B + 1] the first work item of a row; the
// host makes it from the plan's wlen), items its return value: the grid is persistent over them.  Nothing
// outside [0, x_len[b]) of a row of x is read.  No result depends on the grid, the batch, the row block or an address.
constexpr int PITCH_ONE = 1 << 20;  // the fixed-point unit of the time map
constexpr int PITCH_P = 128;        // filter table entries per source sample
constexpr int PITCH_Z = 12;         // zero crossings either side
constexpr int PITCH_TABLE_FLOATS = PITCH_Z * PITCH_P + 2;
constexpr int PITCH_TILE = 1024;    // outputs of a work item
// h[i] = (float) (sinc(i / P) I0(8 sqrt(1 - (i / (Z P))^2)) / I0(8)), in double; exactly 0 at the multiples of P, h[0] = 1,
// h[Z P] = h[Z P + 1] = 0.  Computed once per process.
const std::vector<float>& pitch_table();
void launch_pitch_plan(const int* cum, const int* len, const float* ratio /* null: 1 */, int B, int T, int hop, long long* tq, int* wc,
                       int* wlen, hipStream_t s);
inline size_t pitch_tab_ints(int B) { return 2 * (size_t)B + 1; }
long pitch_fill_tab(const int64_t* wlen, int B, int* tab);  // -> the work items
void launch_pitch(const float* x, long x_bs, const int* x_len, const int* cum, const int* len, const float* ratio /* null: 1 */,
                  const long long* tq, const int* wc, const int* items_tab, long items, const float* table, int B, int T, int hop,
                  float* y, long y_bs, int y_ld, unsigned* peak_bits, hipStream_t s);

// misc
void launch_fill(float* p, float v, size_t n, hipStream_t s);
void launch_zero_row_tails(float* p, int B, int C, long T, const int* len, int factor, hipStream_t s);  // p[b, :, len[b] * factor:] = 0
void launch_mfma_selftest(float* out /*[32*32 + 16*16 + 16*16]*/, hipStream_t s);
// box probe (mi355vits_probe_device): L2-hit 16-byte stream of one table by every CU, L2-hit dependent-load chain, HBM copy
void launch_probe_l2_stream(const void* tbl, int n16, int reps, unsigned* sink, int grid, hipStream_t s);
void launch_probe_l2_latency(const unsigned* chain, int steps, unsigned nlines, unsigned* out, int grid, hipStream_t s);
void launch_probe_copy(const void* src, void* dst, long n16, int grid, hipStream_t s);
void launch_probe_l2_stream1(const void* tbl, int n16, int reps, unsigned* sink, int grid, hipStream_t s);
void launch_probe_l2_mixed(const void* tbl, int n16, int reps, const void* src, void* dst, long slice16, unsigned* sink, int grid, hipStream_t s);

}  // namespace m355
