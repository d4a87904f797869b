// kernels_dp.cpp — the deterministic duration predictor of VITS (upstream models.DurationPredictor, inference) in one launch:
//   x  = x + cond(g)                         (multi-speaker: cond = the speaker term, [B, H])
//   h1 = LN_1(relu(conv_1(x * m)))           (H -> F, kernel K, "same" padding)
//   h2 = LN_2(relu(conv_2(h1 * m)))          (F -> F, kernel K)
//   logw = (proj . h2 + proj_b) * m          (1x1, F -> 1)
// Work item = (row, tile of DPD_COLS - 2 P output columns), P = K / 2.  Both convs run over DPD_COLS = 64 window columns (two
// 32-column MFMA tiles): conv_1 makes h1 at t0 - P .. t0 - P + 63 from x at t0 - 2P .. t0 + 63 + 2P - 2P, conv_2 makes logw at
// t0 .. t0 + 63 of which the first 64 - 2P are kept (the rest would need h1 beyond the window: those columns read zeros and are
// dropped).  Wave w owns the 32 filter rows 32 w .. of both convs (F / 32 waves), so the F channels of a column meet in one
// workgroup: LayerNorm's mean and variance are two passes of per-lane partial sums added up through LDS in a fixed order.
// The convs are exact in every math mode the text side runs: three-term bf16 splits of both operands, six products on
// v_mfma_f32_32x32x16_bf16 with f32 accumulate (b3.h), or v_mfma_f32_32x32x2_f32 in MATH_F32.  The x planes are dead once
// conv_1 has read them, and h1's planes take their place (F = 256, K = 3: 101 KiB).
// Every column sees the same operations in the same order wherever it lands (tile, grid, batch): batched == solo, bitwise.
#include "kernels.h"
#include "b3.h"

namespace m355 {

constexpr int DPD_COLS = 64;
constexpr int DPD_MAX_C = 256;

static inline int dpd_ld(int K) { return DPD_COLS + 2 * (K / 2); }

template <bool F32>
__global__ __launch_bounds__(512) void k_dp_det(DpDetArgs a) {
    DYN_SMEM(float, smem);
    const int P = a.K / 2, NO = DPD_COLS - 2 * P, LD = DPD_COLS + 2 * P;
    const int H = a.H, F = a.F, GX = H / 16, GF = F / 16;
    const int nw = F / 32;
    const int tid = threadIdx.x, lane = tid & 63, w = WAVE_UNIFORM(tid >> 6);
    const int brow = lane >> 5, bcol = lane & 31;
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * NO;
    const int L = a.len[b] < a.T ? a.len[b] : a.T;
    const int region = F32 ? (H > F ? H : F) * LD : 3 * 2 * (GX > GF ? GX : GF) * LD * 4;  // floats
    uint4* planes = reinterpret_cast<uint4*>(smem);  // split-bf16 operand planes [3][G][2][LD] (16-byte records)
    float* X = smem;                                 // MATH_F32: the operand itself [C][LD]
    float* red = smem + region;                      // [nw][2][64] per-lane partial column sums
    int rowc[16];  // the 16 filter rows of a 32 x 32 accumulator tile this lane holds
    MI355_UNROLL
    for (int r = 0; r < 16; ++r) rowc[r] = 32 * w + (r & 3) + 8 * (r >> 2) + 4 * brow;

    // record (group g, half h) of a column: slot e <-> channel 16 g + 8 (e >> 2) + 4 h + (e & 3)  (layout 1, b3.h)
    auto put_record = [&](const float* v8, int PS, int g, int h, int col) MI355_INLINE_LAMBDA {
        uint4 hi, mi, lo;
        split3_pk(v8[0], v8[1], hi.x, mi.x, lo.x);
        split3_pk(v8[2], v8[3], hi.y, mi.y, lo.y);
        split3_pk(v8[4], v8[5], hi.z, mi.z, lo.z);
        split3_pk(v8[6], v8[7], hi.w, mi.w, lo.w);
        const int o = (g * 2 + h) * LD + col;
        planes[o] = hi;
        planes[PS + o] = mi;
        planes[2 * PS + o] = lo;
    };
    // per column: the sum over all F rows of the lanes' partials, in the fixed order (wave, half)
    auto col_sum = [&](float (&s)[2]) MI355_INLINE_LAMBDA {
        __syncthreads();
        MI355_UNROLL
        for (int j = 0; j < 2; ++j) red[(w * 2 + brow) * 64 + 32 * j + bcol] = s[j];
        __syncthreads();
        MI355_UNROLL
        for (int j = 0; j < 2; ++j) {
            float t = 0.0f;
            for (int q = 0; q < 2 * nw; ++q) t += red[q * 64 + 32 * j + bcol];
            s[j] = t;
        }
    };
    // one conv over the staged operand (Cin channels), rows 32 w .., window columns 0 .. 63
    auto conv = [&](const float* wt, int Cin, f32x16 (&acc)[1][2]) MI355_INLINE_LAMBDA {
        MI355_UNROLL
        for (int j = 0; j < 2; ++j)
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) acc[0][j][r] = 0.0f;
        if constexpr (F32) {
            const int cpn = Cin / 2;
            for (int k = 0; k < a.K; ++k) {
                const float* wk = wt + ((long)(w * a.K + k) * cpn) * 64 + lane;
                const float* xk = X + brow * LD + bcol + k;
                for (int cp = 0; cp < cpn; ++cp) {
                    const float av = wk[(long)cp * 64];
                    MI355_UNROLL
                    for (int j = 0; j < 2; ++j) acc[0][j] = MFMA_32x32x2_F32(av, xk[2 * cp * LD + 32 * j], acc[0][j]);
                }
            }
        } else {
            const int G = Cin / 16, PS = G * 2 * LD;
            const uint4* wb = reinterpret_cast<const uint4*>(wt) + (long)w * a.K * G * 192 + lane;
            for (int g = 0; g < G; g += 2) {  // two 16-channel groups per b3_chunk: all K taps of them
                const uint4* wp[1] = {wb + (long)g * 192};
                b3_chunk<1, 2, 2>(acc, wp, planes + (g * 2 + brow) * LD + bcol, PS, LD, a.K, G, 1);
            }
        }
    };
    // relu(acc + bias) -> LayerNorm over the F rows of each column (two passes, biased variance, eps 1e-5)
    auto relu_ln = [&](const f32x16 (&acc)[1][2], const float* bias, const float* gamma, const float* beta, float (&v)[2][16])
        MI355_INLINE_LAMBDA {
        float bs[16], gm[16], bt[16];
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) {
            bs[r] = bias[rowc[r]];
            gm[r] = gamma[rowc[r]];
            bt[r] = beta[rowc[r]];
        }
        float s[2];
        MI355_UNROLL
        for (int j = 0; j < 2; ++j) {
            s[j] = 0.0f;
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) {
                v[j][r] = fmaxf(acc[0][j][r] + bs[r], 0.0f);
                s[j] += v[j][r];
            }
        }
        col_sum(s);
        float mean[2], q[2];
        MI355_UNROLL
        for (int j = 0; j < 2; ++j) {
            mean[j] = s[j] / (float)F;
            q[j] = 0.0f;
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) {
                const float d = v[j][r] - mean[j];
                q[j] += d * d;
            }
        }
        col_sum(q);
        MI355_UNROLL
        for (int j = 0; j < 2; ++j) {
            const float rstd = 1.0f / sqrtf(q[j] / (float)F + 1e-5f);
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) v[j][r] = (v[j][r] - mean[j]) * rstd * gm[r] + bt[r];
        }
    };

    // ---- stage (x + cond) * m at window columns 0 .. LD - 1 (time t0 - 2P + i)
    if constexpr (F32) {
        for (int it = tid; it < H * LD; it += blockDim.x) {
            const int c = it / LD, i = it - c * LD, t = t0 - 2 * P + i;
            const bool in = t >= 0 && t < L;
            float v = 0.0f;
            if (in) {
                v = a.x[((long)b * H + c) * a.T + t];
                if (a.cond) v += a.cond[(long)b * a.cond_bs + c];
            }
            X[c * LD + i] = v;
        }
    } else {
        const int PS = GX * 2 * LD;
        for (int it = tid; it < GX * LD; it += blockDim.x) {
            const int g = it / LD, i = it - g * LD, t = t0 - 2 * P + i;
            const bool in = t >= 0 && t < L;
            const int tc = in ? t : 0;
            float v[16];
            MI355_UNROLL
            for (int e = 0; e < 16; ++e) {
                const int c = 16 * g + e;
                float xv = a.x[((long)b * H + c) * a.T + tc];
                if (a.cond) xv += a.cond[(long)b * a.cond_bs + c];
                v[e] = in ? xv : 0.0f;
            }
            float r0[8] = {v[0], v[1], v[2], v[3], v[8], v[9], v[10], v[11]};
            float r1[8] = {v[4], v[5], v[6], v[7], v[12], v[13], v[14], v[15]};
            put_record(r0, PS, g, 0, i);
            put_record(r1, PS, g, 1, i);
        }
    }
    __syncthreads();

    // ---- conv_1 -> relu -> LN_1 -> * m  -> h1 over the x operand's space (col_sum's first barrier: every wave is past conv_1)
    f32x16 acc[1][2];
    float v[2][16];
    conv(a.w1, H, acc);
    relu_ln(acc, a.b1, a.g1, a.be1, v);
    {
        const int PS = GF * 2 * LD;
        MI355_UNROLL
        for (int j = 0; j < 2; ++j) {
            const int col = 32 * j + bcol, t = t0 - P + col;
            const bool in = t >= 0 && t < L;
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) v[j][r] = in ? v[j][r] : 0.0f;
            if constexpr (F32) {
                MI355_UNROLL
                for (int r = 0; r < 16; ++r) X[rowc[r] * LD + col] = v[j][r];
            } else {
                // the lane's 16 rows are exactly records (2 w + u, brow), u = 0, 1: slots 0..3 <- r = 8u .., 4..7 <- r = 8u + 4 ..
                MI355_UNROLL
                for (int u = 0; u < 2; ++u) put_record(&v[j][8 * u], PS, 2 * w + u, brow, col);
            }
        }
        // columns 64 .. LD - 1 (read only by the dropped outputs): zeros
        const int nz = LD - DPD_COLS;
        if constexpr (F32) {
            for (int it = tid; it < F * nz; it += blockDim.x) X[(it / nz) * LD + DPD_COLS + it % nz] = 0.0f;
        } else {
            const uint4 z = {0u, 0u, 0u, 0u};
            for (int it = tid; it < 3 * GF * 2 * nz; it += blockDim.x) planes[(it / nz) * LD + DPD_COLS + it % nz] = z;
        }
    }
    __syncthreads();

    // ---- conv_2 -> relu -> LN_2 -> proj -> * m
    conv(a.w2, F, acc);
    relu_ln(acc, a.b2, a.g2, a.be2, v);
    float pw[16];
    MI355_UNROLL
    for (int r = 0; r < 16; ++r) pw[r] = a.pw[rowc[r]];
    float s[2];
    MI355_UNROLL
    for (int j = 0; j < 2; ++j) {
        s[j] = 0.0f;
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) s[j] = fmaf(pw[r], v[j][r], s[j]);
    }
    col_sum(s);
    if (w == 0 && brow == 0) {
        const float pb = a.pb[0];
        MI355_UNROLL
        for (int j = 0; j < 2; ++j) {
            const int o = 32 * j + bcol, t = t0 + o;
            if (o < NO && t < a.T) a.out[(long)b * a.out_bs + t] = t < L ? s[j] + pb : 0.0f;
        }
    }
}

bool dp_det_supported(int H, int F, int K) {
    return H >= 32 && H % 32 == 0 && H <= DPD_MAX_C && F >= 32 && F % 32 == 0 && F <= DPD_MAX_C && K >= 1 && K % 2 == 1 && K <= 7;
}

int dp_det_tile_cols(int K) { return DPD_COLS - 2 * (K / 2); }

size_t dp_det_lds_bytes(int H, int F, int K, int math) {
    const int LD = dpd_ld(K), C = H > F ? H : F;
    const size_t region = math == MATH_F32 ? (size_t)C * LD : (size_t)3 * 2 * (C / 16) * LD * 4;
    return (region + (size_t)(F / 32) * 2 * 64) * sizeof(float);
}

void launch_dp_det(const DpDetArgs& a, hipStream_t s) {
    if (a.T <= 0 || a.B <= 0) return;
    if (!dp_det_supported(a.H, a.F, a.K)) throw std::runtime_error("dp_det: unsupported shape");
    const int NO = dp_det_tile_cols(a.K);
    const dim3 grid((a.T + NO - 1) / NO, a.B), block(2 * a.F);  // F / 32 waves
    const size_t sh = dp_det_lds_bytes(a.H, a.F, a.K, a.math);
    auto go = [&](auto kfn) {
#ifndef MI355_EMU
        set_max_dynamic_lds(reinterpret_cast<const void*>(kfn), 160 * 1024);
#endif
        LAUNCH_KERNEL(kfn, grid, block, sh, s, a);
    };
    if (a.math == MATH_F32) go(k_dp_det<true>);
    else go(k_dp_det<false>);
}

}  // namespace m355
