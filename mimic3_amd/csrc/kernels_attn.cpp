// kernels_attn.cpp — relative-position multi-head attention on the fp32 matrix cores.
//
//   s[i,j] = (q_i/sqrt(d)) . k_j + [|j-i|<=W] (q_i/sqrt(d)) . E_k[j-i+W];  masked -> -1e4;  p = softmax_j s
//   o_i    = sum_j p[i,j] v_j + sum_{|j-i|<=W} p[i,j] E_v[j-i+W]
//
// A workgroup of four waves owns 32 query rows of one (batch, head); each wave computes TRANSPOSED score tiles
// S^T[j][i] = K Q^T with v_mfma_f32_32x32x2_f32: in the C/D layout a lane then holds one query column i = lane&31 and 16
// key rows per key tile, so the softmax statistics are in-lane reductions plus one cross-half shuffle, and P^T is directly the B
// operand of the second product O^T[c][i] = V P^T — the probabilities never leave registers (the MFMA k index is
// permuted to "the rows this lane half already holds": k-step (g,m) uses key row 8g+m for lanes 0-31 and 8g+4+m for
// lanes 32-63; V is read with the same permutation).  Both operands of K Q^T are read straight from the [C,T]
// activation layout: 32 consecutive time samples per half-wave (128-byte segments).  The window terms are two tiny
// extra products: (q E_k^T) as a 32-row padded MFMA whose result goes through a 1 KiB LDS table, and E_v^T p_rel with
// the near-diagonal probabilities gathered in the same table.
#include "kernels.h"

namespace m355 {

// Key tile t belongs to wave t % 4, so a wave holds T / 128 score tiles instead of T / 32 (no spills at T = 512, a
// quarter of the dependent MFMA chain).  Softmax statistics and the PV
// partial sums are combined across the waves through LDS in a fixed order (deterministic; key tiles beyond a row's
// length contribute exact zeros, so the result does not depend on how far the batch pads it).
// DP > 0 (= d / 2, the head's channel pairs, known at compile time): EVERY global operand of the kernel — q, E_k, this wave's
// K tiles and V tiles — is loaded up front in one batch (48 (3 + 2 NKW) registers at d = 96), so a workgroup waits for L2
// once instead of once per trip of the two product loops (24 dependent round trips, most of the 30 us a launch took).  The
// MFMA sequence per output is the same as with DP = 0: identical bits.
template <int NKW, int DP = 0>  // key tiles per wave: T <= 128 * NKW
__global__ __launch_bounds__(256) void k_rel_attention_mfma4(const float* __restrict__ qkv, const float* __restrict__ ek,
                                                             const float* __restrict__ ev, const int* __restrict__ len,
                                                             int T, int H, int nh, int W, float* __restrict__ out) {
    DYN_SMEM(float, smem);
    float* tab = smem;                 // [32][32] window table: rel-k logits, later rel probabilities
    float* red = smem + 32 * 32;       // [2][4][32] max / sum per wave and query
    float* ored = red + 2 * 4 * 32;    // [4][16][64] partial O^T tiles
    const int tid = threadIdx.x, lane = tid & 63, w = WAVE_UNIFORM(tid >> 6);
    const int brow = lane >> 5, bcol = lane & 31;
    const int d = H / nh, nrel = 2 * W + 1;
    const int b = blockIdx.z, h = blockIdx.y;
    const int i0 = blockIdx.x * 32;
    const int i = i0 + bcol;
    const int L = len[b];
    const float scale = 1.0f / sqrtf((float)d);
    const float* qb = qkv + ((long)b * 3 * H + h * d) * T;
    const float* kb = qb + (long)H * T;
    const float* vb = qb + (long)2 * H * T;
    const bool iq = i < T;

    f32x16 st[NKW];
    f32x16 rl;
    MI355_UNROLL
    for (int r = 0; r < 16; ++r) rl[r] = 0.0f;
    MI355_UNROLL
    for (int m = 0; m < NKW; ++m)
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) st[m][r] = 0.0f;
    constexpr int NCT = DP > 0 ? (2 * DP + 31) / 32 : 1;  // 32-channel output tiles of O^T (prefetched V)
    float vpre[NCT][NKW][16];
    float evpre[NCT][16];  // wave 0: E_v[r = 2 s2 + brow][channel of this lane], s2 < 16 (window <= 15)
    if constexpr (DP > 0) {
        if (w == 0) {
            MI355_UNROLL
            for (int ct = 0; ct < NCT; ++ct)
                MI355_UNROLL
                for (int s2 = 0; s2 < 16; ++s2) {
                    const int r = 2 * s2 + brow, cr = ct * 32 + bcol;
                    evpre[ct][s2] = ev[(r < nrel ? r : nrel - 1) * d + (cr < d ? cr : 0)];
                }
        }
        float qv[DP], ekv[DP], kv[DP][NKW];
        MI355_UNROLL
        for (int u = 0; u < DP; ++u) {
            const int c = 2 * u + brow;
            const float qraw = qb[(long)c * T + (iq ? i : T - 1)];
            const float eraw = ek[(bcol < nrel ? bcol : nrel - 1) * d + c];
            qv[u] = iq ? qraw * scale : 0.0f;
            ekv[u] = (w == 0 && bcol < nrel) ? eraw : 0.0f;
            MI355_UNROLL
            for (int m = 0; m < NKW; ++m) {
                const int j = (w + 4 * m) * 32 + bcol;
                const float kraw = kb[(long)c * T + (j < T ? j : T - 1)];
                kv[u][m] = j < T ? kraw : 0.0f;
            }
        }
        MI355_UNROLL
        for (int ct = 0; ct < NCT; ++ct) {
            const int cr = ct * 32 + bcol;
            const float* vr = vb + (long)(cr < d ? cr : 0) * T;
            MI355_UNROLL
            for (int m = 0; m < NKW; ++m)
                MI355_UNROLL
                for (int g = 0; g < 4; ++g)
                    MI355_UNROLL
                    for (int q = 0; q < 4; ++q) {
                        const int j = (w + 4 * m) * 32 + 8 * g + 4 * brow + q;
                        vpre[ct][m][4 * g + q] = vr[j < T ? j : T - 1];
                    }
        }
        SCHED_FENCE();
        MI355_UNROLL
        for (int u = 0; u < DP; ++u) {
            if (w == 0) rl = MFMA_32x32x2_F32(ekv[u], qv[u], rl);
            MI355_UNROLL
            for (int m = 0; m < NKW; ++m) st[m] = MFMA_32x32x2_F32(kv[u][m], qv[u], st[m]);
        }
    } else {
        constexpr int U = 4;
        for (int cp0 = 0; cp0 < d / 2; cp0 += U) {
            float qv[U], ekv[U], kv[U][NKW];
            // loads through clamped indices, the out-of-range test applied to the VALUE: a test around each load makes hipcc
            // wait for every load in turn (a chain of ~100 dependent L2 round trips per workgroup: 50 us per launch)
            MI355_UNROLL
            for (int u = 0; u < U; ++u) {
                const int c = 2 * (cp0 + u) + brow;
                const bool cin = c < d;
                const int cc = cin ? c : d - 1;
                const float qraw = qb[(long)cc * T + (iq ? i : T - 1)];
                const float eraw = ek[(bcol < nrel ? bcol : nrel - 1) * d + cc];
                qv[u] = (iq && cin) ? qraw * scale : 0.0f;
                ekv[u] = (w == 0 && bcol < nrel && cin) ? eraw : 0.0f;
                MI355_UNROLL
                for (int m = 0; m < NKW; ++m) {
                    const int j = (w + 4 * m) * 32 + bcol;
                    const float kraw = kb[(long)cc * T + (j < T ? j : T - 1)];
                    kv[u][m] = (j < T && cin) ? kraw : 0.0f;
                }
            }
            MI355_UNROLL
            for (int u = 0; u < U; ++u) {
                if (w == 0) rl = MFMA_32x32x2_F32(ekv[u], qv[u], rl);
                MI355_UNROLL
                for (int m = 0; m < NKW; ++m) st[m] = MFMA_32x32x2_F32(kv[u][m], qv[u], st[m]);
            }
        }
    }
    if (w == 0) {
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) tab[((r & 3) + 8 * (r >> 2) + 4 * brow) * 32 + bcol] = rl[r];
    }
    __syncthreads();

    float mx = -3.0e38f;
    MI355_UNROLL
    for (int m = 0; m < NKW; ++m) {
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) {
            const int j = (w + 4 * m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * brow;
            float sc = st[m][r];
            const int rel = j - i;
            if (rel >= -W && rel <= W) sc += tab[(rel + W) * 32 + bcol];
            if (j >= L || i >= L) sc = -1e4f;
            if (j >= T) sc = -3.0e38f;
            st[m][r] = sc;
            mx = fmaxf(mx, sc);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    if (brow == 0) red[w * 32 + bcol] = mx;
    __syncthreads();  // maxima visible; everyone has read the logits table
    mx = fmaxf(fmaxf(red[bcol], red[32 + bcol]), fmaxf(red[64 + bcol], red[96 + bcol]));
    for (int r = tid >> 5; r < 32; r += 8) tab[r * 32 + bcol] = 0.0f;
    __syncthreads();
    float sum = 0.0f;
    MI355_UNROLL
    for (int m = 0; m < NKW; ++m) {
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) {
            const int j = (w + 4 * m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * brow;
            const float e = j < T ? expf(st[m][r] - mx) : 0.0f;
            st[m][r] = e;
            sum += e;
            const int rel = j - i;
            if (j < T && rel >= -W && rel <= W) tab[(rel + W) * 32 + bcol] = e;
        }
    }
    sum += __shfl_xor(sum, 32);
    if (brow == 0) red[128 + w * 32 + bcol] = sum;
    __syncthreads();
    const float inv = 1.0f / (((red[128 + bcol] + red[160 + bcol]) + red[192 + bcol]) + red[224 + bcol]);

    MI355_UNROLL  // (three straight-line tiles when the head size is a compile-time constant)
    for (int c0 = 0; c0 < (DP > 0 ? 2 * DP : d); c0 += 32) {
        f32x16 o;
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) o[r] = 0.0f;
        const int cr = c0 + bcol;
        const bool cv = cr < d;
        const float* vr = vb + (long)(cv ? cr : 0) * T;
        MI355_UNROLL
        for (int m = 0; m < NKW; ++m) {
            MI355_UNROLL
            for (int g = 0; g < 4; ++g) {
                float vraw[4];
                MI355_UNROLL
                for (int q = 0; q < 4; ++q) {
                    const int j = (w + 4 * m) * 32 + 8 * g + 4 * brow + q;
                    if constexpr (DP > 0) vraw[q] = vpre[c0 / 32][m][4 * g + q];
                    else vraw[q] = vr[j < T ? j : T - 1];
                }
                MI355_UNROLL
                for (int q = 0; q < 4; ++q) {
                    const int j = (w + 4 * m) * 32 + 8 * g + 4 * brow + q;
                    const float vv = (cv && j < T) ? vraw[q] : 0.0f;
                    o = MFMA_32x32x2_F32(vv, st[m][4 * g + q], o);
                }
            }
        }
        if (w == 0) {
            if constexpr (DP > 0) {
                MI355_UNROLL
                for (int s2 = 0; s2 < 16; ++s2) {
                    if (s2 < (nrel + 1) / 2) {
                        const int r = 2 * s2 + brow;
                        const float evv = (cv && r < nrel) ? evpre[c0 / 32][s2] : 0.0f;
                        const float pv = r < nrel ? tab[r * 32 + bcol] : 0.0f;
                        o = MFMA_32x32x2_F32(evv, pv, o);
                    }
                }
            } else {
                for (int s2 = 0; s2 < (nrel + 1) / 2; ++s2) {
                    const int r = 2 * s2 + brow;
                    const float eraw = ev[(r < nrel ? r : nrel - 1) * d + (cv ? cr : 0)];
                    const float evv = (cv && r < nrel) ? eraw : 0.0f;
                    const float pv = r < nrel ? tab[r * 32 + bcol] : 0.0f;
                    o = MFMA_32x32x2_F32(evv, pv, o);
                }
            }
        }
        if (c0 > 0) __syncthreads();  // the previous tile's partials have been consumed
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) ored[(w * 16 + r) * 64 + lane] = o[r];
        __syncthreads();
        if (iq) {
            MI355_UNROLL
            for (int q = 0; q < 4; ++q) {
                const int r = 4 * w + q;
                const float v = ((ored[(0 * 16 + r) * 64 + lane] + ored[(1 * 16 + r) * 64 + lane]) + ored[(2 * 16 + r) * 64 + lane]) +
                                ored[(3 * 16 + r) * 64 + lane];
                const int c = c0 + (r & 3) + 8 * (r >> 2) + 4 * brow;
                if (c < d) out[((long)b * H + h * d + c) * T + i] = v * inv;
            }
        }
    }
}

bool rel_attention_mfma_supported(int T, int H, int n_heads, int window) {
    const int d = H / n_heads;
    return T >= 1 && T <= 512 && (d % 2) == 0 && window >= 0 && 2 * window + 1 <= 32;
}

void launch_rel_attention_mfma(const float* qkv, const float* emb_rel_k, const float* emb_rel_v, const int* len, int B,
                               int T, int H, int n_heads, int window, float* out, hipStream_t s) {
    if (!rel_attention_mfma_supported(T, H, n_heads, window)) throw std::runtime_error("rel_attention_mfma: unsupported shape");
    dim3 grid((T + 31) / 32, n_heads, B);
    const size_t sh4 = (32 * 32 + 2 * 4 * 32 + 4 * 16 * 64) * sizeof(float);
    static const bool no_pre = lab_getenv("MI355VITS_ATTN_NO_PREFETCH") != nullptr;
    // the "_low" / default voices' head: all operands prefetched up front (one L2 wait per workgroup: latency, 256 registers, two
    // workgroups per CU) — on grids of >= 4 workgroups per CU the 76-register form runs six workgroups per CU instead and hides its
    // round trips behind them: 1.01 -> 0.55 ms per step at batch 256, 0.152 -> 0.181 at batch 32 (profiles/r06_attention_ab.txt).
    // The MFMA sequence per output is the same: identical bits, so the choice may follow the grid.
    const bool big = (long)grid.x * grid.y * grid.z >= 4L * current_device_cu_count();
    const bool pre = H / n_heads == 96 && !no_pre && (!big || lab_getenv("MI355VITS_ATTN_PREFETCH"));
    if (T <= 128 && pre) {
        auto k = k_rel_attention_mfma4<1, 48>;
        LAUNCH_KERNEL(k, grid, dim3(256), sh4, s, qkv, emb_rel_k, emb_rel_v, len, T, H, n_heads, window, out);
    } else if (T <= 256 && pre) {
        auto k = k_rel_attention_mfma4<2, 48>;
        LAUNCH_KERNEL(k, grid, dim3(256), sh4, s, qkv, emb_rel_k, emb_rel_v, len, T, H, n_heads, window, out);
    } else if (T <= 128) {
        auto k = k_rel_attention_mfma4<1>;
        LAUNCH_KERNEL(k, grid, dim3(256), sh4, s, qkv, emb_rel_k, emb_rel_v, len, T, H, n_heads, window, out);
    } else if (T <= 256) {
        auto k = k_rel_attention_mfma4<2>;
        LAUNCH_KERNEL(k, grid, dim3(256), sh4, s, qkv, emb_rel_k, emb_rel_v, len, T, H, n_heads, window, out);
    } else {
        auto k = k_rel_attention_mfma4<4>;
        LAUNCH_KERNEL(k, grid, dim3(256), sh4, s, qkv, emb_rel_k, emb_rel_v, len, T, H, n_heads, window, out);
    }
}


// ------------------------------------------------------------------------------------------------
// k_rel_attention_stream — the same function for any sequence length: keys are streamed, not held.
// Layout of k_rel_attention_mfma4 (four waves, 32 query rows, one (batch, head); transposed score tiles S^T = K Q^T on
// v_mfma_f32_32x32x2_f32, P^T the B operand of O^T = V P^T straight from registers), but wave w walks the key tiles
// t = w, w + 4, .. < ceil(L_b / 32) with an online softmax: a running max and sum per query column (in-lane plus one
// cross-half shuffle), the O^T accumulators rescaled when the max grows.  The next tile's K and V fragments are loaded
// while the current tile is in the matrix pipe.  The window terms: the q E_k^T logits live in a 1 KiB LDS table (as in
// mfma4) and are added on the (at most three) key tiles that touch the query tile's band; the raw near-diagonal logits go
// to a second table, and E_v^T p_rel is one small product against exp(logit - final max) at the end.  The four waves'
// (max, sum, O^T) are combined through LDS in a fixed order: deterministic.  Key tiles past L_b are never read and masked
// keys inside the last tile add exact zeros, so a row's result does not depend on tx_max.  Query rows at or past L_b are
// written as zeros (their values never reach a valid frame: the attention's consumer is the 1x1 o-projection, and every
// later length-mixing op masks).  LDS: the two window tables and the combine buffers (~25 KiB); nothing sized by T.
// DP: channel pairs held per lane (the head width d <= 2 DP; channels past d are zero).
template <int DP>
__global__ __launch_bounds__(256) void k_rel_attention_stream(const float* __restrict__ qkv, const float* __restrict__ ek,
                                                              const float* __restrict__ ev, const int* __restrict__ len,
                                                              int T, int H, int nh, int W, float* __restrict__ out) {
    constexpr int NCT = (2 * DP + 31) / 32;  // 32-channel tiles of O^T
    DYN_SMEM(float, smem);
    float* tabk = smem;              // [32][32] rel-k logits q_i . E_k[r]
    float* tabp = smem + 32 * 32;    // [32][32] raw near-diagonal logits (-3e38: no such key)
    float* red = tabp + 32 * 32;     // [2][4][32] max / sum per wave and query
    float* ored = red + 2 * 4 * 32;  // [4][16][64] partial O^T tiles
    const int tid = threadIdx.x, lane = tid & 63, w = WAVE_UNIFORM(tid >> 6);
    const int brow = lane >> 5, bcol = lane & 31;
    const int d = H / nh, nrel = 2 * W + 1;
    const int b = blockIdx.z, h = blockIdx.y;
    const int i0 = blockIdx.x * 32;
    const int i = i0 + bcol;
    const int L = len[b] < T ? len[b] : T;
    float* ob = out + ((long)b * H + h * d) * T;
    if (i0 >= L) {  // a query tile of padding only
        for (int e = tid; e < 32 * d; e += 256) {
            const int c = e >> 5, ii = i0 + (e & 31);
            if (ii < T) ob[(long)c * T + ii] = 0.0f;
        }
        return;
    }
    const float scale = 1.0f / sqrtf((float)d);
    const float* qb = qkv + ((long)b * 3 * H + h * d) * T;
    const float* kb = qb + (long)H * T;
    const float* vb = qb + (long)2 * H * T;
    const bool iq = i < L;
    const int ntile = (L + 31) / 32;
    const int qt = i0 / 32;

    float qv[DP];
    f32x16 rl;
    MI355_UNROLL
    for (int r = 0; r < 16; ++r) rl[r] = 0.0f;
    MI355_UNROLL
    for (int u = 0; u < DP; ++u) {
        const int c = 2 * u + brow;
        const int cc = c < d ? c : d - 1;
        const float qraw = qb[(long)cc * T + (iq ? i : L - 1)];
        const float eraw = ek[(bcol < nrel ? bcol : nrel - 1) * d + cc];
        qv[u] = (iq && c < d) ? qraw * scale : 0.0f;
        const float ekv = (bcol < nrel && c < d) ? eraw : 0.0f;
        if (w == 0) rl = MFMA_32x32x2_F32(ekv, qv[u], rl);
    }
    if (w == 0) {
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) tabk[((r & 3) + 8 * (r >> 2) + 4 * brow) * 32 + bcol] = rl[r];
    }
    for (int e = tid; e < 32 * 32; e += 256) tabp[e] = -3.0e38f;

    // this wave's K / V fragments of key tile t (clamped indices, the range test applied to the value)
    auto load_tile = [&](int t, float (&kv)[DP], float (&vv)[NCT][16]) {
        const int tc = t < ntile ? t : ntile - 1;
        const int j = tc * 32 + bcol;
        const bool jin = j < L;
        const int jc = jin ? j : L - 1;
        MI355_UNROLL
        for (int u = 0; u < DP; ++u) {
            const int c = 2 * u + brow;
            const float kraw = kb[(long)(c < d ? c : d - 1) * T + jc];
            kv[u] = (jin && c < d) ? kraw : 0.0f;
        }
        MI355_UNROLL
        for (int ct = 0; ct < NCT; ++ct) {
            const int cr = ct * 32 + bcol;
            const float* vr = vb + (long)(cr < d ? cr : d - 1) * T;
            MI355_UNROLL
            for (int g = 0; g < 4; ++g)
                MI355_UNROLL
                for (int q = 0; q < 4; ++q) {
                    const int jv = tc * 32 + 8 * g + 4 * brow + q;
                    const float vraw = vr[jv < L ? jv : L - 1];
                    vv[ct][4 * g + q] = (cr < d && jv < L) ? vraw : 0.0f;
                }
        }
    };

    f32x16 o[NCT];
    MI355_UNROLL
    for (int ct = 0; ct < NCT; ++ct)
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) o[ct][r] = 0.0f;
    float mx = -3.0e38f, sum = 0.0f;
    float kc[DP], vc[NCT][16];
    load_tile(w, kc, vc);
    __syncthreads();  // the rel-k table and the cleared band table are visible

    for (int t = w; t < ntile; t += 4) {
        float kn[DP], vn[NCT][16];
        load_tile(t + 4, kn, vn);  // in flight while this tile is in the matrix pipe
        f32x16 s;
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
        MI355_UNROLL
        for (int u = 0; u < DP; ++u) s = MFMA_32x32x2_F32(kc[u], qv[u], s);
        const bool band = t >= qt - 1 && t <= qt + 1;
        float tmx = -3.0e38f;
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) {
            const int j = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * brow;
            float sc = s[r];
            if (band) {
                const int rel = j - i;
                if (rel >= -W && rel <= W) {
                    sc += tabk[(rel + W) * 32 + bcol];
                    if (j < L) tabp[(rel + W) * 32 + bcol] = sc;
                }
            }
            if (j >= L) sc = -3.0e38f;
            s[r] = sc;
            tmx = fmaxf(tmx, sc);
        }
        tmx = fmaxf(tmx, __shfl_xor(tmx, 32));
        const float mnew = fmaxf(mx, tmx);
        const float alpha = expf(mx - mnew);
        mx = mnew;
        sum *= alpha;
        MI355_UNROLL
        for (int ct = 0; ct < NCT; ++ct)
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) o[ct][r] *= alpha;
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) {
            const float e = expf(s[r] - mx);
            s[r] = e;
            sum += e;
        }
        MI355_UNROLL
        for (int ct = 0; ct < NCT; ++ct)
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) o[ct] = MFMA_32x32x2_F32(vc[ct][r], s[r], o[ct]);
        MI355_UNROLL
        for (int u = 0; u < DP; ++u) kc[u] = kn[u];
        MI355_UNROLL
        for (int ct = 0; ct < NCT; ++ct)
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) vc[ct][r] = vn[ct][r];
    }

    // combine the four waves in a fixed order
    sum += __shfl_xor(sum, 32);
    if (brow == 0) red[w * 32 + bcol] = mx;
    __syncthreads();  // maxima and the band table visible
    const float M = fmaxf(fmaxf(red[bcol], red[32 + bcol]), fmaxf(red[64 + bcol], red[96 + bcol]));
    const float f = expf(mx - M);  // 0 for a wave without key tiles
    if (brow == 0) red[128 + w * 32 + bcol] = sum * f;
    __syncthreads();
    const float inv = 1.0f / (((red[128 + bcol] + red[160 + bcol]) + red[192 + bcol]) + red[224 + bcol]);
    MI355_UNROLL
    for (int ct = 0; ct < NCT; ++ct) {
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) o[ct][r] *= f;
        const int cr = ct * 32 + bcol;
        const bool cv = cr < d;
        if (w == 0) {
            for (int s2 = 0; s2 < (nrel + 1) / 2; ++s2) {
                const int r = 2 * s2 + brow;
                const float eraw = ev[(r < nrel ? r : nrel - 1) * d + (cv ? cr : 0)];
                const float evv = (cv && r < nrel) ? eraw : 0.0f;
                const float pv = r < nrel ? expf(tabp[r * 32 + bcol] - M) : 0.0f;
                o[ct] = MFMA_32x32x2_F32(evv, pv, o[ct]);
            }
        }
        if (ct > 0) __syncthreads();  // the previous tile's partials have been consumed
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) ored[(w * 16 + r) * 64 + lane] = o[ct][r];
        __syncthreads();
        if (i < T) {
            MI355_UNROLL
            for (int q = 0; q < 4; ++q) {
                const int r = 4 * w + q;
                const float v = ((ored[(0 * 16 + r) * 64 + lane] + ored[(1 * 16 + r) * 64 + lane]) + ored[(2 * 16 + r) * 64 + lane]) +
                                ored[(3 * 16 + r) * 64 + lane];
                const int c = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * brow;
                if (c < d) ob[(long)c * T + i] = iq ? v * inv : 0.0f;
            }
        }
    }
}

bool rel_attention_stream_supported(int H, int n_heads, int window) {
    const int d = H / n_heads;
    return d >= 2 && d <= 128 && (d % 2) == 0 && window >= 0 && 2 * window + 1 <= 32;
}

void launch_rel_attention_stream(const float* qkv, const float* emb_rel_k, const float* emb_rel_v, const int* len, int B,
                                 int T, int H, int n_heads, int window, float* out, hipStream_t s) {
    if (!rel_attention_stream_supported(H, n_heads, window))
        throw std::runtime_error("rel_attention_stream: needs an even head width <= 128 and a relative window <= 15");
    const int d = H / n_heads;
    dim3 grid((T + 31) / 32, n_heads, B);
    const size_t sh = (2 * 32 * 32 + 2 * 4 * 32 + 4 * 16 * 64) * sizeof(float);
    if (d <= 16) {
        LAUNCH_KERNEL(k_rel_attention_stream<8>, grid, dim3(256), sh, s, qkv, emb_rel_k, emb_rel_v, len, T, H, n_heads, window, out);
    } else if (d <= 32) {
        LAUNCH_KERNEL(k_rel_attention_stream<16>, grid, dim3(256), sh, s, qkv, emb_rel_k, emb_rel_v, len, T, H, n_heads, window, out);
    } else if (d <= 64) {
        LAUNCH_KERNEL(k_rel_attention_stream<32>, grid, dim3(256), sh, s, qkv, emb_rel_k, emb_rel_v, len, T, H, n_heads, window, out);
    } else if (d <= 96) {
        LAUNCH_KERNEL(k_rel_attention_stream<48>, grid, dim3(256), sh, s, qkv, emb_rel_k, emb_rel_v, len, T, H, n_heads, window, out);
    } else {
        LAUNCH_KERNEL(k_rel_attention_stream<64>, grid, dim3(256), sh, s, qkv, emb_rel_k, emb_rel_v, len, T, H, n_heads, window, out);
    }
}

}  // namespace m355
