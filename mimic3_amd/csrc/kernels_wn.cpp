// kernels_wn.cpp — one WaveNet layer of the residual-coupling flow as ONE kernel.
//
//   a  = in_l(h) [+ cond_l(g)]              k=5 conv, H -> 2H
//   u  = tanh(a[:H]) * sigmoid(a[H:])
//   rs = res_skip_l(u)                      1x1 conv, H -> 2H (last layer: H -> H)
//   h' = (h + rs[:H]) * mask ;  skip += rs[H:]        (last layer: skip += rs)
//
// Layer-at-a-time this is two launches and moves u (H x T) through HBM; here a workgroup owns 32 time columns of ALL
// channels: the h tile (+halo) is staged once into LDS, wave p of the H/32 waves computes gate pair p (rows c and
// H + c land in the same lane, so the gate is pure register math), u goes to a second LDS tile, and the same waves
// run the 1x1 conv from it: wave p produces rows {c, H + c} again, i.e. exactly its own slice of h' and of skip.
// Both MFMA operand streams follow the pipeline of kernels_mrf.cpp (A: 8-register rings four steps ahead from
// L2; B: LDS, one step ahead; taps unrolled).  h is read from one buffer and written to another (neighbouring
// workgroups read each other's halo columns).
#include "kernels.h"
#include "b3.h"

namespace m355 {

// two output tiles (A streams wp0 / wp1), one 32-column tile, K taps x CP channel pairs, accumulate into acc0/acc1
template <int CP>
__device__ __forceinline__ void wn_mfma2(f32x16& acc0, f32x16& acc1, const float* __restrict__ wp0,
                                         const float* __restrict__ wp1, const float* __restrict__ xw, int LD, int K, int dil) {
    static_assert(CP % 8 == 0, "channel pairs per tap must be a multiple of 8");
    const int ld2 = 2 * LD;
    float r0[8], r1[8];
    MI355_UNROLL
    for (int u = 0; u < 4; ++u) { r0[u] = wp0[u * 64]; r1[u] = wp1[u * 64]; }
    float bb[2];
    bb[0] = xw[0];
    const float* g0 = wp0;
    const float* g1 = wp1;
    for (int k = 0; k < K; ++k) {
        MI355_UNROLL
        for (int cp0 = 0; cp0 < CP; cp0 += 8) {
            const float* base = xw + k * dil + cp0 * ld2;
            const bool last = (k == K - 1) && (cp0 + 8 == CP);
            const float* nbase = last ? base : ((cp0 + 8 < CP) ? base + 8 * ld2 : xw + (k + 1) * dil);
            const float* h0 = last ? g0 - 8 * 64 : g0;  // the last group prefetches harmlessly from itself
            const float* h1 = last ? g1 - 8 * 64 : g1;
            MI355_UNROLL
            for (int u = 0; u < 8; ++u) {
                const float a0 = r0[u], a1 = r1[u];
                r0[(u + 4) & 7] = (u < 4) ? g0[(u + 4) * 64] : h0[(u + 4) * 64];
                r1[(u + 4) & 7] = (u < 4) ? g1[(u + 4) * 64] : h1[(u + 4) * 64];
                bb[(u + 1) & 1] = (u < 7) ? base[(u + 1) * ld2] : nbase[0];
                acc0 = MFMA_32x32x2_F32(a0, bb[u & 1], acc0);
                acc1 = MFMA_32x32x2_F32(a1, bb[u & 1], acc1);
                SCHED_FENCE();
            }
            g0 += 8 * 64;
            g1 += 8 * 64;
        }
    }
}

template <int NP>  // H = 32 * NP hidden channels, NP waves
__global__ __launch_bounds__(64 * NP) MIN_WAVES_PER_SIMD(NP > 1 ? 5 : 1) void k_wn_layer(WnArgs a) {
    constexpr int H = 32 * NP;
    constexpr int CP = H / 2;
    constexpr int T_B = 32;
    DYN_SMEM(float, smem);
    const int LDX = a.ldx;
    float* X = smem;  // [H][LDX] h tile (+halo), zero outside the row
    float* U = smem;  // [H][32]  gated activations; reuses the h tile's space once the in-layer conv is done
    const int tid = threadIdx.x, lane = tid & 63, p = WAVE_UNIFORM(tid >> 6);
    const int brow = lane >> 5, bcol = lane & 31;
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * T_B;
    int len = a.len ? a.len[b] : a.T;
    if (len > a.T) len = a.T;
    const int pad = (a.K - 1) / 2 * a.dil;
    const int tlo = t0 - pad;
    const int ts = tlo >= 0 ? (tlo & ~3) : -(((-tlo) + 3) & ~3);
    const int toff = tlo - ts;

    if (!(LAB_ABLATE(a) & 2)) {   // stage h[b, :, ts : ts + LDX)
        const float* hb = a.h_in + (long)b * a.h_bs;
        if (a.vec) {
            const int ld4 = LDX >> 2;
            for (int idx = tid; idx < H * ld4; idx += 64 * NP) {
                const int r = idx / ld4, c4 = idx - r * ld4;
                const int t = ts + 4 * c4;
                const float* row = hb + (long)r * a.h_ld;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (t >= 0 && t + 3 < len) {
                    v = *reinterpret_cast<const float4*>(row + t);
                } else {
                    if (t >= 0 && t < len) v.x = row[t];
                    if (t + 1 >= 0 && t + 1 < len) v.y = row[t + 1];
                    if (t + 2 >= 0 && t + 2 < len) v.z = row[t + 2];
                    if (t + 3 >= 0 && t + 3 < len) v.w = row[t + 3];
                }
                *reinterpret_cast<float4*>(X + r * LDX + 4 * c4) = v;
            }
        } else {
            for (int idx = tid; idx < H * LDX; idx += 64 * NP) {
                const int r = idx / LDX, c = idx - r * LDX;
                const int t = ts + c;
                X[idx] = (t >= 0 && t < len) ? hb[(long)r * a.h_ld + t] : 0.0f;
            }
        }
    }
    __syncthreads();

    const int t = t0 + bcol;
    // ---- in-layer conv (gate pair p) + gate
    f32x16 gate, hres;
    {
        f32x16 acc0, acc1;
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) {
            const int c = 32 * p + (r & 3) + 8 * (r >> 2) + 4 * brow;
            float v0 = a.b_in[c], v1 = a.b_in[H + c];
            if (a.cond) { v0 += a.cond[(long)b * a.cond_bs + c]; v1 += a.cond[(long)b * a.cond_bs + H + c]; }
            acc0[r] = v0;
            acc1[r] = v1;
        }
        const float* wp0 = a.w_in + (long)(2 * p) * a.K * CP * 64 + lane;
        const float* wp1 = wp0 + (long)a.K * CP * 64;
        if (!(LAB_ABLATE(a) & 1)) wn_mfma2<CP>(acc0, acc1, wp0, wp1, X + brow * LDX + toff + bcol, LDX, a.K, a.dil);
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) {
            gate[r] = wn_gate_f(acc0[r], acc1[r]);
            const int c = 32 * p + (r & 3) + 8 * (r >> 2) + 4 * brow;
            hres[r] = X[c * LDX + toff + pad + bcol];
        }
    }
    __syncthreads();  // every wave is done with the h tile: U takes its place
    MI355_UNROLL
    for (int r = 0; r < 16; ++r) {
        const int c = 32 * p + (r & 3) + 8 * (r >> 2) + 4 * brow;
        U[c * 32 + bcol] = gate[r];
    }
    __syncthreads();
    // ---- res/skip 1x1 conv: rows c (-> h') and H + c (-> skip); last layer: rows c -> skip
    {
        const bool two = a.Crs == 2 * H;
        f32x16 acc0, acc1;
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) {
            const int c = 32 * p + (r & 3) + 8 * (r >> 2) + 4 * brow;
            acc0[r] = a.b_rs[c];
            acc1[r] = two ? a.b_rs[H + c] : 0.0f;
        }
        const float* wp0 = a.w_rs + (long)p * CP * 64 + lane;
        const float* wp1 = two ? a.w_rs + (long)(NP + p) * CP * 64 + lane : wp0;
        if (!(LAB_ABLATE(a) & 1)) wn_mfma2<CP>(acc0, acc1, wp0, wp1, U + brow * 32 + bcol, 32, 1, 0);
        if (t < a.T && !((LAB_ABLATE(a) & 4) && acc0[0] != 1.2345f)) {
            const bool live = t < len;
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * p + (r & 3) + 8 * (r >> 2) + 4 * brow;
                float* sp = a.skip + (long)b * a.s_bs + (long)c * a.s_ld + t;
                if (two) {
                    a.h_out[(long)b * a.h_bs + (long)c * a.h_ld + t] = live ? hres[r] + acc0[r] : 0.0f;  // same order as k_wn_layer_h192
                    *sp = a.skip_init ? acc1[r] : *sp + acc1[r];
                } else {
                    *sp = a.skip_init ? acc0[r] : *sp + acc0[r];
                }
            }
        }
    }
}


// MT output tiles (A streams wp[m]), one 32-column tile, K taps x CP channel pairs
template <int MT, int CP>
__device__ __forceinline__ void wn_mfma(f32x16 (&acc)[MT], const float* const (&wp)[MT], const float* __restrict__ xw, int LD,
                                        int K, int dil) {
    static_assert(CP % 8 == 0, "channel pairs per tap must be a multiple of 8");
    const int ld2 = 2 * LD;
    float ra[MT][8];
    const float* g[MT];
    MI355_UNROLL
    for (int m = 0; m < MT; ++m) {
        g[m] = wp[m];
        MI355_UNROLL
        for (int u = 0; u < 4; ++u) ra[m][u] = wp[m][u * 64];
    }
    float bb[2];
    bb[0] = xw[0];
    for (int k = 0; k < K; ++k) {
        MI355_UNROLL
        for (int cp0 = 0; cp0 < CP; cp0 += 8) {
            const float* base = xw + k * dil + cp0 * ld2;
            const bool last = (k == K - 1) && (cp0 + 8 == CP);
            const float* nbase = last ? base : ((cp0 + 8 < CP) ? base + 8 * ld2 : xw + (k + 1) * dil);
            const int back = last ? 8 * 64 : 0;  // the last group prefetches harmlessly from itself
            MI355_UNROLL
            for (int u = 0; u < 8; ++u) {
                float av[MT];
                MI355_UNROLL
                for (int m = 0; m < MT; ++m) {
                    av[m] = ra[m][u];
                    ra[m][(u + 4) & 7] = (u < 4) ? g[m][(u + 4) * 64] : (g[m] - back)[(u + 4) * 64];
                }
                bb[(u + 1) & 1] = (u < 7) ? base[(u + 1) * ld2] : nbase[0];
                MI355_UNROLL
                for (int m = 0; m < MT; ++m) acc[m] = MFMA_32x32x2_F32(av[m], bb[u & 1], acc[m]);
                SCHED_FENCE();
            }
            MI355_UNROLL
            for (int m = 0; m < MT; ++m) g[m] += 8 * 64;
        }
    }
}

// Same product with the B operand packed for 16-byte LDS reads: the tile is stored [channel-pair group of 4][brow][column][4]
// (element (c, col) at (((c >> 3) * 2 + (c & 1)) * LD + col) * 4 + ((c >> 1) & 3)), so one ds_read_b128 delivers a
// lane's B fragments for four consecutive k-steps — a quarter of the LDS instructions of the b32 version, worth ~10 % of
// the loop for this tile shape (tools/mfma_ceiling.hip, "B4").  x4 points at (group 0, this lane's brow, its column).
template <int MT, int CP>
__device__ __forceinline__ void wn_mfma_b4(f32x16 (&acc)[MT], const float* const (&wp)[MT], const float4* __restrict__ x4, int LD,
                                           int K, int dil) {
    static_assert(CP % 8 == 0, "channel pairs per tap must be a multiple of 8");
    float ra[MT][8];
    const float* g[MT];
    MI355_UNROLL
    for (int m = 0; m < MT; ++m) {
        g[m] = wp[m];
        MI355_UNROLL
        for (int u = 0; u < 4; ++u) ra[m][u] = wp[m][u * 64];
    }
    float4 b0 = x4[0], b1 = b0;
    for (int k = 0; k < K; ++k) {
        MI355_UNROLL
        for (int cp0 = 0; cp0 < CP; cp0 += 8) {
            const float4* base = x4 + k * dil + (cp0 >> 2) * 2 * LD;
            const bool last = (k == K - 1) && (cp0 + 8 == CP);
            const float4* nbase = last ? base : ((cp0 + 8 < CP) ? base + 4 * LD : x4 + (k + 1) * dil);
            const int back = last ? 8 * 64 : 0;  // the last group prefetches harmlessly from itself
            MI355_UNROLL
            for (int u = 0; u < 8; ++u) {
                float av[MT];
                MI355_UNROLL
                for (int m = 0; m < MT; ++m) {
                    av[m] = ra[m][u];
                    ra[m][(u + 4) & 7] = (u < 4) ? g[m][(u + 4) * 64] : (g[m] - back)[(u + 4) * 64];
                }
                if (u == 0) b1 = base[2 * LD];  // second group of four of this step group
                const float4 bq = u < 4 ? b0 : b1;
                const float bv = (u & 3) == 0 ? bq.x : ((u & 3) == 1 ? bq.y : ((u & 3) == 2 ? bq.z : bq.w));
                if (u == 4) b0 = nbase[0];      // first group of the next step group (b0 is free from here on)
                MI355_UNROLL
                for (int m = 0; m < MT; ++m) acc[m] = MFMA_32x32x2_F32(av[m], bv, acc[m]);
                SCHED_FENCE();
            }
            MI355_UNROLL
            for (int m = 0; m < MT; ++m) g[m] += 8 * 64;
        }
    }
}

// H = 192: four waves, each three of the twelve 32-row tiles of either conv, 32 time columns per workgroup.  With
// three MFMA tiles per wave and three workgroups per CU every SIMD carries exactly three waves (six waves of two
// tiles leave the SIMDs 5/5/4/4), and fewer, fatter waves run the operand streams closer to the matrix-core rate
// (tools/mfma_ceiling.hip).  The price: tanh and sigmoid rows of a gate pair now sit in different waves, so the raw
// in-layer result takes a round trip through LDS (it reuses the h tile's space) before gating.
template <int NW>  // waves per workgroup: 4 (3 tiles each) or 12 (1 tile each: shortest MFMA chain, for tiny grids)
__global__ __launch_bounds__(64 * NW) MIN_WAVES_PER_SIMD(3) void k_wn_layer_h192(WnArgs a) {
    constexpr int H = 192, CP = 96, NTILE = 12, MT = NTILE / NW, NTH = 64 * NW;
    static_assert(NW == 4 || NW == 12, "wave count");
    DYN_SMEM(float, smem);
    const int LDX = a.ldx;
    float* X = smem;  // [H][LDX] h tile (+halo), zero outside the row; later A [2H][32] raw in-layer result, U = A[:H]
    const int tid = threadIdx.x, lane = tid & 63, w = WAVE_UNIFORM(tid >> 6);
    const int brow = lane >> 5, bcol = lane & 31;
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * 32;
    int len = a.len ? a.len[b] : a.T;
    if (len > a.T) len = a.T;
    const int pad = (a.K - 1) / 2 * a.dil;
    const int tlo = t0 - pad;
    const int ts = tlo >= 0 ? (tlo & ~3) : -(((-tlo) + 3) & ~3);
    const int toff = tlo - ts;
    const float* hb = a.h_in + (long)b * a.h_bs;
    // LDS index of element (channel c, column col) of a tile with `ld` columns: see wn_mfma_b4
    auto pk = [](int c, int col, int ld) { return ((((c >> 3) * 2 + (c & 1)) * ld + col) << 2) + ((c >> 1) & 3); };
    if (!(LAB_ABLATE(a) & 2)) {
        // one float4 of LDS = four channels (8g + 2q + brow, q = 0..3) at one column.  A thread moves a 4 x 4 block: four
        // 16-byte loads along time (one per channel), transposed in registers, four 16-byte LDS stores (one per column)
        const int ld4 = LDX >> 2;
        for (int idx = tid; idx < (H / 4) * ld4; idx += NTH) {
            const int gb = idx / ld4, c4 = idx - gb * ld4;  // gb = g * 2 + brow
            const int c0 = (gb >> 1) * 8 + (gb & 1);
            const int tt = ts + 4 * c4;
            float v[4][4];
            MI355_UNROLL
            for (int q = 0; q < 4; ++q) {
                const float* row = hb + (long)(c0 + 2 * q) * a.h_ld;
                if (a.vec && tt >= 0 && tt + 3 < len) {
                    const float4 r4 = *reinterpret_cast<const float4*>(row + tt);
                    v[q][0] = r4.x; v[q][1] = r4.y; v[q][2] = r4.z; v[q][3] = r4.w;
                } else {
                    MI355_UNROLL
                    for (int j = 0; j < 4; ++j) v[q][j] = (tt + j >= 0 && tt + j < len) ? row[tt + j] : 0.0f;
                }
            }
            MI355_UNROLL
            for (int j = 0; j < 4; ++j)
                reinterpret_cast<float4*>(X)[gb * LDX + 4 * c4 + j] = make_float4(v[0][j], v[1][j], v[2][j], v[3][j]);
        }
    }
    __syncthreads();

    const int t = t0 + bcol;
    const bool two = a.Crs == 2 * H;
    f32x16 hres[MT];
    const float* condp = a.cond ? a.cond + (long)b * a.cond_bs : a.b_in;
    const float cond_on = a.cond ? 1.0f : 0.0f;
    {   // ---- in-layer conv: packed tiles 3w .. 3w+2 (tile 2p = rows 32p.. of the tanh half, 2p+1 = same rows, sigmoid half)
        f32x16 acc[MT];
        const float* wp[MT];
        MI355_UNROLL
        for (int m = 0; m < MT; ++m) {
            const int q = MT * w + m;
            const int row0 = ((q & 1) ? H : 0) + 32 * (q >> 1);
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) {
                const int c = row0 + (r & 3) + 8 * (r >> 2) + 4 * brow;
                // unconditional loads (a test per element serialises them); without conditioning the second term is
                // +0.0f * bias: the sum is unchanged bit for bit
                acc[m][r] = a.b_in[c] + cond_on * condp[c];
            }
            wp[m] = a.w_in + (long)q * a.K * CP * 64 + lane;
        }
        if (!(LAB_ABLATE(a) & 1))
            wn_mfma_b4<MT, CP>(acc, wp, reinterpret_cast<const float4*>(X) + brow * LDX + toff + bcol, LDX, a.K, a.dil);
        if (two && MT * w < NTILE / 2) {  // the residual input of this wave's h' tiles, while the h tile is still there
            MI355_UNROLL
            for (int m = 0; m < MT; ++m)
                MI355_UNROLL
                for (int r = 0; r < 16; ++r)
                    hres[m][r] = X[pk(32 * (MT * w + m) + (r & 3) + 8 * (r >> 2) + 4 * brow, toff + pad + bcol, LDX)];
        }
        __syncthreads();  // every wave is done with the h tile
        MI355_UNROLL
        for (int m = 0; m < MT; ++m) {
            const int q = MT * w + m;
            const int row0 = ((q & 1) ? H : 0) + 32 * (q >> 1);
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) {  // both halves in the packed layout of U, so the gate below works in place
                const int cc = 32 * (q >> 1) + (r & 3) + 8 * (r >> 2) + 4 * brow;
                X[((q & 1) ? H * 32 : 0) + pk(cc, bcol, 32)] = acc[m][r];
            }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < H * 32; idx += NTH) {  // gate in place: U[c][t] = tanh(A[c][t]) * sigmoid(A[H + c][t])
        const float at = X[idx], as = X[H * 32 + idx];
        const float gate = wn_gate_f(at, as);
        X[idx] = gate;
    }
    __syncthreads();
    // ---- res/skip 1x1 conv: row tiles q < 6 -> h', q >= 6 -> skip (last layer: 6 tiles, all -> skip)
    const float4* U = reinterpret_cast<const float4*>(X) + brow * 32 + bcol;
    const bool live = t < len;
    auto finish = [&](const f32x16& acc, int q, const f32x16& hr) {
        if (t >= a.T || ((LAB_ABLATE(a) & 4) && acc[0] != 1.2345f)) return;
        if (two && 32 * q < H) {  // wave-uniform: a tile lies entirely in the h' half or in the skip half
            MI355_UNROLL
            for (int r = 0; r < 16; ++r)
                a.h_out[(long)b * a.h_bs + (long)(32 * q + (r & 3) + 8 * (r >> 2) + 4 * brow) * a.h_ld + t] = live ? hr[r] + acc[r] : 0.0f;
            return;
        }
        // skip: the 16 old values under one test, in flight together (a test per element serialises the loads)
        float* sp = a.skip + (long)b * a.s_bs + (long)(32 * q - (two ? H : 0) + 4 * brow) * a.s_ld + t;
        float old[16];
        if (!a.skip_init) {
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) old[r] = sp[(long)((r & 3) + 8 * (r >> 2)) * a.s_ld];
        }
        MI355_UNROLL
        for (int r = 0; r < 16; ++r) sp[(long)((r & 3) + 8 * (r >> 2)) * a.s_ld] = a.skip_init ? acc[r] : old[r] + acc[r];
    };
    if (two) {
        f32x16 acc[MT];
        const float* wp[MT];
        MI355_UNROLL
        for (int m = 0; m < MT; ++m) {
            const int q = MT * w + m;
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) acc[m][r] = a.b_rs[32 * q + (r & 3) + 8 * (r >> 2) + 4 * brow];
            wp[m] = a.w_rs + (long)q * CP * 64 + lane;
        }
        if (!(LAB_ABLATE(a) & 1)) wn_mfma_b4<MT, CP>(acc, wp, U, 32, 1, 0);
        MI355_UNROLL
        for (int m = 0; m < MT; ++m) finish(acc[m], MT * w + m, hres[m]);
    } else if (NW == 12) {  // 6 tiles, one per wave
        if (w < 6) {
            f32x16 a1[1];
            const float* w1[1] = {a.w_rs + (long)w * CP * 64 + lane};
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) a1[0][r] = a.b_rs[32 * w + (r & 3) + 8 * (r >> 2) + 4 * brow];
            if (!(LAB_ABLATE(a) & 1)) wn_mfma_b4<1, CP>(a1, w1, U, 32, 1, 0);
            finish(a1[0], w, hres[0]);
        }
    } else {  // 6 tiles: waves 0, 1 take two, waves 2, 3 one
        const int nq = w < 2 ? 2 : 1;
        f32x16 acc[2];
        const float* wp[2];
        MI355_UNROLL
        for (int m = 0; m < 2; ++m) {
            const int q = m == 0 ? w : w + 4;
            const int qq = q < 6 ? q : w;
            MI355_UNROLL
            for (int r = 0; r < 16; ++r) acc[m][r] = a.b_rs[32 * qq + (r & 3) + 8 * (r >> 2) + 4 * brow];
            wp[m] = a.w_rs + (long)qq * CP * 64 + lane;
        }
        if (!(LAB_ABLATE(a) & 1)) {
            if (nq == 2) {
                wn_mfma_b4<2, CP>(acc, wp, U, 32, 1, 0);
            } else {
                f32x16 a1[1] = {acc[0]};
                const float* w1[1] = {wp[0]};
                wn_mfma_b4<1, CP>(a1, w1, U, 32, 1, 0);
                acc[0] = a1[0];
            }
        }
        finish(acc[0], w, hres[0]);
        if (nq == 2) finish(acc[1], w + 4, hres[0]);
    }
}

// ------------------------------------------------------------------------------------------------
// The same WaveNet layer in MATH_BF16X3 (f32 operands split 3 x bf16, six products on the bf16 matrix cores: v_mfma_f32_16x16x32_bf16
// since the shape A/B of profiles/wn_shape_ab.txt, v_mfma_f32_32x32x16_bf16 before it and still in MATH_F16X2 — WnTiles below).
// At 16x the f32 MFMA rate the 32-column geometry above would be bound by streaming the layer's weights (every
// workgroup reads all of them; 32 columns of reuse), so the tile is turned around:
//   * a workgroup owns 96 time columns (32 / 128: wn_layer_b3_column_tiles) of ALL 2H = 384 in-layer rows: B x T / 96 workgroups (256 for
//     the batch-32 bench shape: one per CU), four waves = one per SIMD with the whole 512-register file each;
//   * a wave computes 96 rows x all columns (32x32x16: 3 row tiles x 3 column tiles, 16x16x32: 6 x 6): every weight fragment feeds all
//     the column tiles, every activation fragment all the wave's row tiles;
//   * h (+halo) is split into three bf16 planes once while it is staged (b3.h); the in-layer result is gated in the accumulators'
//     registers, split, and stored into the dead h planes' space as the B operand of the res/skip conv; u never leaves the CU.
// LDS: the h planes, 3 x 192 ch x (columns + halo) x 2 B = 117 KiB at 96 columns, 153 KiB at 128.
// ------------------------------------------------------------------------------------------------
constexpr int WNB_H = 192, WNB_NG = WNB_H / 16;
constexpr int WNB_RING = 4;  // weight-fragment buffers of the four-wave form
constexpr int WNB_EPI = 1;   // epilogue form of the four-wave, 96-column kernel (template parameter EP; 1 since round 5: profiles/r05_wn_epilogue_ab.txt)
// phase clocks of one workgroup (lab build, MI355VITS_WN_ABLATE bit 64): shader-clock deltas printed by workgroup (3, 5), wave 0
#if defined(MI355_LAB) && !defined(MI355_EMU)
#define WN_TS_DECL() long long wn_ts[7] = {0, 0, 0, 0, 0, 0, 0}
#define WN_TS(i) do { if (a.ablate & 64) wn_ts[i] = __builtin_readcyclecounter(); } while (0)
#define WN_TS_END()                                                                                                                  \
    do {                                                                                                                             \
        if ((a.ablate & 64) && blockIdx.x == 3 && blockIdx.y == 5 && threadIdx.x == 0) {                                            \
            __builtin_amdgcn_s_waitcnt(0);                                                                                           \
            wn_ts[6] = __builtin_readcyclecounter();                                                                                 \
            printf("wn phases (cycles): stage %lld inconv %lld rawstore %lld gate+planes %lld rs %lld epilogue %lld total %lld\n", wn_ts[1] - wn_ts[0], \
                   wn_ts[2] - wn_ts[1], wn_ts[3] - wn_ts[2], wn_ts[4] - wn_ts[3], wn_ts[5] - wn_ts[4], wn_ts[6] - wn_ts[5], wn_ts[6] - wn_ts[0]);   \
        }                                                                                                                            \
    } while (0)
#else
#define WN_TS_DECL() ((void)0)
#define WN_TS(i) ((void)0)
#define WN_TS_END() ((void)0)
#endif

// NT column tiles per workgroup: 3 (96 columns) when the grid fills the chip, 1 (32 columns) for small grids (one
// utterance: a third of the dependent MFMA chain per wave, three times the workgroups).  The arithmetic of an output
// element — chunk, tap, group and product order — is the same in both, so the results are bit-identical and the choice
// may depend on the grid size.

// H2 (MATH_F16X2): operands as two fp16 planes (activations x 2^4 while they are split, weights x 2^13 when packed), three
// products per multiply-add; the accumulators run scaled by 2^17 (bias and conditioning enter scaled) and are unscaled,
// exactly, where they leave the matrix cores — the gate and the residual / skip updates see the same values as before.
// Four waves, one per SIMD with the whole register file each; MW row tiles per wave (S = 32: 3 of the 12, S = 16: 6 of the 24).
// RA (S = 32): weight-fragment ring (b3.h b3_chunk_ra): 2 = one group ahead (nt 1, bf16 weights, f16x2), 4 = three groups ahead.  S = 16:
// b3_chunk16 keeps the fragments one 32-channel step ahead in every form.
// EP: the epilogue's old-value loads (h residual: L2 hits, skip accumulator: HBM) — 0 = 16 values per lane ahead of the stores (one 32 x 32
// tile: rounds 2 - 4), 1 = 48 values ahead (three 32 x 32 or twelve 16 x 16 tiles: a wave's tiles were as many dependent round trips)
//
// The MFMA shape (S) decides how a wave's 96 rows x T_B columns are cut into accumulator tiles, and nothing else: WnTiles<S> holds that
// layout — which row of which conv an accumulator register is, where a lane's gated values go in u's planes, which chunk loop runs.
//   S = 32 (v_mfma_f32_32x32x16_bf16; MATH_F16X2, and MI355VITS_WN_SHAPE=32 in the lab build and the CPU model): 3 x NT tiles of 32 x 32,
//     gate-conv tile q = the tanh rows of channels 16 q .. 16 q + 15 and their sigmoid rows (packed_b3w), plain tiles in row order.
//   S = 16 (v_mfma_f32_16x16x32_bf16, the product's split-bf16 form): 6 x 2 NT tiles of 16 x 16.  Row 4 q + i of 16-row tile n is channel
//     32 (n >> 1) + 8 q + 4 (n & 1) + i (k_mrf_p's map); the gate conv is 12 pairs of a tanh tile and the sigmoid tile of the same 16
//     channels, wave w owns pairs w, w + 4, w + 8, so a lane's tanh and sigmoid values of a channel sit in the same register of two tiles
//     and its four gated values are one half record of u's planes (one 8-byte store per plane).  The res/skip conv has 24 plain tiles,
//     six per wave (last layer: 12, three per wave).  Weights: pack_conv_weights_w16.
template <int S> struct WnTiles;

template <> struct WnTiles<32> {
    typedef f32x16 Acc;
    static constexpr int NR = 16, CW = 32, ROWS = 32, MW = 3, MW_LAST = 2;  // registers per tile, tile width / height, tiles per wave (last layer: with work)
    static __device__ __forceinline__ int col(int lane) { return lane & 31; }
    static __device__ __forceinline__ int krec(int lane) { return lane >> 5; }  // the lane's record within a k-group of the planes
    static __device__ __forceinline__ int lane_row(int lane) { return 4 * (lane >> 5); }
    static __device__ __forceinline__ int reg_row(int r) { return (r & 3) + 8 * (r >> 2); }
    static __device__ __forceinline__ int tile_row0(int q) { return 32 * q; }
    static __device__ __forceinline__ int gate_tile(int w, int i) { return w + 4 * i; }
    static __device__ __forceinline__ int gate_row(int H, int w, int i, int r, int lane) {
        return (r < 8 ? 0 : H) + 16 * (w + 4 * i) + (r & 3) + 8 * ((r >> 2) & 1) + 4 * (lane >> 5);
    }
    template <int MT, int NC, bool W1, bool H2, int RA, bool LAST>
    static __device__ __forceinline__ void conv(Acc (&acc)[MT][NC], const uint4* const (&wp)[MT], const uint4* xq, int PS, int LD, int K, int dil) {
        constexpr int NG = WNB_NG;
        if constexpr (H2) h2_chunk<MT, NC, NG, NC>(acc, wp, xq, PS, LD, K, NG, dil);
        else if constexpr (LAST) b3_chunk<MT, NC, NG, NC, W1>(acc, wp, xq, PS, LD, K, NG, dil);
        else if constexpr (RA > 2 && NC >= 4) b3_chunk_lean_ra<MT, NC, NG, W1, RA>(acc, wp, xq, PS, LD, K, NG, dil);  // (four column tiles: B single-buffered)
        else if constexpr (RA > 2) b3_chunk_ra<MT, NC, NG, NC, W1, RA>(acc, wp, xq, PS, LD, K, NG, dil);
        else b3_chunk<MT, NC, NG, NC, W1>(acc, wp, xq, PS, LD, K, NG, dil);
    }
    // gate in registers (round 6): accumulator r < 8 and r + 8 of a lane are the two halves of ONE channel, and a lane's eight gated values of a
    // (row tile, column tile) are exactly the eight k-slots of one B-operand record (16-channel group q, half brow, its column) of the res/skip
    // conv — the raw result never goes through LDS (rounds 2 - 5: 144 ds_write_b32 + a barrier + 144 ds_read_b32 per lane).
    template <int NC, bool H2>
    static __device__ __forceinline__ void gate_store(const Acc (&acc)[MW][NC], uint4* planes, int w, int lane, float UNACC) {
        constexpr int T_B = 32 * NC, PSU0 = WNB_NG * 2 * T_B;
        const int brow = lane >> 5, bcol = lane & 31;
        MI355_UNROLL
        for (int i = 0; i < MW; ++i)
            MI355_UNROLL
            for (int j = 0; j < NC; ++j) {
                float u[8];
                MI355_UNROLL
                for (int e = 0; e < 8; ++e) u[e] = wn_gate_f(acc[i][j][e] * UNACC, acc[i][j][e + 8] * UNACC);
                const int idx = (2 * (w + 4 * i) + brow) * T_B + 32 * j + bcol;
                if constexpr (H2) {
                    uint4 h4, m4;
                    split2_pk(u[0] * F16X2_X_SCALE, u[1] * F16X2_X_SCALE, h4.x, m4.x);
                    split2_pk(u[2] * F16X2_X_SCALE, u[3] * F16X2_X_SCALE, h4.y, m4.y);
                    split2_pk(u[4] * F16X2_X_SCALE, u[5] * F16X2_X_SCALE, h4.z, m4.z);
                    split2_pk(u[6] * F16X2_X_SCALE, u[7] * F16X2_X_SCALE, h4.w, m4.w);
                    planes[idx] = h4;
                    planes[PSU0 + idx] = m4;
                } else {
                    uint4 h4, m4, l4;
                    split3_pk(u[0], u[1], h4.x, m4.x, l4.x);
                    split3_pk(u[2], u[3], h4.y, m4.y, l4.y);
                    split3_pk(u[4], u[5], h4.z, m4.z, l4.z);
                    split3_pk(u[6], u[7], h4.w, m4.w, l4.w);
                    planes[idx] = h4;
                    planes[PSU0 + idx] = m4;
                    planes[2 * PSU0 + idx] = l4;
                }
            }
    }
};

template <> struct WnTiles<16> {
    typedef f32x4 Acc;
    static constexpr int NR = 4, CW = 16, ROWS = 16, MW = 6, MW_LAST = 3;
    static __device__ __forceinline__ int col(int lane) { return lane & 15; }
    static __device__ __forceinline__ int krec(int lane) { return lane >> 4; }
    static __device__ __forceinline__ int lane_row(int lane) { return 8 * (lane >> 4); }
    static __device__ __forceinline__ int reg_row(int r) { return r; }
    static __device__ __forceinline__ int tile_row0(int n) { return 32 * (n >> 1) + 4 * (n & 1); }
    static __device__ __forceinline__ int gate_tile(int w, int i) { return 2 * (w + 4 * (i >> 1)) + (i & 1); }  // pair w + 4 (i / 2): tanh tile, sigmoid tile
    static __device__ __forceinline__ int gate_row(int H, int w, int i, int r, int lane) {
        return ((i & 1) ? H : 0) + tile_row0(w + 4 * (i >> 1)) + 8 * (lane >> 4) + r;
    }
    template <int MT, int NC, bool W1, bool H2, int RA, bool LAST>
    static __device__ __forceinline__ void conv(Acc (&acc)[MT][NC], const uint4* const (&wp)[MT], const uint4* xq, int PS, int LD, int K, int dil) {
        static_assert(!H2, "MATH_F16X2 runs on the 32x32x16 tiles");
        b3_chunk16<MT, NC, WNB_H / 32, W1>(acc, wp, xq, PS, LD, K, dil);
    }
    // lane (q = lane >> 4, column c) holds channels 32 g + 8 q + 4 hh + 0..3 of pair (g, hh): slots 4 (q & 1) .. + 3 of record (16-channel
    // group 2 g + (q >> 1), half hh) — the record's lower or upper 8 bytes in each plane
    template <int NC, bool H2>
    static __device__ __forceinline__ void gate_store(const Acc (&acc)[MW][NC], uint4* planes, int w, int lane, float) {
        constexpr int T_B = 16 * NC, PSU0 = WNB_NG * 2 * T_B;
        uint2* p2 = reinterpret_cast<uint2*>(planes);
        const int q = lane >> 4, c = lane & 15;
        MI355_UNROLL
        for (int i = 0; i < MW / 2; ++i) {
            const int pr = w + 4 * i;
            const int rec = 2 * (2 * (pr >> 1) + (q >> 1)) + (pr & 1);
            MI355_UNROLL
            for (int j = 0; j < NC; ++j) {
                float u[4];
                MI355_UNROLL
                for (int e = 0; e < 4; ++e) u[e] = wn_gate_f(acc[2 * i][j][e], acc[2 * i + 1][j][e]);
                const int idx = rec * T_B + 16 * j + c;
                uint2 h2, m2, l2;
                split3_pk(u[0], u[1], h2.x, m2.x, l2.x);
                split3_pk(u[2], u[3], h2.y, m2.y, l2.y);
                p2[2 * idx + (q & 1)] = h2;
                p2[2 * (PSU0 + idx) + (q & 1)] = m2;
                p2[2 * (2 * PSU0 + idx) + (q & 1)] = l2;
            }
        }
    }
};

template <int S, bool W1, int NT, bool H2, int RA, int EP>
__device__ __forceinline__ void wn_layer_b3_body(const WnArgs& a) {
    typedef WnTiles<S> TL;
    typedef typename TL::Acc Acc;
    constexpr int MW = TL::MW, NR = TL::NR, NWV = 4, NTH = 256;
    static_assert(!(W1 && H2), "one reduced-operand variant at a time");
    constexpr int H = WNB_H, T_B = 32 * NT, NG = WNB_NG, NC = T_B / TL::CW;  // NC column tiles per wave
    constexpr int GW = H2 ? 128 : 192;  // uint4 per weight-fragment group (two fp16 or three bf16 planes)
    constexpr int TAPW = S == 16 ? (H / 32) * 192 : NG * GW;  // uint4 per (row tile, tap) of the packed weights
    constexpr float ACC = H2 ? F16X2_ACC_SCALE : 1.0f, UNACC = H2 ? 1.0f / F16X2_ACC_SCALE : 1.0f;
    DYN_SMEM(float, smem);
    uint4* planes = reinterpret_cast<uint4*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = WAVE_UNIFORM(tid >> 6);
    const int lrow = TL::lane_row(lane), bcol = TL::col(lane);
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * T_B;
    int len = a.len ? a.len[b] : a.T;
    if (len > a.T) len = a.T;
    if (t0 >= len) return;  // ragged batches (round 6): a tile past its row's length is never computed (kernels_mrfp.cpp next_item)
    const int pad = (a.K - 1) / 2 * a.dil;
    const int tlo = t0 - pad;
    const int ts = tlo >= 0 ? (tlo & ~3) : -(((-tlo) + 3) & ~3);
    const int toff = tlo - ts;
    const int LD = a.ldx;          // staged columns of the h tile
    WN_TS_DECL();
    WN_TS(0);
    const int PS = NG * 2 * LD;    // uint4 per plane
    const bool two = a.Crs == 2 * H;

    if (!(LAB_ABLATE(a) & 2)) stage_planes<NG, NG, H2>(a.h_in + (long)b * a.h_bs, a.h_ld, LD, ts, len, 1.0f, planes, PS, tid, NTH);  // column sets x row batches: one round trip
    __syncthreads();
    WN_TS(1);

    // ---- in-layer conv: the wave's MW row tiles of the 2H (WnTiles: which rows), all NC column tiles
    // (speaker conditioning without a branch per element — a test per load makes hipcc wait for each one in turn)
    const float* condp = a.cond ? a.cond + (long)b * a.cond_bs : a.b_in;
    const float cond_on = a.cond ? 1.0f : 0.0f;
    {
        Acc acc[MW][NC];
        const uint4* wp[MW];
        MI355_UNROLL
        for (int i = 0; i < MW; ++i) {
            MI355_UNROLL
            for (int r = 0; r < NR; ++r) {
                const int c = TL::gate_row(H, w, i, r, lane);
                const float v = (a.b_in[c] + cond_on * condp[c]) * ACC;  // unconditional loads: all in flight together
                MI355_UNROLL
                for (int j = 0; j < NC; ++j) acc[i][j][r] = v;
            }
            wp[i] = reinterpret_cast<const uint4*>(a.w_in) + (long)TL::gate_tile(w, i) * a.K * TAPW + lane;
        }
        if (!(LAB_ABLATE(a) & 1)) TL::template conv<MW, NC, W1, H2, RA, false>(acc, wp, planes + TL::krec(lane) * LD + bcol + toff, PS, LD, a.K, a.dil);
        __syncthreads();  // every wave is done with the h planes: u's planes take their place (column pitch T_B)
        WN_TS(2);
        WN_TS(3);
        // ---- gate in registers: the in-layer conv's rows are stored permuted (Engine::add_conv_data) so that a lane holds both halves of its
        // channels, and its gated values are (part of) one B-operand record of the res/skip conv: WnTiles<S>::gate_store
        TL::template gate_store<NC, H2>(acc, planes, w, lane, UNACC);
    }
    const int ntr = a.Crs / TL::ROWS;
    const float* src[MW];
    float* dst[MW];
    long ldr[MW];
    bool valid[MW], use_old[MW], to_h[MW];
    MI355_UNROLL
    for (int i = 0; i < MW; ++i) {
        const int q = w + NWV * i;
        valid[i] = q < ntr;
        const int qc = valid[i] ? q : ntr - 1;
        const int row0 = TL::tile_row0(qc);  // (a tile's rows lie within one 32-row block)
        to_h[i] = two && row0 < H;  // wave-uniform
        if (to_h[i]) {
            src[i] = a.h_in + (long)b * a.h_bs + (long)row0 * a.h_ld;
            dst[i] = a.h_out + (long)b * a.h_bs + (long)row0 * a.h_ld;
            ldr[i] = a.h_ld;
            use_old[i] = true;
        } else {
            const int sub = two ? H : 0;
            src[i] = a.skip + (long)b * a.s_bs + (long)(row0 - sub) * a.s_ld;
            dst[i] = a.skip + (long)b * a.s_bs + (long)(row0 - sub) * a.s_ld;
            ldr[i] = a.s_ld;
            use_old[i] = !a.skip_init;
        }
    }
    auto load_tile = [&](int i, int j, float (&old)[NR]) {
        const int t = t0 + j * TL::CW + bcol;
        const int tc = t < a.T ? t : a.T - 1;
        if (valid[i] && use_old[i]) {
            MI355_UNROLL
            for (int r = 0; r < NR; ++r) old[r] = src[i][(long)(TL::reg_row(r) + lrow) * ldr[i] + tc];
        } else {
            MI355_UNROLL
            for (int r = 0; r < NR; ++r) old[r] = 0.0f;
        }
    };
    // tiles ahead (EP 0: 16 old values of a lane in flight, EP 1: 48, whatever the tile size); ring of old-value tiles
    constexpr int EPA = (EP == 0 ? 1 : 3) * (16 / NR), EPR = EPA + 1;
    float old[EPR][NR];
    // EP >= 1: the same loads / stores as buffer instructions — a tile's base in the resource, ONE lane offset per tile, the row offsets in
    // SGPRs, and the wave-uniform / per-lane conditions folded into the offset (out of range: the load returns 0, the store is dropped), so
    // nothing between a load's issue and its use is conditional (hipcc's wait-count pass: DESIGN 4.6 item 1)
    auto load_tile_b = [&](int i, int j, float (&o)[NR]) MI355_INLINE_LAMBDA {
        const int t = t0 + j * TL::CW + bcol;
        const int tc = t < a.T ? t : a.T - 1;
        const BufRsrc rs = buf_rsrc(src[i]);
        const unsigned row4 = 4u * (unsigned)ldr[i];
        const unsigned vo = (valid[i] && use_old[i]) ? (unsigned)lrow * row4 + 4u * (unsigned)tc : BUF_OOB;
        MI355_UNROLL
        for (int r = 0; r < NR; ++r) o[r] = buf_load_f32(rs, vo, (unsigned)TL::reg_row(r) * row4);
    };
    constexpr int PSU = NG * 2 * T_B;
    __syncthreads();
    WN_TS(4);
    // ---- res/skip 1x1 conv: Crs / ROWS row tiles, tile q on wave q % 4 (S = 32: 12, last layer 6; S = 16: 24, last layer 12)
    Acc acc[MW][NC];
    {
        const uint4* wp[MW];
        MI355_UNROLL
        for (int i = 0; i < MW; ++i) {
            int q = w + NWV * i;
            if (q >= ntr) q = ntr - 1;  // beyond the last tile: recompute it, discarded below
            MI355_UNROLL
            for (int r = 0; r < NR; ++r) {
                const float v = a.b_rs[TL::tile_row0(q) + TL::reg_row(r) + lrow] * ACC;
                MI355_UNROLL
                for (int j = 0; j < NC; ++j) acc[i][j][r] = v;
            }
            wp[i] = reinterpret_cast<const uint4*>(a.w_rs) + (long)q * TAPW + lane;
        }
        if (!(LAB_ABLATE(a) & 1)) {
            const uint4* xq = planes + TL::krec(lane) * T_B + bcol;
            if (two) {
                TL::template conv<MW, NC, W1, H2, RA, false>(acc, wp, xq, PSU, T_B, 1, 0);
            } else {  // half the tiles.  S = 32, 6 tiles: waves 0, 1 two tiles, waves 2, 3 one (second index clamped); S = 16, 12 tiles: three each
                constexpr int ML = TL::MW_LAST;
                Acc a2[ML][NC];
                const uint4* w2[ML];
                MI355_UNROLL
                for (int i = 0; i < ML; ++i) {
                    w2[i] = wp[i];
                    MI355_UNROLL
                    for (int j = 0; j < NC; ++j) a2[i][j] = acc[i][j];
                }
                TL::template conv<ML, NC, W1, H2, RA, true>(a2, w2, xq, PSU, T_B, 1, 0);
                MI355_UNROLL
                for (int i = 0; i < ML; ++i)
                    MI355_UNROLL
                    for (int j = 0; j < NC; ++j) acc[i][j] = a2[i][j];
            }
        }
        if constexpr (H2) {  // back to the unscaled domain (exact)
            MI355_UNROLL
            for (int i = 0; i < MW; ++i)
                MI355_UNROLL
                for (int j = 0; j < NC; ++j)
                    MI355_UNROLL
                    for (int r = 0; r < NR; ++r) acc[i][j][r] *= UNACC;
        }
    }
    WN_TS(5);
    if ((LAB_ABLATE(a) & 4) && acc[0][0][0] != 1.2345f) return;
    // ---- epilogue: rows < H (two-output layers): h' = (h + rs) * mask; the others: skip (+)= rs.  The old values a
    // lane needs per tile are loaded unconditionally (clamped column) and ahead of the stores: the
    // memory counter retires in order, so a load issued after a store cannot be waited for without waiting for that
    // store's acknowledgement too — with tile k + 1's loads in front of tile k's stores no wait includes a fresh store.
    auto store_tile = [&](int i, int j, const float (&old)[NR]) {
        const int t = t0 + j * TL::CW + bcol;
        if (!valid[i] || t >= a.T) return;
        const bool live = t < len || !to_h[i];  // h' is masked, skip is not (its consumer masks)
        MI355_UNROLL
        for (int r = 0; r < NR; ++r) dst[i][(long)(TL::reg_row(r) + lrow) * ldr[i] + t] = live ? old[r] + acc[i][j][r] : 0.0f;
    };
    if constexpr (EP == 0) {
        MI355_UNROLL
        for (int k = 0; k < EPA && k < MW * NC; ++k) load_tile(k / NC, k % NC, old[k]);
        MI355_UNROLL
        for (int k = 0; k < MW * NC; ++k) {
            if (k + EPA < MW * NC) load_tile((k + EPA) / NC, (k + EPA) % NC, old[(k + EPA) % EPR]);
            SCHED_FENCE();
            store_tile(k / NC, k % NC, old[k % EPR]);
            SCHED_FENCE();
        }
    } else {
        auto store_tile_b = [&](int i, int j, const float (&o)[NR]) MI355_INLINE_LAMBDA {
            const int t = t0 + j * TL::CW + bcol;
            const bool live = t < len || !to_h[i];
            const BufRsrc rs = buf_rsrc(dst[i]);
            const unsigned row4 = 4u * (unsigned)ldr[i];
            const unsigned vo = (valid[i] && t < a.T) ? (unsigned)lrow * row4 + 4u * (unsigned)t : BUF_OOB;
            MI355_UNROLL
            for (int r = 0; r < NR; ++r) buf_store_f32(rs, vo, (unsigned)TL::reg_row(r) * row4, live ? o[r] + acc[i][j][r] : 0.0f);
        };
        MI355_UNROLL
        for (int k = 0; k < EPA && k < MW * NC; ++k) load_tile_b(k / NC, k % NC, old[k]);
        MI355_UNROLL
        for (int k = 0; k < MW * NC; ++k) {
            if (k + EPA < MW * NC) load_tile_b((k + EPA) / NC, (k + EPA) % NC, old[(k + EPA) % EPR]);
            SCHED_FENCE();
            store_tile_b(k / NC, k % NC, old[k % EPR]);
            SCHED_FENCE();
        }
    }
    WN_TS_END();
}

template <int S, bool W1, int NT, bool H2 = false, int RA = 2, int EP = 0>
__global__ __launch_bounds__(256) void k_wn_layer_b3(WnArgs a) {
    wn_layer_b3_body<S, W1, NT, H2, RA, EP>(a);
}

int wn_layer_b3_shape() {
    const char* s = lab_getenv("MI355VITS_WN_SHAPE");  // read per launch: the A/B runs both forms in one process
    return s && atoi(s) == 32 ? 32 : 16;
}

bool wn_layer_b3_supported(int H, int K, int dil) {
    return H == WNB_H && (K % 2) == 1 && K >= 1 && dil >= 1 && (K - 1) * dil <= 24;
}

int wn_layer_b3_column_tiles(const WnArgs& a) {
    // 96-column tiles when they fill the chip, 32-column tiles for small grids (same bits, see k_wn_layer_b3)
    const char* nt_s = lab_getenv("MI355VITS_WN_B3_NT");  // read per launch: tests flip it inside one process
    const long nwg3 = (long)((a.T + 95) / 96) * a.B;
    int nt = nt_s ? atoi(nt_s) : (nwg3 < 128 ? 1 : 3);
    // 128-column tiles (round 6: they fit since the gate left LDS — 153 KiB of h planes; a fragment group feeds 72 instead of 54 MFMAs, the
    // per-workgroup phases are paid once per 128 columns: 0.96 of the 96-column form's time per column, profiles/r06_wn_nt4_ab.txt) when the
    // persistent rounds of the grid come out shorter: rounds x tile cost (4/3 x 0.96 = 1.28 of a 96-column tile).  Same bits.
    if (!nt_s && nt == 3 && a.math != MATH_F16X2) {
        const long cus = current_device_cu_count();
        const long nwg4 = (long)((a.T + 127) / 128) * a.B;
        if ((double)((nwg4 + cus - 1) / cus) * 1.28 < (double)((nwg3 + cus - 1) / cus)) nt = 4;
    }
    if (nt == 4 && (a.math == MATH_F16X2 || ((long)a.h_ld * 128 >= 0x7fffffffL || (long)a.s_ld * 128 >= 0x7fffffffL || (a.K - 1) * a.dil > 8))) nt = 3;  // (buffer-addressed epilogue; 160 KiB of LDS)
    return nt;
}

void launch_wn_layer_b3(WnArgs a, hipStream_t s) {
    if (a.T <= 0 || a.B <= 0) return;
    if (!wn_layer_b3_supported(a.H, a.K, a.dil)) throw std::runtime_error("wn_layer_b3: unsupported shape");
    static const int ablate = lab_getenv("MI355VITS_WN_ABLATE") ? atoi(lab_getenv("MI355VITS_WN_ABLATE")) : 0;
    a.ablate = ablate;
    a.vec = (a.h_ld % 4 == 0) && (a.h_bs % 4 == 0) && (reinterpret_cast<uintptr_t>(a.h_in) % 16 == 0);
    const int nt = wn_layer_b3_column_tiles(a);
    const int tb = 32 * nt;
    a.ldx = (tb + (a.K - 1) * a.dil + 3 + 3) & ~3;
    const size_t shmem = (size_t)3 * WNB_NG * 2 * a.ldx * 16;  // the h planes; u's planes (column pitch tb <= ldx) take their place
    dim3 grid((a.T + tb - 1) / tb, a.B);
    // four waves (one per SIMD, the whole register file each).  A twelve-wave form (three per SIMD) was bit-identical and measured
    // EQUAL (16 layers 1.77 vs 1.76 ms, profiles/r04_wn_experiments.txt); a two-workgroups-per-CU form (64-column tiles) 8.5 % slower
    // at batch 256 (profiles/r05_wn_two_per_cu_ab.txt)
    auto go = [&](auto kfn) {
#ifndef MI355_EMU
        set_max_dynamic_lds(reinterpret_cast<const void*>(kfn), 160 * 1024);
#endif
        LAUNCH_KERNEL(kfn, grid, dim3(256), shmem, s, a);
    };
    // the epilogue of the 96-column form (WNB_EPI: the loads three 32 x 32 tiles ahead; MI355VITS_WN_EPI=0: one tile ahead, the form past the buffer range)
    int epi = WNB_EPI;
    if (const char* f = lab_getenv("MI355VITS_WN_EPI")) epi = atoi(f);
    if ((long)a.h_ld * 128 >= 0x7fffffffL || (long)a.s_ld * 128 >= 0x7fffffffL) epi = 0;  // the rows of a tile (32 from its base) must fit the buffer range
    if (a.math == MATH_F16X2) {  // two fp16 planes, on the 32x32x16 tiles
        if (nt == 1) go(k_wn_layer_b3<32, false, 1, true>);
        else go(k_wn_layer_b3<32, false, 3, true>);
        return;
    }
    const bool w1 = a.math == MATH_BF16W;
    if (a.shape != 32) {
        // v_mfma_f32_16x16x32_bf16 (b3_chunk16: the weight fragments one 32-channel step ahead in every form — there is no ring to size,
        // so the RA argument, left at 2 here, is not read by WnTiles<16>)
        if (nt == 4) { if (w1) go(k_wn_layer_b3<16, true, 4, false, 2, 1>); else go(k_wn_layer_b3<16, false, 4, false, 2, 1>); }
        else if (nt == 1) { if (w1) go(k_wn_layer_b3<16, true, 1>); else go(k_wn_layer_b3<16, false, 1>); }
        else if (w1) go(k_wn_layer_b3<16, true, 3>);
        else if (epi == 1) go(k_wn_layer_b3<16, false, 3, false, 2, 1>);
        else go(k_wn_layer_b3<16, false, 3>);
        return;
    }
#if defined(MI355_LAB) || defined(MI355_EMU)
    // MI355VITS_WN_SHAPE=32: the 32x32x16 form this kernel had before the shape A/B (profiles/wn_shape_ab.txt), with its own packing
    if (nt == 4) {
        // weight fragments three groups ahead as in the 96-column form, the B fragments single-buffered (b3_chunk_lean_ra: with both
        // double-buffered the loop spills 148 B at four column tiles)
        if (w1) go(k_wn_layer_b3<32, true, 4, false, WNB_RING, 1>);
        else go(k_wn_layer_b3<32, false, 4, false, WNB_RING, 1>);
    } else if (nt == 1) {
        if (w1) go(k_wn_layer_b3<32, true, 1>);
        else go(k_wn_layer_b3<32, false, 1>);
    } else {
        // large grids: the weight fragments three groups ahead (WNB_RING)
        if (w1) go(k_wn_layer_b3<32, true, 3>);
        else if (epi == 1) go(k_wn_layer_b3<32, false, 3, false, WNB_RING, 1>);
        else go(k_wn_layer_b3<32, false, 3, false, WNB_RING>);
    }
#else
    throw std::runtime_error("wn_layer_b3: the 32x32x16 form exists in the lab build only");
#endif
}

bool wn_layer_fused_supported(int H, int K, int dil) {
    return (H == 32 || H == 192) && (K % 2) == 1 && K >= 1 && dil >= 1 && (size_t)H * (32 + (K - 1) * dil + 8) * 4 <= 48 * 1024;
}

int wn_layer_geometry(const WnArgs& a) {
    const char* six_s = lab_getenv("MI355VITS_WN_SIX_WAVES");  // read per launch: tests flip it inside one process
    const int six_env = six_s ? atoi(six_s) : -1;
    const long nwg = (long)((a.T + 31) / 32) * a.B;
    return six_env >= 0 ? six_env : (nwg < 128 ? 2 : (nwg < 512 ? 1 : 0));  // 0: 4x3, 1: 6x2, 2: 12x1
}

void launch_wn_layer(WnArgs a, hipStream_t s) {
    if (a.T <= 0 || a.B <= 0) return;
    if (!wn_layer_fused_supported(a.H, a.K, a.dil)) throw std::runtime_error("wn_layer: unsupported shape");
    a.ldx = (32 + (a.K - 1) * a.dil + 3 + 3) & ~3;
    static const int ablate = lab_getenv("MI355VITS_WN_ABLATE") ? atoi(lab_getenv("MI355VITS_WN_ABLATE")) : 0;
    a.ablate = ablate;
    a.vec = (a.h_ld % 4 == 0) && (a.h_bs % 4 == 0) && (reinterpret_cast<uintptr_t>(a.h_in) % 16 == 0);
    const size_t shmem = (size_t)a.H * a.ldx * sizeof(float);  // ldx >= 32: U fits in the h tile
    dim3 grid((a.T + 31) / 32, a.B);
    // Three geometries with identical arithmetic (same bits): 4 waves x 3 tiles keeps the SIMDs evenly loaded when the
    // grid fills the chip; 6 x 2 and 12 x 1 have ever shorter dependent MFMA chains per wave, which is what matters when
    // only a few dozen workgroups exist (one utterance: 31 workgroups per layer).
    const int geom = wn_layer_geometry(a);
    const size_t sh4 = (size_t)a.H * (a.ldx > 64 ? a.ldx : 64) * sizeof(float);  // h tile, then [2H][32] raw result
    if (a.H == 192 && geom == 0) {
        LAUNCH_KERNEL(k_wn_layer_h192<4>, grid, dim3(256), sh4, s, a);
    } else if (a.H == 192 && geom == 2) {
        LAUNCH_KERNEL(k_wn_layer_h192<12>, grid, dim3(768), sh4, s, a);
    } else if (a.H == 192) {
        auto k = k_wn_layer<6>;
        LAUNCH_KERNEL(k, grid, dim3(384), shmem, s, a);
    } else {
        auto k = k_wn_layer<1>;
        LAUNCH_KERNEL(k, grid, dim3(64), shmem, s, a);
    }
}

}  // namespace m355
