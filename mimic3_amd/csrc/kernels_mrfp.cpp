// kernels_mrfp.cpp — one HiFi-GAN multi-receptive-field stage in MATH_BF16X3 with every element split ONCE.
//
//   y = (1/n) * sum_j RB_j(x),   RB_j: x1 = x + conv_{k_j,d1_j}(lrelu_0.1(x));  x2 = x1 + conv_{k_j,d2_j}(lrelu_0.1(x1))
//
// k_mrf_fused (kernels_mrf.cpp) keeps f32 tiles in LDS and splits a lane's operands into three bf16 terms again for every
// tap: 36 VALU per six MFMAs, as much issue time as the matrix work they feed (MFMA pipe 0.41 busy, 10.7 VALU per
// MFMA).  Here the VALU work is proportional to the ELEMENTS, not to elements x taps:
//   * both LDS tiles hold three bf16 PLANES (x = h + m + l exactly, 6 B per element): x (+halo) is split while it is staged,
//     x1 in conv1's epilogue; a record = the 8 consecutive channels 32 g + 8 q .. + 7 of one column (16 B), stored
//     [plane][k-group g][quarter q][column] — exactly one lane's B operand of v_mfma_f32_16x16x32_bf16 (k = 32 input channels =
//     one k-group per tap and MFMA), consecutive lanes on consecutive records (conflict-free ds_read_b128 when the row pitch
//     is a multiple of 16 columns);
//   * the WEIGHTS of the running conv live in registers: a wave owns ONE 16-row tile of output channels, K x (C / 32) x 3
//     fragments of 4 VGPRs (84 registers for 7 taps of 32 channels), loaded once per conv and wave from L2 — the matrix-core
//     loop carries no VALU and no global loads at all: three ds_read_b128 per six MFMAs, two steps ahead;
//   * 16-column tiles: eight waves = NWM row tiles x NWC column groups; conv2 owns NT2 output tiles per wave whose
//     accumulators persist over the resblocks (statically indexed), conv1 walks its share of the extended range
//     (T_B + 2 r2 columns) in a runtime loop: init (residual + bias, rebuilt exactly from the planes) -> K x C/32 steps of six
//     MFMAs on two independent accumulator chains -> epilogue (leaky-relu, mask, split, one 8-byte store per plane).  Two
//     waves per SIMD: one wave's init / epilogue VALU runs beside its partner's MFMAs;
//   * output-channel <-> (tile, row) map chosen so that a lane's four accumulator rows are four consecutive k-slots of a
//     record: row 4 q + i of tile mt = channel 32 (mt >> 1) + 8 q + 4 (mt & 1) + i (the weights are packed to match,
//     pack_conv_weights_p16).
// HBM traffic = read x (+halo) + write y, as before.
#include <cstdlib>
#include <type_traits>

#include "items.h"
#include "kernels.h"

namespace m355 {

// MRFP_SCALAR (with -fno-slp-vectorize for this file): no packed f32 VALU in the kernel
#ifdef MRFP_SCALAR
#define MRFP_SPLIT split3_sc
#else
#define MRFP_SPLIT split3_pk
#endif

namespace {
constexpr int MRFP_KMAX = 7;  // taps whose fragments fit a wave's registers next to the accumulators
constexpr size_t MRFP_LDS_LIMIT = 160 * 1024;
}  // namespace

// one k-group of the running conv's fragments of row tile `mt`: [tap][plane] x (64 lanes x 16 B); consecutive taps are
// `tap_stride` uint4 apart (= C / 32 k-groups x 3 planes x 64 lanes)
// wp is wave-uniform (one base register pair for all fragments), the lane index a 32-bit offset
template <int K>
__device__ __forceinline__ void mrfp_load_w(uint4 (&W)[MRFP_KMAX][3], const uint4* __restrict__ wp, int lane, int tap_stride) {
    MI355_UNROLL
    for (int k = 0; k < K; ++k)
        MI355_UNROLL
        for (int p = 0; p < 3; ++p) W[k][p] = wp[lane + k * tap_stride + p * 64];
}

// One 16-column tile, one k-group (32 input channels) of one conv for this wave's 16 output rows: (accb + accs) += sum over
// K taps.  xq = (plane 0, this k-group, this lane's quarter, first tap's column) in the LDS planes; PS = plane stride (uint4).
// B fragments travel AHEAD steps ahead (ring of AHEAD + 1); the six products of a step alternate between two accumulator
// chains (small terms -> accs, large terms -> accb) so that consecutive MFMAs never wait on each other's result.
// filler(s) is called inside step s: independent VALU work (the previous tile's epilogue) that the scheduler is asked to deal
// out between this step's MFMAs — on this part VALU work overlaps matrix work only from inside the same instruction stream.
// KN > 0 (the last tile a conv's k-group is used for): tap s of the NEXT fragments (wn, KN taps) is loaded into W[s] as soon
// as step s has issued its MFMAs — the weight stream of the next conv travels under the rest of this tile, the epilogue and
// the barrier instead of in front of the next conv (the L1 delivers 64 B per clock: 9 - 21 KiB per wave and conv).
template <int K, int AHEAD, int KN, typename Filler>
__device__ __forceinline__ void mrfp_sweep(f32x4& accb, f32x4& accs, uint4 (&W)[MRFP_KMAX][3], const uint4* __restrict__ xq, int PS, int dil,
                                           Filler filler, const uint4* __restrict__ wn, int lane, int tap_stride) {
    constexpr int RING = AHEAD + 1;
    uint4 bf[RING][3];
    auto rd = [&](int s, int slot) MI355_INLINE_LAMBDA {
        const uint4* p = xq + s * dil;
        MI355_UNROLL
        for (int pl = 0; pl < 3; ++pl) bf[slot][pl] = p[pl * PS];
    };
    MI355_UNROLL
    for (int s = 0; s < AHEAD && s < K; ++s) rd(s, s);
    MI355_UNROLL
    for (int s = 0; s < K; ++s) {
        if (s + AHEAD < K) rd(s + AHEAD, (s + AHEAD) % RING);
        SCHED_FENCE();
        const int c = s % RING;
        accs = MFMA_16x16x32_BF16(W[s][2], bf[c][0], accs);  // small terms first
        accb = MFMA_16x16x32_BF16(W[s][1], bf[c][0], accb);
        accs = MFMA_16x16x32_BF16(W[s][0], bf[c][2], accs);
        accb = MFMA_16x16x32_BF16(W[s][0], bf[c][1], accb);
        accs = MFMA_16x16x32_BF16(W[s][1], bf[c][1], accs);
        accb = MFMA_16x16x32_BF16(W[s][0], bf[c][0], accb);
        filler(s);
        MI355_UNROLL
        for (int u = 0; u < 6; ++u) {
            SCHED_GROUP(0x8, 1);  // one MFMA ...
            SCHED_GROUP(0x2, 3);  // ... then up to three VALU of the filler
        }
        SCHED_FENCE();
        if (KN > 0 && s < KN) {
            MI355_UNROLL
            for (int p = 0; p < 3; ++p) W[s][p] = wn[lane + s * tap_stride + p * 64];
        }
    }
    if (KN > K) {
        MI355_UNROLL
        for (int s = K; s < KN; ++s)
            MI355_UNROLL
            for (int p = 0; p < 3; ++p) W[s][p] = wn[lane + s * tap_stride + p * 64];
    }
}

// C channels; NWM = C / 16 row tiles x NWC column groups = 8 waves; T_B = 16 NWC NT2 output columns per work item.
// PERSISTENT: one workgroup per CU walks the (row, column block) items — a workgroup start costs ~6 us here (160 KiB of LDS:
// nothing overlaps it).
// K0, K1, K2: the resblocks' tap counts (0 = no such resblock) — compile-time, so that every weight fragment has its own
// registers and the whole stage is straight-line code between the barriers.
// A wave keeps ONE k-group (32 input channels) of the running conv in registers: with C = 64 a conv is two passes over the
// wave's column tiles (the accumulators persist between the passes, statically indexed).
// Column tiles: conv2's NT2 output tiles of a wave start at t0 + 16 (cg NT2 + i).  conv1 computes x1 over the extended range
// [t0 - r2, t0 + T_B + r2): the INTERIOR tiles sit on conv2's grid and belong to the same wave, so conv2's residual (raw x1 at
// its own columns) never leaves the registers; the halo is covered by ceil(r2 / 16) tiles per side that start at the range's
// ends (they overlap the interior: the same bits are written twice), dealt round-robin to the column groups, at most NHMAX
// per wave.  conv1's own residual (raw x) comes straight from global memory (L2 hits: the tile was staged from there).
// SH: row pitches and dilations when known at compile time (the "_low" voices' stage shapes: every LDS access of a tile then
// carries its offset as an immediate on one base register), or MrfPDyn = take them from the arguments.
template <int LDX_, int LD1_, int D10, int D20, int D11, int D21, int D12, int D22>
struct MrfPShape {
    static constexpr int LDX = LDX_, LD1 = LD1_;
    static constexpr int d1(int j) { return j == 0 ? D10 : (j == 1 ? D11 : D12); }
    static constexpr int d2(int j) { return j == 0 ? D20 : (j == 1 ? D21 : D22); }
};
using MrfPDyn = MrfPShape<0, 0, 0, 0, 0, 0, 0, 0>;

// how k_mrf_p's cursor (items.h) reads a row's length: a plain load; no table = every row is full
struct MrfPRowLen {
    const MrfArgs* a;
    __device__ __forceinline__ int operator()(int bb) const {
        int ln = a->len ? a->len[bb] : a->T;
        return ln > a->T ? a->T : ln;
    }
};

template <int C, int NWM, int NWC, int NT2, int NHMAX, int K0, int K1, int K2, typename SH>
__global__ __launch_bounds__(512) void k_mrf_p(MrfArgs a) {
    static_assert(NWM * NWC == 8 && NWM * 16 == C, "eight waves: C / 16 row tiles x column groups");
    constexpr int G = C / 32, T_B = 16 * NWC * NT2, TAP = G * 3 * 64, NT1 = NT2 + NHMAX;
    constexpr int AH = G == 1 ? 2 : 1;  // B fragments ahead of their MFMAs
    constexpr int RB = 4;               // records a thread stages per item (4 G records per column, column sets share them)
    // PIPE (32 channels; round 6): the x tile is dead once the LAST resblock's conv1 is through, so the NEXT item's x is staged
    // under that resblock's conv2 — record u's eight loads at the start of tile u, its leaky-relu / split / plane stores dealt out
    // between the MFMAs of tile u + 1 — and the stage's output leaves tile by tile behind the following tile's loads instead of
    // in one burst at the end.  Shader-clock stamps of round 5's form (profiles/r06_mrfp_clocks.txt): 4.4 k cycles of staging +
    // 3 k at its barrier + 1.5 - 2.7 k of stores per 56 k-cycle item with no MFMA in flight.  Same bits.
    constexpr bool PIPE = G == 1;
    static_assert(!PIPE || NT2 >= RB + 1, "one staged record per conv2 tile, finished under the next one");
    DYN_SMEM(float, smem);
    const int LDX = SH::LDX ? SH::LDX : a.ldx, LD1 = SH::LD1 ? SH::LD1 : a.ld1, R = a.R;
    const int PSX = G * 4 * LDX, PS1 = G * 4 * LD1;
    uint4* Xp = reinterpret_cast<uint4*>(smem);   // [3][G][4][LDX]   lrelu(x), zero outside the row
    uint4* X1p = Xp + 3 * PSX;                    // [3][G][4][LD1]   lrelu(x1) of the current resblock, zero outside the row
    float* BS = reinterpret_cast<float*>(X1p + 3 * PS1);  // [nrb][2][C] biases
    const int tid = threadIdx.x, lane = tid & 63, wid = WAVE_UNIFORM(tid >> 6);
    const int mt = wid % NWM;
    // work items = the (row, block of T_B columns) pairs that HAVE work, a.nvalid of them, numbered row by row; this workgroup takes
    // first, first + stride, ... of its XCD's contiguous eighth, a forward-only cursor turns an index into (row, block): items.h
    const int nitems = a.nvalid;
    // (grids of fewer than eight workgroups: as many groups as workgroups, so that every group's items have a workgroup)
    const int nblk = gridDim.x, ngrp = nblk < 8 ? nblk : 8, xcd = blockIdx.x % ngrp, slot = blockIdx.x / ngrp;
    const int per_xcd = (nitems + ngrp - 1) / ngrp, nslot = (nblk + ngrp - 1 - xcd) / ngrp;  // blocks on this XCD (nblk need not be a multiple of 8)
    const int item_end = (xcd + 1) * per_xcd < nitems ? (xcd + 1) * per_xcd : nitems;
    const MrfPRowLen row_len{&a};
    using Cursor = ItemCursor<T_B, 0, MrfPRowLen>;
    int item = xcd * per_xcd + slot;
    Cursor cur(row_len, a.B, nitems, 0);
    if (item < item_end) cur.advance(item);

    uint4 W[MRFP_KMAX][3];
    // fragments of (resblock j, conv c, k-group g) for this wave's row tile (wave-uniform; the lane is a 32-bit index on top)
    auto wptr = [&](int j, int c, int K, int g) MI355_INLINE_LAMBDA {
        return reinterpret_cast<const uint4*>(a.w[j][c]) + (long)mt * K * TAP + g * (3 * 64);
    };
    if (item < item_end) mrfp_load_w<K0>(W, wptr(0, 0, K0, 0), lane, TAP);

    for (int i = tid; i < a.nrb * 2 * C; i += 512) BS[i] = a.bias[i / (2 * C)][(i / C) & 1][i % C];

    // ---- staging of x[:, t0 - R : t0 - R + LDX) as planes: a thread takes one column of RB (k-group, quarter) records — eight
    // 4-byte loads per record (256 contiguous bytes per wave and channel), all in flight together —, applies leaky-relu, splits
    // and stores one conflict-free 16-byte record per plane.  Narrow tiles: the waves form column sets that share the records.
    const int wpc = (LDX + 63) >> 6;  // waves per column set
    const int nparts = 8 / wpc > 0 ? 8 / wpc : 1;
    int spart = 0, scol = 0;
    bool stager = false;
    auto stage_item = [&](int bb, int tt0, int ln) MI355_INLINE_LAMBDA {
        if (!stager || (LAB_ABLATE(a) & 2)) return;
        const int lst = ln > 0 ? ln - 1 : 0;
        const int tt = tt0 - R + scol;
        const bool s_in = tt >= 0 && tt < ln;
        const int tc = tt < 0 ? 0 : (tt > lst ? lst : tt);  // every load unconditional (clamped), masked afterwards
        const float* xs = a.x + (long)bb * a.x_bs + tc;
        float sv[RB][8];
        MI355_UNROLL
        for (int u = 0; u < RB; ++u)
            MI355_UNROLL
            for (int e = 0; e < 8; ++e) sv[u][e] = xs[(long)(8 * (spart * RB + u) + e) * a.x_ld];
        SCHED_FENCE();  // the 8 RB loads stay in flight together
        MI355_UNROLL
        for (int u = 0; u < RB; ++u) {
            float v[8];
            MI355_UNROLL
            for (int e = 0; e < 8; ++e) v[e] = s_in ? fmaxf(sv[u][e], 0.1f * sv[u][e]) : 0.0f;  // = lrelu_f(v, 0.1f) bit for bit, one instruction fewer
            uint4 h, m, l;
            MRFP_SPLIT(v[0], v[1], h.x, m.x, l.x);
            MRFP_SPLIT(v[2], v[3], h.y, m.y, l.y);
            MRFP_SPLIT(v[4], v[5], h.z, m.z, l.z);
            MRFP_SPLIT(v[6], v[7], h.w, m.w, l.w);
            const int o = (spart * RB + u) * LDX + scol;
            Xp[o] = h;
            Xp[PSX + o] = m;
            Xp[2 * PSX + o] = l;
        }
    };
    static_assert(4 * G <= 2 * RB, "one batch of RB records per thread covers a column (at most two column sets)");
    // PIPE: a thread's column of the NEXT item (every wave takes part: columns past the tile are clamped to its last one, their
    // lanes write the same bits to the same slots — no divergent branch inside the matrix stream), record u = channels 8 u .. + 7
    struct NextItem { int b, t0, len; };
    auto pipe_load = [&](const NextItem& nx, int pc, int u, float (&sv)[8]) MI355_INLINE_LAMBDA {
        const int lst = nx.len > 0 ? nx.len - 1 : 0;
        const int tt = nx.t0 - R + pc;
        const int tc = tt < 0 ? 0 : (tt > lst ? lst : tt);
        const BufRsrc xr = buf_rsrc(a.x + (long)nx.b * a.x_bs);
        MI355_UNROLL
        for (int e = 0; e < 8; ++e) sv[e] = buf_load_f32(xr, 4u * (unsigned)tc, 4u * (unsigned)((8 * u + e) * a.x_ld));
    };
    auto pipe_finish = [&](const NextItem& nx, int pc, int u, const float (&sv)[8], unsigned (&h4)[4], unsigned (&m4)[4], unsigned (&l4)[4], int piece) MI355_INLINE_LAMBDA {
        if (piece < 0 || piece > 3) return;
        const int tt = nx.t0 - R + pc;
        const bool s_in = tt >= 0 && tt < nx.len;
        const float a0 = sv[2 * piece], a1 = sv[2 * piece + 1];  // (leaky-relu as max(v, 0.1 v): the bits of lrelu_f, one instruction fewer)
        const float v0 = s_in ? fmaxf(a0, 0.1f * a0) : 0.0f, v1 = s_in ? fmaxf(a1, 0.1f * a1) : 0.0f;
        MRFP_SPLIT(v0, v1, h4[piece], m4[piece], l4[piece]);
        if (piece == 3) {
            const int o = u * LDX + pc;
            uint4 h, m, l;
            h.x = h4[0]; h.y = h4[1]; h.z = h4[2]; h.w = h4[3];
            m.x = m4[0]; m.y = m4[1]; m.z = m4[2]; m.w = m4[3];
            l.x = l4[0]; l.y = l4[1]; l.z = l4[2]; l.w = l4[3];
            Xp[o] = h;
            Xp[PSX + o] = m;
            Xp[2 * PSX + o] = l;
        }
    };


    // conv1's epilogue of one tile in three pieces (dealt out between the next tile's MFMAs): x1 (zero outside the row) ->
    // leaky-relu -> three bf16 planes (truncation split: v = h + m + l exactly) -> one 8-byte store per plane
    struct Pend { f32x4 x1; int e; bool live; float v[4], r[4]; uint2* base; };
    auto epi_piece = [&](Pend& pd, int piece) MI355_INLINE_LAMBDA {
        if (LAB_ABLATE(a) & 16) return;
        uint2* p2 = pd.base + 2 * pd.e;
        if (piece == 0) {
            MI355_UNROLL
            for (int r = 0; r < 4; ++r) pd.v[r] = pd.live ? fmaxf(pd.x1[r], 0.1f * pd.x1[r]) : 0.0f;
        } else if (piece == 1) {
            unsigned u[4];
            MI355_UNROLL
            for (int r = 0; r < 4; ++r) u[r] = __float_as_uint(pd.v[r]);
            uint2 h;
            h.x = pack_hi16(u[0], u[1]);
            h.y = pack_hi16(u[2], u[3]);
            p2[0] = h;
            MI355_UNROLL
            for (int r = 0; r < 4; ++r) pd.r[r] = pd.v[r] - __uint_as_float(u[r] & 0xffff0000u);
            uint2 m;
            m.x = pack_hi16(__float_as_uint(pd.r[0]), __float_as_uint(pd.r[1]));
            m.y = pack_hi16(__float_as_uint(pd.r[2]), __float_as_uint(pd.r[3]));
            p2[2 * PS1] = m;
        } else if (piece == 2) {
            float s4[4];
            MI355_UNROLL
            for (int r = 0; r < 4; ++r) s4[r] = pd.r[r] - __uint_as_float(__float_as_uint(pd.r[r]) & 0xffff0000u);
            uint2 l;
            l.x = pack_hi16(__float_as_uint(s4[0]), __float_as_uint(s4[1]));
            l.y = pack_hi16(__float_as_uint(s4[2]), __float_as_uint(s4[3]));
            p2[4 * PS1] = l;
        }
    };
    auto no_fill = [&](int) MI355_INLINE_LAMBDA {};
    const float inv_rb = 1.0f / (float)a.nrb;  // the mean as one multiply per element (k_mrf_s does the same: the two agree bit for bit)
    // MRFP_CLOCKS (a throw-away lab build): shader-clock stamps of waves 0 and 4 (one SIMD's pair) of workgroup 7, 32 per item
    [[maybe_unused]] int clk_item = 0;
    auto stamp = [&](int k) MI355_INLINE_LAMBDA {
#if defined(MRFP_CLOCKS) && !defined(MI355_EMU)
        if (a.clk) {
            const unsigned t = (unsigned)__builtin_readcyclecounter();
            const BufRsrc dbg = buf_rsrc(a.clk);
            const int sl = wid == 0 ? 0 : (wid == 4 ? 1 : -1);
            const unsigned o = (lane == 0 && sl >= 0 && blockIdx.x == 7 && clk_item < 8) ? 4u * (unsigned)((sl * 8 + clk_item) * 32 + k) : BUF_OOB;
            buf_store_f32(dbg, o, 0u, __uint_as_float(t));
        }
#else
        (void)k;
#endif
    };

    if constexpr (PIPE) {  // the workgroup's first item is staged here, every later one under its predecessor's last conv2
        if (item < item_end) {
            const int b0 = cur.r, t00 = (item - cur.base) * T_B;
            const int len0 = row_len(b0);
            spart = wid / wpc;
            scol = wid * 64 + lane - spart * wpc * 64;
            stager = spart < nparts && scol < LDX && spart * RB < 4 * G;
            stage_item(b0, t00, len0);
        }
    }
    for (int item_next = item; item < item_end; item = item_next) {
        // lane / wave coordinates, re-derived per item from values the optimiser cannot see through: everything computed
        // from them stays inside the loop body (hoisted out, the invariant addresses of ~50 unrolled tiles spill)
        int lane_o = lane, wid_o = wid;
        OPAQUE_V(lane_o);
        OPAQUE_S(wid_o);
        const int cg = wid_o / NWM;
        const int q = lane_o >> 4, n = lane_o & 15;
        spart = wid_o / wpc;
        scol = wid_o * 64 + lane_o - spart * wpc * 64;
        stager = spart < nparts && scol < LDX && spart * RB < 4 * G;
        const int gq = mt >> 1, hh = mt & 1;
        const int co0 = 32 * gq + 8 * q + 4 * hh;  // this lane's four output channels co0 .. co0 + 3 = half hh of record (gq, q)
        const int b = cur.r, t0 = WAVE_UNIFORM((item - cur.base) * T_B);  // scalar registers
        const int len = WAVE_UNIFORM(row_len(b));
        const int last = len > 0 ? len - 1 : 0;
        const float* xb = a.x + (long)b * a.x_bs;
        item_next = item + nslot;
        const bool more = item_next < item_end;  // wave-uniform
        Cursor cn = cur;
        if (more) cn.advance(item_next);

        stamp(0);
        if constexpr (!PIPE) stage_item(b, t0, len);
        stamp(1);
        // PIPE: the next item of this workgroup (the current one again behind the last: its x tile is dead, the loads hit the L2)
        NextItem nx;
        nx.b = more ? cn.r : b;
        nx.t0 = more ? WAVE_UNIFORM((item_next - cn.base) * T_B) : t0;
        nx.len = WAVE_UNIFORM(row_len(nx.b));
        const int pcol = wid_o * 64 + lane_o < LDX ? wid_o * 64 + lane_o : LDX - 1;
        __syncthreads();  // x is staged; every wave is done with the previous item's x1
        stamp(2);

        f32x4 out[NT2];
        MI355_UNROLL
        for (int i = 0; i < NT2; ++i)
            MI355_UNROLL
            for (int r = 0; r < 4; ++r) out[i][r] = 0.0f;

        auto resblock = [&](auto KC, auto KN, auto JC) MI355_INLINE_LAMBDA {
            constexpr int K = decltype(KC)::value, KNEXT = decltype(KN)::value, j = decltype(JC)::value;
            constexpr bool last_rb = KNEXT == 0;  // after it: the next item's first conv (K0)
            constexpr int KAFTER = last_rb ? K0 : KNEXT;
            static_assert(K >= 3, "the epilogue pieces ride in the first three steps of the next tile");
            const int d1 = SH::d1(j) ? SH::d1(j) : a.d1[j], d2 = SH::d2(j) ? SH::d2(j) : a.d2[j];
            const int r1 = (K - 1) / 2 * d1, r2 = (K - 1) / 2 * d2;
            const int nh = (r2 + 15) >> 4;  // halo tiles per side
            // X1 column of this wave's conv1 tile `ti`: interior tiles (ti < NT2) on conv2's grid, halo tile m = ti - NT2 is
            // number hx = cg + NWC m of the 2 nh halo tiles: left ones from column 0 up, right ones from T_B + 2 r2 down
            auto tile_e0 = [&](int ti) MI355_INLINE_LAMBDA {
                if (ti < NT2) return r2 + (cg * NT2 + ti) * 16;
                const int hx = cg + NWC * (ti - NT2);
                return hx < nh ? hx * 16 : T_B + 2 * r2 - 16 * (hx - nh + 1);
            };
            auto tile_on = [&](int ti) MI355_INLINE_LAMBDA { return ti < NT2 || cg + NWC * (ti - NT2) < 2 * nh; };  // wave-uniform
            const float* bs1 = BS + (j * 2 + 0) * C;
            const float4 bv1 = *reinterpret_cast<const float4*>(bs1 + co0);
            const float b1[4] = {bv1.x, bv1.y, bv1.z, bv1.w};
            // ---- conv1: raw x at every tile's own columns (global, clamped: columns outside the row are masked in the epilogue)
            f32x4 acc1[NT1];
            // (buffer loads: the row's base in SGPRs, this lane's channel row + column in ONE VGPR, the four channels' row offsets in
            // SGPRs — no 64-bit address arithmetic per element; the same values)
            const BufRsrc xres = buf_rsrc(xb);
            const unsigned rowb = 4u * (unsigned)(co0 * a.x_ld);
            MI355_UNROLL
            for (int ti = 0; ti < NT1; ++ti) {
                if (tile_on(ti)) {
                    const int t = t0 - r2 + tile_e0(ti) + n;
                    const int tc = t < 0 ? 0 : (t > last ? last : t);
                    MI355_UNROLL
                    for (int r = 0; r < 4; ++r) acc1[ti][r] = (LAB_ABLATE(a) & 32) ? 0.0f : buf_load_f32(xres, rowb + 4u * (unsigned)tc, 4u * (unsigned)(r * a.x_ld));
                }
            }
            stamp(3 + 8 * j);
            Pend pend;
            pend.base = reinterpret_cast<uint2*>(X1p + (gq * 4 + q) * LD1) + hh;  // this lane's half records of x1, column 0
            MI355_UNROLL
            for (int g = 0; g < G; ++g) {
                // the fragments this k-group's last tile pulls in behind its steps: the conv's next k-group, or conv2's first
                const uint4* wn = g + 1 < G ? wptr(j, 0, K, g + 1) : wptr(j, 1, K, 0);
                // order: interior tile 0, the halo tiles, interior tiles 1 .. NT2 - 1 (first and last are unconditional)
                MI355_UNROLL
                for (int oi = 0; oi < NT1; ++oi) {
                    const int ti = oi == 0 ? 0 : (oi <= NHMAX ? NT2 + oi - 1 : oi - NHMAX);
                    if (tile_on(ti)) {
                        const int e = tile_e0(ti) + n;
                        f32x4 ab = acc1[ti], as;
                        MI355_UNROLL
                        for (int r = 0; r < 4; ++r) {
                            if (g == 0) ab[r] += b1[r];
                            as[r] = 0.0f;
                        }
                        const uint4* xq = Xp + (g * 4 + q) * LDX + (R - r2 - r1) + e;
                        const bool fin = g == G - 1;
                        if (!(LAB_ABLATE(a) & 1)) {
                            auto fl = [&](int s) MI355_INLINE_LAMBDA { if (fin && oi > 0) epi_piece(pend, s); };
                            if (oi == NT1 - 1 && !(LAB_ABLATE(a) & 8)) mrfp_sweep<K, AH, K>(ab, as, W, xq, PSX, d1, fl, wn, lane_o, TAP);
                            else mrfp_sweep<K, AH, 0>(ab, as, W, xq, PSX, d1, fl, wn, lane_o, TAP);
                        } else {
                            if (fin && oi > 0) { epi_piece(pend, 0); epi_piece(pend, 1); epi_piece(pend, 2); }
                            if (oi == NT1 - 1 && !(LAB_ABLATE(a) & 8)) mrfp_load_w<K>(W, wn, lane_o, TAP);
                        }
                        MI355_UNROLL
                        for (int r = 0; r < 4; ++r) acc1[ti][r] = ab[r] + as[r];
                        if (fin) {
                            if (oi == 0) stamp(4 + 8 * j);
                            if (j > 0 && oi == 0) __syncthreads();  // every wave is done reading the previous resblock's x1
                            if (oi == 0) stamp(10 + 8 * j);
                            const int t = t0 - r2 + e;
                            pend.x1 = acc1[ti];
                            pend.e = e;
                            pend.live = t >= 0 && t < len;
                        }
                    }
                }
            }
            stamp(5 + 8 * j);
            epi_piece(pend, 0); epi_piece(pend, 1); epi_piece(pend, 2);  // the last tile's epilogue has no MFMAs left to hide behind
            stamp(6 + 8 * j);
            __syncthreads();
            stamp(7 + 8 * j);
            // ---- conv2 into the output registers: out += x1 + bias + conv(lrelu(x1)); this wave: tiles cg NT2 .. + NT2 - 1
            const float* bs2 = BS + (j * 2 + 1) * C;
            const float4 bv2 = *reinterpret_cast<const float4*>(bs2 + co0);
            const float b2[4] = {bv2.x, bv2.y, bv2.z, bv2.w};
            [[maybe_unused]] float sv[2][8];          // PIPE: the staged records in flight (loaded under tile u, finished under tile u + 1)
            [[maybe_unused]] unsigned h4[4], m4[4], l4[4];
            constexpr bool piped = PIPE && last_rb;
            static_assert(!piped || K >= 4, "a staged record's four element pairs ride in four steps of a conv2 tile");
            const float oscale = a.out_scale > 0.0f ? a.out_scale : inv_rb;
            auto store_tile = [&](int i) MI355_INLINE_LAMBDA {  // (PIPE) the finished output tile i: lanes past the row switched off by the buffer's range check
                const int t = t0 + (cg * NT2 + i) * 16 + n;
                const BufRsrc yr = buf_rsrc(a.y + (long)b * a.y_bs);
                const unsigned vo = t < a.T ? 4u * (unsigned)(co0 * a.y_ld + t) : BUF_OOB;
                MI355_UNROLL
                for (int r = 0; r < 4; ++r) buf_store_f32(yr, vo, 4u * (unsigned)(r * a.y_ld), out[i][r] * oscale);
            };
            MI355_UNROLL
            for (int g = 0; g < G; ++g) {
                const uint4* wn = g + 1 < G ? wptr(j, 1, K, g + 1) : (last_rb ? wptr(0, 0, K0, 0) : wptr(j + 1, 0, KNEXT, 0));
                MI355_UNROLL
                for (int i = 0; i < NT2; ++i) {
                    if constexpr (piped) {  // loads first, then the previous tile's stores: waiting for a record never waits for a store issued after it
                        if (i < RB) pipe_load(nx, pcol, i, sv[i & 1]);
                        if (i > 0) store_tile(i - 1);
                    }
                    auto c2fill = [&](int s) MI355_INLINE_LAMBDA {
                        if constexpr (piped) {
                            if (i > 0 && i <= RB) pipe_finish(nx, pcol, i - 1, sv[(i - 1) & 1], h4, m4, l4, s);
                        }
                    };
                    f32x4 ab = out[i], as;
                    MI355_UNROLL
                    for (int r = 0; r < 4; ++r) {
                        if (g == 0) ab[r] += acc1[i][r] + b2[r];  // the residual: raw x1 of the same columns, still in this wave's registers
                        as[r] = 0.0f;
                    }
                    const uint4* xq = X1p + (g * 4 + q) * LD1 + (cg * NT2 + i) * 16 + n;
                    if (!(LAB_ABLATE(a) & 1)) {
                        if (i == NT2 - 1 && !(LAB_ABLATE(a) & 8)) {
                            if (g + 1 < G) mrfp_sweep<K, AH, K>(ab, as, W, xq, PS1, d2, c2fill, wn, lane_o, TAP);
                            else if (!last_rb || more) mrfp_sweep<K, AH, KAFTER>(ab, as, W, xq, PS1, d2, c2fill, wn, lane_o, TAP);
                            else mrfp_sweep<K, AH, 0>(ab, as, W, xq, PS1, d2, c2fill, wn, lane_o, TAP);
                        } else {
                            mrfp_sweep<K, AH, 0>(ab, as, W, xq, PS1, d2, c2fill, wn, lane_o, TAP);
                        }
                    } else if (i == NT2 - 1 && !(LAB_ABLATE(a) & 8)) {
                        if (g + 1 < G) mrfp_load_w<K>(W, wn, lane_o, TAP);
                        else if (!last_rb || more) mrfp_load_w<KAFTER>(W, wn, lane_o, TAP);
                    }
                    MI355_UNROLL
                    for (int r = 0; r < 4; ++r) out[i][r] = ab[r] + as[r];
                    if (g == G - 1 && i == 0) stamp(8 + 8 * j);
                }
            }
            if constexpr (piped) store_tile(NT2 - 1);
            stamp(9 + 8 * j);
        };

        resblock(std::integral_constant<int, K0>{}, std::integral_constant<int, K1>{}, std::integral_constant<int, 0>{});
        if constexpr (K1 > 0) resblock(std::integral_constant<int, K1>{}, std::integral_constant<int, K2>{}, std::integral_constant<int, 1>{});
        if constexpr (K2 > 0) resblock(std::integral_constant<int, K2>{}, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});

        auto store_all = [&](auto MEAN) MI355_INLINE_LAMBDA {  // the mean / scale choice once, outside the loops
            MI355_UNROLL
            for (int i = 0; i < NT2; ++i) {
                const int t = t0 + (cg * NT2 + i) * 16 + n;
                if (t < a.T && !(LAB_ABLATE(a) & 4)) {
                    float* yp = a.y + (long)b * a.y_bs + (long)co0 * a.y_ld + t;
                    MI355_UNROLL
                    for (int r = 0; r < 4; ++r) yp[(long)r * a.y_ld] = decltype(MEAN)::value ? out[i][r] * inv_rb : out[i][r] * a.out_scale;
                }
            }
        };
        if constexpr (!PIPE) {
            if (a.out_scale > 0.0f) store_all(std::false_type{});
            else store_all(std::true_type{});
        }
        stamp(27);
        ++clk_item;
        cur = cn;
    }
}

// ------------------------------------------------------------------------------------------------ host side
size_t p16_packed_words(int Cout, int Cin, int K) { return (size_t)(Cout / 16) * K * (Cin / 32) * 3 * 64 * 4; }

static inline uint32_t p16_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
static inline float p16_bf16_float(uint32_t b) {
    const uint32_t u = b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// [row tile mt][tap][k-group g][plane h, m, l][64 lanes][8 bf16]: lane = (quarter q = l >> 4, row m = l & 15) holds the
// input channels 32 g + 8 q + 0..7 of output channel 32 (mt >> 1) + 8 (m >> 2) + 4 (mt & 1) + (m & 3); w = h + m + l exactly,
// each term rounded to nearest on the host.
void pack_conv_weights_p16(const float* w, int Cout, int Cin, int K, uint32_t* out) {
    const int G = Cin / 32;
    for (int mt = 0; mt < Cout / 16; ++mt)
        for (int k = 0; k < K; ++k)
            for (int g = 0; g < G; ++g)
                for (int l = 0; l < 64; ++l) {
                    const int q = l >> 4, m = l & 15;
                    const int co = 32 * (mt >> 1) + 8 * (m >> 2) + 4 * (mt & 1) + (m & 3);
                    uint32_t plane[3][8];
                    for (int e = 0; e < 8; ++e) {
                        const int ci = 32 * g + 8 * q + e;
                        const float v = w[((size_t)co * Cin + ci) * K + k];
                        const uint32_t h = p16_bf16_rne(v);
                        const float r1 = v - p16_bf16_float(h);
                        const uint32_t mm = p16_bf16_rne(r1);
                        const float r2 = r1 - p16_bf16_float(mm);
                        plane[0][e] = h; plane[1][e] = mm; plane[2][e] = p16_bf16_rne(r2);
                    }
                    for (int p = 0; p < 3; ++p) {
                        uint32_t* o = out + (((((size_t)mt * K + k) * G + g) * 3 + p) * 64 + l) * 4;
                        for (int jj = 0; jj < 4; ++jj) o[jj] = plane[p][2 * jj] | (plane[p][2 * jj + 1] << 16);
                    }
                }
}

namespace {
struct GeoP { int T_B, NWC, NHMAX; };
inline bool geometry_p(int C, GeoP* g) {
    if (C == 32) { *g = {320, 4, 2}; return true; }  // 5 interior + at most 2 halo tiles of conv1 per wave
    if (C == 64) { *g = {96, 2, 3}; return true; }   // 3 interior + at most 3 halo tiles
    return false;
}
// halo, row pitches (multiples of 16 columns: conflict-free 16-byte fragment reads) and LDS bytes of a stage
inline bool shape_p(int C, int nrb, const int* k, const int* d1, const int* d2, const GeoP& g, int* R, int* ldx, int* ld1, size_t* lds) {
    int Rm = 0, r2max = 0;
    for (int j = 0; j < nrb; ++j) {
        if (!(k[j] == 3 || k[j] == 5 || k[j] == 7) || d1[j] < 1 || d2[j] < 1) return false;
        const int r1 = (k[j] - 1) / 2 * d1[j], r2 = (k[j] - 1) / 2 * d2[j];
        Rm = Rm > r1 + r2 ? Rm : r1 + r2;
        r2max = r2max > r2 ? r2max : r2;
        const int nh = (r2 + 15) / 16;  // halo tiles per side, dealt round-robin to the column groups
        if ((2 * nh + g.NWC - 1) / g.NWC > g.NHMAX || 16 * nh > g.T_B) return false;
    }
    *R = Rm;
    *ldx = (g.T_B + 2 * Rm + 15) & ~15;
    *ld1 = (g.T_B + 2 * r2max + 15) & ~15;
    *lds = (size_t)(C / 32) * 4 * 3 * 16 * (size_t)(*ldx + *ld1) + (size_t)nrb * 2 * C * sizeof(float);
    return *lds <= MRFP_LDS_LIMIT && *ldx <= 512;  // (the staging loop: one column per thread)
}
}  // namespace

bool mrf_p_supported(int C, int nrb, const int* k, const int* d1, const int* d2) {
    GeoP g;
    int R, ldx, ld1;
    size_t lds;
    // instantiated tap sequences: (3, 5, 7) — the "_low" voices' resblock_kernel_sizes
    if (!(nrb == 3 && k[0] == 3 && k[1] == 5 && k[2] == 7)) return false;
#ifndef MI355_EMU
    // the product library instantiates the "_low" voices' dilations only (compile-time shapes)
    if (!(d1[0] == 1 && d2[0] == 2 && d1[1] == 2 && d2[1] == 6 && d1[2] == 3 && d2[2] == 12)) return false;
#endif
    return geometry_p(C, &g) && shape_p(C, nrb, k, d1, d2, g, &R, &ldx, &ld1, &lds);
}

bool mrf_p_plan(int C, int nrb, const int* k, const int* d1, const int* d2, MrfPlan* out) {
    GeoP g;
    int R, ldx, ld1;
    size_t lds;
    if (!out || !mrf_p_supported(C, nrb, k, d1, d2) || !geometry_p(C, &g) || !shape_p(C, nrb, k, d1, d2, g, &R, &ldx, &ld1, &lds)) return false;
    *out = MrfPlan{g.T_B, R, 0, 0};  // the halo the kernel stages with (shape_p's)
    return true;
}

void launch_mrf_p(MrfArgs a, hipStream_t s) {
    if (a.T <= 0 || a.B <= 0) return;
    GeoP g;
    size_t shmem = 0;
    if (!geometry_p(a.C, &g) || a.nrb < 1 || a.nrb > MRF_MAX_RB || !shape_p(a.C, a.nrb, a.k, a.d1, a.d2, g, &a.R, &a.ldx, &a.ld1, &shmem))
        throw std::runtime_error("mrf_p: unsupported stage shape");
    const ItemLaunch il = item_launch(a.len_host, a.len, a.B, a.T, g.T_B, 0, current_device_cu_count(), 0);  // (the kernel walks contiguous eighths: no remap)
    a.nvalid = il.nvalid;
    if (il.nvalid <= 0) return;
    dim3 grid((unsigned)il.grid);  // persistent: one workgroup per CU (160 KiB of LDS each)
#ifdef MI355_LAB
    {
        const char* ab = lab_getenv("MI355VITS_MRF_ABLATE");
        a.ablate = ab ? (int)strtol(ab, nullptr, 0) : 0;
    }
#endif
    auto go = [&](auto kfn) {
        set_max_dynamic_lds(reinterpret_cast<const void*>(kfn), (int)MRFP_LDS_LIMIT);
#if defined(MRFP_CLOCKS) && !defined(MI355_EMU)
        static int shots = 0;
        if (a.C == 32 && getenv("MI355VITS_MRFP_CLOCKS") && grid.x > 7 && shots < 3) {  // (the first launch warms the caches)
            ++shots;
            unsigned* dbg = nullptr;
            const size_t nb = 2 * 8 * 32 * sizeof(unsigned);
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dbg), nb));
            HIP_CHECK(hipMemsetAsync(dbg, 0, nb, s));
            MrfArgs c = a;
            c.clk = dbg;
            LAUNCH_KERNEL(kfn, grid, dim3(512), shmem, s, c);
            HIP_CHECK(hipStreamSynchronize(s));
            unsigned h[2 * 8 * 32];
            HIP_CHECK(hipMemcpy(h, dbg, nb, hipMemcpyDeviceToHost));
            (void)hipFree(dbg);
            for (int sl = 0; sl < 2; ++sl)
                for (int it = 1; it < 6; ++it) {
                    const unsigned* t = &h[(sl * 8 + it) * 32];
                    fprintf(stderr, "mrf_p<32> clocks shot %d wave %d item %d: stage %u bar %u |", shots, sl * 4, it, t[1] - t[0], t[2] - t[1]);
                    for (int j = 0; j < 3; ++j) {
                        const unsigned* r = t + 3 + 8 * j;  // r[0] conv1 start, r[1] first tile done, r[7] after the x1 barrier (j > 0), r[2] last sweep done, r[3] epilogue tail, r[4] barrier, r[5] conv2 first tile, r[6] conv2 done
                        fprintf(stderr, " rb%d: c1.init+tile0 %u x1bar %u c1.rest %u tail %u bar %u c2.tile0 %u c2.rest %u |", j, r[1] - r[0], r[7] - r[1], r[2] - r[7], r[3] - r[2],
                                r[4] - r[3], r[5] - r[4], r[6] - r[5]);
                    }
                    fprintf(stderr, " stores %u | item %u\n", t[27] - t[3 + 16 + 6], t[27] - t[0]);
                }
            return;
        }
#endif
        LAUNCH_KERNEL(kfn, grid, dim3(512), shmem, s, a);
    };
    const int k1 = a.nrb > 1 ? a.k[1] : 0, k2 = a.nrb > 2 ? a.k[2] : 0;
    if (!(a.k[0] == 3 && k1 == 5 && k2 == 7)) throw std::runtime_error("mrf_p: unsupported tap counts");
    const bool low = a.d1[0] == 1 && a.d2[0] == 2 && a.d1[1] == 2 && a.d2[1] == 6 && a.d1[2] == 3 && a.d2[2] == 12;  // the "_low" voices
    // product: the compile-time shapes of the "_low" voices only (the run-time-shape instantiation needs > 256 registers at
    // 32 channels: hipcc spills ~100 of them); every other shape runs k_mrf_fused.  The CPU model keeps the run-time-shape
    // instantiation so that the tests cover other dilation sets.
    if (a.C == 32) {
        if (low && a.ldx == 416 && a.ld1 == 400) { go(k_mrf_p<32, 2, 4, 5, 2, 3, 5, 7, MrfPShape<416, 400, 1, 2, 2, 6, 3, 12>>); return; }
    } else {
        if (low && a.ldx == 192 && a.ld1 == 176) { go(k_mrf_p<64, 4, 2, 3, 3, 3, 5, 7, MrfPShape<192, 176, 1, 2, 2, 6, 3, 12>>); return; }
    }
#ifdef MI355_EMU
    if (a.C == 32) go(k_mrf_p<32, 2, 4, 5, 2, 3, 5, 7, MrfPDyn>);
    else go(k_mrf_p<64, 4, 2, 3, 3, 3, 5, 7, MrfPDyn>);
#else
    throw std::runtime_error("mrf_p: unsupported stage shape");
#endif
}

}  // namespace m355
