// kernels_speaker.cpp — k_speaker_cond_mix: the speaker vector g of every row as a blend of emb_g rows or as the caller's own
// vector, and every consumer's 1x1 projection of it (dp.cond, dec.cond, each flow's enc.cond_layer), in ONE launch
// (mi355vits_run_speakers).  In such a run it takes the place of the 2 + flow_n_flows launches of k_speaker_cond; the rule is in
// kernels.h (SpeakerMixArgs) / include/mi355vits.h:
//   g[i]       = fl(w_0 * e_0[i]), then fl(g[i] + fl(w_k * e_k[i])) over the terms whose weight is not 0, in order of k
//   out[b, co] = wave_reduce_sum(lane l: fmaf(W[co, i], g[i], acc) over i = l, l + 64, .. from 0.0f) + bias[co]
// Every product and sum of the blend is ONE f32 operation rounded to nearest: this file is compiled with -ffp-contract=off
// (build.py PER_FILE_FLAGS, the CPU model's g++ likewise) — hipcc's default would fuse w * e into the sum that follows, and HIP's
// __fmul_rn / __fadd_rn are plain operators that fuse just the same.  The projection's fmaf is asked for by name and is
// k_speaker_cond's arithmetic element for element: a plain run on a voice that carries g as a table row gives the same bits.
// Nothing depends on the row block, the grid, the batch or an address.
//   * A 256-lane workgroup owns SPEAKER_MIX_TILE output channels of one job and a block of rows.  Grid x walks the tiles of all
//     jobs (a job's first tile comes with the job), grid y the row blocks.
//   * The block's g vectors are made once and stay in LDS (rows x gin floats); a wave stages rows wid, wid + 4, ..  The weights and
//     sids of all its rows come in one load per lane and reach the row's loop by shuffle, and a row's table values are all in
//     flight before the first sum: the staging is a few memory round trips, not one per term and slice.  A term of weight 0 is
//     skipped before its sid is looked at.
//   * gin <= 512: a wave holds the weight slices W[co, l + 64 j] of its four channels in 32 registers and streams the rows over
//     them — a weight row is read once per row block, and a g value once for four channels.  A larger gin walks the weight row per
//     row (it comes from the L1 / L2 after the first).
//   * After the butterfly every lane holds the sum, so lane c stores channel c: one 16-byte run per wave and row.  Plain vector
//     stores, no atomics.  The workgroups of tile 0 also write g itself (the "g" tap).
#include "kernels.h"

#include <algorithm>

namespace m355 {

namespace {
constexpr int MIX_CPW = SPEAKER_MIX_TILE / 4;  // channels of a wave
constexpr int MIX_NJ = 8;                      // register slices of a weight row: gin <= 64 * MIX_NJ
}  // namespace

__global__ __launch_bounds__(256) void k_speaker_cond_mix(SpeakerMixArgs a, int rb) {
    DYN_SMEM(float, gl);
    const int lane = threadIdx.x & 63, wid = WAVE_UNIFORM(threadIdx.x >> 6);
    const int gin = a.gin, K = a.K;
    const int b0 = blockIdx.y * rb;
    const int nrows = a.B - b0 < rb ? a.B - b0 : rb;

    // ---- this workgroup's job (static indices: the table stays in the kernel's argument segment)
    const float* W = a.jobs[0].w;
    const float* bias = a.jobs[0].bias;
    float* out = a.jobs[0].out;
    int Cout = a.jobs[0].Cout, first = 0;
    MI355_UNROLL
    for (int q = 1; q < SPEAKER_MIX_MAX_JOBS; ++q) {
        if (q < a.n_jobs && (int)blockIdx.x >= a.jobs[q].first_tile) {
            W = a.jobs[q].w;
            bias = a.jobs[q].bias;
            out = a.jobs[q].out;
            Cout = a.jobs[q].Cout;
            first = a.jobs[q].first_tile;
        }
    }
    const int c_base = ((int)blockIdx.x - first) * SPEAKER_MIX_TILE + wid * MIX_CPW;

    // ---- the weight slices of the wave's four channels first (gin <= 512): their latency passes under the staging below
    const bool small = gin <= 64 * MIX_NJ;
    float wr[MIX_CPW][MIX_NJ];
    if (small) {
        MI355_UNROLL
        for (int c = 0; c < MIX_CPW; ++c) {
            const int co = c_base + c < Cout ? c_base + c : Cout - 1;  // clamped: a tile's tail loads the last row, and stores nothing
            MI355_UNROLL
            for (int j = 0; j < MIX_NJ; ++j) {
                const int i = lane + 64 * j;
                wr[c][j] = i < gin ? W[(long)co * gin + i] : 0.0f;
            }
        }
    }

    // ---- g of the block's rows -> LDS (and, from tile 0, to the g buffer).  Wave `wid` stages rows wid, wid + 4, .. (eight at the
    // most); lane l first fetches term l & 7 of the wave's row l >> 3, so no row waits for its own weights and sids: a skipped
    // term's sid is not read
    const bool write_g = blockIdx.x == 0;
    float wv = 0.0f;
    long long sv = 0;
    {
        const int my_r = wid + 4 * (lane >> 3), my_k = lane & 7;
        if (!a.vectors && my_k < K && my_r < nrows) {
            wv = a.weight[(long)(b0 + my_r) * K + my_k];
            if (wv != 0.0f) sv = a.sid[(long)(b0 + my_r) * K + my_k];
        }
    }
    for (int rr = 0, r = wid; r < nrows; ++rr, r += 4) {
        const long b = b0 + r;
        if (a.vectors) {
            if (small) {
                float v[MIX_NJ];
                MI355_UNROLL
                for (int j = 0; j < MIX_NJ; ++j) v[j] = lane + 64 * j < gin ? a.vectors[b * gin + lane + 64 * j] : 0.0f;
                MI355_UNROLL
                for (int j = 0; j < MIX_NJ; ++j) {
                    const int i = lane + 64 * j;
                    if (i < gin) {
                        gl[r * gin + i] = v[j];
                        if (write_g) a.g[b * gin + i] = v[j];
                    }
                }
            } else {
                for (int i = lane; i < gin; i += 64) {
                    const float g = a.vectors[b * gin + i];
                    gl[r * gin + i] = g;
                    if (write_g) a.g[b * gin + i] = g;
                }
            }
            continue;
        }
        float wk[SPEAKER_MIX_MAX_TERMS];
        const float* ek[SPEAKER_MIX_MAX_TERMS];
        MI355_UNROLL
        for (int k = 0; k < SPEAKER_MIX_MAX_TERMS; ++k) {
            wk[k] = __shfl(wv, rr * 8 + k);  // the same in every lane
            ek[k] = a.emb_g + __shfl(sv, rr * 8 + k) * (long long)gin;  // a skipped term: the table's first row, never read
        }
        if (small) {
            // every load of the row first, then the sums in order of k: products and sums never fused (-ffp-contract=off)
            float e[SPEAKER_MIX_MAX_TERMS][MIX_NJ];
            MI355_UNROLL
            for (int k = 0; k < SPEAKER_MIX_MAX_TERMS; ++k) {
                MI355_UNROLL
                for (int j = 0; j < MIX_NJ; ++j) e[k][j] = (wk[k] != 0.0f && lane + 64 * j < gin) ? ek[k][lane + 64 * j] : 0.0f;
            }
            MI355_UNROLL
            for (int j = 0; j < MIX_NJ; ++j) {
                const int i = lane + 64 * j;
                float g = 0.0f;
                bool any = false;
                MI355_UNROLL
                for (int k = 0; k < SPEAKER_MIX_MAX_TERMS; ++k) {
                    if (wk[k] != 0.0f) {
                        const float p = wk[k] * e[k][j];
                        g = any ? g + p : p;
                        any = true;
                    }
                }
                if (i < gin) {
                    gl[r * gin + i] = g;
                    if (write_g) a.g[b * gin + i] = g;
                }
            }
        } else {
            for (int i = lane; i < gin; i += 64) {
                float g = 0.0f;
                bool any = false;
                MI355_UNROLL
                for (int k = 0; k < SPEAKER_MIX_MAX_TERMS; ++k) {
                    if (wk[k] != 0.0f) {
                        const float p = wk[k] * ek[k][i];
                        g = any ? g + p : p;
                        any = true;
                    }
                }
                gl[r * gin + i] = g;
                if (write_g) a.g[b * gin + i] = g;
            }
        }
    }
    __syncthreads();
    if (c_base >= Cout) return;  // the whole wave: a tile's tail

    // lane c stores channel c_base + c (guarded at the store)
    const int co_lane = c_base + (lane < MIX_CPW ? lane : 0);
    const bool store = lane < MIX_CPW && co_lane < Cout;
    const float bias_lane = (bias && store) ? bias[co_lane] : 0.0f;

    if (small) {
        for (int r = 0; r < nrows; ++r) {
            float gv[MIX_NJ];
            MI355_UNROLL
            for (int j = 0; j < MIX_NJ; ++j) {
                const int i = lane + 64 * j;
                gv[j] = i < gin ? gl[r * gin + i] : 0.0f;
            }
            float res = 0.0f;
            MI355_UNROLL
            for (int c = 0; c < MIX_CPW; ++c) {
                float acc = 0.0f;
                MI355_UNROLL
                for (int j = 0; j < MIX_NJ; ++j)
                    if (lane + 64 * j < gin) acc = fmaf(wr[c][j], gv[j], acc);
                acc = wave_reduce_sum(acc);
                if (lane == c) res = acc;
            }
            if (store) out[(long)(b0 + r) * Cout + co_lane] = res + (bias ? bias_lane : 0.0f);
        }
    } else {
        for (int r = 0; r < nrows; ++r) {
            float res = 0.0f;
            MI355_UNROLL
            for (int c = 0; c < MIX_CPW; ++c) {
                const int co = c_base + c < Cout ? c_base + c : Cout - 1;
                float acc = 0.0f;
                for (int i = lane; i < gin; i += 64) acc = fmaf(W[(long)co * gin + i], gl[r * gin + i], acc);
                acc = wave_reduce_sum(acc);
                if (lane == c) res = acc;
            }
            if (store) out[(long)(b0 + r) * Cout + co_lane] = res + (bias ? bias_lane : 0.0f);
        }
    }
}

void launch_speaker_cond_mix(SpeakerMixArgs a, hipStream_t s) {
    if (a.B <= 0) return;
    if (a.gin < 1 || a.gin > SPEAKER_MIX_LDS_FLOATS / 2 || a.n_jobs < 1 || a.n_jobs > SPEAKER_MIX_MAX_JOBS || !a.g ||
        (a.vectors ? a.K != 0 : (a.K < 1 || a.K > SPEAKER_MIX_MAX_TERMS || !a.emb_g || !a.sid || !a.weight)))
        throw std::runtime_error("launch_speaker_cond_mix: bad arguments");
    int tiles = 0;
    for (int q = 0; q < a.n_jobs; ++q) {
        if (a.jobs[q].Cout < 1 || !a.jobs[q].w || !a.jobs[q].out) throw std::runtime_error("launch_speaker_cond_mix: bad job");
        a.jobs[q].first_tile = tiles;
        tiles += (a.jobs[q].Cout + SPEAKER_MIX_TILE - 1) / SPEAKER_MIX_TILE;
    }
    const int rb = std::min(SPEAKER_MIX_ROWS, SPEAKER_MIX_LDS_FLOATS / a.gin);
    const size_t shmem = (size_t)std::min(rb, a.B) * a.gin * sizeof(float);
    LAUNCH_KERNEL(k_speaker_cond_mix, dim3(tiles, (a.B + rb - 1) / rb), dim3(256), shmem, s, a, rb);
}

}  // namespace m355
