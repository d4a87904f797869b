// mfma_fillers.hip — how many single-issue instructions ride for free beside a bf16 MFMA on gfx950, per MFMA shape and per
// waves-per-SIMD?  Development tool (not part of libmi355vits.so):
//   hipcc --offload-arch=gfx950 -O3 tools/mfma_fillers.hip -o tools/mfma_fillers && tools/mfma_fillers
// Every wave runs a loop of MFMAs on two independent accumulator chains; between two MFMAs it issues F independent
// v_fma_f32 fillers (and optionally one ds_read_b128 per two MFMAs).  One workgroup per CU.  Prints ns per MFMA and the
// cycles that is at the clock measured by s_memtime.
//   tools/mfma_fillers random : the SHAPE question on random data (MI355X lowers its clock under matrix load, and by how much can depend
// on the MFMA shape; ramp or zero operands hide that).  Both bf16 shapes at the WaveNet layer's output tile per wave, 96 rows x 128
// columns, one wave per SIMD, every operand uniform in [-1, 1) and re-read from LDS with ds_read_b128 one step ahead.  Prints ns per
// FLOP, cycles per MFMA and the in-kernel clock (s_memtime / s_memrealtime) after two seconds of back-to-back launches.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <random>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cstring>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

template <int SHAPE, int F, int LDS>
__global__ __launch_bounds__(512) void k(float* out, int iters, long long* cyc) {
    extern __shared__ uint4 sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < 2048; i += blockDim.x) sm[i] = uint4{(unsigned)i, 1u, 2u, 3u};
    __syncthreads();
    bf16x8 a, b;
    for (int i = 0; i < 8; ++i) { a[i] = (__bf16)(0.001f * (lane + i)); b[i] = (__bf16)(0.002f * (lane - i)); }
    float x[8];
    for (int i = 0; i < 8; ++i) x[i] = 0.5f + i + lane;
    const float m = 1.0001f, c = 0.25f;
    uint4 r = sm[lane];
    long long t0 = 0;
    if (tid == 0) t0 = __builtin_readcyclecounter();
    if constexpr (SHAPE == 16) {
        f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc0, 0, 0, 0);
#pragma unroll
                for (int f = 0; f < F; ++f) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[f]) : "v"(m), "v"(c));
                if (LDS) { asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"((lane * 16 + u * 1024) & 32767)); }
                acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc1, 0, 0, 0);
#pragma unroll
                for (int f = 0; f < F; ++f) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[f]) : "v"(m), "v"(c));
            }
            if (LDS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        out[blockIdx.x * blockDim.x + tid] = acc0[0] + acc1[1] + x[0] + x[1] + x[2] + x[3] + x[4] + x[5] + x[6] + x[7] + (float)r.x;
    } else {
        f32x16 acc0, acc1;
        for (int i = 0; i < 16; ++i) { acc0[i] = 0; acc1[i] = 0; }
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc0, 0, 0, 0);
#pragma unroll
                for (int f = 0; f < F; ++f) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[f & 7]) : "v"(m), "v"(c));
                if (LDS) { asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"((lane * 16 + u * 1024) & 32767)); }
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc1, 0, 0, 0);
#pragma unroll
                for (int f = 0; f < F; ++f) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[f & 7]) : "v"(m), "v"(c));
            }
            if (LDS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        out[blockIdx.x * blockDim.x + tid] = acc0[0] + acc1[1] + x[0] + x[1] + x[2] + x[3] + x[4] + x[5] + x[6] + x[7] + (float)r.x;
    }
    if (tid == 0 && blockIdx.x == 0) cyc[0] = __builtin_readcyclecounter() - t0;
}

template <int SHAPE, int F, int LDS>
void run(int waves, float* d_out, long long* d_cyc) {
    const int iters = 4000, grid = 256;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    k<SHAPE, F, LDS><<<grid, waves * 64, 32768>>>(d_out, 100, d_cyc);
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    k<SHAPE, F, LDS><<<grid, waves * 64, 32768>>>(d_out, iters, d_cyc);
    CHECK(hipEventRecord(e1));
    CHECK(hipDeviceSynchronize());
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    long long cyc = 0;
    CHECK(hipMemcpy(&cyc, d_cyc, 8, hipMemcpyDeviceToHost));
    const double mfma_per_simd = (double)iters * 16 * (waves / 4.0);
    printf("shape %2d  waves/SIMD %d  fillers/MFMA %d  lds %d : %.2f ns per MFMA and SIMD, %.1f shader cycles per MFMA and SIMD (clock %.2f GHz)\n", SHAPE,
           waves / 4, F, LDS, ms * 1e6 / mfma_per_simd, (double)cyc / mfma_per_simd, cyc / (ms * 1e6));
}

// ---- shape A/B on random operands.  A step is 32 channels of k: 96 x 128 x 32 per wave = 48 16x16x32 or 24 32x32x16 MFMAs, and 14
// ds_read_b128 (6 + 8 or 2 x (3 + 4) fragments) either way.  LDS holds four steps' fragments (896 uint4 each), walked round.
#define RND_FENCE() __builtin_amdgcn_sched_barrier(0)
// accumulate in place, as inline assembly: with the builtin hipcc rotates the accumulators of this two-step loop through copies
// (v_accvgpr_mov between the MFMAs: 30 instead of 16 cycles per 16x16x32)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void mfma16_ip(f32x4& c, const uint4& a, const uint4& b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(__builtin_bit_cast(u32x4, a)), "v"(__builtin_bit_cast(u32x4, b)));
}
__device__ __forceinline__ void mfma32_ip(f32x16& c, const uint4& a, const uint4& b) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(__builtin_bit_cast(u32x4, a)), "v"(__builtin_bit_cast(u32x4, b)));
}
template <int SHAPE>
__global__ __launch_bounds__(256) void k_rnd(const uint4* __restrict__ src, float* out, int steps, unsigned long long* stamps) {
    __shared__ uint4 sm[4 * 896];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < 4 * 896; i += 256) sm[i] = src[i];
    __syncthreads();
    uint4 fr[2][14];
#pragma unroll
    for (int f = 0; f < 14; ++f) fr[0][f] = sm[f * 64 + lane];
    unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    if constexpr (SHAPE == 16) {
        f32x4 acc[6][8];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
        for (int s = 0; s < steps; s += 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int nb = ((s + h + 1) & 3) * 896 + lane;
#pragma unroll
                for (int f = 0; f < 14; ++f) fr[h ^ 1][f] = sm[nb + f * 64];
                RND_FENCE();
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int i = 0; i < 6; ++i)
                        mfma16_ip(acc[i][j], fr[h][i], fr[h][6 + j]);
                RND_FENCE();
            }
        }
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // the last MFMAs' results, before anything reads them
        float t = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) t += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
        out[blockIdx.x * 256 + tid] = t;
    } else {
        f32x16 acc[3][4];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
        for (int s = 0; s < steps; s += 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int nb = ((s + h + 1) & 3) * 896 + lane;
#pragma unroll
                for (int f = 0; f < 14; ++f) fr[h ^ 1][f] = sm[nb + f * 64];
                RND_FENCE();
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < 3; ++i)
                            mfma32_ip(acc[i][j], fr[h][kk * 7 + i], fr[h][kk * 7 + 3 + j]);
                RND_FENCE();
            }
        }
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
        float t = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) t += acc[i][j][r];
        out[blockIdx.x * 256 + tid] = t;
    }
    unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) { stamps[2 * blockIdx.x] = c1 - c0; stamps[2 * blockIdx.x + 1] = r1 - r0; }  // (a buffer of their own: no output reads them)
}

static int run_random(bool zeros) {
    const int grid = 256, steps = 20000;  // 20000 steps x 768 cycles: about 7 ms per launch
    std::vector<unsigned short> h(4 * 896 * 8);
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    for (auto& v : h) {
        const float f = zeros ? 0.0f : U(rng);
        unsigned u;
        memcpy(&u, &f, 4);
        v = (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
    uint4* d_src;
    float* d_out;
    unsigned long long* d_st;
    CHECK(hipMalloc(&d_src, h.size() * 2));
    CHECK(hipMalloc(&d_out, grid * 256 * 4));
    CHECK(hipMalloc(&d_st, grid * 16));
    CHECK(hipMemcpy(d_src, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    auto launch = [&](int shape) {
        if (shape == 16) k_rnd<16><<<grid, 256>>>(d_src, d_out, steps, d_st);
        else k_rnd<32><<<grid, 256>>>(d_src, d_out, steps, d_st);
    };
    printf("operands: %s, 256 workgroups x 4 waves, output tile per wave 96 x 128, %d steps of k = 32 per launch\n", zeros ? "all zero" : "uniform [-1, 1) bf16", steps);
    double ns_flop[2][5];
    for (int round = 0; round < 5; ++round)
        for (int si = 0; si < 2; ++si) {  // the two shapes alternate
            const int shape = si ? 32 : 16;
            const auto w0 = std::chrono::steady_clock::now();
            do {  // two seconds (first round; 0.5 s later) of back-to-back launches of this shape before the timed one
                for (int i = 0; i < 8; ++i) launch(shape);
                CHECK(hipDeviceSynchronize());
            } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < (round ? 0.5 : 2.0));
            CHECK(hipEventRecord(e0));
            launch(shape);
            CHECK(hipEventRecord(e1));
            CHECK(hipDeviceSynchronize());
            float ms = 0;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            std::vector<unsigned long long> st(2 * grid);
            CHECK(hipMemcpy(st.data(), d_st, grid * 16, hipMemcpyDeviceToHost));
            std::vector<double> clk(grid), cyc(grid);
            for (int b = 0; b < grid; ++b) { clk[b] = (double)st[2 * b] / (double)st[2 * b + 1] * 0.1; cyc[b] = (double)st[2 * b]; }
            std::sort(clk.begin(), clk.end());
            std::sort(cyc.begin(), cyc.end());
            const double flop = 2.0 * 96 * 128 * 32 * (double)steps * 4 * grid;
            const double mfmas = (double)steps * (shape == 16 ? 48 : 24);
            ns_flop[si][round] = ms * 1e6 / flop;
            printf("round %d  shape %s : %.3f ms  %.4e ns per FLOP  %.0f TF/s  %.2f cycles per MFMA  in-kernel clock %.3f GHz (median of %d workgroups)\n", round,
                   shape == 16 ? "16x16x32" : "32x32x16", ms, ms * 1e6 / flop, flop / (ms * 1e-3) * 1e-12, cyc[grid / 2] / mfmas, clk[grid / 2], grid);
        }
    std::sort(ns_flop[0], ns_flop[0] + 5);
    std::sort(ns_flop[1], ns_flop[1] + 5);
    printf("median ns per FLOP: 16x16x32 %.4e, 32x32x16 %.4e: the 16x16x32 loop delivers %.3f x the FLOP/s of the 32x32x16 loop\n", ns_flop[0][2], ns_flop[1][2],
           ns_flop[1][2] / ns_flop[0][2]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "random")) return run_random(false) || run_random(true);
    float* d_out;
    long long* d_cyc;
    CHECK(hipMalloc(&d_out, 256 * 512 * 4));
    CHECK(hipMalloc(&d_cyc, 8));
    for (int waves : {4, 8}) {
        run<16, 0, 0>(waves, d_out, d_cyc); run<16, 1, 0>(waves, d_out, d_cyc); run<16, 2, 0>(waves, d_out, d_cyc); run<16, 3, 0>(waves, d_out, d_cyc);
        run<16, 4, 0>(waves, d_out, d_cyc); run<16, 6, 0>(waves, d_out, d_cyc); run<16, 2, 1>(waves, d_out, d_cyc);
        run<32, 0, 0>(waves, d_out, d_cyc); run<32, 2, 0>(waves, d_out, d_cyc); run<32, 4, 0>(waves, d_out, d_cyc); run<32, 6, 0>(waves, d_out, d_cyc);
        run<32, 8, 0>(waves, d_out, d_cyc); run<32, 12, 0>(waves, d_out, d_cyc); run<32, 4, 1>(waves, d_out, d_cyc);
    }
    return 0;
}
