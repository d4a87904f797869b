// kernels_edges.cpp — the quiet edges of every row of a run (mi355vits_set_edge_trim, mi355vits_fetch_edges, trimmed packed streams).
//   thr = peak * ratio in ONE f32 multiply (round to nearest); sample k of a row is loud iff fabsf(y[k]) >= thr; the kernel finds
//   the first and the last loud sample of each row's valid samples [0, n).  keep_samples and the clamps to [0, n] are the host's.
//   * A work item is (row, tile of 4,096 samples): grid (tiles of the longest row, B), so one long row spreads over the chip like
//     many short ones; a tile past its row's end leaves at once.
//   * 256 lanes take 16 samples each as four 16-byte loads; load j of lane l is the quad at j * 1024 + 4 l of the tile, so a
//     wave's load is 1 KB in a row.  Row bases are b * audio_bs floats and need not be 16-byte aligned: the tiles start at the
//     16-byte boundary at or before the row's first sample (up to 3 floats before it), and a quad that is not wholly inside [0, n)
//     — the first of such a row, the last of any row — goes sample by sample through a clamped index.  No load leaves [0, n).
//   * A sample takes part by SELECT on 0 <= k < n, never by a multiply: what lies behind a row in the workspace (NaN, Inf) is
//     neither loaded nor looked at.  A NaN among the valid samples compares false and is not loud.
//   * Per lane the smallest and the largest loud index, then min / max over the wave by xor butterfly, over the four waves through
//     LDS, and per tile that holds a loud sample ONE integer atomicMin and ONE atomicMax on the row's two words.  Integer min / max
//     are exact in any order: the result does not depend on the grid, the batch or the order the tiles finish in.  No float atomics.
//   * The two words of a row are set to (n, -1) by k_edges_init on the same stream before: nothing is assumed about what the
//     workspace holds.  A row without a loud sample (NaN peak, n = 0) keeps them.
#include "kernels.h"

#include <algorithm>

namespace m355 {

#ifdef MI355_EMU
// the CPU model's header has neither; a lone f32 multiply whose result is only compared cannot be contracted there
static inline int atomicMin(int* p, int v) {
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static inline float __fmul_rn(float a, float b) {
    volatile float r = a * b;
    return r;
}
#endif

constexpr int EDGES_TILE = 4096;  // samples per work item: 256 lanes x four 16-byte loads
constexpr int EDGES_NONE = 0x7fffffff;

__global__ __launch_bounds__(256) void k_edges_init(const int* __restrict__ alen, int B, int* __restrict__ first, int* __restrict__ last) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int n = alen[b];
    first[b] = n > 0 ? n : 0;
    last[b] = -1;
}

__device__ __forceinline__ void edges_take(float v, bool in, float thr, int k, int& lo, int& hi) {
    const bool loud = in && fabsf(v) >= thr;  // NaN: false
    lo = loud ? (k < lo ? k : lo) : lo;
    hi = loud ? (k > hi ? k : hi) : hi;
}

__global__ __launch_bounds__(256) void k_edges(const float* __restrict__ audio, long audio_bs, const int* __restrict__ alen,
                                               const unsigned* __restrict__ peak_bits, float ratio, int* __restrict__ first,
                                               int* __restrict__ last) {
    __shared__ int sh_lo[4], sh_hi[4];
    const int b = blockIdx.y;
    const int n = alen[b];
    if (n <= 0) return;
    const float* y = audio + (long)b * audio_bs;
    // floats of the row's base past a 16-byte boundary: sample `-mis` is where the tiles start (never loaded when mis > 0)
    const int mis = (int)((reinterpret_cast<uintptr_t>(y) >> 2) & 3);
    const long base = (long)blockIdx.x * EDGES_TILE - mis;
    if (base >= n) return;  // block-uniform: nobody waits at the barrier below
    const float thr = __fmul_rn(__uint_as_float(peak_bits[b]), ratio);
    int lo = EDGES_NONE, hi = -1;
    if (base >= 0 && base + EDGES_TILE <= n) {
        // a tile wholly inside the row: four aligned 16-byte loads in flight, then the compares in ascending order
        float4 q[4];
        MI355_UNROLL
        for (int j = 0; j < 4; ++j) q[j] = *reinterpret_cast<const float4*>(y + base + j * 1024 + 4 * (int)threadIdx.x);
        MI355_UNROLL
        for (int j = 0; j < 4; ++j) {
            const int k = (int)base + j * 1024 + 4 * (int)threadIdx.x;
            edges_take(q[j].x, true, thr, k, lo, hi);
            edges_take(q[j].y, true, thr, k + 1, lo, hi);
            edges_take(q[j].z, true, thr, k + 2, lo, hi);
            edges_take(q[j].w, true, thr, k + 3, lo, hi);
        }
    } else {
        MI355_UNROLL
        for (int j = 0; j < 4; ++j) {
            const long k = base + j * 1024 + 4 * (long)threadIdx.x;
            if (k >= 0 && k + 4 <= n) {
                const float4 q = *reinterpret_cast<const float4*>(y + k);
                edges_take(q.x, true, thr, (int)k, lo, hi);
                edges_take(q.y, true, thr, (int)k + 1, lo, hi);
                edges_take(q.z, true, thr, (int)k + 2, lo, hi);
                edges_take(q.w, true, thr, (int)k + 3, lo, hi);
            } else if (k + 4 > 0 && k < n) {
                // the row's first or last quad: a clamped index, the value selected afterwards
                MI355_UNROLL
                for (int c = 0; c < 4; ++c) {
                    const long kc = k + c;
                    const bool in = kc >= 0 && kc < n;
                    const float v = y[in ? kc : 0L];
                    edges_take(v, in, thr, (int)kc, lo, hi);
                }
            }
        }
    }
    MI355_UNROLL
    for (int m = 32; m >= 1; m >>= 1) {
        const int ol = __shfl_xor(lo, m), oh = __shfl_xor(hi, m);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh_lo[wave] = lo;
        sh_hi[wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        MI355_UNROLL
        for (int w = 1; w < 4; ++w) {
            lo = sh_lo[w] < lo ? sh_lo[w] : lo;
            hi = sh_hi[w] > hi ? sh_hi[w] : hi;
        }
        if (hi >= 0) {
            atomicMin(first + b, lo);
            atomicMax(last + b, hi);
        }
    }
}

void launch_edges(const float* audio, long audio_bs, const int* alen, const unsigned* peak_bits, int B, long l_max, float ratio,
                  int* first, int* last, hipStream_t s) {
    if (B <= 0) return;
    LAUNCH_KERNEL(k_edges_init, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, alen, B, first, last);
    if (l_max <= 0) return;
    const long tiles = (l_max + 3 + EDGES_TILE - 1) / EDGES_TILE;  // + 3: a row may start up to 3 floats into its first tile
    for (int b0 = 0; b0 < B; b0 += 65535) {  // (a grid's y extent)
        const int nb = std::min(B - b0, 65535);
        LAUNCH_KERNEL(k_edges, dim3((unsigned)tiles, (unsigned)nb), dim3(256), 0, s, audio + (long)b0 * audio_bs, audio_bs, alen + b0,
                      peak_bits + b0, ratio, first + b0, last + b0);
    }
}

}  // namespace m355
