// kernels_limit.cpp — k_limit: the look-ahead peak limiter of the packed streams (mi355vits_set_loudness_limiter,
// mi355vits_fetch_limiter): the per-sample scale of a row whose peak the ceiling would otherwise hold below its loudness target.
// The rule (include/mi355vits.h) is exact — integers wherever an order could matter:
//     a[t]  = g * fabs((double) x[t])                              rq[t] = a[t] > c ? (int) floor((c / a[t]) * 2^30) : 2^30  (NaN, t < 0, t >= n: 2^30)
//     mq[i] = min rq[i .. i + L]                                   sq[k] = sum mq[k - L .. k]   (int64)
//     scale[k] = (float)(U * (g * ((double) sq[k] / ((double)(L + 1) * 2^30))))
//   * A job is one row under one (g, c, U); a work item is (job, tile of 4,096 consecutive samples); the grid is the items of the
//     jobs and nothing else.  What an item computes depends on (n, L, its tile) only — not on the grid, the batch or the row's address.
//   * The tile and L samples on each side are staged as rq into LDS (at most 12,288 int32 = 48 KB) with 16-byte loads from the
//     aligned quad at or before the first sample; a quad not wholly inside the row goes sample by sample through a clamped index,
//     and a value takes part by SELECT on 0 <= t < n: no load leaves the row.
//   * Window minimum in place by doubling passes: a pass widens every window from w to w + min(w, L + 1 - w) samples — each lane
//     reads its (at most 48) pairs into registers, barrier, stores them, barrier; ceil(log2(L + 1)) passes.
//   * Window sum: every lane sums an odd number E of consecutive mq (odd: the lanes' strided reads fall on distinct banks), a
//     Hillis-Steele scan over the 256 sums gives the prefix at every E-th element, a lane then makes sq of its first sample from
//     two prefixes and slides over its 17 consecutive samples (sq[k + 1] = sq[k] + mq[k + 1] - mq[k - L]).  int64 throughout: exact
//     in any order.
//   * Every curve element has exactly one writer (a plain store).  The two statistics of a job — min sq and the count of
//     sq < (L + 1) 2^30 — are reduced over the workgroup and go through ONE integer atomicMin and ONE atomicAdd per item, on words
//     k_limit_init set on the same stream before: the workspace is never assumed clean.
//   * k_limit<true> (the true-peak ceiling mode, kernels_truepeak.cpp): a[t] = g * e[t] with e[t] read from the envelope array
//     k_true_peak_env wrote for the same job table; everything behind rq is the same code.
#include "kernels.h"

#include <algorithm>

namespace m355 {

#ifdef MI355_EMU
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) {
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
#endif

constexpr int LIMIT_ONE = 1 << 30;
constexpr int LIMIT_NE = (LIMIT_TILE + 2 * LIMIT_MAX_WINDOW + 255) / 256;  // staged elements per lane at the largest window: 48
constexpr int LIMIT_BUF = LIMIT_NE * 256;
constexpr int LIMIT_C = 17;  // consecutive samples a lane slides over: odd, 256 * 17 >= LIMIT_TILE
static_assert(256 * LIMIT_C >= LIMIT_TILE, "the lanes' samples cover the tile");
static_assert(256 * (((LIMIT_TILE + LIMIT_MAX_WINDOW + 255) / 256) | 1) <= LIMIT_BUF, "the lanes' summed elements stay inside the buffer");

__global__ __launch_bounds__(256) void k_limit_init(LimitStat* __restrict__ stats, int n_jobs, int L) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_jobs) return;
    stats[j].sq_min = (unsigned long long)(L + 1) << 30;
    stats[j].reduced = 0;
    stats[j].pad = 0;
}

__device__ __forceinline__ int limit_rq_abs(double ax, bool in, double g, double c) {
    const double a = g * ax;
    const bool over = in && a > c;  // NaN compares false
    const int q = (int)floor((c / (over ? a : c)) * 1073741824.0);  // (the quotient of a sample that is not over is 1: no division by 0)
    return over ? q : LIMIT_ONE;
}
__device__ __forceinline__ int limit_rq(float x, bool in, double g, double c) { return limit_rq_abs(fabs((double)x), in, g, c); }

// ENV: the true-peak ceiling mode — a sample's rq is made from env[job.off + t] (k_true_peak_env's e[t], never NaN) and the audio is
// not read.  ENV = false is the sample-peak kernel as it always was.
template <bool ENV>
__global__ __launch_bounds__(256) void k_limit(const LimitJob* __restrict__ jobs, int n_jobs, int L, const float* __restrict__ audio,
                                               long audio_bs, LimitStat* __restrict__ stats, float* __restrict__ curve,
                                               const double* __restrict__ env) {
    __shared__ int buf[LIMIT_BUF];
    __shared__ long long sc[2][256];
    __shared__ long long tp[257];
    __shared__ unsigned long long sh_min[4];
    __shared__ int sh_cnt[4];
    const int tid = threadIdx.x;
    // the job this item belongs to: the last one whose first item is at or before it (uniform per workgroup)
    int jl = 0, jh = n_jobs;
    while (jl < jh) {
        const int mid = (jl + jh) >> 1;
        if (jobs[mid].tile0 <= (int)blockIdx.x) jl = mid + 1;
        else jh = mid;
    }
    const int job = jl - 1;
    const double g = jobs[job].g, c = jobs[job].c, U = jobs[job].U;
    const int n = jobs[job].n;
    const long k0 = (long)((int)blockIdx.x - jobs[job].tile0) * LIMIT_TILE;  // the tile's first sample
    if (k0 >= n) return;                                                     // (block-uniform; the host makes no such item)
    const int Te = n - k0 < LIMIT_TILE ? (int)(n - k0) : LIMIT_TILE;         // the tile's samples
    const int N = Te + 2 * L, M = Te + L;                                    // staged rq: samples [k0 - L, k0 + Te + L); mq: [k0 - L, k0 + Te)
    const float* y = audio + (long)jobs[job].row * audio_bs;
    const int mis = (int)((reinterpret_cast<uintptr_t>(y) >> 2) & 3);
    // ---- stage rq of [t0, t0 + N) from the aligned quad at or before t0
    const long t0 = k0 - L;
    const int sh = (int)((mis + t0) & 3);
    const long w0 = t0 - sh;
    const int nq = (N + sh + 3) >> 2;
    if constexpr (ENV) {  // (doubles in the limiter's own workspace, one per sample of the job: no quads, no alignment question)
        const double* e = env + (long)jobs[job].off;
        for (int j = tid; j < N; j += 256) {
            const long k = t0 + j;
            const bool in = k >= 0 && k < n;
            buf[j] = limit_rq_abs(e[in ? k : 0L], in, g, c);
        }
    } else {
        for (int q = tid; q < nq; q += 256) {
            const long k = w0 + 4L * q;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            bool in[4] = {false, false, false, false};
            if (k >= 0 && k + 4 <= n) {
                const float4 a = *reinterpret_cast<const float4*>(y + k);
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
                in[0] = in[1] = in[2] = in[3] = true;
            } else if (k + 4 > 0 && k < n) {
                MI355_UNROLL
                for (int cc = 0; cc < 4; ++cc) {
                    const long kc = k + cc;
                    in[cc] = kc >= 0 && kc < n;
                    v[cc] = y[in[cc] ? kc : 0L];
                }
            }
            MI355_UNROLL
            for (int cc = 0; cc < 4; ++cc) {
                const int j = 4 * q + cc - sh;
                if (j >= 0 && j < N) buf[j] = limit_rq(v[cc], in[cc], g, c);
            }
        }
    }
    __syncthreads();
    // ---- mq in place: buf[i] = min rq[i .. i + L] for i < M (what lies at and past M is never read as a minimum)
    {
        const int W = L + 1;
        int cur = 1;
        while (cur < W) {  // uniform
            const int step = cur < W - cur ? cur : W - cur;
            int r[LIMIT_NE];
            MI355_UNROLL
            for (int e = 0; e < LIMIT_NE; ++e) {
                const int i = tid + 256 * e;
                if (i < N) {
                    const int a = buf[i], b = buf[i + step < N ? i + step : i];
                    r[e] = a < b ? a : b;
                }
            }
            __syncthreads();
            MI355_UNROLL
            for (int e = 0; e < LIMIT_NE; ++e) {
                const int i = tid + 256 * e;
                if (i < N) buf[i] = r[e];
            }
            __syncthreads();
            cur += step;
        }
    }
    // ---- the prefix of mq at every E-th element: tp[j] = sum buf[0 .. j E)
    const int E = ((M + 255) >> 8) | 1;
    {
        long long u = 0;
        for (int e = 0; e < E; ++e) {
            const int i = tid * E + e;
            const int m = buf[i < M ? i : 0];
            u += i < M ? (long long)m : 0LL;
        }
        MI355_UNROLL
        for (int st = 0; st < 8; ++st) {
            const int d = 1 << st, b = st & 1;
            sc[b][tid] = u;
            __syncthreads();
            if (tid >= d) u += sc[b][tid - d];
        }
        tp[tid + 1] = u;
        if (tid == 0) tp[0] = 0;
        __syncthreads();
    }
    auto prefix = [&](int x) {  // sum buf[0 .. x), 0 <= x <= M
        const int ch = x / E;
        long long r = tp[ch];
        for (int i = ch * E; i < x; ++i) r += buf[i];
        return r;
    };
    // ---- sq, the scale and the statistics of the lane's samples: sample k0 + o has its window's mq at buf[o .. o + L]
    const long long full = (long long)(L + 1) << 30;
    const double den = (double)(L + 1) * 1073741824.0;
    unsigned long long lmin = (unsigned long long)full;
    int cnt = 0;
    const int o0 = tid * LIMIT_C;
    if (o0 < Te) {
        long long s = prefix(o0 + L + 1) - prefix(o0);
        const long cbase = (long)jobs[job].off + k0;
        for (int cc = 0; cc < LIMIT_C; ++cc) {
            const int o = o0 + cc;
            if (o >= Te) break;
            if (cc > 0) s += (long long)buf[o + L] - (long long)buf[o - 1];
            const double sd = (double)s / den;
            const float scale = (float)(U * (g * sd));
            if (curve) curve[cbase + o] = scale;
            lmin = (unsigned long long)s < lmin ? (unsigned long long)s : lmin;
            cnt += s < full ? 1 : 0;
        }
    }
    MI355_UNROLL
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long om = __shfl_xor(lmin, m);
        const int oc = __shfl_xor(cnt, m);
        lmin = om < lmin ? om : lmin;
        cnt += oc;
    }
    if ((tid & 63) == 0) {
        sh_min[tid >> 6] = lmin;
        sh_cnt[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        MI355_UNROLL
        for (int w = 1; w < 4; ++w) {
            lmin = sh_min[w] < lmin ? sh_min[w] : lmin;
            cnt += sh_cnt[w];
        }
        if (cnt > 0) {  // (a tile whose every sq is full leaves the words as k_limit_init set them)
            atomicMin(&stats[job].sq_min, lmin);
            atomicAdd(&stats[job].reduced, cnt);
        }
    }
}

long limit_place_jobs(LimitJob* jobs, int n_jobs, long* curve_floats) {
    long off = 0, tiles = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (jobs[j].n < 1) return -1;
        jobs[j].off = (int)off;
        jobs[j].tile0 = (int)tiles;
        off += jobs[j].n;
        tiles += (jobs[j].n + LIMIT_TILE - 1) / LIMIT_TILE;
        if (off > LIMIT_MAX_CURVE) return -1;
    }
    if (curve_floats) *curve_floats = off;
    return tiles;
}

void launch_limit(const LimitJob* jobs, int n_jobs, long tiles, int L, const float* audio, long audio_bs, LimitStat* stats, float* curve,
                  hipStream_t s, const double* env) {
    if (n_jobs <= 0 || L < 1 || L > LIMIT_MAX_WINDOW) return;
    LAUNCH_KERNEL(k_limit_init, dim3((unsigned)((n_jobs + 255) / 256)), dim3(256), 0, s, stats, n_jobs, L);
    if (tiles <= 0) return;
    if (env) {
        LAUNCH_KERNEL(k_limit<true>, dim3((unsigned)tiles), dim3(256), 0, s, jobs, n_jobs, L, audio, audio_bs, stats, curve, env);
    } else {
        LAUNCH_KERNEL(k_limit<false>, dim3((unsigned)tiles), dim3(256), 0, s, jobs, n_jobs, L, audio, audio_bs, stats, curve, env);
    }
}

}  // namespace m355
