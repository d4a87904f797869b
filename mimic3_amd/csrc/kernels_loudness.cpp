// kernels_loudness.cpp — ITU-R BS.1770-4 / EBU R128 integrated loudness of every row of a run (mi355vits_set_loudness_target,
// mi355vits_fetch_loudness, normalised packed streams).  All arithmetic is IEEE double.
//   K-weighting = two biquads in cascade (high shelf, high pass; coefficients by the bilinear formulas of include/mi355vits.h for
//   any rate), zero state at sample 0; E_j = sum of y^2 over the 100 ms step j (S = (fs + 5) / 10 samples); 400 ms blocks every
//   step; absolute gate -70 LUFS, relative gate -10 LU.
//   * k_loud: the recurrence is linear with a 4-vector state (transposed direct form II, two words per biquad), so it is cut
//     exactly.  A work item is (row, K consecutive steps), grid (items of the longest row, B); an item past its row's end leaves
//     at once.  An item that does not begin at sample 0 begins W samples earlier from zero state: W(fs) is the smallest W with
//     sum_{k >= W} |h[k]| <= 2^-40 sum |h| of the cascade's impulse response, and K the smallest count with K S >= 4 W (the
//     warm-up is at most a quarter of the work).  Where an item starts and what it sums depend on (n, fs) only — not on the grid,
//     the CU count, the batch or the row's address.
//   * An item walks its samples in tiles of 8,192: 256 lanes x 32 consecutive samples.  A tile is staged into LDS with 16-byte
//     loads from the 16-byte boundary at or before its first sample (row bases need not be aligned; the lanes read at the
//     remaining shift of 0 .. 3 floats, so which lane owns which sample never depends on the address); a quad not wholly inside
//     the row goes sample by sample through a clamped index, and a value takes part by SELECT on 0 <= k < n, never by a multiply:
//     no load leaves the row and what a workspace holds behind it is never read.  One pad float per 32 keeps the lanes' strided
//     LDS reads on distinct banks.
//   * Pass 1: every lane runs its 32 samples from zero state (lane 0 from the state the previous tile left).  Scan: the end
//     states are combined by s_{l+1} = P s_l + v_l, P = A^32, as a Hillis-Steele scan over the 256 lanes through LDS with the
//     matrices P^(2^k) the host computed (8 steps of one 4x4 product).  Pass 2: every lane runs its samples again from its true
//     start state and sums y^2 into the one or two steps its chunk overlaps; warm-up samples are skipped by select.
//   * Per step one thread adds the lanes' partial sums in ascending lane order, tile after tile, and every E[row][j] is written
//     by exactly one plain store.  No atomics.
//   * k_loud_gate: one wave per row: z_i, both gates and (lufs, blocks, gated) with lane-strided sums and an xor butterfly — one
//     fixed order.
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>

namespace m355 {

constexpr int LOUD_C = 32;                   // consecutive samples a lane owns in a tile
constexpr int LOUD_TILE = 256 * LOUD_C;      // samples per tile
constexpr int LOUD_XS = LOUD_TILE + 4 + (LOUD_TILE + 4) / 32 + 1;  // staged floats: the tile, the alignment shift, one pad per 32

// One sample through the cascade.  c = {b0, b1, b2, a1, a2} of the shelf, then {a1, a2} of the high pass (b = 1, -2, 1).
#ifndef MI355_EMU
__host__
#endif
__device__ __forceinline__ double kw_step(const double* c, double x, double& s1, double& s2, double& t1, double& t2) {
    const double y1 = c[0] * x + s1;
    s1 = c[1] * x - c[3] * y1 + s2;
    s2 = c[2] * x - c[4] * y1;
    const double y2 = y1 + t1;
    t1 = t2 - 2.0 * y1 - c[5] * y2;
    t2 = y1 - c[6] * y2;
    return y2;
}

struct LoudParams {
    double c[7];
    double P[8][16];  // (A^32)^(2^k), row-major
    int S, W, K;
};

__device__ __forceinline__ int loud_slot(int p) { return p + (p >> 5); }

__global__ __launch_bounds__(256) void k_loud(LoudParams pr, const float* __restrict__ audio, long audio_bs, const int* __restrict__ alen,
                                              double* __restrict__ E, long ldE) {
    __shared__ float xs[LOUD_XS];
    __shared__ double sc[2][256][4];
    __shared__ double pa[256], pb[256];
    __shared__ double bins[LOUD_MAX_K];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int n = alen[b];
    const int S = pr.S;
    const long item0 = (long)blockIdx.x * pr.K * S;  // the item's first counted sample
    if (item0 >= n) return;                          // block-uniform (and n <= 0)
    const long item1 = item0 + (long)pr.K * S < n ? item0 + (long)pr.K * S : (long)n;
    const long first = item0 > pr.W ? item0 - pr.W : 0L;  // zero state here: exact at 0, W samples of warm-up elsewhere
    const float* y = audio + (long)b * audio_bs;
    const int mis = (int)((reinterpret_cast<uintptr_t>(y) >> 2) & 3);
    if (tid < LOUD_MAX_K) bins[tid] = 0.0;
    double carry[4] = {0.0, 0.0, 0.0, 0.0};
    for (long tk = first; tk < item1; tk += LOUD_TILE) {
        // ---- stage [tk, tk + TILE) from the aligned quad at or before it
        const int sh = (int)((mis + tk) & 3);
        const long w0 = tk - sh;
        for (int q = tid; q <= LOUD_TILE / 4; q += 256) {
            const long k = w0 + 4L * q;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (k >= 0 && k + 4 <= item1) {
                v = *reinterpret_cast<const float4*>(y + k);
            } else if (k + 4 > 0 && k < item1) {
                float e[4];
                MI355_UNROLL
                for (int cc = 0; cc < 4; ++cc) {
                    const long kc = k + cc;
                    const bool in = kc >= 0 && kc < item1;
                    const float a = y[in ? kc : 0L];
                    e[cc] = in ? a : 0.0f;
                }
                v = make_float4(e[0], e[1], e[2], e[3]);
            }
            const int p = loud_slot(4 * q);  // a quad never straddles a pad
            xs[p] = v.x;
            xs[p + 1] = v.y;
            xs[p + 2] = v.z;
            xs[p + 3] = v.w;
        }
        __syncthreads();
        const long k0 = tk + (long)tid * LOUD_C;  // the lane's first sample
        const int p0 = sh + tid * LOUD_C;
        const bool live = k0 < item1;
        // ---- pass 1: the chunk's end state from zero (lane 0: from the previous tile's)
        double u[4] = {0.0, 0.0, 0.0, 0.0};
        if (tid == 0) {
            MI355_UNROLL
            for (int i = 0; i < 4; ++i) u[i] = carry[i];
        }
        if (live) {
            for (int j = 0; j < LOUD_C; ++j) (void)kw_step(pr.c, (double)xs[loud_slot(p0 + j)], u[0], u[1], u[2], u[3]);
        }
        // ---- inclusive scan of the affine maps s -> P s + v over the lanes
        MI355_UNROLL
        for (int st = 0; st < 8; ++st) {
            const int d = 1 << st, buf = st & 1;
            MI355_UNROLL
            for (int i = 0; i < 4; ++i) sc[buf][tid][i] = u[i];
            __syncthreads();
            if (tid >= d) {
                double o[4];
                MI355_UNROLL
                for (int i = 0; i < 4; ++i) o[i] = sc[buf][tid - d][i];
                MI355_UNROLL
                for (int i = 0; i < 4; ++i) {
                    double a = u[i];
                    MI355_UNROLL
                    for (int j = 0; j < 4; ++j) a += pr.P[st][4 * i + j] * o[j];
                    u[i] = a;
                }
            }
        }
        MI355_UNROLL
        for (int i = 0; i < 4; ++i) sc[0][tid][i] = u[i];  // (step 7 read buffer 1)
        __syncthreads();
        double s[4];
        MI355_UNROLL
        for (int i = 0; i < 4; ++i) s[i] = tid == 0 ? carry[i] : sc[0][tid > 0 ? tid - 1 : 0][i];
        MI355_UNROLL
        for (int i = 0; i < 4; ++i) carry[i] = sc[0][255][i];
        // ---- pass 2: again from the true state; y^2 into the step the chunk starts in (pa) and the next one (pb)
        double sa = 0.0, sb = 0.0;
        if (live) {
            const long kb = (k0 / S + 1) * S;  // S >= LOUD_C: a chunk meets at most one step boundary
            for (int j = 0; j < LOUD_C; ++j) {
                const long k = k0 + j;
                const double v = kw_step(pr.c, (double)xs[loud_slot(p0 + j)], s[0], s[1], s[2], s[3]);
                const double e = (k >= item0 && k < item1) ? v * v : 0.0;
                sa += k < kb ? e : 0.0;
                sb += k < kb ? 0.0 : e;
            }
        }
        pa[tid] = sa;
        pb[tid] = sb;
        __syncthreads();
        // ---- per step of this tile one thread, the lanes in ascending order
        {
            const long j = tk / S + tid;  // the tile's steps: tk / S .. (tk + TILE - 1) / S, fewer than 256
            const long lo = j * S, hi = lo + S;
            if (lo < tk + LOUD_TILE && lo < item1 && hi > item0 && j >= (long)blockIdx.x * pr.K) {
                const int la = lo <= tk ? 0 : (int)((lo - tk) / LOUD_C);
                const long lh = (hi - 1 - tk) / LOUD_C;
                const int lb = lh < 255 ? (int)lh : 255;
                double acc = 0.0;
                for (int l = la; l <= lb; ++l) {
                    const long j0 = (tk + (long)l * LOUD_C) / S;
                    acc += j0 == j ? pa[l] : pb[l];
                }
                bins[(int)(j - (long)blockIdx.x * pr.K)] += acc;
            }
        }
        __syncthreads();  // xs, pa / pb and sc are written again by the next tile
    }
    if (tid < pr.K) {
        const long j = (long)blockIdx.x * pr.K + tid;
        if (j * S < item1) E[(long)b * ldE + j] = bins[tid];
    }
}

__device__ __forceinline__ double loud_wave_sum(double v) {
    MI355_UNROLL
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(64) void k_loud_gate(const double* __restrict__ E, long ldE, const int* __restrict__ alen, int S,
                                                  double* __restrict__ lufs, int* __restrict__ blocks, int* __restrict__ gated) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = alen[b];
    const double NEG_INF = -HUGE_VAL;
    if (n <= 0) {  // wave-uniform
        if (lane == 0) {
            lufs[b] = NEG_INF;
            blocks[b] = 0;
            gated[b] = 0;
        }
        return;
    }
    const double* e = E + (long)b * ldE;
    const bool whole = n >= 4 * S;
    const int nb = whole ? (n - 4 * S) / S + 1 : 1;
    const int ns = (n + S - 1) / S;
    const double den = whole ? 4.0 * (double)S : (double)n;
    auto z_of = [&](int i) {
        double a = e[i];
        if (whole) {
            a = ((a + e[i + 1]) + e[i + 2]) + e[i + 3];
        } else {
            for (int j = 1; j < ns; ++j) a += e[j];  // the short row's one block: all of its (at most four) steps
        }
        return a / den;
    };
    double sum = 0.0;
    int cnt = 0;
    for (int i = lane; i < nb; i += 64) {
        const double z = z_of(i);
        const bool in = -0.691 + 10.0 * log10(z) > -70.0;
        sum += in ? z : 0.0;
        cnt += in ? 1 : 0;
    }
    sum = loud_wave_sum(sum);
    cnt = (int)loud_wave_sum((double)cnt);
    double out = NEG_INF;
    int ng = 0;
    if (cnt > 0) {  // wave-uniform: every lane holds the same sums
        const double rel = -0.691 + 10.0 * log10(sum / (double)cnt) - 10.0;
        double sum2 = 0.0;
        int cnt2 = 0;
        for (int i = lane; i < nb; i += 64) {
            const double z = z_of(i);
            const double l = -0.691 + 10.0 * log10(z);
            const bool in = l > -70.0 && l > rel;
            sum2 += in ? z : 0.0;
            cnt2 += in ? 1 : 0;
        }
        sum2 = loud_wave_sum(sum2);
        ng = (int)loud_wave_sum((double)cnt2);
        if (ng > 0) out = -0.691 + 10.0 * log10(sum2 / (double)ng);
    }
    if (lane == 0) {
        lufs[b] = out;
        blocks[b] = nb;
        gated[b] = ng;
    }
}

// ---------------------------------------------------------------- the host's side: coefficients, W(fs), K and the scan matrices
static void mat4_mul(const double* a, const double* b, double* out) {
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double v = 0.0;
            for (int k = 0; k < 4; ++k) v += a[4 * i + k] * b[4 * k + j];
            r[4 * i + j] = v;
        }
    std::copy(r, r + 16, out);
}

static void loudness_design(int fs, LoudnessPlan& p, LoudParams& q) {
    const double PI = 3.14159265358979323846;
    p.fs = fs;
    p.S = (fs + 5) / 10;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(PI * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        p.c[0] = (Vh + Vb * K / Q + K * K) / a0;
        p.c[1] = 2.0 * (K * K - Vh) / a0;
        p.c[2] = (Vh - Vb * K / Q + K * K) / a0;
        p.c[3] = 2.0 * (K * K - 1.0) / a0;
        p.c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(PI * f0 / fs), a0 = 1.0 + K / Q + K * K;
        p.c[5] = 2.0 * (K * K - 1.0) / a0;
        p.c[6] = (1.0 - K / Q + K * K) / a0;
    }
    // W: the impulse response out to where it has stayed below 1e-25 of its sum for 4,096 samples, then the tail sums from the end
    std::vector<double> h;
    {
        double s1 = 0, s2 = 0, t1 = 0, t2 = 0, total = 0;
        int quiet = 0;
        for (long k = 0; k < (1L << 22) && quiet < 4096; ++k) {
            const double v = std::fabs(kw_step(p.c, k == 0 ? 1.0 : 0.0, s1, s2, t1, t2));
            h.push_back(v);
            total += v;
            quiet = v < 1e-25 * total ? quiet + 1 : 0;
        }
    }
    double total = 0.0;
    for (double v : h) total += v;
    const double lim = std::ldexp(total, -40);
    double tail = 0.0;
    long W = (long)h.size();
    while (W > 0 && tail + h[W - 1] <= lim) tail += h[--W];
    p.W = (int)W;
    p.K = (int)std::min<long>(LOUD_MAX_K, std::max<long>(1, (4L * W + p.S - 1) / p.S));
    // A: one zero-input step on each unit state; P[0] = A^32, P[k] = P[k-1]^2
    double A[16];
    for (int j = 0; j < 4; ++j) {
        double s[4] = {0, 0, 0, 0};
        s[j] = 1.0;
        (void)kw_step(p.c, 0.0, s[0], s[1], s[2], s[3]);
        for (int i = 0; i < 4; ++i) A[4 * i + j] = s[i];
    }
    std::copy(p.c, p.c + 7, q.c);
    std::copy(A, A + 16, q.P[0]);
    for (int k = 0; k < 5; ++k) mat4_mul(q.P[0], q.P[0], q.P[0]);  // A^(2^5)
    for (int k = 1; k < 8; ++k) mat4_mul(q.P[k - 1], q.P[k - 1], q.P[k]);
    q.S = p.S;
    q.W = p.W;
    q.K = p.K;
}

namespace {
struct LoudEntry {
    LoudnessPlan plan;
    LoudParams params;
};
const LoudEntry* loud_entry(int fs) {
    static std::mutex mu;
    static std::map<int, LoudEntry> cache;
    if (fs < LOUD_MIN_HZ) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(fs);
    if (it == cache.end()) {
        LoudEntry e;
        loudness_design(fs, e.plan, e.params);
        it = cache.emplace(fs, e).first;
    }
    return &it->second;  // (a map's nodes stay where they are)
}
}  // namespace

bool loudness_plan(int fs, LoudnessPlan& out) {
    const LoudEntry* e = loud_entry(fs);
    if (!e) return false;
    out = e->plan;
    return true;
}

void launch_loudness(int fs, const float* audio, long audio_bs, const int* alen, int B, long l_max, double* E, long ldE, double* lufs,
                     int* blocks, int* gated, hipStream_t s) {
    const LoudEntry* e = loud_entry(fs);
    if (!e || B <= 0) return;
    const long item = (long)e->plan.K * e->plan.S;
    const long items = (l_max + item - 1) / item;
    for (int b0 = 0; b0 < B; b0 += 65535) {  // (a grid's y extent)
        const int nb = std::min(B - b0, 65535);
        if (items > 0) LAUNCH_KERNEL(k_loud, dim3((unsigned)items, (unsigned)nb), dim3(256), 0, s, e->params, audio + (long)b0 * audio_bs, audio_bs, alen + b0, E + (long)b0 * ldE, ldE);
    }
    LAUNCH_KERNEL(k_loud_gate, dim3((unsigned)B), dim3(64), 0, s, E, ldE, alen, e->plan.S, lufs, blocks, gated);
}

}  // namespace m355
