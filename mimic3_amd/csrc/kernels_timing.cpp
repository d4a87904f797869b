// kernels_timing.cpp — k_durations_timed: per-phoneme rate, minimum frames and a fitted row length in the run that predicts the
// durations (mi355vits_run_timed).  It takes k_durations' place in such a run: EA^-1 and logw exactly as there, then the rule of
// kernels.h (DurTimedArgs) / include/mi355vits.h:
//   u[t] = fl(w[t] * stretch[t])      f[t](s) = max(c(fl(u[t] * s)), min_frames[t])      F(s) = sum over t < L of f[t](s)
// Every product is ONE f32 multiply rounded to nearest (__fmul_rn: nothing to contract, nothing reassociated), everything else is
// integers: a row's result depends on the row alone — not on the grid, the batch, the CU count or an address.
//   * One 256-lane workgroup (four waves) per row.  u and the row's min_frames are made once and stay in LDS across the whole
//     bisection (rows up to TIMING_LDS_T phonemes: 8 bytes each; a longer row re-reads them from the u array and the upload).
//   * F(s): lane l of the block sums phonemes l, l + 256, .. as int64, then an xor butterfly over the wave and four LDS words.
//     Integer sums: any order gives the same bits.
//   * Positive floats sort like their bit patterns and F never falls as s grows, so the largest s with F(s) <= N is a bisection over
//     the 2^29 patterns of [2^-30, 2^30]: 2 + 29 evaluations of F at the most.
//   * The frames still missing at s* go in index order to the phonemes that step at the next float: an exclusive int64 prefix of
//     their steps.  That prefix and the inclusive scan `cum` are block-parallel: a wave owns a quarter of the row, sums it, and
//     walks it in 64-wide tiles (a shuffle scan per tile, the carry in a register).
//   * No atomics.  Positions at or past the row's length: frames 0, cum flat, u 0 — by select, whatever stretch or min_frames hold.
#include "kernels.h"

namespace m355 {

#ifdef MI355_EMU
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }  // one IEEE multiply (SSE: no wider register)
#endif

namespace {
constexpr unsigned TIMING_S_MIN = 0x30800000u;  // 2^-30
constexpr unsigned TIMING_S_MAX = 0x4e800000u;  // 2^30
constexpr int TIMING_RED_BYTES = 64;            // four int64 wave sums in front of the row's LDS arrays

__device__ __forceinline__ int timed_frames(float u, int mn, float s) {
    const int c = duration_count(__fmul_rn(u, s));
    return c > mn ? c : mn;
}

// the block's sum of one int64 per lane, returned to every lane
__device__ __forceinline__ long long timed_block_sum(long long v, long long* red) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    __syncthreads();  // whoever still reads the last sum is done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// out(t, val(t), val(0) + .. + val(t)) for every t < T; returns the total.  Wave w owns [w * seg, (w + 1) * seg).
template <typename V, typename O> __device__ __forceinline__ long long timed_block_scan(int T, long long* red, V val, O out) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int seg = ((T + 255) / 256) * 64;
    const int t0 = wid * seg, t1 = t0 + seg < T ? t0 + seg : T;
    long long tot = 0;
    for (int t = t0 + lane; t < t1; t += 64) tot += val(t);
    for (int m = 32; m >= 1; m >>= 1) tot += __shfl_xor(tot, m);
    __syncthreads();
    if (lane == 0) red[wid] = tot;
    __syncthreads();
    long long carry = 0;
    for (int w = 0; w < wid; ++w) carry += red[w];
    for (int tb = t0; tb < t1; tb += 64) {
        const int t = tb + lane;
        const long long v = t < t1 ? val(t) : 0;
        long long inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const long long n = __shfl_up(inc, o);
            if (lane >= o) inc += n;
        }
        if (t < t1) out(t, v, carry + inc);
        carry += __shfl(inc, 63);
    }
    return red[0] + red[1] + red[2] + red[3];
}
}  // namespace

__global__ __launch_bounds__(256) void k_durations_timed(DurTimedArgs a, int in_lds) {
    DYN_SMEM(unsigned char, smem);
    long long* red = reinterpret_cast<long long*>(smem);
    float* lu = reinterpret_cast<float*>(smem + TIMING_RED_BYTES);
    int* lm = reinterpret_cast<int*>(lu + a.T);
    const int b = blockIdx.x, T = a.T, tid = threadIdx.x;
    const long row = (long)b * T;
    const int Lr = a.len[b];
    const int L = Lr < 0 ? 0 : (Lr > T ? T : Lr);

    // ---- u (and logw), once
    const float length_scale = a.u_in ? 1.0f : a.scales[(long)b * 3 + 1];
    const float es = expf(-a.ea_logs);
    for (int t = tid; t < T; t += 256) {
        float u;
        if (a.u_in) {
            u = t < L ? a.u_in[row + t] : 0.0f;
        } else {
            const float m = t < L ? 1.0f : 0.0f;
            const float lw = duration_logw(a.z[((long)b * 2 + a.ch) * T + t], a.ea_m, es, m);
            a.logw[row + t] = lw;
            const float w = duration_float(lw, m, length_scale);
            u = t < L ? (a.stretch ? __fmul_rn(w, a.stretch[row + t]) : w) : 0.0f;
        }
        a.u[row + t] = u;
        if (in_lds) {
            lu[t] = u;
            lm[t] = (a.min_frames && t < L) ? a.min_frames[row + t] : 0;
        }
    }
    __syncthreads();
    const float* up = in_lds ? lu : a.u + row;
    const int* mp = in_lds ? lm : (a.min_frames ? a.min_frames + row : nullptr);
    auto frames_at = [&](int t, float s) { return timed_frames(up[t], mp ? mp[t] : 0, s); };
    auto F = [&](unsigned sbits) {
        const float s = __uint_as_float(sbits);
        long long acc = 0;
        for (int t = tid; t < L; t += 256) acc += frames_at(t, s);
        return timed_block_sum(acc, red);
    };

    // ---- s*: every branch below is taken by the whole block (F returns the same sum to every lane)
    const int N = a.target ? a.target[b] : 0;
    unsigned sb = 0x3f800000u;  // 1.0f
    int status = TIMING_OK;
    long long d = 0;
    if (N > 0) {
        unsigned lo = TIMING_S_MIN, hi = TIMING_S_MAX;
        long long Fl = F(lo);
        if (Fl > N) {
            status = TIMING_BELOW_FLOOR;
            sb = lo;
        } else {
            const long long Fh = F(hi);
            if (Fh <= N) {
                sb = hi;
                if (Fh < N) status = TIMING_UNREACHABLE;
            } else {
                while (hi - lo > 1) {
                    const unsigned mid = lo + ((hi - lo) >> 1);
                    const long long Fm = F(mid);
                    if (Fm <= N) { lo = mid; Fl = Fm; } else hi = mid;
                }
                sb = lo;
                d = N - Fl;
            }
        }
    }

    // ---- frames at s*, then the d missing ones in index order among the phonemes that step at the next float
    const float s = __uint_as_float(sb);
    for (int t = tid; t < T; t += 256) a.w_ceil[row + t] = t < L ? frames_at(t, s) : 0;
    __syncthreads();
    if (d > 0) {
        const float s2 = __uint_as_float(sb + 1u);
        timed_block_scan(
            L, red, [&](int t) { return (long long)(frames_at(t, s2) - frames_at(t, s)); },
            [&](int t, long long e, long long incl) {
                const long long left = d - (incl - e);
                const long long extra = left <= 0 ? 0 : (e < left ? e : left);
                if (extra > 0) a.w_ceil[row + t] += (int)extra;
            });
        __syncthreads();
    }
    // ---- cum: the inclusive scan saturated at 2 CAP (the terms are >= 0: the saturated running sum is the clamped prefix)
    const long long sat = 2LL * DURATION_FRAME_CAP;
    const long long total = timed_block_scan(
        T, red, [&](int t) { return (long long)a.w_ceil[row + t]; },
        [&](int t, long long, long long incl) { a.cum[row + t] = (int)(incl > sat ? sat : incl); });
    if (tid == 0) {
        const long long acc = total > sat ? sat : total;
        a.ylen[b] = acc < 1 ? 1 : (int)acc;
        a.factor[b] = s;
        a.status[b] = status;
    }
}

void launch_durations_timed(const DurTimedArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.T <= 0) return;
    const int in_lds = a.T <= TIMING_LDS_T ? 1 : 0;
    const size_t shmem = (size_t)TIMING_RED_BYTES + (in_lds ? (size_t)a.T * 8 : 0);
#ifndef MI355_EMU
    if (shmem > 64 * 1024) set_max_dynamic_lds(reinterpret_cast<const void*>(k_durations_timed), 160 * 1024);
#endif
    LAUNCH_KERNEL(k_durations_timed, dim3(a.B), dim3(256), shmem, s, a, in_lds);
}

}  // namespace m355
