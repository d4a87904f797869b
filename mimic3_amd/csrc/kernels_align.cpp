// kernels_align.cpp — where in a run's audio each phoneme sits, and how loud it is there (mi355vits_fetch_alignment).
//   c[t] = frames[0] + .. + frames[t] (k_durations' inclusive scan), c[-1] = 0, hop = samples per latent frame, L / M = the run's
//   reduced rate ratio (1 / 1 native):
//     start[t]   = ceil(hop c[t-1] L / M)                 the first output sample whose time is not before the phoneme's native start
//     samples[t] = ceil(hop c[t] L / M) - start[t]        (k_resample has zero delay: output sample k sits at native time k M / L)
//   in exact 64-bit integers.  ceil(n L / M) is the resampler's length rule, so the spans tile the row: they sum to its length.
//   Positions at or past the row's phoneme count: frames = samples = 0, start = the end of the covered part, levels 0 — selected by
//   t < len[b], so neither frames nor cum is read there, whatever the workspace holds.
//   A pitch run (mi355vits_run_pitch) gives wc, the warped boundaries of k_pitch_plan: wc[t] stands where hop c[t] stood.
// Levels (optional): peak = max |y|, rms = (float) sqrt(sum((double) y y) / samples) over the span of the row's float waveform.
//   * One wave per phoneme.  Lane l takes samples l, l + 64, .. of the span in ascending order: the 64 lanes of a pass load 256
//     consecutive bytes.  Each lane keeps a double sum of squares (every square is exact in double) and a float max.
//   * Then one xor butterfly over the 64 lanes (32, 16, .. 1).  The order of every addition is fixed by the span alone — not by the
//     grid, the batch or the row's place in it: a row of a batch is bitwise the row alone.  max is exact in any order, so the
//     largest peak of a row is bitwise the row peak the waveform's own kernel found.
//   * A sample takes part by SELECT on k < span end (clamped to the row's valid samples, so no load leaves the row): nothing is
//     multiplied by a mask, what lies behind a row in the workspace is never looked at.
//   * No atomics; lane 0 stores the five results with ordinary stores.
// Without levels the timing needs no wave: one thread per (row, phoneme).
#include "kernels.h"

#include <algorithm>

namespace m355 {

struct AlignArgs {
    const int* w_ceil; const int* cum; const int* len; const int* wc; int B, T;
    const float* audio; long audio_bs; const int* alen;
    long long hop, L, M;
    int *frames, *start, *samples;
    float *peak, *rms;
};

__device__ __forceinline__ long long align_ceil_div(long long a, long long m) { return (a + m - 1) / m; }

// frames / start / end of (b, t); every index read is below len[b]
__device__ __forceinline__ void align_span(const AlignArgs& a, int b, int t, int& fr, long long& s0, long long& s1) {
    const int n = a.len[b] < a.T ? a.len[b] : a.T;
    const int* cb = a.cum + (long)b * a.T;
    const bool in = t < n;
    fr = in ? a.w_ceil[(long)b * a.T + t] : 0;
    if (a.wc) {
        const int* wb = a.wc + (long)b * a.T;
        const long long w_end = n > 0 ? wb[n - 1] : 0;
        const long long w0 = in ? (t > 0 ? (long long)wb[t - 1] : 0LL) : w_end;
        const long long w1 = in ? (long long)wb[t] : w_end;
        s0 = align_ceil_div(w0 * a.L, a.M);
        s1 = align_ceil_div(w1 * a.L, a.M);
        return;
    }
    const long long c_end = n > 0 ? cb[n - 1] : 0;
    const long long c0 = in ? (t > 0 ? (long long)cb[t - 1] : 0LL) : c_end;
    const long long c1 = in ? (long long)cb[t] : c_end;
    s0 = align_ceil_div(a.hop * c0 * a.L, a.M);
    s1 = align_ceil_div(a.hop * c1 * a.L, a.M);
}

template <bool LEVELS> __global__ __launch_bounds__(256) void k_align(AlignArgs a) {
    const long total = (long)a.B * a.T;
    if (!LEVELS) {
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i >= total) return;
        int fr;
        long long s0, s1;
        align_span(a, (int)(i / a.T), (int)(i % a.T), fr, s0, s1);
        a.frames[i] = fr;
        a.start[i] = (int)s0;
        a.samples[i] = (int)(s1 - s0);
        return;
    }
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform: the whole wave leaves or stays
    if (i >= total) return;
    const int b = (int)(i / a.T), t = (int)(i % a.T);
    int fr;
    long long s0, s1;
    align_span(a, b, t, fr, s0, s1);
    // no load leaves the row's valid samples (a row of zero frames still has one frame of audio and all-empty spans)
    const long long valid = a.alen[b] > 0 ? a.alen[b] : 0;
    const long long e = s1 < valid ? s1 : valid;
    const float* y = a.audio + (long)b * a.audio_bs;
    double sum = 0.0;
    float pk = 0.0f;
    for (long long k0 = s0; k0 < e; k0 += 256) {  // wave-uniform trip count; four passes' loads in flight, added in ascending order
        float v[4];
        MI355_UNROLL
        for (int j = 0; j < 4; ++j) {
            const long long k = k0 + 64 * j + lane;
            v[j] = y[k < e ? k : s0];  // s0 < e here: a valid sample of this span
        }
        MI355_UNROLL
        for (int j = 0; j < 4; ++j) {
            const bool in = k0 + 64 * j + lane < e;
            const double d = (double)v[j];
            sum += in ? d * d : 0.0;
            pk = in ? fmaxf(pk, fabsf(v[j])) : pk;
        }
    }
    MI355_UNROLL
    for (int m = 32; m >= 1; m >>= 1) {
        sum += __shfl_xor(sum, m);
        pk = fmaxf(pk, __shfl_xor(pk, m));
    }
    if (lane == 0) {
        const long long n = s1 - s0;
        a.frames[i] = fr;
        a.start[i] = (int)s0;
        a.samples[i] = (int)n;
        a.peak[i] = n > 0 ? pk : 0.0f;
        a.rms[i] = n > 0 ? (float)sqrt(sum / (double)n) : 0.0f;
    }
}

void launch_align(const int* w_ceil, const int* cum, const int* len, int B, int T, const float* audio, long audio_bs, const int* alen,
                  int hop, int L, int M, int* frames, int* start, int* samples, float* peak, float* rms, hipStream_t s, const int* wc) {
    if (B <= 0 || T <= 0) return;
    AlignArgs a;
    a.w_ceil = w_ceil; a.cum = cum; a.len = len; a.wc = wc; a.B = B; a.T = T;
    a.audio = audio; a.audio_bs = audio_bs; a.alen = alen;
    a.hop = hop; a.L = L; a.M = M;
    a.frames = frames; a.start = start; a.samples = samples; a.peak = peak; a.rms = rms;
    const long total = (long)B * T;
    if (peak && rms) {
        LAUNCH_KERNEL(k_align<true>, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, a);
    } else {
        LAUNCH_KERNEL(k_align<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    }
}

}  // namespace m355
