// kernels_truepeak.cpp — k_true_peak: the 4x oversampled ("true") peak of a run's rows and its per-sample envelope
// (mi355vits_set_loudness_ceiling_mode, mi355vits_fetch_true_peak; the ceiling of the loudness target and what the limiter looks at
// in true-peak mode).  The rule (include/mi355vits.h) is exact: IEEE double, every product and every sum rounded once — this file is
// compiled with -ffp-contract=off and spells the operations out besides — in one fixed order:
//     u[4 t + p] = sum_{i = 0 .. 20, ascending, from 0.0} h[p + 4 i] * (double) x[t + 10 - i]        p = 1, 2, 3; x = 0 outside [0, n)
//     w[t]   = max |u[4 t + 1 .. 4 t + 3]|                     ("v > m" from m = 0.0: a NaN is never taken)
//     e[t]   = max(w[t - 1], |x[t]|, w[t])                     tp = max_t e[t]
//   * h = the 81 taps of scipy.signal.resample_poly(., 4, 1)'s default filter (Kaiser beta 5, half 40), literal doubles below, with
//     three zeros behind them: the rule's 21st product of the phases 1 .. 3 is 0.0 * x — kept, so that a NaN sample spoils exactly
//     the outputs the rule says it spoils.
//   * A work item is (row, tile of 4,096 consecutive samples).  The tile with 11 samples before and 10 behind is staged into LDS
//     with 16-byte loads from the aligned quad at or before its first sample; a quad not wholly inside the row goes sample by
//     sample through a clamped index, and a value takes part by SELECT on 0 <= t < n: no load leaves the row.
//   * Lane l owns the samples l, l + 256, .. of the tile (consecutive lanes read consecutive LDS words: no bank conflict), holds the
//     21 doubles of a sample's window in registers and runs the three phases: 63 products, 63 sums.  w goes to LDS as doubles
//     (consecutive 8-byte words), and after one barrier every lane makes e of its samples from w[t - 1], |x[t]|, w[t].
//   * Measurement form: grid (tiles of the longest row, B); the row maximum is reduced over the workgroup (on the bits of the
//     non-negative doubles: integer order = value order) and goes through ONE integer atomicMax per item on a word k_true_peak_init
//     set on the same stream before.  A maximum does not depend on the order it is taken in: placement cannot change it.
//   * Envelope form: the work items of a list of jobs (the limiter's: the rows over the ceiling); every e[t] has exactly one writer.
#include "kernels.h"

namespace m355 {

#ifdef MI355_EMU
static inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static inline long long __double_as_longlong(double v) {
    long long r;
    __builtin_memcpy(&r, &v, 8);
    return r;
}
static inline double tp_mul(double a, double b) { return a * b; }
static inline double tp_add(double a, double b) { return a + b; }
#else
__device__ __forceinline__ double tp_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double tp_add(double a, double b) { return __dadd_rn(a, b); }
#endif

// h[m], m = 0 .. 83: the 81 taps and the three zeros behind them.  A function with the table inside it: after unrolling every index is
// a constant and the taps are literals of the instruction stream on the device — no table is loaded, nothing is passed.
#ifndef MI355_EMU
__host__ __device__
#endif
constexpr double tp_tap(int m) {
    constexpr double H[TRUE_PEAK_TAPS + 3] = {
        -1.4319646207876959e-18, -0.0011305975791844622, -0.0021031678617178767, -0.0019016679348927714,
        3.7090410940238969e-18, 0.0029265141089618875, 0.0050185309234718227, 0.0042523190668551066,
        -6.9891223043616017e-18, -0.0059320518437837163, -0.0097908339711988927, -0.0080261254612654948,
        1.1214237028997423e-17, 0.010605090076805452, 0.017115155028976113, 0.013753959070631754,
        -1.6183952382363036e-17, -0.017579165251157443, -0.027983277010958114, -0.022219885567699764,
        2.156483064750302e-17, 0.02786691635952088, 0.044051484099836266, 0.034795254750361118,
        -2.692255913458819e-17, -0.043423086442114837, -0.068688534985681365, -0.054425491068782521,
        3.177298294598318e-17, 0.068972338798174965, 0.11058973007292547, 0.089283348532046156,
        -3.5644656557647819e-17, -0.12013435015454692, -0.20188442282305535, -0.17397774297154056,
        3.8143133424221195e-17, 0.29654281960437517, 0.63347608687987345, 0.89963257101020855,
        1.000636565089112, 0.89963257101020855, 0.63347608687987345, 0.29654281960437517,
        3.8143133424221195e-17, -0.17397774297154056, -0.20188442282305535, -0.12013435015454692,
        -3.5644656557647819e-17, 0.089283348532046156, 0.11058973007292547, 0.068972338798174965,
        3.177298294598318e-17, -0.054425491068782521, -0.068688534985681365, -0.043423086442114837,
        -2.692255913458819e-17, 0.034795254750361118, 0.044051484099836266, 0.02786691635952088,
        2.156483064750302e-17, -0.022219885567699764, -0.027983277010958114, -0.017579165251157443,
        -1.6183952382363036e-17, 0.013753959070631754, 0.017115155028976113, 0.010605090076805452,
        1.1214237028997423e-17, -0.0080261254612654948, -0.0097908339711988927, -0.0059320518437837163,
        -6.9891223043616017e-18, 0.0042523190668551066, 0.0050185309234718227, 0.0029265141089618875,
        3.7090410940238969e-18, -0.0019016679348927714, -0.0021031678617178767, -0.0011305975791844622,
        -1.4319646207876959e-18, 0.0, 0.0, 0.0,
    };
    return H[m];
}

const double* true_peak_taps() {
    static const struct Table {
        double h[TRUE_PEAK_TAPS];
        Table() { for (int m = 0; m < TRUE_PEAK_TAPS; ++m) h[m] = tp_tap(m); }
    } t;
    return t.h;
}

constexpr int TP_BEFORE = 11, TP_BEHIND = 10;                       // staged samples around the tile
constexpr int TP_XS = TRUE_PEAK_TILE + TP_BEFORE + TP_BEHIND + 7;   // + the alignment shift (0 .. 3) rounded up to whole quads

__global__ __launch_bounds__(256) void k_true_peak_init(unsigned long long* __restrict__ tp, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) tp[b] = 0ULL;  // the bits of 0.0
}

// One work item: samples [k0, k0 + Te) of the row y[0 .. n).  Returns the lane's maximum of e over its samples (as a double >= 0);
// env != nullptr: e[k0 + o] also goes to env[o].
__device__ __forceinline__ double tp_item(const float* __restrict__ y, int n, long k0, int Te, float* xs, double* wb,
                                          double* __restrict__ env) {
    const int tid = threadIdx.x;
    const int mis = (int)((reinterpret_cast<uintptr_t>(y) >> 2) & 3);
    // ---- stage x of [t0, t0 + N) from the aligned quad at or before t0; 0.0f outside the row
    const long t0 = k0 - TP_BEFORE;
    const int N = Te + TP_BEFORE + TP_BEHIND;
    const int sh = (int)((mis + t0) & 3);
    const long w0 = t0 - sh;
    const int nq = (N + sh + 3) >> 2;
    for (int q = tid; q < nq; q += 256) {
        const long k = w0 + 4L * q;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (k >= 0 && k + 4 <= n) {
            const float4 a = *reinterpret_cast<const float4*>(y + k);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else if (k + 4 > 0 && k < n) {
            MI355_UNROLL
            for (int cc = 0; cc < 4; ++cc) {
                const long kc = k + cc;
                const bool in = kc >= 0 && kc < n;
                const float a = y[in ? kc : 0L];
                v[cc] = in ? a : 0.0f;
            }
        }
        MI355_UNROLL
        for (int cc = 0; cc < 4; ++cc) {
            const int j = 4 * q + cc - sh;
            if (j >= 0 && j < N) xs[j] = v[cc];
        }
    }
    __syncthreads();
    // ---- w of the samples k0 - 1 .. k0 + Te - 1 at wb[0 .. Te]: sample k0 + o reads xs[o + 1 .. o + 21]
    for (int idx = tid; idx <= Te; idx += 256) {
        const int o = idx - 1;
        double m = 0.0;
        if (k0 + o >= 0) {  // (w[-1] lies before the row: nothing of it takes part)
            double xd[21];
            MI355_UNROLL
            for (int i = 0; i < 21; ++i) xd[i] = (double)xs[o + 21 - i];  // x[t + 10 - i]
            MI355_UNROLL
            for (int p = 1; p < 4; ++p) {
                double u = 0.0;
                MI355_UNROLL
                for (int i = 0; i < 21; ++i) u = tp_add(u, tp_mul(tp_tap(p + 4 * i), xd[i]));
                const double v = fabs(u);
                m = v > m ? v : m;  // NaN compares false
            }
        }
        wb[idx] = m;
    }
    __syncthreads();
    // ---- e of the lane's samples
    double lmax = 0.0;
    for (int o = tid; o < Te; o += 256) {
        const double a = fabs((double)xs[o + TP_BEFORE]);
        double e = wb[o];
        e = a > e ? a : e;
        const double w1 = wb[o + 1];
        e = w1 > e ? w1 : e;
        if (env) env[o] = e;
        lmax = e > lmax ? e : lmax;
    }
    return lmax;
}

// measurement: grid (tiles of the longest row, B)
__global__ __launch_bounds__(256) void k_true_peak(const float* __restrict__ audio, long audio_bs, const int* __restrict__ alen,
                                                   unsigned long long* __restrict__ tp) {
    __shared__ float xs[TP_XS];
    __shared__ double wb[TRUE_PEAK_TILE + 1];
    __shared__ unsigned long long sh_max[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int n = alen[b];
    const long k0 = (long)blockIdx.x * TRUE_PEAK_TILE;
    if (k0 >= n) return;  // block-uniform
    const int Te = n - k0 < TRUE_PEAK_TILE ? (int)(n - k0) : TRUE_PEAK_TILE;
    const double lmax = tp_item(audio + (long)b * audio_bs, n, k0, Te, xs, wb, nullptr);
    unsigned long long bits = (unsigned long long)__double_as_longlong(lmax);  // lmax >= 0, never NaN: integer order = value order
    MI355_UNROLL
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(bits, m);
        bits = o > bits ? o : bits;
    }
    if ((tid & 63) == 0) sh_max[tid >> 6] = bits;
    __syncthreads();
    if (tid == 0) {
        MI355_UNROLL
        for (int w = 1; w < 4; ++w) bits = sh_max[w] > bits ? sh_max[w] : bits;
        if (bits > 0ULL) atomicMax(&tp[b], bits);  // (a silent tile leaves the word as k_true_peak_init set it)
    }
}

// envelope: the work items of the jobs (the limiter's table: row, n, off, tile0 — TRUE_PEAK_TILE == LIMIT_TILE)
__global__ __launch_bounds__(256) void k_true_peak_env(const LimitJob* __restrict__ jobs, int n_jobs, const float* __restrict__ audio,
                                                       long audio_bs, double* __restrict__ env) {
    __shared__ float xs[TP_XS];
    __shared__ double wb[TRUE_PEAK_TILE + 1];
    int jl = 0, jh = n_jobs;
    while (jl < jh) {  // the last job whose first item is at or before this one (uniform per workgroup)
        const int mid = (jl + jh) >> 1;
        if (jobs[mid].tile0 <= (int)blockIdx.x) jl = mid + 1;
        else jh = mid;
    }
    const int job = jl - 1;
    const int n = jobs[job].n;
    const long k0 = (long)((int)blockIdx.x - jobs[job].tile0) * TRUE_PEAK_TILE;
    if (k0 >= n) return;  // (block-uniform; the host makes no such item)
    const int Te = n - k0 < TRUE_PEAK_TILE ? (int)(n - k0) : TRUE_PEAK_TILE;
    (void)tp_item(audio + (long)jobs[job].row * audio_bs, n, k0, Te, xs, wb, env + (long)jobs[job].off + k0);
}

void launch_true_peak(const float* audio, long audio_bs, const int* alen, int B, long l_max, double* tp, hipStream_t s) {
    if (B <= 0) return;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(tp);
    LAUNCH_KERNEL(k_true_peak_init, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, w, B);
    const long tiles = (l_max + TRUE_PEAK_TILE - 1) / TRUE_PEAK_TILE;
    if (tiles <= 0) return;
    LAUNCH_KERNEL(k_true_peak, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, s, audio, audio_bs, alen, w);
}

void launch_true_peak_env(const LimitJob* jobs, int n_jobs, long tiles, const float* audio, long audio_bs, double* env, hipStream_t s) {
    if (n_jobs <= 0 || tiles <= 0) return;
    LAUNCH_KERNEL(k_true_peak_env, dim3((unsigned)tiles), dim3(256), 0, s, jobs, n_jobs, audio, audio_bs, env);
}

}  // namespace m355
