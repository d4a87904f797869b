// kernels_resample.cpp — the finished waveform at a requested sample rate (mi355vits_set_output_rate): a polyphase FIR resampler.
//   y[k] = sum_j h[k M - j L + half] x[j],   x = 0 outside [0, n),   n_out = ceil(n L / M),   L / M = out_hz / in_hz reduced,
//   h = L x the Kaiser-windowed sinc (beta 5, cut-off 1 / max(L, M) of Nyquist, 2 half + 1 taps, half = 10 max(L, M), unit DC gain):
// the filter and the edge rule of scipy.signal.resample_poly(x, L, M).  Output k sits on phase p = (k M + half) mod L and reads the
// taps h[p], h[p + L], ... against x[j_hi], x[j_hi - 1], ..., j_hi = (k M + half) div L.
//
// Work item = (row, tile of `tile` consecutive outputs); the grid is persistent and deals the items of all rows out in consecutive
// runs, so a ragged batch costs the sum of its rows' lengths.  A workgroup keeps in LDS
//   * the whole filter, PHASE-MAJOR [L][tp]: the tpp taps of a phase side by side, highest tap index first, so that tap i of the row
//     meets x[j_hi - tpp + 1 + i] and both operands are walked upwards; a lane fetches four taps with one 16-byte read instead of a
//     stride-L gather.  tp = tpp rounded up to a multiple of four with tp / 4 odd (the rest zeros): the lanes of a wave sit on
//     different phases, and with an odd number of 16-byte slots per row consecutive phases start on different slots of the 16
//     that a bank row has — rows of 24 floats (6 slots) would put every eighth phase on the same one;
//   * the tile's input window (16-byte loads where the row allows; samples outside [0, n) are selected to zero while staging, so
//     what lies beside a row in the workspace is never looked at).
// Lane l of a pass takes output k0 + l: neighbouring lanes store neighbouring samples, and read LDS words that are equal
// (upsampling: broadcast) or a few words apart.
// Every output is ONE chain of tp fused multiply-adds in ascending i — whatever the tile, the workgroup, the batch or the row's
// place in it: a row of a batch is bitwise the row alone.  Zero taps add nothing (the window holds finite numbers).
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace m355 {

struct ResampleArgs {
    const float* x; long x_bs; const int* x_len;
    const float* coef; const int* tab; int B; long items;
    float* y; long y_bs; int y_ld; unsigned* peak_bits;
    int L, M, half, tpp, tp, tile, vec;
};

__global__ __launch_bounds__(256) void k_resample(ResampleArgs a) {
    DYN_SMEM(float, smem);
    float* hc = smem;                // [L][tp]
    float* xs = smem + a.L * a.tp;   // the tile's input window
    const int tid = threadIdx.x, lane = tid & 63;
    const int* ylen = a.tab;         // [B] output samples of a row
    const int* first = a.tab + a.B;  // [B + 1] first work item of a row
    // consecutive items per workgroup (the first `rem` take one more): the row cursor below only moves forward
    const long per = a.items / gridDim.x, rem = a.items % gridDim.x;
    long it = blockIdx.x * per + (blockIdx.x < rem ? (long)blockIdx.x : rem);
    const long it_end = it + per + (blockIdx.x < rem ? 1 : 0);
    if (it >= it_end) return;
    for (int q = tid; q < (a.L * a.tp) >> 2; q += 256)
        reinterpret_cast<float4*>(hc)[q] = reinterpret_cast<const float4*>(a.coef)[q];
    int b;
    {
        int lo = 0, hi = a.B;  // the last row whose first item is at or before `it`
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (first[mid] <= it) lo = mid + 1;
            else hi = mid;
        }
        b = lo - 1;
    }
    for (; it < it_end; ++it) {
        while (b + 1 < a.B && first[b + 1] <= it) ++b;
        const int t = (int)(it - first[b]), nt = first[b + 1] - first[b];
        const int n = a.x_len[b] > 0 ? a.x_len[b] : 0, no = ylen[b];
        const float* xrow = a.x + (long)b * a.x_bs;
        float* yrow = a.y + (long)b * a.y_bs;
        const long long k0 = (long long)t * a.tile;
        const long long idx0 = k0 * a.M + a.half;
        const long long jb = idx0 / a.L;
        const int pb = (int)(idx0 - jb * a.L);
        // the window: x[xa ..], xa = the first tap's sample of output k0 rounded down to a multiple of four (it may be negative)
        const long long xa = (jb - a.tpp + 1) & ~3LL;
        const int dmax = (pb + (a.tile - 1) * a.M) / a.L;
        const int nw4 = ((int)(jb + dmax + (a.tp - a.tpp) - xa) + 4) >> 2;
        __syncthreads();  // the previous item's readers are done (first item: nothing yet)
        for (int q = tid; q < nw4; q += 256) {
            const long long g = xa + 4 * q;
            float4 v;
            if (a.vec && g >= 0 && g + 3 < n) {
                v = *reinterpret_cast<const float4*>(xrow + g);
            } else {
                v.x = (g >= 0 && g < n) ? xrow[g] : 0.0f;
                v.y = (g + 1 >= 0 && g + 1 < n) ? xrow[g + 1] : 0.0f;
                v.z = (g + 2 >= 0 && g + 2 < n) ? xrow[g + 2] : 0.0f;
                v.w = (g + 3 >= 0 && g + 3 < n) ? xrow[g + 3] : 0.0f;
            }
            reinterpret_cast<float4*>(xs)[q] = v;
        }
        __syncthreads();
        float pk = 0.0f;
        const int x0 = (int)(jb - a.tpp + 1 - xa);  // window index of output k0's first sample
        for (int d = tid; d < a.tile; d += 256) {
            const long long k = k0 + d;
            if (k >= a.y_ld) break;
            float acc = 0.0f;
            if (k < no) {
                const int u = pb + d * a.M, dj = u / a.L, p = u - dj * a.L;
                const float* hp = hc + p * a.tp;
                const float* xp = xs + x0 + dj;
                for (int c = 0; c < a.tp; c += 4) {
                    const float4 h4 = *reinterpret_cast<const float4*>(hp + c);
                    acc = fmaf(h4.x, xp[c], acc);
                    acc = fmaf(h4.y, xp[c + 1], acc);
                    acc = fmaf(h4.z, xp[c + 2], acc);
                    acc = fmaf(h4.w, xp[c + 3], acc);
                }
                pk = fmaxf(pk, fabsf(acc));
            }
            yrow[k] = acc;  // zero at and past the row's length: the padding of this tile
        }
        // the row's padding behind its last tile, in tile-sized chunks dealt round-robin to the row's items
        for (long long c = (long long)nt + t; c * a.tile < a.y_ld; c += nt)
            for (int d = tid; d < a.tile; d += 256) {
                const long long k = c * a.tile + d;
                if (k < a.y_ld) yrow[k] = 0.0f;
            }
        pk = wave_reduce_max(pk);
        if (lane == 0 && pk > 0.0f) atomicMax(a.peak_bits + b, __float_as_uint(pk));  // non-negative floats order like their bits
    }
}

// ---------------------------------------------------------------- host side: the filter, the per-call table, the launch
namespace {
long double bessel_i0(long double x) {  // sum_k ((x / 2)^k / k!)^2: x <= 5 here, 40 terms are far past the last bit
    const long double q = x * x / 4;
    long double term = 1, sum = 1;
    for (int k = 1; k < 64; ++k) {
        term *= q / ((long double)k * k);
        sum += term;
        if (term < sum * 1e-22L) break;
    }
    return sum;
}
int gcd_int(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}
constexpr size_t RESAMPLE_LDS_LIMIT = 160 * 1024;
// floats of the input window of a tile (k_resample: nw4 * 4 at most)
size_t resample_window(int L, int M, int tp, int tile) { return (((size_t)(L - 1) + (size_t)(tile - 1) * M) / L + tp + 3 + 3 + 4) & ~size_t(3); }
}  // namespace

bool resample_design(int in_hz, int out_hz, ResampleFilter& f) {
    if (in_hz < 1 || out_hz < 1) return false;
    const int g = gcd_int(in_hz, out_hz), L = out_hz / g, M = in_hz / g, mx = L > M ? L : M;
    if (mx > RESAMPLE_MAX_RATIO) return false;
    ResampleFilter r;
    r.in_hz = in_hz; r.out_hz = out_hz; r.L = L; r.M = M;
    r.half = 10 * mx;
    const int nt = 2 * r.half + 1;
    const double fc = 1.0 / mx, beta = 5.0, pi = 3.14159265358979323846;
    const long double i0b = bessel_i0(beta);
    std::vector<double> h(nt);
    long double sum = 0;
    for (int i = 0; i < nt; ++i) {
        const int m = i - r.half;
        const double rr = (double)m / r.half, arg = 1.0 - rr * rr;
        const double w = (double)(bessel_i0(beta * std::sqrt(arg > 0 ? arg : 0.0)) / i0b);
        const double xx = fc * m, sinc = m == 0 ? 1.0 : std::sin(pi * xx) / (pi * xx);
        h[i] = fc * sinc * w;
        sum += h[i];
    }
    for (int i = 0; i < nt; ++i) h[i] = (L * h[i]) / (double)sum;
    r.tpp = (nt + L - 1) / L;
    r.tp = (r.tpp + 3) & ~3;
    if (((r.tp >> 2) & 1) == 0) r.tp += 4;
    r.table.assign((size_t)L * r.tp, 0.0f);
    for (int p = 0; p < L; ++p)
        for (int i = 0; i < r.tpp; ++i) {
            const int t = p + (r.tpp - 1 - i) * L;
            if (t < nt) r.table[(size_t)p * r.tp + i] = (float)h[t];
        }
    r.tile = 1024;
    while (r.tile > 1 && 4 * ((size_t)L * r.tp + resample_window(L, M, r.tp, r.tile)) > RESAMPLE_LDS_LIMIT) r.tile /= 2;
    f = std::move(r);
    return true;
}

long resample_fill_tab(const ResampleFilter& f, const int* n_in, int B, int* tab) {
    long items = 0;
    for (int b = 0; b < B; ++b) {
        const long long no = resample_out_len(n_in[b] > 0 ? n_in[b] : 0, f.L, f.M);
        tab[b] = (int)no;
        tab[B + b] = (int)items;
        const long long nt = (no + f.tile - 1) / f.tile;
        items += nt > 0 ? (long)nt : 1;
    }
    tab[2 * B] = (int)items;
    return items;
}

void launch_resample(const ResampleFilter& f, const float* coef, const float* x, long x_bs, const int* x_len, int B, const int* tab,
                     long items, float* y, long y_bs, int y_ld, unsigned* peak_bits, hipStream_t s) {
    if (B <= 0 || items <= 0) return;
    if (items > 0x7fffffffL) throw std::runtime_error("resample: too many work items");
    ResampleArgs a;
    a.x = x; a.x_bs = x_bs; a.x_len = x_len;
    a.coef = coef; a.tab = tab; a.B = B; a.items = items;
    a.y = y; a.y_bs = y_bs; a.y_ld = y_ld; a.peak_bits = peak_bits;
    a.L = f.L; a.M = f.M; a.half = f.half; a.tpp = f.tpp; a.tp = f.tp; a.tile = f.tile;
    a.vec = (x_bs % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0);
    const size_t shmem = 4 * ((size_t)f.L * f.tp + resample_window(f.L, f.M, f.tp, f.tile));
    if (shmem > RESAMPLE_LDS_LIMIT) throw std::runtime_error("resample: filter does not fit the LDS");
    long per_cu = (long)(RESAMPLE_LDS_LIMIT / shmem);  // workgroups of four waves a compute unit holds
    if (per_cu > 4) per_cu = 4;
    const long gx = std::min<long>(items, per_cu * current_device_cu_count());
#ifndef MI355_EMU
    if (shmem > 64 * 1024) set_max_dynamic_lds(reinterpret_cast<const void*>(k_resample), 160 * 1024);
#endif
    LAUNCH_KERNEL(k_resample, dim3((unsigned)gx), dim3(256), shmem, s, a);
}

}  // namespace m355
