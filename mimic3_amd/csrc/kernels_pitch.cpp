// kernels_pitch.cpp — k_pitch_plan and k_pitch: a pitch ratio per phoneme, duration kept (mi355vits_run_pitch; the rule is in
// include/mi355vits.h and has no tolerance).  The run synthesizes every phoneme p times longer (the stretch of a timed run); these
// kernels play it back p times faster: a band-limited variable-rate warp of the native waveform along the run's own phoneme
// boundaries.  Per row, with c the inclusive scan of the run's frames, n = hop max(1, c[L-1]), ONE = 2^20, P = 128, Z = 12:
//     inv[t] = (int) rintf(2^20 / p[t])                    Tq[t] = sum over u <= t of hop fs[u] inv[u]   (int64)
//     wc[t]  = ceil(Tq[t] / ONE)                           wlen  = wc[L-1]   (hop for a row without frames: one pseudo-phoneme, inv = ONE)
//     output k lies in the smallest t with Tq[t] > k ONE, i.e. with wc[t] > k;  (q, r) = divmod(k ONE - Tq[t-1], inv[t]);
//     i0 = hop c[t-1] + q;  D = max(inv, ONE);  y[k] = x[i0] when inv = ONE and r = 0, else the sum over the source samples j ascending
//     with |N| < Z D, N = (i0 - j) inv + r, of fl(coef x[j]), coef = fl(h[idx] + fl(phi fl(h[idx+1] - h[idx]))),
//     (idx, rem) = divmod(|N| P, D), phi = (float) rem / (float) D; times fl((float) inv 2^-20) when inv < ONE.
//   * k_pitch_plan: one workgroup per row, a chunked int64 scan (256 phonemes a pass, the carry in a register).  Integer sums: any
//     order gives the same bits.  wc and wlen saturate at 2^31 - 1 (the host refuses such a row at the sizing synchronisation).
//   * k_pitch: a work item is (row, tile of 1,024 outputs), 256 lanes, four outputs a lane (tid, tid + 256, ..: consecutive lanes
//     store consecutive samples).  The grid is persistent and deals the items of all rows out in consecutive runs, as k_resample's
//     does (the table of first items rides in the stage table's upload), so a ragged batch costs the sum of its rows' tiles; a row's
//     padding up to the stride is written as zeros by the row's own items.  In LDS: the filter table; the phonemes the tile
//     reaches, one entry each, staged 256 at a time — a reach of more phonemes is WALKED IN CHUNKS, every output computed in the
//     one chunk that holds its phoneme; and the tile's
//     source window, from the first and the last output's position -+ 2 Z samples (the map's slope is at most 2: 2,100 floats),
//     loaded 16 bytes at a time where the ADDRESS allows and the quad lies inside [0, n), else sample by sample with a SELECT to
//     zero outside the row: no load leaves the row.
//   * No 64-bit division per sample: ONE divmod per table entry, for the tile's first output in that phoneme (q0, r0); an output dk
//     further on has (r0 + dk ONE) / inv, which fits 32 bits.  With inv >= ONE, |N| P / inv splits into a whole part per tap and ONE
//     32-bit divmod of r P per output, so phi takes two values (before and behind i0): two float divisions per output.  With
//     inv < ONE, D = 2^20: shifts.
//   * The peak: fmaxf over the lane's valid outputs, wave_reduce_max, the four waves through LDS, ONE integer atomicMax per tile on
//     the bits of the non-negative float (the caller zeroes the words on the same stream before).
// Every output is one chain of singly rounded operations in ascending j, whatever the tile, the grid, the batch or an address: a
// row of a batch is bitwise the row alone.  Compiled with -ffp-contract=off (build.py): the rule rounds every product and sum once.
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <stdexcept>

namespace m355 {

namespace {
struct PitchPlanArgs {
    const int* cum; const int* len; const float* ratio;
    int T, hop;
    long long* tq; int* wc; int* wlen;
};

struct PitchArgs {
    const float* x; long x_bs; const int* x_len;
    const int* cum; const int* len; const float* ratio; const long long* tq; const int* wc;
    const int* items_tab; int B; long items;  // pitch_fill_tab's: [B] wlen, [B + 1] first work item of a row
    const float* tab;
    int T, hop;
    float* y; long y_bs; int y_ld;
    unsigned* peak_bits;
};

// a tile's phoneme: everything an output of it needs, in tile-relative 32-bit numbers
struct alignas(16) PitchEntry {
    int end;   // wc[t] - k0, at most PITCH_TILE: the phoneme owns the outputs kf <= dk < end
    int inv;
    int kf;    // max(wc[t-1], k0) - k0: its first output of this tile
    int src;   // window index of hop c[t-1] + q0
    int r0;    // (q0, r0) = divmod((k0 + kf) ONE - Tq[t-1], inv)
    int pad[3];
};

constexpr int PITCH_ENTRIES = 256;                  // phonemes staged at once (one per lane); more: walked in chunks
constexpr int PITCH_REACH = 2 * PITCH_Z;            // source samples either side of i0 a tap can lie (inv >= ONE / 2)
constexpr int PITCH_WINDOW = 2112;                  // 2 * 1023 + 1 + 2 * PITCH_REACH + 1 + 3 (alignment) = 2099, rounded up
constexpr int PITCH_SAT = 0x7fffffff;

// inv of a ratio; a ratio the host would have refused (it is read below len[b] only, where it was checked) is clamped: the
// division and every index stay defined whatever the array holds
__device__ __forceinline__ int pitch_inv(const float* ratio, long i) {
    if (!ratio) return PITCH_ONE;
    const float p = ratio[i];
    const float pc = p >= 0.5f ? (p <= 2.0f ? p : 2.0f) : 0.5f;  // a NaN: 0.5
    return (int)rintf(1048576.0f / pc);
}

__device__ __forceinline__ int pitch_ceil_sat(long long tq) {
    const long long v = (tq + (PITCH_ONE - 1)) >> 20;
    return v > PITCH_SAT ? PITCH_SAT : (int)v;
}

// first t in [0, L) with wc[t] > k, L when there is none (uniform over the workgroup)
__device__ __forceinline__ int pitch_first_past(const int* __restrict__ wc, int L, int k) {
    int lo = 0, hi = L;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (wc[mid] <= k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ float pitch_coef(const float* h, int idx, float phi) {
    const float h0 = h[idx], h1 = h[idx + 1];
    const float d = h1 - h0;
    const float m = phi * d;
    return h0 + m;
}
}  // namespace

__global__ __launch_bounds__(256) void k_pitch_plan(PitchPlanArgs a) {
    __shared__ long long red[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, b = blockIdx.x;
    const int Lr = a.len[b];
    const int L = Lr < 0 ? 0 : (Lr > a.T ? a.T : Lr);
    const int* cb = a.cum + (long)b * a.T;
    long long carry = 0;
    for (int t0 = 0; t0 < a.T; t0 += 256) {  // block-uniform trip count
        const int t = t0 + tid;
        const bool valid = t < L;
        const int c1 = valid ? cb[t] : 0;
        const int c0 = (valid && t > 0) ? cb[t - 1] : 0;
        const int fs = c1 > c0 ? c1 - c0 : 0;
        const int inv = valid ? pitch_inv(a.ratio, (long)b * a.T + t) : PITCH_ONE;
        long long inc = valid ? (long long)a.hop * fs * inv : 0LL;
        MI355_UNROLL
        for (int o = 1; o < 64; o <<= 1) {
            const long long nv = __shfl_up(inc, (unsigned)o);
            if (lane >= o) inc += nv;
        }
        if (lane == 63) red[wid] = inc;
        __syncthreads();
        long long before = 0, all = 0;
        MI355_UNROLL
        for (int w = 0; w < 4; ++w) {
            if (w < wid) before += red[w];
            all += red[w];
        }
        if (t < a.T) {  // at and past the row's length: the row's end (the valid phonemes of a pass come first)
            const long long v = carry + before + inc;
            a.tq[(long)b * a.T + t] = v;
            a.wc[(long)b * a.T + t] = pitch_ceil_sat(v);
        }
        carry += all;
        __syncthreads();  // red is free for the next pass
    }
    if (tid == 0) {
        const int frames = L > 0 ? cb[L - 1] : 0;
        a.wlen[b] = frames > 0 ? pitch_ceil_sat(carry) : a.hop;  // a row without frames: one pseudo-phoneme of hop samples
    }
}

__global__ __launch_bounds__(256) void k_pitch(PitchArgs a) {
    __shared__ float hs[PITCH_TABLE_FLOATS];
    __shared__ float xs[PITCH_WINDOW];
    __shared__ PitchEntry tab[PITCH_ENTRIES];
    __shared__ float red_max[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int* wlen = a.items_tab;         // [B] warped samples of a row
    const int* first = a.items_tab + a.B;  // [B + 1] first work item of a row
    // consecutive items per workgroup (the first `rem` take one more): the row cursor below only moves forward
    const long per = a.items / gridDim.x, rem = a.items % gridDim.x;
    long it = blockIdx.x * per + (blockIdx.x < rem ? (long)blockIdx.x : rem);
    const long it_end = it + per + (blockIdx.x < rem ? 1 : 0);
    if (it >= it_end) return;
    for (int i = tid; i < PITCH_TABLE_FLOATS; i += 256) hs[i] = a.tab[i];
    int b;
    {
        int lo = 0, hi = a.B;  // the last row whose first item is at or before `it`
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (first[mid] <= it) lo = mid + 1; else hi = mid;
        }
        b = lo - 1;
    }
    for (; it < it_end; ++it) {
        while (b + 1 < a.B && first[b + 1] <= it) ++b;
        const int ti = (int)(it - first[b]), nt = first[b + 1] - first[b];
        const int k0 = ti * PITCH_TILE;
        float* yrow = a.y + (long)b * a.y_bs;
        const int wl = wlen[b];
        __syncthreads();  // the previous item's readers are done (first item: nothing yet)
        const int n = a.x_len[b] > 0 ? a.x_len[b] : 0;
        const float* xrow = a.x + (long)b * a.x_bs;
        const int Lr = a.len[b];
        const int L = Lr < 0 ? 0 : (Lr > a.T ? a.T : Lr);
        const int* cb = a.cum + (long)b * a.T;
        const int* wcb = a.wc + (long)b * a.T;
        const long long* tqb = a.tq + (long)b * a.T;
        const long long hop = a.hop;
        const bool framed = L > 0 && cb[L - 1] > 0;
        const int k_last = (k0 + PITCH_TILE < wl ? k0 + PITCH_TILE : wl) - 1;

        // ---- the phonemes the tile's outputs lie in, [t_lo, t_hi], and the source positions of its first and last output
        int t_lo = 0, t_hi = 0;
        long long i0_first = k0, i0_last = k_last;  // a row without frames: the identity
        if (framed) {
            t_lo = pitch_first_past(wcb, L, k0);
            t_hi = pitch_first_past(wcb, L, k_last);
            if (t_lo > L - 1) t_lo = L - 1;
            if (t_hi > L - 1) t_hi = L - 1;
            const long long tq_lo = t_lo > 0 ? tqb[t_lo - 1] : 0LL, tq_hi = t_hi > 0 ? tqb[t_hi - 1] : 0LL;
            const long long n_lo = (long long)k0 * PITCH_ONE - tq_lo, n_hi = (long long)k_last * PITCH_ONE - tq_hi;
            i0_first = hop * (t_lo > 0 ? cb[t_lo - 1] : 0) + (n_lo > 0 ? n_lo : 0LL) / pitch_inv(a.ratio, (long)b * a.T + t_lo);
            i0_last = hop * (t_hi > 0 ? cb[t_hi - 1] : 0) + (n_hi > 0 ? n_hi : 0LL) / pitch_inv(a.ratio, (long)b * a.T + t_hi);
        }
        // ---- the source window: xs[i] = x[j_base + i], xrow + j_base on a 16-byte line
        const int mis = (int)((reinterpret_cast<uintptr_t>(xrow) >> 2) & 3);
        const long long j_base = ((i0_first - PITCH_REACH + mis) & ~3LL) - mis;
        long long nw = i0_last + PITCH_REACH + 1 - j_base;
        if (nw > PITCH_WINDOW) nw = PITCH_WINDOW;  // (the slope of the map is at most 2: it never is)
        const int nw4 = nw > 0 ? (int)((nw + 3) >> 2) : 0;
        for (int q = tid; q < nw4; q += 256) {
            const long long g = j_base + 4 * q;
            float4 v;
            if (g >= 0 && g + 3 < n) {
                v = *reinterpret_cast<const float4*>(xrow + g);
            } else {
                float w[4];
                MI355_UNROLL
                for (int cc = 0; cc < 4; ++cc) {
                    const long long j = g + cc;
                    const bool in = j >= 0 && j < n;
                    const float s = xrow[in ? j : 0LL];  // (n = 0 cannot be: every row has a frame of audio; the select drops it anyway)
                    w[cc] = in ? s : 0.0f;
                }
                v = make_float4(w[0], w[1], w[2], w[3]);
            }
            reinterpret_cast<float4*>(xs)[q] = v;
        }

        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int lo_rel = 0;  // the outputs below it were computed in an earlier chunk
        int tb = t_lo;
        do {  // block-uniform trip count; one pass in every real voice
            // ---- stage the chunk's entries: one per lane
            int cnt = 1;
            if (!framed) {
                if (tid == 0) {
                    PitchEntry e;
                    e.end = wl - k0 < PITCH_TILE ? wl - k0 : PITCH_TILE;
                    e.inv = PITCH_ONE; e.kf = 0; e.src = (int)(k0 - j_base); e.r0 = 0;
                    e.pad[0] = e.pad[1] = e.pad[2] = 0;
                    tab[0] = e;
                }
            } else {
                cnt = t_hi - tb + 1 < PITCH_ENTRIES ? t_hi - tb + 1 : PITCH_ENTRIES;
                if (tid < cnt) {
                    const int t = tb + tid;
                    const int wce = wcb[t], wcp = t > 0 ? wcb[t - 1] : 0;
                    const long long tqp = t > 0 ? tqb[t - 1] : 0LL;
                    const int inv = pitch_inv(a.ratio, (long)b * a.T + t);
                    const int kf = wcp > k0 ? wcp : k0;
                    PitchEntry e;
                    e.end = wce - k0 < PITCH_TILE ? (wce > k0 ? wce - k0 : 0) : PITCH_TILE;
                    e.inv = inv;
                    e.kf = kf - k0 < PITCH_TILE ? kf - k0 : PITCH_TILE;
                    e.src = 0; e.r0 = 0;
                    e.pad[0] = e.pad[1] = e.pad[2] = 0;
                    if (wce > kf) {  // it owns an output of this tile: the one 64-bit divmod
                        const long long num = (long long)kf * PITCH_ONE - tqp;  // >= 0: kf >= wc[t-1] = ceil(Tq[t-1] / ONE)
                        const long long q0 = num / inv;
                        e.r0 = (int)(num - q0 * inv);
                        e.src = (int)(hop * (t > 0 ? cb[t - 1] : 0) + q0 - j_base);
                    }
                    tab[tid] = e;
                }
            }
            __syncthreads();  // the entries, and on the first pass the window and the filter table
            const int hi_rel = tab[cnt - 1].end;
            MI355_NOUNROLL
            for (int u = 0; u < 4; ++u) {
                const int dk = tid + 256 * u;
                if (dk < lo_rel || dk >= hi_rel) continue;  // another chunk's, or past the row
                int lo = 0, hi = cnt - 1;  // the first entry whose end is past dk
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (tab[mid].end <= dk) lo = mid + 1; else hi = mid;
                }
                const PitchEntry e = tab[lo];
                const unsigned inv = (unsigned)e.inv;
                const unsigned num = (unsigned)e.r0 + ((unsigned)(dk - e.kf) << 20);  // < 2^21 + 2^30
                const unsigned qd = num / inv, r = num - qd * inv;
                int c0 = e.src + (int)qd;  // the window index of i0
                c0 = c0 < PITCH_REACH ? PITCH_REACH : (c0 > PITCH_WINDOW - PITCH_REACH - 1 ? PITCH_WINDOW - PITCH_REACH - 1 : c0);  // (never moves it)
                float y;
                if (inv == (unsigned)PITCH_ONE && r == 0u) {
                    y = xs[c0];
                } else if (inv >= (unsigned)PITCH_ONE) {  // D = inv: |N| P / inv = a whole part per tap and one divmod of r P
                    const unsigned rp = r * (unsigned)PITCH_P;  // < 2^28
                    const unsigned a0 = rp / inv, rem0 = rp - a0 * inv;
                    const unsigned rem1 = rem0 ? inv - rem0 : 0u, up = rem0 ? 1u : 0u;
                    const float finv = (float)inv;
                    const float phi_a = (float)rem0 / finv, phi_b = (float)rem1 / finv;
                    float acc = 0.0f;
                    for (int d = PITCH_Z - 1; d >= 0; --d) {  // j = i0 - d: N = d inv + r
                        const float cf = pitch_coef(hs, d * PITCH_P + (int)a0, phi_a);
                        const float pr = cf * xs[c0 - d];
                        acc = acc + pr;
                    }
                    const int dmax = r ? PITCH_Z : PITCH_Z - 1;
                    for (int d = 1; d <= dmax; ++d) {  // j = i0 + d: |N| = d inv - r
                        const float cf = pitch_coef(hs, d * PITCH_P - (int)a0 - (int)up, phi_b);
                        const float pr = cf * xs[c0 + d];
                        acc = acc + pr;
                    }
                    y = acc;
                } else {  // D = ONE: the prototype stretched by the span's step
                    const int zd = PITCH_Z * PITCH_ONE;
                    const int dlo = (int)(((unsigned)zd - r - 1u) / inv), dhi = (int)(((unsigned)zd + r - 1u) / inv);
                    int N = dlo * (int)inv + (int)r;
                    float acc = 0.0f;
                    for (int d = -dlo; d <= dhi; ++d) {  // j = i0 + d
                        const unsigned an = (unsigned)(N < 0 ? -N : N);
                        const float phi = (float)((an & 8191u) << 7) / 1048576.0f;
                        const float cf = pitch_coef(hs, (int)(an >> 13), phi);
                        const float pr = cf * xs[c0 + d];
                        acc = acc + pr;
                        N -= (int)inv;
                    }
                    const float g = (float)inv * 9.5367431640625e-07f;  // 2^-20
                    y = g * acc;
                }
                o[u] = y;
            }
            lo_rel = hi_rel;
            tb += PITCH_ENTRIES;
            __syncthreads();  // the entries are free for the next chunk
        } while (framed && tb <= t_hi);

        float pk = 0.0f;
        MI355_UNROLL
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + tid + 256 * u;
            const bool in = k < wl;
            pk = in ? fmaxf(pk, fabsf(o[u])) : pk;
            if (k < a.y_ld) yrow[k] = in ? o[u] : 0.0f;  // zeros at and past the row's length: the padding of this tile
        }
        pk = wave_reduce_max(pk);
        if (lane == 0) red_max[wid] = pk;
        __syncthreads();
        if (tid == 0) {
            MI355_UNROLL
            for (int w = 1; w < 4; ++w) pk = fmaxf(pk, red_max[w]);
            if (pk > 0.0f) atomicMax(a.peak_bits + b, __float_as_uint(pk));  // non-negative floats order like their bit patterns
        }
        // the row's padding behind its last tile, in tile-sized chunks dealt round-robin to the row's items
        for (long long c = (long long)nt + ti; c * PITCH_TILE < a.y_ld; c += nt)
            for (int d = tid; d < PITCH_TILE; d += 256) {
                const long long k = c * PITCH_TILE + d;
                if (k < a.y_ld) yrow[k] = 0.0f;
            }
    }  // the items of this workgroup
}

// ---------------------------------------------------------------- host side
namespace {
double pitch_i0(double x) {  // sum_k ((x / 2)^k / k!)^2: x <= 8 here
    const double q = x * x / 4;
    double term = 1, sum = 1;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}
}  // namespace

const std::vector<float>& pitch_table() {
    static std::vector<float> tab;
    static std::once_flag once;
    std::call_once(once, [] {
        const int zp = PITCH_Z * PITCH_P;
        const double pi = 3.14159265358979323846, i0b = pitch_i0(8.0);
        std::vector<float> h(PITCH_TABLE_FLOATS, 0.0f);
        for (int i = 1; i < zp; ++i) {
            if (i % PITCH_P == 0) continue;  // the zeros of the sinc: exactly 0
            const double x = (double)i / PITCH_P, rr = (double)i / zp, arg = 1.0 - rr * rr;
            const double w = pitch_i0(8.0 * std::sqrt(arg > 0 ? arg : 0.0)) / i0b;
            h[i] = (float)(std::sin(pi * x) / (pi * x) * w);
        }
        h[0] = 1.0f;
        tab = std::move(h);
    });
    return tab;
}

void launch_pitch_plan(const int* cum, const int* len, const float* ratio, int B, int T, int hop, long long* tq, int* wc, int* wlen,
                       hipStream_t s) {
    if (B <= 0 || T <= 0) return;
    PitchPlanArgs a;
    a.cum = cum; a.len = len; a.ratio = ratio; a.T = T; a.hop = hop; a.tq = tq; a.wc = wc; a.wlen = wlen;
    LAUNCH_KERNEL(k_pitch_plan, dim3((unsigned)B), dim3(256), 0, s, a);
}

long pitch_fill_tab(const int64_t* wlen, int B, int* tab) {
    long items = 0;
    for (int b = 0; b < B; ++b) {
        const long long w = wlen[b] > 0 ? wlen[b] : 0;
        tab[b] = (int)w;
        tab[B + b] = (int)items;
        const long long nt = (w + PITCH_TILE - 1) / PITCH_TILE;
        items += nt > 0 ? (long)nt : 1;  // (a row always has a frame of audio; an item of its own writes its padding anyway)
    }
    tab[2 * B] = (int)items;
    return items;
}

void launch_pitch(const float* x, long x_bs, const int* x_len, const int* cum, const int* len, const float* ratio, const long long* tq,
                  const int* wc, const int* items_tab, long items, const float* table, int B, int T, int hop, float* y, long y_bs,
                  int y_ld, unsigned* peak_bits, hipStream_t s) {
    if (B <= 0 || T <= 0 || y_ld <= 0 || items <= 0) return;
    if (items > 0x7fffffffL) throw std::runtime_error("pitch: too many work items");
    PitchArgs a;
    a.x = x; a.x_bs = x_bs; a.x_len = x_len; a.cum = cum; a.len = len; a.ratio = ratio; a.tq = tq; a.wc = wc;
    a.items_tab = items_tab; a.B = B; a.items = items;
    a.tab = table; a.T = T; a.hop = hop; a.y = y; a.y_bs = y_bs; a.y_ld = y_ld; a.peak_bits = peak_bits;
    // the workgroups a compute unit holds at once: seven by the kernel's 22.8 KB of LDS (and by its registers)
    const long gx = std::min<long>(items, 7L * current_device_cu_count());
    LAUNCH_KERNEL(k_pitch, dim3((unsigned)gx), dim3(256), 0, s, a);
}

}  // namespace m355
