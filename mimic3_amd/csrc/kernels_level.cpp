// kernels_level.cpp — k_levels: a gain per phoneme with exact ramps, applied to a run's native waveform in place
// (mi355vits_run_levels; the rule is in include/mi355vits.h and has no tolerance).  Per row, in native samples, with c the
// inclusive scan of the run's frames, n = alen[b] = hop max(1, c[L-1]) and R = ramp[b]:
//     q[t]  = (int) rintf(gain[t] * 2^20)                       qs(i) = q of the phoneme sample i lies in (zero-frame phonemes own
//     S[k]  = sum of qs(i) over k - R <= i <= k + R              no sample; 2^20 in a row without frames; edge values repeat)
//     y[k]  = x[k] * (float) ((double) S[k] / (double) ((2 R + 1) 2^20))      peak = max |y[k]| (a NaN is never taken)
//   * S is a difference of two prefix values.  qs is constant over a phoneme's span, so its prefix P(j) = sum of qs(i) over i < j
//     is piecewise linear: with a phoneme's end sample e, its q and P(e), P(j) = P(e) - (e - j) q for every j of its span — and, as
//     edge values repeat, the same line continues P before the first span (j < 0) and behind the last (j > n).
//     S[k] = P(k + R + 1) - P(k - R), in int64: exact, and any common offset of P cancels, so P counts from the first phoneme a
//     tile reaches.
//   * A work item is (row, tile of 4,096 samples), 256 lanes; the tiles are cut where the ADDRESS is a multiple of 16 bytes (tile i
//     of a row whose base is `mis` floats past one holds the samples [4096 i - mis, 4096 (i + 1) - mis)), so a lane's four quads
//     (tid, tid + 256, ..: the 64 lanes of a wave move 1 KiB) are aligned.  The rule is exact, so where the tiles are cut changes
//     no bit.  A quad wholly inside [0, n) moves as 16 bytes, any other sample by sample through a clamped index with a SELECT on
//     0 <= k < n: no load or store leaves the row.
//   * Per tile: two binary searches in c find the phonemes that reach into [k0 - R, k0 + 4096 + R]; 256 of them per pass are
//     looked at (one per lane), the non-empty ones compacted into an LDS table {end, q, P(end)} by a workgroup scan of their count
//     and of q (e - start).  Each lane finds the entry of the two points of a quad by a binary search over the table and steps on
//     from there for the quad's other samples (the points of consecutive samples are consecutive).  (Counting in place of the
//     searches and asking for all samples first, to shorten the chains of dependent loads, was measured and bought nothing: the
//     kernel is bound by its arithmetic)
//   * Dense boundaries: the table holds LEVELS_TABLE entries.  A reach of more phonemes than that is WALKED IN CHUNKS, by the same
//     two functions: per quad the table is filled chunk after chunk, each continuing the prefix, and a point adds its P in the one
//     chunk whose span it lies in.  Every real voice is the one-table case (hop 256: about 50 entries), staged once per tile.
//   * The peak: fmaxf over the lane's valid samples, wave_reduce_max, the four waves through LDS, ONE integer atomicMax per tile on
//     the bits of the non-negative float (the caller zeroes the words on the same stream before).  A maximum does not depend on
//     the order it is taken in.
// Nothing depends on the grid, the CU count, the batch, the row block or an address.  Plain vector stores, no float atomics.  The
// rule has no product followed by a sum: there is nothing to contract.
#include "kernels.h"

namespace m355 {

namespace {
// Positions inside a tile are 32-bit and count from the tile's first sample k0: every point lies in [-R - 3, LEVELS_TILE + R], so
// (end - j) q is ONE 32 x 32 -> 64 bit multiply-add (64-bit positions cost three multiplies and 64-bit compares per point: the
// first version of this kernel spent three times the time of its bytes on them).
struct alignas(16) LevelEntry {
    int end;        // the phoneme's end sample (exclusive) hop * c[t] - k0 — or, past the tile's last point jh and for the row's last
                    // phoneme (whose line goes on behind the row: edge values repeat), jh itself
    int q;
    long long pre;  // P(end), counted from the start of the first phoneme the tile reaches
};

struct LevelsArgs {
    const int* cum; const int* len; const float* gain; const int* ramp;
    int T, hop;
    float* audio; long audio_bs; const int* alen;
    unsigned* peak_bits;
};

// first t in [0, L) with hop * c[t] > x, L when there is none (uniform over the workgroup)
__device__ __forceinline__ int levels_first_past(const int* __restrict__ cb, int L, long long hop, long long x) {
    int lo = 0, hi = L;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (hop * (long long)cb[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the first entry of tab[0 .. cnt) whose end is >= j (cnt >= 1; the last one when there is none)
__device__ __forceinline__ int levels_entry(const LevelEntry* tab, int cnt, int j) {
    int lo = 0, hi = cnt - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].end < j) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// A table-full: the non-empty phonemes among [t0, t_hi], 256 looked at per pass while another pass is sure to fit, compacted into
// tab with P continued from `base`.  Advances t0 and base; returns the entries.  Every lane of the workgroup calls it; ends on a
// barrier, so the table can be read at once.
__device__ __forceinline__ int levels_stage(const int* __restrict__ cb, const float* __restrict__ gb, long long hop, int t_hi, int& t0,
                                            long long& base, long long k0, int jh, int n, LevelEntry* tab, int* red_cnt,
                                            long long* red_sum) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int cnt = 0;
    while (t0 <= t_hi && cnt + 256 <= LEVELS_TABLE) {
        const int t = t0 + tid;
        const bool valid = t <= t_hi;
        const int c1 = valid ? cb[t] : 0;
        const int c0 = (valid && t > 0) ? cb[t - 1] : 0;
        const float g = valid ? gb[t] : 0.0f;  // (asked for with c: one round trip; a gain below len[b] is a checked input)
        const bool ne = valid && c1 > c0;
        const int q = ne ? (int)rintf(g * 1048576.0f) : 0;
        int ic = ne ? 1 : 0;
        long long is = ne ? (long long)q * (hop * (long long)(c1 - c0)) : 0LL;
        MI355_UNROLL
        for (int o = 1; o < 64; o <<= 1) {
            const int nc = __shfl_up(ic, (unsigned)o);
            const long long ns = __shfl_up(is, (unsigned)o);
            if (lane >= o) { ic += nc; is += ns; }
        }
        if (lane == 63) { red_cnt[wid] = ic; red_sum[wid] = is; }
        __syncthreads();
        int c_before = 0, c_all = 0;
        long long s_before = 0, s_all = 0;
        MI355_UNROLL
        for (int w = 0; w < 4; ++w) {
            if (w < wid) { c_before += red_cnt[w]; s_before += red_sum[w]; }
            c_all += red_cnt[w];
            s_all += red_sum[w];
        }
        if (ne) {
            const long long e_abs = hop * c1, e_rel = e_abs - k0;
            LevelEntry e;
            e.end = (e_abs >= n || e_rel > jh) ? jh : (int)e_rel;
            e.q = q;
            e.pre = base + s_before + is - (e_rel - e.end) * q;  // P along the phoneme's line, at the end kept
            tab[cnt + c_before + ic - 1] = e;
        }
        cnt += c_all;
        base += s_all;
        t0 += 256;
        __syncthreads();  // red_* are free for the next pass; the entries are there
    }
    return cnt;
}

// The two points of each sample of the quad at jq (from k0), k - R and k + R + 1: S[cc] += P(k + R + 1) - P(k - R).  ONE: the table
// holds the tile's whole reach.  Else for those of the points that lie in the span this table covers, (cs, ce] (the reach's first
// table: cs below every point — the first phoneme's line goes on before the row).
template <bool ONE>
__device__ __forceinline__ void levels_points(const LevelEntry* tab, int cnt, int cs, int ce, int jq, int R, long long S[4]) {
    MI355_UNROLL
    for (int side = 0; side < 2; ++side) {
        const int j0 = side ? jq + R + 1 : jq - R;  // the quad's first point of this side; the others follow it
        int idx = levels_entry(tab, cnt, ONE ? j0 : (j0 < cs ? cs : (j0 > ce ? ce : j0)));
        MI355_UNROLL
        for (int cc = 0; cc < 4; ++cc) {
            const int j = j0 + cc;
            while (idx < cnt - 1 && tab[idx].end < j) ++idx;
            const LevelEntry e = tab[idx];
            const long long P = e.pre - (long long)(e.end - j) * (long long)e.q;  // 32 x 32 -> 64
            const long long add = (ONE || (j > cs && j <= ce)) ? P : 0LL;
            S[cc] = side ? S[cc] + add : S[cc] - add;
        }
    }
}
}  // namespace

__global__ __launch_bounds__(256) void k_levels(LevelsArgs a) {
    __shared__ LevelEntry tab[LEVELS_TABLE];
    __shared__ int red_cnt[4];
    __shared__ long long red_sum[4];
    __shared__ float red_max[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, b = blockIdx.y;
    const int n = a.alen[b];
    float* y = a.audio + (long)b * a.audio_bs;
    const int mis = (int)((reinterpret_cast<uintptr_t>(y) >> 2) & 3);
    const long long k0 = (long long)blockIdx.x * LEVELS_TILE - mis;  // y + k0 is 16-byte aligned
    if (n <= 0 || k0 >= n) return;  // block-uniform
    const int Lr = a.len[b];
    const int L = Lr < 0 ? 0 : (Lr > a.T ? a.T : Lr);
    const int* cb = a.cum + (long)b * a.T;
    const float* gb = a.gain + (long)b * a.T;
    const long long hop = a.hop;
    const int R = a.ramp ? a.ramp[b] : 0;

    // ---- the phonemes the tile's points reach: [t_lo, t_hi]
    const long long k_first = k0 < 0 ? 0 : k0, k_end = k0 + LEVELS_TILE < n ? k0 + LEVELS_TILE : (long long)n;
    const long long j_lo = k_first - R < 0 ? 0 : k_first - R;  // the points, clamped into [0, n]
    const long long j_hi = k_end + R > n ? (long long)n : k_end + R;
    const long long x_lo = (j_lo > 1 ? j_lo : 1) - 1, x_hi = j_hi - 1;
    const bool framed = L > 0 && cb[L - 1] > 0;  // else: a row without frames, qs = 2^20 throughout
    int t_lo = 0, t_hi = -1;
    if (L > 0) {
        t_lo = levels_first_past(cb, L, hop, x_lo);
        t_hi = levels_first_past(cb, L, hop, x_hi);
    }
    if (framed) {  // t_lo is a non-empty phoneme: hop c[t_lo - 1] <= the bound < hop c[t_lo]
        if (t_lo > L - 1) t_lo = L - 1;
        if (t_hi > L - 1) t_hi = L - 1;
    } else {
        t_lo = 0;
        t_hi = -1;
    }
    const int jh = LEVELS_TILE + R + 1;  // every point of the tile, counted from k0, lies below it
    // one table holds the reach (every pass of 256 phonemes fits): staged once, it serves the lane's four quads
    const bool single = t_hi - t_lo < LEVELS_TABLE;
    int cnt = 0;
    if (!framed) {
        if (tid == 0) {
            tab[0].end = jh;
            tab[0].q = LEVELS_ONE;
            tab[0].pre = (long long)jh * LEVELS_ONE;
        }
        __syncthreads();
        cnt = 1;
    } else if (single) {
        int t0 = t_lo;
        long long base = 0;
        cnt = levels_stage(cb, gb, hop, t_hi, t0, base, k0, jh, n, tab, red_cnt, red_sum);
    }

    const double den = (double)((2LL * R + 1) * (long long)LEVELS_ONE);
    float pk = 0.0f;
    MI355_NOUNROLL
    for (int u = 0; u < 4; ++u) {  // rolled: one copy of the code, few registers
        const long long kq = k0 + 4LL * (tid + 256 * u);
        const bool whole = kq >= 0 && kq + 4 <= n;
        float x[4];
        if (whole) {
            const float4 v = *reinterpret_cast<const float4*>(y + kq);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
            MI355_UNROLL
            for (int cc = 0; cc < 4; ++cc) {
                const long long k = kq + cc;
                const bool in = k >= 0 && k < n;
                const float v = y[in ? k : 0LL];
                x[cc] = in ? v : 0.0f;
            }
        }
        long long S[4] = {0, 0, 0, 0};
        const int jq = 4 * (tid + 256 * u);
        if (single) {
            levels_points<true>(tab, cnt, 0, 0, jq, R, S);
        } else {
            int t0 = t_lo, cs = -(1 << 30);
            long long base = 0;
            do {  // block-uniform trip count
                cnt = levels_stage(cb, gb, hop, t_hi, t0, base, k0, jh, n, tab, red_cnt, red_sum);
                const int ce = tab[cnt > 0 ? cnt - 1 : 0].end;
                levels_points<false>(tab, cnt, cs, ce, jq, R, S);
                cs = ce;
                __syncthreads();  // the table is free for the next chunk
            } while (t0 <= t_hi);
        }
        float o[4];
        MI355_UNROLL
        for (int cc = 0; cc < 4; ++cc) {
            const long long k = kq + cc;
            const bool in = k >= 0 && k < n;
            // 0 <= S < 2^45: the two halves convert exactly and add up exactly — (double) S without the signed 64-bit conversion
            const double Sd = (double)(unsigned)((unsigned long long)S[cc] >> 32) * 4294967296.0 + (double)(unsigned)S[cc];
            const float scale = (float)(Sd / den);
            o[cc] = x[cc] * scale;
            pk = in ? fmaxf(pk, fabsf(o[cc])) : pk;
        }
        if (whole) {
            *reinterpret_cast<float4*>(y + kq) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            MI355_UNROLL
            for (int cc = 0; cc < 4; ++cc) {
                const long long k = kq + cc;
                if (k >= 0 && k < n) y[k] = o[cc];
            }
        }
    }
    pk = wave_reduce_max(pk);
    if (lane == 0) red_max[wid] = pk;
    __syncthreads();
    if (tid == 0) {
        MI355_UNROLL
        for (int w = 1; w < 4; ++w) pk = fmaxf(pk, red_max[w]);
        if (pk > 0.0f) atomicMax(a.peak_bits + b, __float_as_uint(pk));  // non-negative floats order like their bit patterns
    }
}

void launch_levels(const int* cum, const int* len, const float* gain, const int* ramp, int B, int T, int hop, float* audio,
                   long audio_bs, const int* alen, long l_max, unsigned* peak_bits, hipStream_t s) {
    if (B <= 0 || T <= 0 || l_max <= 0) return;
    LevelsArgs a;
    a.cum = cum; a.len = len; a.gain = gain; a.ramp = ramp; a.T = T; a.hop = hop;
    a.audio = audio; a.audio_bs = audio_bs; a.alen = alen; a.peak_bits = peak_bits;
    const long tiles = (l_max + 3 + LEVELS_TILE - 1) / LEVELS_TILE;  // a row's base may sit up to three floats past a 16-byte line
    LAUNCH_KERNEL(k_levels, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, s, a);
}

}  // namespace m355
