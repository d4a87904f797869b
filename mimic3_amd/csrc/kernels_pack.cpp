// kernels_pack.cpp — k_pack: a batch's audio as ONE contiguous stream (mi355vits_run_packed / mi355vits_fetch_packed) in the sample
// encoding the caller ships (mi355vits_set_output_encoding): int16, G.711 mu-law / A-law bytes, or the float samples themselves.
//   * destination-major: a work item is one chunk of 256 x 16 output BYTES; a lane owns the samples of one 16-byte store
//     (8 int16, 16 G.711 codes, 4 floats), whatever the (odd) offsets of the rows inside the stream;
//   * a persistent grid deals the chunks out in consecutive runs, the entry cursor only moves forward, a binary search finds the
//     entry the first chunk starts in;
//   * every byte of [0, capacity) has exactly one writer — no atomics —, and the silences are the code of sample 0 (0 / 0xFF /
//     0xD5 / 0.0f) because this kernel stores them: the workspace is never assumed clean;
//   * loads go through a clamped index and the value is selected afterwards (never masked by a multiply).
// An int16 sample is pcm16_quant's (pcm_quant.h): audio_float_to_int16 and the row's audioop.mul volume, operation for operation
// what k_pcm16 does.  A G.711 sample is that int16 through g711_ulaw / g711_alaw: 5 bytes move per sample where the int16 stream
// moves 6.  The float stream applies neither (as MI355VITS_WANT_FLOAT): bits in, bits out.
#include "kernels.h"
#include "pcm_quant.h"

#include <algorithm>

namespace m355 {

// ---- what differs between the encodings: samples of a lane's 16-byte store, the silence code, one sample's code, the four words
constexpr int pack_lane_samples(int enc) { return 16 / pack_bytes_per_sample(enc); }
constexpr unsigned pack_silence(int enc) { return enc == PACK_ENC_ULAW ? 0xFFu : enc == PACK_ENC_ALAW ? 0xD5u : 0u; }  // g711_*(0); int16 0; the bits of 0.0f

// an entry's scale: NORM (packs with a loudness target only) the table's — 32767 * gain in place of 32767 / max(0.01, peak), for
// F32 the gain itself (one f32 multiply); a float stream without a target has none and reads no peak
template <int ENC, bool NORM>
__device__ __forceinline__ float pack_scale(const int* s_scale, const unsigned* peak_bits, int entry, int row) {
    if constexpr (NORM) return __int_as_float(s_scale[entry]);
    else if constexpr (ENC == PACK_ENC_F32) return 1.0f;
    else return 32767.0f / fmaxf(0.01f, __uint_as_float(peak_bits[row]));
}
template <int ENC, bool NORM> __device__ __forceinline__ unsigned pack_sample(float a, float scale, double volume) {
    if constexpr (ENC == PACK_ENC_F32) {
        return __float_as_uint(NORM ? a * scale : a);
    } else {
        const int q = pcm16_quant(a, scale, volume);
        return ENC == PACK_ENC_S16 ? (unsigned)q : ENC == PACK_ENC_ULAW ? g711_ulaw(q) : g711_alaw(q);
    }
}
__device__ __forceinline__ unsigned pcm16_pair(unsigned lo, unsigned hi) { return (lo & 0xffffu) | (hi << 16); }
__device__ __forceinline__ unsigned pack_quad(unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}
template <int ENC> __device__ __forceinline__ uint4 pack_words(const unsigned (&c)[pack_lane_samples(ENC)]) {
    unsigned w[4];
    MI355_UNROLL
    for (int k = 0; k < 4; ++k) {
        if constexpr (ENC == PACK_ENC_F32) w[k] = c[k];
        else if constexpr (ENC == PACK_ENC_S16) w[k] = pcm16_pair(c[2 * k], c[2 * k + 1]);
        else w[k] = pack_quad(c[4 * k], c[4 * k + 1], c[4 * k + 2], c[4 * k + 3]);
    }
    uint4 st;
    st.x = w[0]; st.y = w[1]; st.z = w[2]; st.w = w[3];
    return st;
}

// TRIM / NORM / CURVE: the table's optional rows (kernels.h: pack_seg_*).  CURVE (behind NORM: a pack whose limiter engaged): an
// entry with a curve offset >= 0 takes sample k's scale from curve[offset + k] (k counted in its ROW, so a trimmed entry reads the
// curve where the untrimmed one does) in place of the entry's one scale; -1: the entry's scale, as without CURVE.
template <int ENC, bool TRIM, bool NORM, bool CURVE>
__device__ __forceinline__ void pack_body(const float* __restrict__ audio, long audio_bs, const unsigned* __restrict__ peak_bits,
                                          const double* __restrict__ volumes, const int* __restrict__ seg, int n,
                                          uint8_t* __restrict__ out, long total, const float* __restrict__ curve) {
    constexpr int S = pack_lane_samples(ENC);       // samples of a lane's 16-byte store
    constexpr int BPS = pack_bytes_per_sample(ENC);
    constexpr long CHUNK = 256L * S;                // output samples per work item
    constexpr unsigned SILENCE = pack_silence(ENC);
    constexpr bool VOL = ENC != PACK_ENC_F32;       // the float stream carries no volume
    const int* s_off = seg + PACK_SEG_OFFSET * n;   // first sample of entry i's audio in the stream, ascending
    const int* s_row = seg + PACK_SEG_ROW * n;      // its batch row
    const int* s_len = seg + PACK_SEG_LENGTH * n;   // its valid samples
    const int* s_skip = seg + PACK_SEG_SKIP * n;    // TRIM only: the row's sample the entry starts at
    const int* s_scale = seg + pack_seg_scale_row(TRIM) * n;  // NORM only: the bits of the entry's f32 scale
    const int* s_curve = seg + pack_seg_curve_row(TRIM) * n;  // CURVE only: the entry's curve offset, or -1
    const long nchunks = (total + CHUNK - 1) / CHUNK;
    // consecutive chunks per workgroup (the first `rem` workgroups take one more): the cursor below then crosses each entry once
    const long per = nchunks / gridDim.x, rem = nchunks % gridDim.x;
    long chunk = blockIdx.x * per + (blockIdx.x < rem ? (long)blockIdx.x : rem);
    const long chunk_end = chunk + per + (blockIdx.x < rem ? 1 : 0);
    if (chunk >= chunk_end) return;
    // the entry the first chunk starts in: the last one whose audio begins at or before the chunk's first sample (-1: the
    // stream's leading silence).  Uniform per workgroup; afterwards the cursor only moves forward.
    int e;
    {
        const long c0 = chunk * CHUNK;
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= c0) lo = mid + 1;
            else hi = mid;
        }
        e = lo - 1;
    }
    for (; chunk < chunk_end; ++chunk) {
        const long c0 = chunk * CHUNK;
        while (e + 1 < n && s_off[e + 1] <= c0) ++e;
        const long s0 = c0 + S * (long)threadIdx.x;
        if (s0 >= total) continue;  // (the last store of the stream may run up to 15 bytes into the buffer's padding)
        int le = e;
        while (le + 1 < n && s_off[le + 1] <= s0) ++le;
        const int lc = le < 0 ? 0 : le;
        const long off = s_off[lc];
        const int row = s_row[lc], len = s_len[lc];
        unsigned c[S];  // the lane's samples as their codes
        if (le >= 0 && s0 + S <= off + len) {
            // the lane's samples all inside one row's audio: 4 S contiguous source bytes, in the widest loads their alignment allows
            const float* src = audio + (long)row * audio_bs + (TRIM ? s_skip[lc] : 0) + (s0 - off);
            const float scale = pack_scale<ENC, NORM>(s_scale, peak_bits, lc, row);
            const double volume = (VOL && volumes) ? volumes[row] : 1.0;
            const float* cv = nullptr;  // CURVE: the scales of the lane's samples
            if constexpr (CURVE) {
                const int co = s_curve[lc];
                if (co >= 0) cv = curve + co + (TRIM ? s_skip[lc] : 0) + (s0 - off);
            }
            float v[S];
            const uintptr_t al = reinterpret_cast<uintptr_t>(src);
            if ((al & 15) == 0) {
                MI355_UNROLL
                for (int k = 0; k < S / 4; ++k) {
                    const float4 a = reinterpret_cast<const float4*>(src)[k];
                    v[4 * k] = a.x; v[4 * k + 1] = a.y; v[4 * k + 2] = a.z; v[4 * k + 3] = a.w;
                }
            } else if ((al & 7) == 0) {
                MI355_UNROLL
                for (int k = 0; k < S / 2; ++k) {
                    const float2 a = reinterpret_cast<const float2*>(src)[k];
                    v[2 * k] = a.x; v[2 * k + 1] = a.y;
                }
            } else {
                MI355_UNROLL
                for (int k = 0; k < S; ++k) v[k] = src[k];
            }
            MI355_UNROLL
            for (int k = 0; k < S; ++k) {
                if constexpr (CURVE) c[k] = pack_sample<ENC, NORM>(v[k], cv ? cv[k] : scale, volume);
                else c[k] = pack_sample<ENC, NORM>(v[k], scale, volume);
            }
        } else {
            // a boundary inside the lane's samples (row end, silence, next row's start, head or tail of the stream): sample by
            // sample with a cursor of its own; loads go through a clamped index, the value is selected afterwards
            int ce = le;
            MI355_UNROLL
            for (int k = 0; k < S; ++k) {
                const long sp = s0 + k;
                while (ce + 1 < n && s_off[ce + 1] <= sp) ++ce;
                const int cc = ce < 0 ? 0 : ce;
                const long o = s_off[cc];
                const int r = s_row[cc];
                const bool valid = ce >= 0 && sp < o + s_len[cc];
                const float a = audio[valid ? (long)r * audio_bs + (TRIM ? s_skip[cc] : 0) + (sp - o) : 0L];
                float scale = pack_scale<ENC, NORM>(s_scale, peak_bits, cc, r);
                if constexpr (CURVE) {
                    const int co = s_curve[cc];
                    const bool curved = valid && co >= 0;
                    const float cs = curve[curved ? (long)co + (TRIM ? s_skip[cc] : 0) + (sp - o) : 0L];
                    scale = curved ? cs : scale;
                }
                const double volume = (VOL && volumes) ? volumes[r] : 1.0;
                c[k] = valid ? pack_sample<ENC, NORM>(a, scale, volume) : SILENCE;
            }
        }
        *reinterpret_cast<uint4*>(out + (size_t)s0 * BPS) = pack_words<ENC>(c);  // 64-bit byte offset: a float stream can pass 4 GB
    }
}

template <int ENC, bool TRIM, bool NORM>
__global__ __launch_bounds__(256) void k_pack(const float* __restrict__ audio, long audio_bs, const unsigned* __restrict__ peak_bits,
                                              const double* __restrict__ volumes, const int* __restrict__ seg, int n,
                                              uint8_t* __restrict__ out, long total) {
    pack_body<ENC, TRIM, NORM, false>(audio, audio_bs, peak_bits, volumes, seg, n, out, total, nullptr);
}
// a pack whose limiter engaged on some entry: k_pack<ENC, TRIM, true> with the table's curve row and the curves
template <int ENC, bool TRIM>
__global__ __launch_bounds__(256) void k_pack_curve(const float* __restrict__ audio, long audio_bs, const unsigned* __restrict__ peak_bits,
                                                    const double* __restrict__ volumes, const int* __restrict__ seg, int n,
                                                    uint8_t* __restrict__ out, long total, const float* __restrict__ curve) {
    pack_body<ENC, TRIM, true, true>(audio, audio_bs, peak_bits, volumes, seg, n, out, total, curve);
}

void launch_pack(int enc, const float* audio, long audio_bs, const unsigned* peak_bits, const double* volumes, const int* seg, int n,
                 uint8_t* out, long total, hipStream_t s, bool trimmed, bool normalised, const float* curve) {
    if (total <= 0 || n <= 0) return;
    if (curve) {
        using CurveKernel = void (*)(const float*, long, const unsigned*, const double*, const int*, int, uint8_t*, long, const float*);
#define PACK_CURVE_FORMS(ENC) {k_pack_curve<ENC, false>, k_pack_curve<ENC, true>}
        static const CurveKernel curve_forms[4][2] = {PACK_CURVE_FORMS(PACK_ENC_S16), PACK_CURVE_FORMS(PACK_ENC_ULAW), PACK_CURVE_FORMS(PACK_ENC_ALAW), PACK_CURVE_FORMS(PACK_ENC_F32)};
#undef PACK_CURVE_FORMS
        const long cchunk = 256L * pack_lane_samples(enc);
        const long cn = (total + cchunk - 1) / cchunk;
        const long cgx = std::min<long>(cn, 8L * current_device_cu_count());
        LAUNCH_KERNEL(curve_forms[enc][trimmed], dim3((unsigned)cgx), dim3(256), 0, s, audio, audio_bs, peak_bits, volumes, seg, n, out, total, curve);
        return;
    }
    using Kernel = void (*)(const float*, long, const unsigned*, const double*, const int*, int, uint8_t*, long);
#define PACK_FORMS(ENC) {{k_pack<ENC, false, false>, k_pack<ENC, false, true>}, {k_pack<ENC, true, false>, k_pack<ENC, true, true>}}
    static const Kernel forms[4][2][2] = {PACK_FORMS(PACK_ENC_S16), PACK_FORMS(PACK_ENC_ULAW), PACK_FORMS(PACK_ENC_ALAW), PACK_FORMS(PACK_ENC_F32)};
#undef PACK_FORMS
    const long chunk = 256L * pack_lane_samples(enc);
    const long nchunks = (total + chunk - 1) / chunk;
    const long gx = std::min<long>(nchunks, 8L * current_device_cu_count());  // 8 workgroups of 4 waves per CU: every SIMD full
    LAUNCH_KERNEL(forms[enc][trimmed][normalised], dim3((unsigned)gx), dim3(256), 0, s, audio, audio_bs, peak_bits, volumes, seg, n, out, total);
}

// ---- k_pack_streams: SEVERAL streams in one block (mi355vits_run_streams / _fetch_streams), each with its own encoding, header, trim
// and scale.  k_pack's structure addressed in BYTES of the block (kernels.h: PACK_ENT_* / PACK_STREAM_*):
//   * a work item is 256 lanes x one 16-byte store at a 16-byte-aligned block offset; every stream's data starts at such an offset, so
//     inside a data region a lane owns whole samples (16 G.711 codes, 8 int16, 4 floats);
//   * the persistent grid, the binary search and the forward-only cursors are k_pack's — one cursor over the entries, one over the
//     streams;
//   * a lane whose 16 bytes lie inside one entry's audio takes the wide-load path of that entry's encoding, a lane wholly inside one
//     stream's silence stores its code, and everything else — an entry end, a silence, the next entry, a pad byte, a gap, a header, the
//     end of the block — walks its 16 byte positions with cursors of its own;
//   * every byte of [0, n_bytes) and of the last store's overrun has exactly one writer; the header bytes are the table's.
// The sample arithmetic is pack_scale / pack_sample / pcm16_quant / g711_* above, chosen per entry at run time.
constexpr int pack_bps_shift(int enc) { return enc == PACK_ENC_S16 ? 1 : enc == PACK_ENC_F32 ? 2 : 0; }  // log2(pack_bytes_per_sample): no 64-bit division
__device__ __forceinline__ float streams_scale(int encw, int scale_bits, const unsigned* peak_bits, int row) {
    if (encw & PACK_ENT_SCALED) return __int_as_float(scale_bits);  // pack_scale<.., true>
    if ((encw & 3) == PACK_ENC_F32) return 1.0f;                     // a float stream without a target reads no peak
    return 32767.0f / fmaxf(0.01f, __uint_as_float(peak_bits[row]));
}
// one sample's code in the low bytes_per_sample bytes
__device__ __forceinline__ unsigned streams_code(int encw, float a, float scale, double volume) {
    switch (encw & 3) {
    case PACK_ENC_S16: return pack_sample<PACK_ENC_S16, false>(a, scale, volume) & 0xffffu;
    case PACK_ENC_ULAW: return pack_sample<PACK_ENC_ULAW, false>(a, scale, volume);
    case PACK_ENC_ALAW: return pack_sample<PACK_ENC_ALAW, false>(a, scale, volume);
    default: return (encw & PACK_ENT_SCALED) ? pack_sample<PACK_ENC_F32, true>(a, scale, volume) : pack_sample<PACK_ENC_F32, false>(a, scale, volume);
    }
}
// a lane's 16 bytes inside one entry's audio: 4 S contiguous source bytes, in the widest loads their alignment allows (as k_pack)
// (CURVE with cv != nullptr: sample k's scale is cv[k] in place of the entry's)
template <int ENC, bool CURVE> __device__ __forceinline__ uint4 streams_lane(const float* src, bool scaled, float scale, double volume, const float* cv) {
    constexpr int S = pack_lane_samples(ENC);
    float v[S];
    const uintptr_t al = reinterpret_cast<uintptr_t>(src);
    if ((al & 15) == 0) {
        MI355_UNROLL
        for (int k = 0; k < S / 4; ++k) {
            const float4 a = reinterpret_cast<const float4*>(src)[k];
            v[4 * k] = a.x; v[4 * k + 1] = a.y; v[4 * k + 2] = a.z; v[4 * k + 3] = a.w;
        }
    } else if ((al & 7) == 0) {
        MI355_UNROLL
        for (int k = 0; k < S / 2; ++k) {
            const float2 a = reinterpret_cast<const float2*>(src)[k];
            v[2 * k] = a.x; v[2 * k + 1] = a.y;
        }
    } else {
        MI355_UNROLL
        for (int k = 0; k < S; ++k) v[k] = src[k];
    }
    unsigned c[S];
    MI355_UNROLL
    for (int k = 0; k < S; ++k) {
        float sk = scale;
        if constexpr (CURVE) sk = cv ? cv[k] : scale;
        c[k] = (ENC == PACK_ENC_F32 && scaled) ? pack_sample<ENC, true>(v[k], sk, volume) : pack_sample<ENC, false>(v[k], sk, volume);
    }
    return pack_words<ENC>(c);
}

// CURVE: the entry table has the PACK_ENT_CURVE row; an entry flagged PACK_ENT_CURVED takes sample k's scale from curve[offset + k]
// (k counted in its row) — a block some of whose entries the limiter engaged on
template <bool CURVE>
__device__ __forceinline__ void streams_body(const float* __restrict__ audio, long audio_bs, const unsigned* __restrict__ peak_bits,
                                             const double* __restrict__ volumes, const int* __restrict__ tab, int n, int ns,
                                             uint8_t* __restrict__ out, long total, const float* __restrict__ curve) {
    constexpr long ITEM = PACK_STREAMS_ITEM_BYTES;
    constexpr int W = PACK_STREAM_WORDS;
    const int* e_off = tab + PACK_ENT_OFFSET * n;   // block byte offset of entry i's first sample, ascending over all streams
    const int* e_row = tab + PACK_ENT_ROW * n;
    const int* e_len = tab + PACK_ENT_LENGTH * n;   // in samples
    const int* e_skip = tab + PACK_ENT_SKIP * n;
    const int* e_enc = tab + PACK_ENT_ENC * n;      // the encoding, + PACK_ENT_SCALED
    const int* e_scale = tab + PACK_ENT_SCALE * n;
    const int* e_curve = tab + PACK_ENT_CURVE * n;  // CURVE only
    const int* st = tab + pack_ent_rows(CURVE) * n;  // [ns][W]: the streams
    const long nitems = (total + ITEM - 1) / ITEM;
    const long per = nitems / gridDim.x, rem = nitems % gridDim.x;
    long item = blockIdx.x * per + (blockIdx.x < rem ? (long)blockIdx.x : rem);
    const long item_end = item + per + (blockIdx.x < rem ? 1 : 0);
    if (item >= item_end) return;
    // the entry and the stream the first work item starts in: the last ones that begin at or before its first byte (-1: none yet).
    // Uniform per workgroup; afterwards both cursors only move forward.
    int e, s;
    {
        const long c0 = item * ITEM;
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (e_off[mid] <= c0) lo = mid + 1;
            else hi = mid;
        }
        e = lo - 1;
        lo = 0, hi = ns;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (st[mid * W + PACK_STREAM_BEGIN] <= c0) lo = mid + 1;
            else hi = mid;
        }
        s = lo - 1;
    }
    for (; item < item_end; ++item) {
        const long c0 = item * ITEM;
        while (e + 1 < n && e_off[e + 1] <= c0) ++e;
        while (s + 1 < ns && st[(s + 1) * W + PACK_STREAM_BEGIN] <= c0) ++s;
        const long p0 = c0 + 16L * threadIdx.x;
        if (p0 >= total) continue;  // (the block's last store may run up to 15 bytes into the buffer's padding)
        int le = e, ls = s;
        while (le + 1 < n && e_off[le + 1] <= p0) ++le;
        while (ls + 1 < ns && st[(ls + 1) * W + PACK_STREAM_BEGIN] <= p0) ++ls;
        const int lc = le < 0 ? 0 : le;
        const long off = e_off[lc];
        const int encw = e_enc[lc], enc = encw & 3;
        const int sh = pack_bps_shift(enc);
        const long aend = off + ((long)e_len[lc] << sh);  // one past the entry's audio
        uint4 w;
        if (le >= 0 && p0 + 16 <= aend) {
            // data regions start 16-byte aligned and samples are aligned inside them: p0 - off is a whole number of samples
            const int row = e_row[lc];
            const float* src = audio + (long)row * audio_bs + e_skip[lc] + ((p0 - off) >> sh);
            const float scale = streams_scale(encw, e_scale[lc], peak_bits, row);
            const double volume = (enc != PACK_ENC_F32 && volumes) ? volumes[row] : 1.0;
            const bool scaled = (encw & PACK_ENT_SCALED) != 0;
            const float* cv = nullptr;
            if constexpr (CURVE) {
                if (encw & PACK_ENT_CURVED) cv = curve + e_curve[lc] + e_skip[lc] + ((p0 - off) >> sh);
            }
            switch (enc) {
            case PACK_ENC_S16: w = streams_lane<PACK_ENC_S16, CURVE>(src, scaled, scale, volume, cv); break;
            case PACK_ENC_ULAW: w = streams_lane<PACK_ENC_ULAW, CURVE>(src, scaled, scale, volume, cv); break;
            case PACK_ENC_ALAW: w = streams_lane<PACK_ENC_ALAW, CURVE>(src, scaled, scale, volume, cv); break;
            default: w = streams_lane<PACK_ENC_F32, CURVE>(src, scaled, scale, volume, cv); break;
            }
        } else {
            const int sc = ls < 0 ? 0 : ls;
            const long d0 = st[sc * W + PACK_STREAM_DATA], d1 = st[sc * W + PACK_STREAM_END];
            const long quiet0 = (le >= 0 && aend > d0) ? aend : d0;                 // behind the entry's audio, inside the stream's data
            const long next = le + 1 < n ? (long)e_off[le + 1] : 0x7fffffffffffL;  // the next entry's audio
            if (ls >= 0 && p0 >= quiet0 && p0 + 16 <= (d1 < next ? d1 : next)) {
                // 16 bytes of one stream's silence: its code in every byte (0 / 0xFF / 0xD5 / the bytes of 0.0f)
                const unsigned q = pack_silence(st[sc * W + PACK_STREAM_ENC]) * 0x01010101u;
                w.x = q; w.y = q; w.z = q; w.w = q;
            } else {
                // a boundary inside the lane's bytes: byte by byte with cursors of its own; loads go through clamped indices, the value
                // is selected afterwards.  A sample's bytes never straddle two lanes, so its code is made at its first byte (and only
                // there) and kept.
                int ce = le, cs = ls;
                unsigned code = 0, ww[4] = {0u, 0u, 0u, 0u};
                MI355_UNROLL
                for (int k = 0; k < 16; ++k) {
                    const long p = p0 + k;
                    while (ce + 1 < n && e_off[ce + 1] <= p) ++ce;
                    while (cs + 1 < ns && st[(cs + 1) * W + PACK_STREAM_BEGIN] <= p) ++cs;
                    const int cc = ce < 0 ? 0 : ce;
                    const int ew = e_enc[cc], bs = pack_bps_shift(ew & 3);
                    const long rel = p - e_off[cc];
                    const bool in_audio = ce >= 0 && rel < ((long)e_len[cc] << bs);
                    const int sub = (int)(rel & ((1 << bs) - 1));  // the byte of its sample
                    const bool first = in_audio && sub == 0;
                    const int r = e_row[cc];
                    const float a = audio[first ? (long)r * audio_bs + e_skip[cc] + (rel >> bs) : 0L];
                    if (first) {  // header, gap, silence and a sample's later bytes pay no sample arithmetic
                        float scale = streams_scale(ew, e_scale[cc], peak_bits, r);
                        if constexpr (CURVE) {
                            if (ew & PACK_ENT_CURVED) scale = curve[(long)e_curve[cc] + e_skip[cc] + (rel >> bs)];
                        }
                        const double volume = ((ew & 3) != PACK_ENC_F32 && volumes) ? volumes[r] : 1.0;
                        code = streams_code(ew, a, scale, volume);
                    }
                    // outside every entry's audio: a header byte, the stream's silence code, or zero (pad byte, gap, in front of stream 0)
                    const int* sr = st + (cs < 0 ? 0 : cs) * W;
                    const long hb = sr[PACK_STREAM_BEGIN], db = sr[PACK_STREAM_DATA], de = sr[PACK_STREAM_END];
                    const int hrel = (cs >= 0 && p < db) ? (int)(p - hb) : 0;
                    const unsigned hbyte = ((unsigned)sr[PACK_STREAM_HEADER + (hrel >> 2)] >> (8 * (hrel & 3))) & 0xffu;
                    const unsigned quiet = cs < 0 ? 0u : p < db ? hbyte : p < de ? pack_silence(sr[PACK_STREAM_ENC]) : 0u;
                    const unsigned byte = in_audio ? (code >> (8 * sub)) & 0xffu : quiet;
                    ww[k >> 2] |= byte << (8 * (k & 3));
                }
                w.x = ww[0]; w.y = ww[1]; w.z = ww[2]; w.w = ww[3];
            }
        }
        *reinterpret_cast<uint4*>(out + p0) = w;
    }
}

__global__ __launch_bounds__(256) void k_pack_streams(const float* __restrict__ audio, long audio_bs, const unsigned* __restrict__ peak_bits,
                                                      const double* __restrict__ volumes, const int* __restrict__ tab, int n, int ns,
                                                      uint8_t* __restrict__ out, long total) {
    streams_body<false>(audio, audio_bs, peak_bits, volumes, tab, n, ns, out, total, nullptr);
}
__global__ __launch_bounds__(256) void k_pack_streams_curve(const float* __restrict__ audio, long audio_bs, const unsigned* __restrict__ peak_bits,
                                                            const double* __restrict__ volumes, const int* __restrict__ tab, int n, int ns,
                                                            uint8_t* __restrict__ out, long total, const float* __restrict__ curve) {
    streams_body<true>(audio, audio_bs, peak_bits, volumes, tab, n, ns, out, total, curve);
}

void launch_pack_streams(const float* audio, long audio_bs, const unsigned* peak_bits, const double* volumes, const int* tab, int n_entries,
                         int n_streams, uint8_t* out, long n_bytes, hipStream_t s, const float* curve) {
    if (n_bytes <= 0 || n_entries <= 0 || n_streams <= 0) return;
    const long nitems = (n_bytes + PACK_STREAMS_ITEM_BYTES - 1) / PACK_STREAMS_ITEM_BYTES;
    const long gx = std::min<long>(nitems, 8L * current_device_cu_count());  // as k_pack: 8 workgroups of 4 waves per CU
    if (curve) {
        LAUNCH_KERNEL(k_pack_streams_curve, dim3((unsigned)gx), dim3(256), 0, s, audio, audio_bs, peak_bits, volumes, tab, n_entries, n_streams, out, n_bytes, curve);
        return;
    }
    LAUNCH_KERNEL(k_pack_streams, dim3((unsigned)gx), dim3(256), 0, s, audio, audio_bs, peak_bits, volumes, tab, n_entries, n_streams, out, n_bytes);
}

// the encoders alone over an array (mi355vits_lab_g711_encode): exhaustive tests on the CPU model and on the device
__global__ __launch_bounds__(256) void k_g711_encode(int law, const int16_t* __restrict__ in, long n, uint8_t* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int q = in[i];
        out[i] = (uint8_t)(law == PACK_ENC_ULAW ? g711_ulaw(q) : g711_alaw(q));
    }
}

void launch_g711_encode(int law, const int16_t* in, long n, uint8_t* out, hipStream_t s) {
    if (n <= 0) return;
    const long gx = std::min<long>((n + 255) / 256, 2048);
    LAUNCH_KERNEL(k_g711_encode, dim3((unsigned)gx), dim3(256), 0, s, law, in, n, out);
}

}  // namespace m355
