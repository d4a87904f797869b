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

// TRIM / NORM: the table's optional rows (kernels.h: pack_seg_*)
template <int ENC, bool TRIM, bool NORM>
__global__ __launch_bounds__(256) void k_pack(const float* __restrict__ audio, long audio_bs, const unsigned* __restrict__ peak_bits,
                                              const double* __restrict__ volumes, const int* __restrict__ seg, int n,
                                              uint8_t* __restrict__ out, long total) {
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
            for (int k = 0; k < S; ++k) c[k] = pack_sample<ENC, NORM>(v[k], scale, volume);
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
                const float scale = pack_scale<ENC, NORM>(s_scale, peak_bits, cc, r);
                const double volume = (VOL && volumes) ? volumes[r] : 1.0;
                c[k] = valid ? pack_sample<ENC, NORM>(a, scale, volume) : SILENCE;
            }
        }
        *reinterpret_cast<uint4*>(out + (size_t)s0 * BPS) = pack_words<ENC>(c);  // 64-bit byte offset: a float stream can pass 4 GB
    }
}

void launch_pack(int enc, const float* audio, long audio_bs, const unsigned* peak_bits, const double* volumes, const int* seg, int n,
                 uint8_t* out, long total, hipStream_t s, bool trimmed, bool normalised) {
    if (total <= 0 || n <= 0) return;
    using Kernel = void (*)(const float*, long, const unsigned*, const double*, const int*, int, uint8_t*, long);
#define PACK_FORMS(ENC) {{k_pack<ENC, false, false>, k_pack<ENC, false, true>}, {k_pack<ENC, true, false>, k_pack<ENC, true, true>}}
    static const Kernel forms[4][2][2] = {PACK_FORMS(PACK_ENC_S16), PACK_FORMS(PACK_ENC_ULAW), PACK_FORMS(PACK_ENC_ALAW), PACK_FORMS(PACK_ENC_F32)};
#undef PACK_FORMS
    const long chunk = 256L * pack_lane_samples(enc);
    const long nchunks = (total + chunk - 1) / chunk;
    const long gx = std::min<long>(nchunks, 8L * current_device_cu_count());  // 8 workgroups of 4 waves per CU: every SIMD full
    LAUNCH_KERNEL(forms[enc][trimmed][normalised], dim3((unsigned)gx), dim3(256), 0, s, audio, audio_bs, peak_bits, volumes, seg, n, out, total);
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
