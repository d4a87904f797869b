// kernels_pack.cpp — the packed stream in the sample encoding the caller ships (mi355vits_set_output_encoding): G.711 mu-law /
// A-law bytes, or the float samples themselves.  The int16 stream stays k_pcm16_pack's (kernels_conv.cpp); these are its
// encoded forms and keep its structure:
//   * destination-major: a work item is one chunk of 256 x 16 output BYTES; a lane owns the samples of one 16-byte store
//     (16 G.711 codes, 4 floats), whatever the (odd) offsets of the rows inside the stream;
//   * a persistent grid deals the chunks out in consecutive runs, the entry cursor only moves forward, a binary search finds the
//     entry the first chunk starts in;
//   * every byte of [0, capacity) has exactly one writer: the silences are the code of sample 0 (0xFF / 0xD5) or 0.0f because
//     this kernel stores them — the workspace is never assumed clean;
//   * loads go through a clamped index and the value is selected afterwards (never masked by a multiply).
// A G.711 sample is pcm16_quant's int16 — audio_float_to_int16 and the row's audioop.mul volume, operation for operation what
// k_pcm16 / k_pcm16_pack do — through g711_ulaw / g711_alaw (pcm_quant.h): 5 bytes move per sample where the int16 stream moves 6.
// The float stream applies neither (as MI355VITS_WANT_FLOAT): bits in, bits out.
#include "kernels.h"
#include "pcm_quant.h"

#include <algorithm>

namespace m355 {

template <int ENC> __device__ __forceinline__ unsigned pack_code(int q) {
    return ENC == PACK_ENC_ULAW ? g711_ulaw(q) : g711_alaw(q);
}
__device__ __forceinline__ unsigned pack_quad(unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

// NORM (packs with a loudness target only): one more table row behind the others, the entry's f32 scale — 32767 * gain in place of
// 32767 / max(0.01, peak) for the int16-based encodings, the gain itself for F32 (one f32 multiply)
template <int ENC, bool TRIM, bool NORM>
__global__ __launch_bounds__(256) void k_pack_enc(const float* __restrict__ audio, long audio_bs, const unsigned* __restrict__ peak_bits,
                                                  const double* __restrict__ volumes, const int* __restrict__ seg, int n,
                                                  uint8_t* __restrict__ out, long total) {
    constexpr bool F32 = ENC == PACK_ENC_F32;
    constexpr int S = F32 ? 4 : 16;      // samples of a lane's 16-byte store
    constexpr int BPS = F32 ? 4 : 1;     // bytes per sample
    constexpr long CHUNK = 256L * S;     // output samples per work item
    constexpr unsigned SILENCE = ENC == PACK_ENC_ULAW ? 0xFFu : ENC == PACK_ENC_ALAW ? 0xD5u : 0u;  // g711_*(0); the bits of 0.0f
    const int* s_off = seg;          // first sample of entry i's audio in the stream, ascending
    const int* s_row = seg + n;      // its batch row
    const int* s_len = seg + 2 * n;  // its valid samples
    const int* s_skip = seg + 3 * n;  // TRIM only (a [4][n] table): the row's sample the entry starts at
    const int* s_scale = seg + (TRIM ? 4 : 3) * n;  // NORM only: the bits of the entry's f32 scale
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
        unsigned w[4];
        if (le >= 0 && s0 + S <= off + len) {
            // the lane's samples all inside one row's audio: 4 S contiguous source bytes, in the widest loads their alignment allows
            const float* src = audio + (long)row * audio_bs + (TRIM ? s_skip[lc] : 0) + (s0 - off);
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
            if constexpr (F32) {
                MI355_UNROLL
                for (int k = 0; k < 4; ++k) w[k] = __float_as_uint(NORM ? v[k] * __int_as_float(s_scale[lc]) : v[k]);
            } else {
                const float scale = NORM ? __int_as_float(s_scale[lc]) : 32767.0f / fmaxf(0.01f, __uint_as_float(peak_bits[row]));
                const double volume = volumes ? volumes[row] : 1.0;
                MI355_UNROLL
                for (int k = 0; k < 4; ++k)
                    w[k] = pack_quad(pack_code<ENC>(pcm16_quant(v[4 * k], scale, volume)), pack_code<ENC>(pcm16_quant(v[4 * k + 1], scale, volume)),
                                     pack_code<ENC>(pcm16_quant(v[4 * k + 2], scale, volume)), pack_code<ENC>(pcm16_quant(v[4 * k + 3], scale, volume)));
            }
        } else {
            // a boundary inside the lane's samples (row end, silence, next row's start, head or tail of the stream): sample by
            // sample with a cursor of its own; loads go through a clamped index, the value is selected afterwards
            int ce = le;
            unsigned c[S];
            MI355_UNROLL
            for (int k = 0; k < S; ++k) {
                const long sp = s0 + k;
                while (ce + 1 < n && s_off[ce + 1] <= sp) ++ce;
                const int cc = ce < 0 ? 0 : ce;
                const long o = s_off[cc];
                const int r = s_row[cc];
                const bool valid = ce >= 0 && sp < o + s_len[cc];
                const float a = audio[valid ? (long)r * audio_bs + (TRIM ? s_skip[cc] : 0) + (sp - o) : 0L];
                if constexpr (F32) {
                    c[k] = valid ? __float_as_uint(NORM ? a * __int_as_float(s_scale[cc]) : a) : SILENCE;
                } else {
                    const float scale = NORM ? __int_as_float(s_scale[cc]) : 32767.0f / fmaxf(0.01f, __uint_as_float(peak_bits[r]));
                    const double volume = volumes ? volumes[r] : 1.0;
                    c[k] = valid ? pack_code<ENC>(pcm16_quant(a, scale, volume)) : SILENCE;
                }
            }
            MI355_UNROLL
            for (int k = 0; k < 4; ++k) {
                if constexpr (F32) w[k] = c[k];
                else w[k] = pack_quad(c[4 * k], c[4 * k + 1], c[4 * k + 2], c[4 * k + 3]);
            }
        }
        uint4 st;
        st.x = w[0]; st.y = w[1]; st.z = w[2]; st.w = w[3];
        *reinterpret_cast<uint4*>(out + (size_t)s0 * BPS) = st;  // 64-bit byte offset: a float stream can pass 4 GB
    }
}

template <int ENC>
static void launch_pack_enc(const float* audio, long audio_bs, const unsigned* peak_bits, const double* volumes, const int* seg, int n,
                            uint8_t* out, long total, hipStream_t s, bool trimmed, bool normalised) {
    const long chunk = 256L * (ENC == PACK_ENC_F32 ? 4 : 16);
    const long nchunks = (total + chunk - 1) / chunk;
    const long gx = std::min<long>(nchunks, 8L * current_device_cu_count());  // 8 workgroups of 4 waves per CU: every SIMD full
    if (normalised) {
        if (trimmed) {
            LAUNCH_KERNEL((k_pack_enc<ENC, true, true>), dim3((unsigned)gx), dim3(256), 0, s, audio, audio_bs, peak_bits, volumes, seg, n, out, total);
        } else {
            LAUNCH_KERNEL((k_pack_enc<ENC, false, true>), dim3((unsigned)gx), dim3(256), 0, s, audio, audio_bs, peak_bits, volumes, seg, n, out, total);
        }
    } else if (trimmed) {
        LAUNCH_KERNEL((k_pack_enc<ENC, true, false>), dim3((unsigned)gx), dim3(256), 0, s, audio, audio_bs, peak_bits, volumes, seg, n, out, total);
    } else {
        LAUNCH_KERNEL((k_pack_enc<ENC, false, false>), dim3((unsigned)gx), dim3(256), 0, s, audio, audio_bs, peak_bits, volumes, seg, n, out, total);
    }
}

void launch_pack_encoded(int enc, const float* audio, long audio_bs, const unsigned* peak_bits, const double* volumes, const int* seg,
                         int n, uint8_t* out, long total, hipStream_t s, bool trimmed, bool normalised) {
    if (total <= 0 || n <= 0) return;
    switch (enc) {
        case PACK_ENC_ULAW: launch_pack_enc<PACK_ENC_ULAW>(audio, audio_bs, peak_bits, volumes, seg, n, out, total, s, trimmed, normalised); break;
        case PACK_ENC_ALAW: launch_pack_enc<PACK_ENC_ALAW>(audio, audio_bs, peak_bits, volumes, seg, n, out, total, s, trimmed, normalised); break;
        case PACK_ENC_F32: launch_pack_enc<PACK_ENC_F32>(audio, audio_bs, peak_bits, volumes, seg, n, out, total, s, trimmed, normalised); break;
        default: launch_pcm16_pack(audio, audio_bs, peak_bits, volumes, seg, n, reinterpret_cast<int16_t*>(out), total, s, trimmed, normalised);
    }
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
