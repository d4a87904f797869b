// pcm_quant.h — the one float -> int16 sample conversion of the packed streams (k_pack in kernels_pack.cpp), operation for operation
// k_pcm16's, and the G.711 companders that work on its result (k_pack, k_g711_encode).
#pragma once
#include "hipx.h"

#include <cmath>

namespace m355 {

// One valid sample, operation for operation what k_pcm16 does to it (audio_float_to_int16, then audioop.mul):
__device__ __forceinline__ int pcm16_quant(float a, float scale, double volume) {
    float v = a * scale;
    v = fminf(fmaxf(v, -32767.0f), 32767.0f);
    int q = (int)v;
    if (volume != 1.0) {
        double d = (double)q * volume;
        if (d > 32767.0) d = 32767.0;
        else if (d < -32768.0 + 1.0) d = -32768.0;
        q = (int)floor(d);
    }
    return q;
}

// G.711 of an int16 sample q (what pcm16_quant returns): the codes of CPython's audioop.lin2ulaw(x, 2) / lin2alaw(x, 2)
// (Modules/audioop.c, st_14linear2ulaw / st_linear2alaw and their segment tables), for all 65,536 inputs.  Integer arithmetic
// only; the segment search over 0x3F, 0x7F, ... / 0x1F, 0x3F, ... is the position of the magnitude's leading bit (__clz), and
// every choice is a select.
__device__ __forceinline__ unsigned g711_ulaw(int q) {
    const int v = q >> 2;  // 14-bit sample, arithmetic shift
    const unsigned mask = v < 0 ? 0x7Fu : 0xFFu;
    const int a = v < 0 ? -v : v;
    const int m = (a < 8159 ? a : 8159) + 33;  // 33 .. 8192: leading bit 5 .. 13
    const int seg = 26 - __clz(m);             // first of 0x3F, 0x7F, .., 0x1FFF that is >= m; 8 when m == 8192
    const unsigned code = seg >= 8 ? 0x7Fu : (unsigned)((seg << 4) | ((m >> (seg + 1)) & 15));
    return code ^ mask;
}

__device__ __forceinline__ unsigned g711_alaw(int q) {
    const int v = q >> 3;  // 13-bit sample, arithmetic shift
    const unsigned mask = v >= 0 ? 0xD5u : 0x55u;
    const int m = v >= 0 ? v : -v - 1;  // 0 .. 4095
    const int lead = 27 - __clz(m);     // leading bit 5 .. 11 -> 1 .. 7; below 0x20 (m == 0: __clz = 32) -> <= 0
    const int seg = lead > 0 ? lead : 0;  // first of 0x1F, 0x3F, .., 0xFFF that is >= m
    const unsigned code = (unsigned)((seg << 4) | ((m >> (seg < 2 ? 1 : seg)) & 15));
    return code ^ mask;
}

}  // namespace m355
