// kernels_flac.cpp — the S16LE packed stream as FLAC frames (mi355vits_set_output_compression; RFC 9639, the subset DESIGN.md §4.15
// writes out): mono, 16 bit, fixed block size 4096, one subframe per frame — constant, fixed predictor of order 0 .. 4 with
// partitioned Rice residuals (partition order 4 for a full block, 0 for the short last one), or verbatim.
//   k_flac_frames   one 256-lane workgroup per frame, persistent over a job table of (source, samples, first frame number); lane l
//                   owns samples 16 l .. 16 l + 15, a partition of a full block is 16 lanes.  Exact bit counts choose the Rice
//                   parameters, the order and the verbatim fallback; the codes are ORed into a zeroed LDS bit buffer (a code is
//                   its stop bit and remainder: the unary run is the zeros already there); CRC-8 / CRC-16 close the frame, which
//                   goes to its slot of FLAC_SLOT_BYTES with its size in the size table.
//   k_flac_scan     one workgroup: the exclusive scan of the sizes and their total.
//   k_flac_gather   the frames back to back in the output, one writer per byte.
//   k_flac_place / k_flac_gather_streams   several files in one block (the streams calls): the places of every
//                   frame and file and the 42 header bytes made on the device, then one 16-byte store per lane.
// Integer arithmetic only; the only atomics are LDS ORs and k_flac_place's integer maxima.  The bytes are a function of (samples, rate, first frame number) alone.
#include "kernels.h"

#include <algorithm>

namespace m355 {

namespace {
constexpr int FLAC_MAX_ORDER = 4;
constexpr int FLAC_RICE_PARAMS = 15;  // k = 0 .. 14: the escape code 1111 is never used
constexpr int FLAC_LS_LD = 257;       // lane sums [k][lane], padded: the group sums read 16 consecutive lanes per thread

struct FlacLds {
    unsigned bits[FLAC_SLOT_BYTES / 4 + 4];  // the frame, MSB first: bit b is bit 31 - (b & 31) of word b >> 5
    int16_t x[FLAC_BLOCK];
    unsigned ls[FLAC_RICE_PARAMS][FLAC_LS_LD];               // one order's sum(u >> k) per lane
    unsigned gs[FLAC_MAX_ORDER + 1][16][FLAC_RICE_PARAMS];   // ... per group of 16 lanes (a partition of a full block)
    unsigned best_bits[FLAC_MAX_ORDER + 1][16];              // the partition's minimum of sum(u >> k) + count (1 + k)
    int best_k[FLAC_MAX_ORDER + 1][16];
    unsigned cnt[256];   // per lane: bits (then the prefix), later CRC parts
    unsigned gt[16];     // per group of 16 lanes
    unsigned crc_tab[256];
    int varied;          // some sample differs from the first
};

// the 4-bit sample-rate code of a frame header, and the field behind the frame number it may ask for
__host__ __device__ inline void flac_rate_code(int rate, int* code, int* field_bits, unsigned* field) {
    *field_bits = 0;
    *field = 0;
    switch (rate) {
    case 88200: *code = 1; return;
    case 176400: *code = 2; return;
    case 192000: *code = 3; return;
    case 8000: *code = 4; return;
    case 16000: *code = 5; return;
    case 22050: *code = 6; return;
    case 24000: *code = 7; return;
    case 32000: *code = 8; return;
    case 44100: *code = 9; return;
    case 48000: *code = 10; return;
    case 96000: *code = 11; return;
    default: break;
    }
    if (rate <= 65535) {
        *code = 13; *field_bits = 16; *field = (unsigned)rate;
    } else if (rate % 10 == 0 && rate / 10 <= 65535) {
        *code = 14; *field_bits = 16; *field = (unsigned)(rate / 10);
    } else {
        *code = 0;  // "as STREAMINFO says"
    }
}

__device__ __forceinline__ void put_bits(unsigned* bits, int pos, int nb, unsigned v) {  // 1 <= nb <= 32, v < 2^nb
    const int w = pos >> 5, sh = pos & 31, room = 32 - sh;
    if (nb <= room) {
        atomicOr(&bits[w], v << (room - nb));
    } else {
        const int r = nb - room;  // 1 .. 31
        atomicOr(&bits[w], v >> r);
        atomicOr(&bits[w + 1], v << (32 - r));
    }
}
__device__ __forceinline__ unsigned frame_byte(const unsigned* bits, int i) { return (bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu; }
__device__ __forceinline__ unsigned fold(int r) { return r >= 0 ? 2u * (unsigned)r : 2u * (unsigned)(-r) - 1u; }
__device__ __forceinline__ unsigned crc8_step(unsigned crc, unsigned byte) {  // polynomial 0x07, MSB first
    crc ^= byte;
    for (int i = 0; i < 8; ++i) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xffu : (crc << 1) & 0xffu;
    return crc;
}
// GF(2)[x] mod x^16 + x^15 + x^2 + 1: the product of two residues, and x^e
__device__ __forceinline__ unsigned crc16_mul(unsigned a, unsigned b) {
    unsigned r = 0;
    for (int i = 15; i >= 0; --i) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x18005u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
__device__ __forceinline__ unsigned crc16_xpow(unsigned e) {
    unsigned r = 1, base = 2;
    while (e) {
        if (e & 1u) r = crc16_mul(r, base);
        base = crc16_mul(base, base);
        e >>= 1;
    }
    return r;
}

// the lane's window of the frame as differences of order `o`: d[4 + k] = r_o[i0 + k] wherever i0 + k >= o (d[0 .. 3] start as the
// four samples in front of the lane's, zero in front of the frame)
__device__ __forceinline__ void difference(int (&d)[20]) {
    MI355_UNROLL
    for (int j = 19; j >= 1; --j) d[j] -= d[j - 1];
}
}  // namespace

__global__ __launch_bounds__(256) void k_flac_frames(const FlacJob* __restrict__ jobs, int n_jobs, long n_frames, int rate,
                                                     uint8_t* __restrict__ slots, int* __restrict__ sizes) {
    DYN_SMEM(FlacLds, L);
    const int t = threadIdx.x;
    {
        unsigned c = (unsigned)t << 8;  // CRC-16, polynomial 0x8005, MSB first: the table of one byte
        for (int i = 0; i < 8; ++i) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xffffu : (c << 1) & 0xffffu;
        L->crc_tab[t] = c;
    }
    int rate_code, rate_bits;
    unsigned rate_field;
    flac_rate_code(rate, &rate_code, &rate_bits, &rate_field);
    for (long w = blockIdx.x; w < n_frames; w += gridDim.x) {
        __syncthreads();  // the frame before is out of the LDS
        int j = 0;
        while (j + 1 < n_jobs && jobs[j + 1].slot0 <= w) ++j;
        const FlacJob job = jobs[j];
        const long fl = w - job.slot0;                 // the frame inside its job
        const long start = fl * FLAC_BLOCK;
        const int bs = (int)(job.n - start < FLAC_BLOCK ? job.n - start : FLAC_BLOCK);
        const unsigned fno = (unsigned)(job.first_frame + fl);
        const int16_t* __restrict__ src = job.src + start;
        for (int i = t; i < FLAC_SLOT_BYTES / 4 + 4; i += 256) L->bits[i] = 0u;
        if (t == 0) L->varied = 0;
        // ---- stage: the lane's 16 samples (two 16-byte loads where the source allows), the whole frame in the LDS
        const int i0 = 16 * t;
        int own[16];
        if (i0 + 16 <= bs && (reinterpret_cast<uintptr_t>(src + i0) & 15) == 0) {
            const uint4 a = reinterpret_cast<const uint4*>(src + i0)[0], b = reinterpret_cast<const uint4*>(src + i0)[1];
            const unsigned wd[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            MI355_UNROLL
            for (int k = 0; k < 8; ++k) {
                own[2 * k] = (int)(int16_t)(wd[k] & 0xffffu);
                own[2 * k + 1] = (int)(int16_t)(wd[k] >> 16);
            }
        } else {
            MI355_UNROLL
            for (int k = 0; k < 16; ++k) own[k] = src[i0 + k < bs ? i0 + k : 0];  // clamped; selected below
        }
        MI355_UNROLL
        for (int k = 0; k < 16; ++k) {
            if (i0 + k >= bs) own[k] = 0;
            L->x[i0 + k] = (int16_t)own[k];
        }
        __syncthreads();
        const int first = L->x[0];
        int pre[4];
        MI355_UNROLL
        for (int k = 0; k < 4; ++k) pre[k] = i0 - 4 + k >= 0 ? (int)L->x[i0 - 4 + k < 0 ? 0 : i0 - 4 + k] : 0;
        {
            bool differs = false;
            MI355_UNROLL
            for (int k = 0; k < 16; ++k) differs = differs || (i0 + k < bs && own[k] != first);
            if (differs) L->varied = 1;
        }
        __syncthreads();
        const bool constant = L->varied == 0;
        const int p = bs == FLAC_BLOCK ? 4 : 0, parts = 1 << p;
        const int omax = bs - 1 < FLAC_MAX_ORDER ? bs - 1 : FLAC_MAX_ORDER;
        int order = 0;
        bool verbatim = false;
        if (!constant) {
            // ---- per order: the fifteen sums of every group of 16 lanes
            int d[20];
            MI355_UNROLL
            for (int k = 0; k < 4; ++k) d[k] = pre[k];
            MI355_UNROLL
            for (int k = 0; k < 16; ++k) d[4 + k] = own[k];
            for (int o = 0; o <= omax; ++o) {
                if (o > 0) difference(d);
                unsigned s[FLAC_RICE_PARAMS];
                MI355_UNROLL
                for (int k = 0; k < FLAC_RICE_PARAMS; ++k) s[k] = 0u;
                MI355_UNROLL
                for (int i = 0; i < 16; ++i) {
                    const bool in = i0 + i >= o && i0 + i < bs;
                    const unsigned u = in ? fold(d[4 + i]) : 0u;
                    MI355_UNROLL
                    for (int k = 0; k < FLAC_RICE_PARAMS; ++k) s[k] += u >> k;
                }
                MI355_UNROLL
                for (int k = 0; k < FLAC_RICE_PARAMS; ++k) L->ls[k][t] = s[k];
                __syncthreads();
                if (t < 16 * FLAC_RICE_PARAMS) {
                    const int g = t / FLAC_RICE_PARAMS, k = t - g * FLAC_RICE_PARAMS;
                    unsigned a = 0u;
                    for (int l = 0; l < 16; ++l) a += L->ls[k][16 * g + l];
                    L->gs[o][g][k] = a;
                }
                __syncthreads();
            }
            // ---- the Rice parameter of every (order, partition): the exact minimum, the smallest k on a tie
            if (t < 16 * (FLAC_MAX_ORDER + 1)) {
                const int o = t >> 4, part = t & 15;
                if (o <= omax && part < parts) {
                    const unsigned count = (unsigned)((bs >> p) - (part == 0 ? o : 0));
                    unsigned best = 0xffffffffu;
                    int bk = 0;
                    for (int k = 0; k < FLAC_RICE_PARAMS; ++k) {
                        unsigned sum;
                        if (p == 4) {
                            sum = L->gs[o][part][k];
                        } else {
                            sum = 0u;
                            for (int g = 0; g < 16; ++g) sum += L->gs[o][g][k];
                        }
                        const unsigned cost = sum + count * (unsigned)(1 + k);  // < 2^32: u < 2^20, count < 2^12 (4096 only with p = 4)
                        if (cost < best) {
                            best = cost;
                            bk = k;
                        }
                    }
                    L->best_bits[o][part] = best;
                    L->best_k[o][part] = bk;
                }
            }
            __syncthreads();
            // ---- the order: the smallest bits(o), the lowest on a tie; verbatim when that saves nothing (every lane the same sum)
            unsigned best = 0xffffffffu;
            for (int o = 0; o <= omax; ++o) {
                unsigned b = 16u * (unsigned)o + 6u;
                for (int part = 0; part < parts; ++part) b += 4u + L->best_bits[o][part];
                if (b < best) {
                    best = b;
                    order = o;
                }
            }
            verbatim = best >= 16u * (unsigned)bs;
        }
        // ---- the frame header (lane 0); its length is every lane's to know
        const int fno_bytes = fno < 0x80u ? 1 : fno < 0x800u ? 2 : fno < 0x10000u ? 3 : 4;
        const int bs_bits = bs == FLAC_BLOCK ? 0 : bs <= 256 ? 8 : 16;
        const int hdr = 4 + fno_bytes + (bs_bits >> 3) + (rate_bits >> 3) + 1;  // with its CRC-8
        if (t == 0) {
            unsigned crc = 0;
            int pos = 0;
            auto put = [&](unsigned byte) MI355_INLINE_LAMBDA {
                crc = crc8_step(crc, byte);
                put_bits(L->bits, pos, 8, byte);
                pos += 8;
            };
            put(0xffu);
            put(0xf8u);
            put((unsigned)((bs == FLAC_BLOCK ? 12 : bs <= 256 ? 6 : 7) << 4) | (unsigned)rate_code);
            put(0x08u);
            if (fno_bytes == 1) {
                put(fno);
            } else {
                put((fno_bytes == 2 ? 0xc0u : fno_bytes == 3 ? 0xe0u : 0xf0u) | (fno >> (6 * (fno_bytes - 1))));
                for (int k = fno_bytes - 2; k >= 0; --k) put(0x80u | ((fno >> (6 * k)) & 0x3fu));
            }
            if (bs_bits == 16) put((unsigned)(bs - 1) >> 8);
            if (bs_bits) put((unsigned)(bs - 1) & 0xffu);
            if (rate_bits) {
                put(rate_field >> 8);
                put(rate_field & 0xffu);
            }
            put_bits(L->bits, pos, 8, crc);
            pos += 8;
            // the subframe header; constant: its value; fixed: the warm-up samples, the coding method and the partition order
            put_bits(L->bits, pos, 8, constant ? 0x00u : verbatim ? 0x02u : (unsigned)(0x10 + 2 * order));
            pos += 8;
            if (constant) {
                put_bits(L->bits, pos, 16, (unsigned)first & 0xffffu);
            } else if (!verbatim) {
                for (int k = 0; k < order; ++k) {
                    put_bits(L->bits, pos, 16, (unsigned)(int)L->x[k] & 0xffffu);
                    pos += 16;
                }
                put_bits(L->bits, pos, 6, (unsigned)p);
            }
        }
        const int body = 8 * (hdr + 1);  // the first bit behind the subframe header
        int end_bits;
        if (constant) {
            end_bits = body + 16;
        } else if (verbatim) {
            MI355_UNROLL
            for (int k = 0; k < 16; ++k)
                if (i0 + k < bs) put_bits(L->bits, body + 16 * (i0 + k), 16, (unsigned)own[k] & 0xffffu);
            end_bits = body + 16 * bs;
        } else {
            // ---- the residual: every lane's bit count, the block-wide exclusive prefix, then the codes
            int d[20];
            MI355_UNROLL
            for (int k = 0; k < 4; ++k) d[k] = pre[k];
            MI355_UNROLL
            for (int k = 0; k < 16; ++k) d[4 + k] = own[k];
            for (int o = 0; o < order; ++o) difference(d);
            const int part = p == 4 ? t >> 4 : 0;
            const int rk = L->best_k[order][part];
            const bool opens = p == 4 ? (t & 15) == 0 : t == 0;  // the partition's first lane writes its parameter
            unsigned nbits = opens ? 4u : 0u;
            MI355_UNROLL
            for (int i = 0; i < 16; ++i)
                if (i0 + i >= order && i0 + i < bs) nbits += (fold(d[4 + i]) >> rk) + 1u + (unsigned)rk;
            L->cnt[t] = nbits;
            __syncthreads();
            if (t < 16) {
                unsigned a = 0u;
                for (int l = 0; l < 16; ++l) a += L->cnt[16 * t + l];
                L->gt[t] = a;
            }
            __syncthreads();
            unsigned before = 0u, all = 0u;
            for (int g = 0; g < 16; ++g) {
                const unsigned v = L->gt[g];
                before += g < (t >> 4) ? v : 0u;
                all += v;
            }
            for (int l = 0; l < (t & 15); ++l) before += L->cnt[(t & ~15) + l];
            int pos = body + 16 * order + 6 + (int)before;
            if (opens) {
                put_bits(L->bits, pos, 4, (unsigned)rk);
                pos += 4;
            }
            MI355_UNROLL
            for (int i = 0; i < 16; ++i) {
                if (i0 + i >= order && i0 + i < bs) {
                    const unsigned u = fold(d[4 + i]);
                    pos += (int)(u >> rk);  // the unary run: zeros already there
                    put_bits(L->bits, pos, rk + 1, (1u << rk) | (u & ((1u << rk) - 1u)));
                    pos += rk + 1;
                }
            }
            end_bits = body + 16 * order + 6 + (int)all;
        }
        // ---- zero bits to the byte boundary, then CRC-16 of everything so far: a chunk per lane, each part shifted by what follows it
        const int nb = (end_bits + 7) >> 3;
        __syncthreads();
        {
            const int chunk = (nb + 255) >> 8;
            const int b0 = t * chunk < nb ? t * chunk : nb, b1 = b0 + chunk < nb ? b0 + chunk : nb;
            unsigned c = 0u;
            for (int i = b0; i < b1; ++i) c = ((c << 8) ^ L->crc_tab[((c >> 8) ^ frame_byte(L->bits, i)) & 0xffu]) & 0xffffu;
            if (c) c = crc16_mul(c, crc16_xpow(8u * (unsigned)(nb - b1)));
            L->cnt[t] = c;
        }
        __syncthreads();
        if (t < 16) {
            unsigned a = 0u;
            for (int l = 0; l < 16; ++l) a ^= L->cnt[16 * t + l];
            L->gt[t] = a;
        }
        __syncthreads();
        if (t == 0) {
            unsigned c = 0u;
            for (int g = 0; g < 16; ++g) c ^= L->gt[g];
            put_bits(L->bits, 8 * nb, 16, c);
            sizes[w] = nb + 2;
        }
        __syncthreads();
        // ---- the frame to its slot, as whole words (the slot is 16-byte aligned; behind the frame's last byte the word holds zeros)
        unsigned* __restrict__ dst = reinterpret_cast<unsigned*>(slots + (size_t)w * FLAC_SLOT_BYTES);
        for (int i = t; i < (nb + 2 + 3) >> 2; i += 256) dst[i] = __builtin_bswap32(L->bits[i]);
    }
}

// offsets[f] = the bytes of the frames in front of frame f; sizes[n_frames] = the low 32 bits of the total.  One workgroup.
__global__ __launch_bounds__(256) void k_flac_scan(int* __restrict__ sizes, long n_frames, long long* __restrict__ offsets) {
    __shared__ unsigned long long part[256];
    const int t = threadIdx.x;
    const long per = (n_frames + 255) / 256;
    const long f0 = t * per < n_frames ? t * per : n_frames, f1 = f0 + per < n_frames ? f0 + per : n_frames;
    unsigned long long a = 0;
    for (long f = f0; f < f1; ++f) a += (unsigned long long)sizes[f];
    part[t] = a;
    __syncthreads();
    unsigned long long before = 0;
    for (int l = 0; l < t; ++l) before += part[l];
    for (long f = f0; f < f1; ++f) {
        offsets[f] = (long long)before;
        before += (unsigned long long)sizes[f];
    }
    if (t == 255) sizes[n_frames] = (int)(unsigned)before;
}

__global__ __launch_bounds__(256) void k_flac_gather(const uint8_t* __restrict__ slots, const int* __restrict__ sizes,
                                                     const long long* __restrict__ offsets, long n_frames, uint8_t* __restrict__ out) {
    for (long w = blockIdx.x; w < n_frames; w += gridDim.x) {
        const uint8_t* __restrict__ src = slots + (size_t)w * FLAC_SLOT_BYTES;
        uint8_t* __restrict__ dst = out + offsets[w];
        const int n = sizes[w];
        for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
    }
}

void launch_flac_frames(const FlacJob* jobs, int n_jobs, long n_frames, int rate, uint8_t* slots, int* sizes, hipStream_t s) {
    if (n_frames <= 0 || n_jobs <= 0) return;
    // 147 VGPRs: three waves per SIMD, so three 4-wave workgroups are resident per CU (the 39 KB of LDS would allow four)
    const long gx = std::min<long>(n_frames, 3L * current_device_cu_count());
    LAUNCH_KERNEL(k_flac_frames, dim3((unsigned)gx), dim3(256), sizeof(FlacLds), s, jobs, n_jobs, n_frames, rate, slots, sizes);
}

void launch_flac_gather(const uint8_t* slots, int* sizes, long long* offsets, long n_frames, uint8_t* out, hipStream_t s) {
    if (n_frames <= 0) return;
    LAUNCH_KERNEL(k_flac_scan, dim3(1), dim3(256), 0, s, sizes, n_frames, offsets);
    const long gx = std::min<long>(n_frames, 8L * current_device_cu_count());
    LAUNCH_KERNEL(k_flac_gather, dim3((unsigned)gx), dim3(256), 0, s, slots, (const int*)sizes, (const long long*)offsets, n_frames, out);
}

// ---- several files in one block (kernels.h: launch_flac_place / launch_flac_gather_streams)
namespace {
constexpr int PLACE_THREADS = 1024;   // 16 waves: a trip takes 4,096 frames, four per lane in 16-byte loads
constexpr int PLACE_LDS_JOBS = 1024;  // up to this many jobs the job table lives in the LDS (20 KB), beyond it in global memory
enum { JT_SLOT0 = 0, JT_BASE = 1, JT_PRE0 = 2, JT_NEGMIN = 3, JT_MAX = 4, JT_ROWS = 5 };  // the job table's rows, [row][job]

// the workgroup's exclusive prefix of v (and the sum over all lanes): a shuffle scan per wave, the waves' sums through the LDS.
// Unsigned adds: exact in any order.  ws holds PLACE_THREADS / 64 words; two barriers, the second frees ws for the next call.
__device__ __forceinline__ unsigned place_scan(unsigned v, unsigned* ws, unsigned* all) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned inc = v;
    MI355_UNROLL
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, (unsigned)d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    unsigned before = 0u, sum = 0u;
    MI355_UNROLL
    for (int w = 0; w < PLACE_THREADS / 64; ++w) {
        const unsigned x = ws[w];
        before += w < wave ? x : 0u;
        sum += x;
    }
    __syncthreads();
    *all = sum;
    return before + inc - v;
}
}  // namespace

// One workgroup, four phases behind the scan, each a pass of coalesced accesses with the per-job values in the LDS:
//   scan    pre[f] = the bytes of the frames in front of frame f over all jobs (16-byte loads and stores, a shuffle scan);
//   jobs    per job its bytes (two reads of pre) and its place (a second scan, over the places rounded up to 16);
//   frames  per frame its block offset and its job (ftab), its size into the job's smallest / largest — integer maxima in the LDS,
//           one per run of frames a lane holds of one job: the same in any order;
//   finish  per job FLAC_INFO_* and the 42 header bytes; per work item of the gather the last frame at or before its first byte.
__global__ __launch_bounds__(1024) void k_flac_place(const FlacJob* __restrict__ jobs, int n_jobs, long n_frames, int rate, long base0,
                                                     int* __restrict__ sizes, unsigned* __restrict__ pre, int2* __restrict__ ftab,
                                                     unsigned* __restrict__ hdr, int* __restrict__ item_first, int* __restrict__ jtab) {
    __shared__ unsigned ws[PLACE_THREADS / 64];
    __shared__ int ls[JT_ROWS * PLACE_LDS_JOBS];
    const int t = threadIdx.x;
    int* __restrict__ info = sizes + n_frames;
    const bool staged = n_jobs <= PLACE_LDS_JOBS;
    int* const tab = staged ? ls : jtab;
    const int ld = staged ? PLACE_LDS_JOBS : n_jobs;
    // ---- scan: four sizes per lane and trip
    unsigned carry = 0u;
    for (long f0 = 0; f0 < n_frames; f0 += 4L * PLACE_THREADS) {
        const long f = f0 + 4L * t;
        unsigned v[4] = {0u, 0u, 0u, 0u};
        if (f + 4 <= n_frames) {
            const uint4 a = *reinterpret_cast<const uint4*>(sizes + f);  // (sizes is 16-byte aligned, f a multiple of 4)
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else {
            MI355_UNROLL
            for (int k = 0; k < 4; ++k) v[k] = f + k < n_frames ? (unsigned)sizes[f + k] : 0u;
        }
        unsigned all;
        const unsigned b0 = carry + place_scan(v[0] + v[1] + v[2] + v[3], ws, &all);
        uint4 o;
        o.x = b0; o.y = b0 + v[0]; o.z = o.y + v[1]; o.w = o.z + v[2];
        if (f + 4 <= n_frames) {
            *reinterpret_cast<uint4*>(pre + f) = o;
        } else {
            if (f < n_frames) pre[f] = o.x;
            if (f + 1 < n_frames) pre[f + 1] = o.y;
            if (f + 2 < n_frames) pre[f + 2] = o.z;
        }
        carry += all;
    }
    if (t == 0) pre[n_frames] = carry;
    __syncthreads();
    // ---- jobs: bytes, and place = base0 + the places (rounded up to 16) of the jobs in front
    unsigned at = (unsigned)base0;
    for (int j0 = 0; j0 < n_jobs; j0 += PLACE_THREADS) {
        const int j = j0 + t;
        unsigned bytes = 0u, room = 0u, p0 = 0u;
        int s0 = 0;
        if (j < n_jobs) {
            s0 = jobs[j].slot0;
            const long s1 = j + 1 < n_jobs ? (long)jobs[j + 1].slot0 : n_frames;
            p0 = pre[s0];
            bytes = (unsigned)FLAC_HEADER_BYTES + (pre[s1] - p0);
            room = (bytes + 15u) & ~15u;
        }
        unsigned all;
        const unsigned base = at + place_scan(room, ws, &all);
        if (j < n_jobs) {
            tab[JT_SLOT0 * ld + j] = s0;
            tab[JT_BASE * ld + j] = (int)base;
            tab[JT_PRE0 * ld + j] = (int)p0;
            tab[JT_NEGMIN * ld + j] = -0x7fffffff;  // minus the smallest frame, under the integer maximum below
            tab[JT_MAX * ld + j] = 0;
            info[FLAC_INFO_WORDS * j + FLAC_INFO_BASE] = (int)base;
            info[FLAC_INFO_WORDS * j + FLAC_INFO_BYTES] = (int)bytes;
            if (j == n_jobs - 1) info[FLAC_INFO_WORDS * n_jobs] = (int)(base + bytes);  // the block's end
        }
        at += all;
    }
    __syncthreads();
    // ---- frames: four per lane and trip
    for (long f0 = 0; f0 < n_frames; f0 += 4L * PLACE_THREADS) {
        const long f = f0 + 4L * t;
        if (f >= n_frames) continue;
        unsigned pv[4] = {0u, 0u, 0u, 0u}, sv[4] = {0u, 0u, 0u, 0u};
        if (f + 4 <= n_frames) {
            const uint4 a = *reinterpret_cast<const uint4*>(pre + f), b = *reinterpret_cast<const uint4*>(sizes + f);
            pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
            sv[0] = b.x; sv[1] = b.y; sv[2] = b.z; sv[3] = b.w;
        } else {
            MI355_UNROLL
            for (int k = 0; k < 4; ++k) {
                pv[k] = f + k < n_frames ? pre[f + k] : 0u;
                sv[k] = f + k < n_frames ? (unsigned)sizes[f + k] : 0u;
            }
        }
        int j;
        {
            int lo = 0, hi = n_jobs;  // the last job whose first slot is at or before f: the jobs without a frame in front of it are passed
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((long)tab[JT_SLOT0 * ld + mid] <= f) lo = mid + 1;
                else hi = mid;
            }
            j = lo - 1;
        }
        int run = j, neg = -0x7fffffff, mx = 0;
        MI355_UNROLL
        for (int k = 0; k < 4; ++k) {
            if (f + k < n_frames) {
                while (j + 1 < n_jobs && (long)tab[JT_SLOT0 * ld + j + 1] <= f + k) ++j;
                if (j != run) {
                    atomicMax(&tab[JT_NEGMIN * ld + run], neg);
                    atomicMax(&tab[JT_MAX * ld + run], mx);
                    run = j; neg = -0x7fffffff; mx = 0;
                }
                const int sz = (int)sv[k];
                neg = -sz > neg ? -sz : neg;
                mx = sz > mx ? sz : mx;
                int2 e;
                e.x = tab[JT_BASE * ld + j] + FLAC_HEADER_BYTES + (int)(pv[k] - (unsigned)tab[JT_PRE0 * ld + j]);
                e.y = j;
                ftab[f + k] = e;
            }
        }
        atomicMax(&tab[JT_NEGMIN * ld + run], neg);
        atomicMax(&tab[JT_MAX * ld + run], mx);
    }
    __syncthreads();
    // ---- finish, per job: FLAC_INFO_MIN / _MAX and the 42 bytes of flac_stream_header as little-endian words
    for (int j = t; j < n_jobs; j += PLACE_THREADS) {
        const long s0 = tab[JT_SLOT0 * ld + j], s1 = j + 1 < n_jobs ? (long)tab[JT_SLOT0 * ld + j + 1] : n_frames;
        const unsigned fmin = s1 > s0 ? (unsigned)(-tab[JT_NEGMIN * ld + j]) : 0u;
        const unsigned fmax = (unsigned)tab[JT_MAX * ld + j];
        info[FLAC_INFO_WORDS * j + FLAC_INFO_MIN] = (int)fmin;
        info[FLAC_INFO_WORDS * j + FLAC_INFO_MAX] = (int)fmax;
        const unsigned long long v = ((unsigned long long)(unsigned)rate << 44) | (15ULL << 36) | ((unsigned long long)jobs[j].n & 0xfffffffffULL);
        auto byte = [&](int sh) { return (unsigned)(v >> sh) & 0xffu; };
        unsigned* __restrict__ h = hdr + (size_t)FLAC_HDR_WORDS * j;
        h[0] = 0x43614c66u;  // "fLaC"
        h[1] = 0x80u | (34u << 24);
        h[2] = (unsigned)(FLAC_BLOCK >> 8) | ((unsigned)(FLAC_BLOCK & 0xff) << 8) | ((unsigned)(FLAC_BLOCK >> 8) << 16) | ((unsigned)(FLAC_BLOCK & 0xff) << 24);
        h[3] = ((fmin >> 16) & 0xffu) | (((fmin >> 8) & 0xffu) << 8) | ((fmin & 0xffu) << 16) | (((fmax >> 16) & 0xffu) << 24);
        h[4] = ((fmax >> 8) & 0xffu) | ((fmax & 0xffu) << 8) | (byte(56) << 16) | (byte(48) << 24);
        h[5] = byte(40) | (byte(32) << 8) | (byte(24) << 16) | (byte(16) << 24);
        h[6] = byte(8) | (byte(0) << 8);
        MI355_UNROLL
        for (int k = 7; k < FLAC_HDR_WORDS; ++k) h[k] = 0u;
    }
    // ---- finish, per work item of the gather: item_first[i] = the last frame that starts at or before byte base0 + i ITEM (-1: none),
    // for i = 0 .. the items of the block inclusive.  Frame f owns the item starts in [its offset, the next frame's offset): one writer each.
    const long end = (long)tab[JT_BASE * ld + n_jobs - 1] + (long)(unsigned)info[FLAC_INFO_WORDS * (n_jobs - 1) + FLAC_INFO_BYTES];
    const long last_item = (end - base0 + FLAC_GATHER_ITEM_BYTES - 1) / FLAC_GATHER_ITEM_BYTES;
    const long first_off = n_frames > 0 ? (long)ftab[0].x : 0x7fffffffffffL;
    for (long i = t; i <= last_item && base0 + i * FLAC_GATHER_ITEM_BYTES < first_off; i += PLACE_THREADS) item_first[i] = -1;
    for (long f = t; f < n_frames; f += PLACE_THREADS) {
        const long o = ftab[f].x, lim = f + 1 < n_frames ? (long)ftab[f + 1].x : 0x7fffffffffffL;
        for (long i = (o - base0 + FLAC_GATHER_ITEM_BYTES - 1) / FLAC_GATHER_ITEM_BYTES; i <= last_item && base0 + i * FLAC_GATHER_ITEM_BYTES < lim; ++i)
            item_first[i] = (int)f;
    }
}

// Destination-major: a work item is 256 lanes x one 16-byte store.  item_first bounds the lane's search for its frame to the frames
// that start inside the item; a lane whose 16 bytes lie in one frame shifts them out of the aligned words that hold them; a lane on a
// boundary — a frame's end, up to two frame starts, one file start, a header, a gap, the block's end — loads what can cover its
// bytes at once and picks byte by byte.
__global__ __launch_bounds__(256) void k_flac_gather_streams(int n_jobs, long n_frames, const uint8_t* __restrict__ slots,
                                                             const int* __restrict__ sizes, const int2* __restrict__ ftab,
                                                             const unsigned* __restrict__ hdr, const int* __restrict__ item_first,
                                                             long base0, long bound_bytes, uint8_t* __restrict__ out) {
    const int* __restrict__ info = sizes + n_frames;
    const long dev_end = info[FLAC_INFO_WORDS * n_jobs];
    const long end = dev_end < base0 + bound_bytes ? dev_end : base0 + bound_bytes;  // (never past what out holds, whatever the sizes say)
    const long nitems = (end - base0 + FLAC_GATHER_ITEM_BYTES - 1) / FLAC_GATHER_ITEM_BYTES;
    for (long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const long p0 = base0 + item * FLAC_GATHER_ITEM_BYTES + 16L * threadIdx.x;
        const int flo = item_first[item], fhi = item_first[item + 1];  // uniform
        if (p0 >= end) continue;  // (the block's last store may run up to 15 bytes into the buffer's padding)
        // the last frame that starts at or before the lane's first byte (-1: none)
        long f;
        {
            long lo = flo < 0 ? 0 : flo, hi = (long)fhi + 1;
            while (lo < hi) {
                const long mid = (lo + hi) >> 1;
                if ((long)ftab[mid].x <= p0) lo = mid + 1;
                else hi = mid;
            }
            f = lo - 1;
        }
        const long fc = f < 0 ? 0 : f;
        int2 fe;
        fe.x = 0; fe.y = 0;
        int fsz = 0;
        if (n_frames > 0) {
            fe = ftab[fc];
            fsz = sizes[fc];
        }
        const long q = p0 - (long)fe.x;
        uint4 w;
        if (f >= 0 && q + 16 <= fsz) {
            // 16 bytes of one frame, from any byte of its 16-byte-aligned slot: the aligned words that hold them, shifted.  The fifth
            // word starts inside the frame, so it lies in the slot (whose last word k_flac_frames wrote whole).
            const unsigned* __restrict__ sw = reinterpret_cast<const unsigned*>(slots + (size_t)f * FLAC_SLOT_BYTES) + (q >> 2);
            const int sh = 8 * (int)(q & 3);
            const unsigned a0 = sw[0], a1 = sw[1], a2 = sw[2], a3 = sw[3], a4 = sh ? sw[4] : 0u;
            auto join = [&](unsigned l, unsigned h) { return (unsigned)((((unsigned long long)h << 32) | l) >> sh); };
            w.x = join(a0, a1); w.y = join(a1, a2); w.z = join(a2, a3); w.w = join(a3, a4);
        } else {
            // The file the lane's first byte lies in: the frame's, or one further on (a header, or files without a frame).  Inside
            // the 16 bytes at most one more file starts (a file holds 42 bytes at least) and at most frames f + 1 and f + 2 (a frame
            // holds 11): their places are loaded at once, then every byte picks its source.
            int j = f >= 0 ? fe.y : 0;
            if (j + 1 < n_jobs && (long)info[FLAC_INFO_WORDS * (j + 1) + FLAC_INFO_BASE] <= p0) {
                int lo = j + 2, hi = n_jobs;  // past the frame's file: the last file that starts at or before p0, by bisection
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((long)info[FLAC_INFO_WORDS * mid + FLAC_INFO_BASE] <= p0) lo = mid + 1;
                    else hi = mid;
                }
                j = lo - 1;
            }
            const long b0 = info[FLAC_INFO_WORDS * j + FLAC_INFO_BASE];
            const long b1 = j + 1 < n_jobs ? (long)info[FLAC_INFO_WORDS * (j + 1) + FLAC_INFO_BASE] : 0x7fffffffffffL;
            long go[3], gz[3], gi[3];
            MI355_UNROLL
            for (int c = 0; c < 3; ++c) {
                const long g = f + c;
                const bool ok = g >= 0 && g < n_frames;
                gi[c] = ok ? g : 0;
                go[c] = ok ? (long)ftab[gi[c]].x : 0x7fffffffffffL;
                gz[c] = ok ? (long)sizes[gi[c]] : 0;
            }
            unsigned ww[4] = {0u, 0u, 0u, 0u};
            MI355_UNROLL
            for (int k = 0; k < 16; ++k) {
                const long p = p0 + k;
                const int c = go[2] <= p ? 2 : go[1] <= p ? 1 : 0;
                const long r = p - go[c];  // (negative where no frame starts at or before p)
                const bool in_frame = r >= 0 && r < gz[c];
                const int jj = b1 <= p ? j + 1 : j;
                const long hrel = p - (b1 <= p ? b1 : b0);
                const bool in_hdr = p < end && hrel < FLAC_HEADER_BYTES;
                unsigned byte = 0u;
                if (in_hdr) byte = (hdr[(size_t)FLAC_HDR_WORDS * jj + (hrel >> 2)] >> (8 * (int)(hrel & 3))) & 0xffu;
                else if (p < end && in_frame) byte = slots[(size_t)gi[c] * FLAC_SLOT_BYTES + r];
                ww[k >> 2] |= byte << (8 * (k & 3));
            }
            w.x = ww[0]; w.y = ww[1]; w.z = ww[2]; w.w = ww[3];
        }
        *reinterpret_cast<uint4*>(out + (p0 - base0)) = w;
    }
}

void launch_flac_place(const FlacJob* jobs, int n_jobs, long n_frames, int rate, long base0, int* sizes, unsigned* pre, int2* ftab,
                       unsigned* hdr, int* item_first, int* jtab, hipStream_t s) {
    if (n_jobs <= 0) return;
    LAUNCH_KERNEL(k_flac_place, dim3(1), dim3(PLACE_THREADS), 0, s, jobs, n_jobs, n_frames, rate, base0, sizes, pre, ftab, hdr, item_first, jtab);
}

void launch_flac_gather_streams(int n_jobs, long n_frames, const uint8_t* slots, const int* sizes, const int2* ftab, const unsigned* hdr,
                                const int* item_first, long base0, long bound_bytes, uint8_t* out, hipStream_t s) {
    if (n_jobs <= 0 || bound_bytes <= 0) return;
    const long nitems = (bound_bytes + FLAC_GATHER_ITEM_BYTES - 1) / FLAC_GATHER_ITEM_BYTES;
    const long gx = std::min<long>(nitems, 8L * current_device_cu_count());  // as k_pack_streams: 8 workgroups of 4 waves per CU
    LAUNCH_KERNEL(k_flac_gather_streams, dim3((unsigned)gx), dim3(256), 0, s, n_jobs, n_frames, slots, sizes, ftab, hdr, item_first, base0, bound_bytes, out);
}

// "fLaC", the one metadata block (STREAMINFO, flagged last) — 42 bytes; the MD5 stays zero: not computed
void flac_stream_header(uint8_t* h, int rate, int64_t total, const int* sizes, long n_frames) {
    unsigned fmin = 0, fmax = 0;
    for (long f = 0; f < n_frames; ++f) {
        const unsigned v = (unsigned)sizes[f];
        fmin = f == 0 ? v : std::min(fmin, v);
        fmax = std::max(fmax, v);
    }
    memset(h, 0, FLAC_HEADER_BYTES);
    memcpy(h, "fLaC", 4);
    h[4] = 0x80; h[7] = 34;
    h[8] = h[10] = (uint8_t)(FLAC_BLOCK >> 8);
    h[9] = h[11] = (uint8_t)(FLAC_BLOCK & 0xff);
    h[12] = (uint8_t)(fmin >> 16); h[13] = (uint8_t)(fmin >> 8); h[14] = (uint8_t)fmin;
    h[15] = (uint8_t)(fmax >> 16); h[16] = (uint8_t)(fmax >> 8); h[17] = (uint8_t)fmax;
    // 20 bits rate, 3 bits channels - 1 (0), 5 bits bits per sample - 1 (15), 36 bits total samples
    const uint64_t v = ((uint64_t)(unsigned)rate << 44) | ((uint64_t)15 << 36) | ((uint64_t)total & 0xfffffffffULL);
    for (int k = 0; k < 8; ++k) h[18 + k] = (uint8_t)(v >> (56 - 8 * k));
}

}  // namespace m355
