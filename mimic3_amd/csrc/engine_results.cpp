// engine_results.cpp — everything behind the waveform of a completed run: the padded results (copy_out, fetch), the packed stream
// (plan, place, launch, copy-out), phoneme timing, the quiet edges, loudness, and the host blocks all of them hand to the caller.
// The synthesis graph itself, up to the finished float audio, is engine.cpp.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace m355 {

// ---------------------------------------------------------------- the host blocks of a result
namespace {
// Pinned host buffers for results, recycled process-wide: hipHostMalloc costs milliseconds for a 12 MB block (page
// pinning + IOMMU mapping), more than the D2H itself, so a buffer released by mi355vits_free_result goes back on a
// free list and the next call of any handle takes the smallest one that fits.  Buffers are handed out exclusively
// (a result stays valid until its free_result, whatever runs meanwhile); at most POOL_KEEP_BYTES stay cached.
class PinnedPool {
  public:
    static PinnedPool& get() {
        static PinnedPool* p = new PinnedPool();  // never destroyed: no hipHostFree after the runtime has shut down
        return *p;
    }
    void* take(size_t bytes, size_t* cap) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = free_.lower_bound(bytes);
            // a block more than twice as large as needed is left for a caller that needs it
            if (it != free_.end() && it->first <= 2 * bytes + (1 << 16)) {
                void* p = it->second;
                *cap = it->first;
                cached_ -= it->first;
                free_.erase(it);
                return p;
            }
        }
        const size_t want = ((bytes + (1 << 16) - 1) >> 16) << 16;  // 64 KiB granules: nearby sizes share blocks
        void* p = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            trim(0);
            if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess)
                throw EngineError(MI355VITS_ERR_NOMEM, "out of pinned host memory (result buffer)");
        }
        *cap = want;
        return p;
    }
    void give(void* p, size_t cap) {
        if (!p) return;
        {
            std::lock_guard<std::mutex> lk(mu_);
            free_.emplace(cap, p);
            cached_ += cap;
        }
        trim(POOL_KEEP_BYTES);
    }

  private:
    static constexpr size_t POOL_KEEP_BYTES = size_t(1) << 30;
    void trim(size_t keep) {
        std::vector<void*> drop;
        {
            std::lock_guard<std::mutex> lk(mu_);
            while (cached_ > keep && !free_.empty()) {
                auto it = std::prev(free_.end());
                cached_ -= it->first;
                drop.push_back(it->second);
                free_.erase(it);
            }
        }
        for (void* p : drop) (void)hipHostFree(p);
    }
    std::mutex mu_;
    std::multimap<size_t, void*> free_;
    size_t cached_ = 0;
};

// What the owner_ of every result struct points to, whichever of the five it is: the pinned blocks its pointers point into (with
// the capacities the pool wants back) and the heap blocks.  A block belongs to the owner from the moment it exists, so a call that
// fails half way leaves nothing behind once its struct is freed.
struct Owner {
    std::vector<std::pair<void*, size_t>> pinned;
    std::vector<void*> heap;
    void* take_pinned(size_t bytes) {
        pinned.emplace_back(nullptr, 0);
        pinned.back().first = PinnedPool::get().take(bytes, &pinned.back().second);
        return pinned.back().first;
    }
    template <typename T> T* alloc(size_t n) {
        heap.push_back(nullptr);
        heap.back() = malloc(sizeof(T) * n);
        if (!heap.back()) throw EngineError(MI355VITS_ERR_NOMEM, "out of host memory");
        return static_cast<T*>(heap.back());
    }
};
template <typename R> Owner* new_owner(R* out) {
    auto* own = new Owner();
    out->owner_ = own;
    return own;
}
}  // namespace

void release_result_owner(void* owner) {
    auto* own = static_cast<Owner*>(owner);
    if (!own) return;
    for (auto& b : own->pinned) PinnedPool::get().give(b.first, b.second);
    for (void* p : own->heap) free(p);
    delete own;
}

template <typename R> void Engine::begin_fetch(R* out, const char* call, bool call_in_null_text) {
    if (!out) throw EngineError(MI355VITS_ERR_INVALID, (call_in_null_text ? std::string(call) + ": " : std::string()) + "result pointer is null");
    memset(out, 0, sizeof(*out));
    if (!have_result_) throw EngineError(MI355VITS_ERR_INVALID, std::string(call) + ": no completed run on this handle");
    HIP_CHECK(hipSetDevice(device_));
}

// ---------------------------------------------------------------- the padded results (mi355vits_run / mi355vits_fetch)
void Engine::copy_out(uint32_t want, mi355vits_result* out) {
    const int B = B_;
    Owner* own = new_owner(out);
    out->batch = B;
    out->l_max = Lo_;
    out->ty_max = Ty_;
    out->lengths = own->alloc<int64_t>(B);
    out->peaks = own->alloc<float>(B);
    for (int b = 0; b < B; ++b) out->lengths[b] = h_olen_[b];
    std::vector<unsigned> pk(B);
    HIP_CHECK(hipMemcpyAsync(pk.data(), o_peaks_, sizeof(unsigned) * B, hipMemcpyDeviceToHost, stream_));
    const bool dev_only = (want & MI355VITS_DEVICE_ONLY) != 0;
    if (!dev_only && (want & MI355VITS_WANT_FLOAT)) {
        out->audio = static_cast<float*>(own->take_pinned(sizeof(float) * (size_t)B * Lo_ + 16));
        HIP_CHECK(hipMemcpyAsync(out->audio, o_audio_, sizeof(float) * (size_t)B * Lo_, hipMemcpyDeviceToHost, stream_));
    }
    if (!dev_only && (want & MI355VITS_WANT_PCM16)) {
        if (!have_pcm_) {
            launch_pcm16(o_audio_, Lo_, o_peaks_, o_alen_, B, (int)Lo_, d_pcm_, Lo_, stream_, nullptr);
            have_pcm_ = true;
        }
        out->pcm = static_cast<int16_t*>(own->take_pinned(sizeof(int16_t) * (size_t)B * Lo_ + 16));
        HIP_CHECK(hipMemcpyAsync(out->pcm, d_pcm_, sizeof(int16_t) * (size_t)B * Lo_, hipMemcpyDeviceToHost, stream_));
    }
    HIP_CHECK(hipStreamSynchronize(stream_));
    for (int b = 0; b < B; ++b) memcpy(&out->peaks[b], &pk[b], 4);
}

void Engine::fetch(uint32_t want, mi355vits_result* out) {
    begin_fetch(out, "fetch", false);
    copy_out(want & ~MI355VITS_DEVICE_ONLY, out);
}

void Engine::device_buffers(const int16_t** pcm, const float** audio, long* row_stride, int* batch, const int** dev_lengths) {
    if (!have_result_) throw EngineError(MI355VITS_ERR_INVALID, "device_buffers: no completed run on this handle");
    HIP_CHECK(hipSetDevice(device_));
    if (pcm && !have_pcm_) {
        launch_pcm16(o_audio_, Lo_, o_peaks_, o_alen_, B_, (int)Lo_, d_pcm_, Lo_, stream_, nullptr);
        have_pcm_ = true;
    }
    HIP_CHECK(hipStreamSynchronize(stream_));  // the caller reads them from another stream (RCCL)
    if (pcm) *pcm = d_pcm_;
    if (audio) *audio = o_audio_;
    if (row_stride) *row_stride = Lo_;
    if (batch) *batch = B_;
    if (dev_lengths) *dev_lengths = o_alen_;
}

// ---------------------------------------------------------------- packed results (mi355vits_run_packed / mi355vits_fetch_packed)
static_assert(MI355VITS_ENC_S16LE == PACK_ENC_S16 && MI355VITS_ENC_ULAW == PACK_ENC_ULAW && MI355VITS_ENC_ALAW == PACK_ENC_ALAW &&
                  MI355VITS_ENC_F32LE == PACK_ENC_F32, "the ABI's encoding values are the kernels' own");
// The sample encoding of the packed streams made after this (read by run_packed / fetch_packed when they plan their pack).
void Engine::set_output_encoding(int enc) {
    if (enc != MI355VITS_ENC_S16LE && enc != MI355VITS_ENC_ULAW && enc != MI355VITS_ENC_ALAW && enc != MI355VITS_ENC_F32LE)
        throw EngineError(MI355VITS_ERR_INVALID, "output encoding " + std::to_string(enc) + " unknown (0 = s16le, 1 = ulaw, 2 = alaw, 3 = f32le)");
    pack_.enc = enc;
}

// The compression of the packed stream made after this (read by run_packed / fetch_packed when they plan their pack; never by a
// streams call).
void Engine::set_output_compression(int mode) {
    if (mode != MI355VITS_COMPRESS_NONE && mode != MI355VITS_COMPRESS_FLAC)
        throw EngineError(MI355VITS_ERR_INVALID, "output compression " + std::to_string(mode) + " unknown (0 = none, 1 = flac)");
    pack_.compress = mode;
}

namespace {
constexpr int64_t PACK_MAX_SAMPLES = 0x7fffffffLL;                       // total_samples <= 2^31 - 1
constexpr int64_t RIFF_MAX_SAMPLES = (0xffffffffLL - 36) / 2;            // 36 + 2 * total_samples must fit RIFF's 32-bit size
EngineError pack_error(int entry, const std::string& what) {
    return EngineError(MI355VITS_ERR_INVALID, (entry >= 0 ? "pack entry " + std::to_string(entry) + ": " : std::string("pack: ")) + what);
}
// FLAC's STREAMINFO holds the rate in 20 bits
void check_flac_rate(int hz) {
    if (hz > FLAC_MAX_RATE)
        throw pack_error(-1, "a FLAC stream holds rates up to " + std::to_string(FLAC_MAX_RATE) + " Hz; the run's rate is " + std::to_string(hz) + " Hz");
}
void check_pack_size(int entry, int64_t samples, bool wav, int enc) {
    if (samples > PACK_MAX_SAMPLES) throw pack_error(entry, "total_samples exceeds 2^31 - 1");
    if (!wav) return;
    if (enc == PACK_ENC_S16) {
        if (samples > RIFF_MAX_SAMPLES) throw pack_error(entry, "WAV data size does not fit RIFF's 32-bit fields (36 + 2 * total_samples > 2^32 - 1)");
        return;
    }
    // the 58-byte non-PCM form: RIFF size = 50 + data (+ one pad byte behind an odd data size: G.711 only)
    const int64_t bps = pack_bytes_per_sample(enc), data = bps * samples;
    if (50 + data + (data & 1) > 0xffffffffLL)
        throw pack_error(entry, "WAV data size does not fit RIFF's 32-bit fields (50 + " + std::to_string(bps) + " * total_samples > 2^32 - 1)");
}

// An entry's span of its row's n samples from the row's first / last loud sample (n / -1 when it has none) and the samples kept
// around them: [first, end).  A row without a loud sample — a NaN peak — keeps nothing.
void trimmed_span(int64_t n, int64_t first_loud, int64_t last_loud, int64_t keep, int64_t* first, int64_t* end) {
    *first = std::min(n, std::max<int64_t>(0, first_loud - keep));
    *end = std::max(*first, std::min(n, last_loud + 1 + keep));
}

// RIFF/WAVE, mono, little-endian fields, in front of `data` bytes of `total` samples at h.  int16: the 44 bytes the stdlib `wave`
// module writes (PCM, format tag 1).  Any other encoding: the non-PCM form — an 18-byte fmt chunk with cbSize 0, then a fact chunk with
// the sample count —, 58 bytes, what scipy.io.wavfile.write puts in front of float32 data; format tag 7 = mu-law, 6 = A-law,
// 3 = IEEE float.  RIFF chunks are word-aligned: behind an odd data size (G.711 only) goes one zero byte, written here as well.
// (with_pad = false: the header's own bytes only — a streams block, whose pad bytes the kernel writes)
void write_wav_header(uint8_t* h, int enc, uint32_t rate, int64_t total, size_t data, bool with_pad = true) {
    const bool pcm = enc == PACK_ENC_S16;
    const uint32_t bps = (uint32_t)pack_bytes_per_sample(enc), pad = (uint32_t)(data & 1);
    size_t at = 0;
    auto tag = [&](const char* t) { memcpy(h + at, t, 4); at += 4; };
    auto u32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) h[at++] = (uint8_t)(v >> (8 * k)); };
    auto u16 = [&](uint32_t v) { h[at++] = (uint8_t)v; h[at++] = (uint8_t)(v >> 8); };
    tag("RIFF");
    u32((uint32_t)((pcm ? 36 : 50) + data + pad));
    tag("WAVE");
    tag("fmt ");
    u32(pcm ? 16 : 18);
    u16(pcm ? 1 : enc == PACK_ENC_ULAW ? 7 : enc == PACK_ENC_ALAW ? 6 : 3);
    u16(1);
    u32(rate);
    u32(rate * bps);
    u16(bps);
    u16(8 * bps);
    if (!pcm) {
        u16(0);
        tag("fact");
        u32(4);
        u32((uint32_t)total);
    }
    tag("data");
    u32((uint32_t)data);
    if (pad && with_pad) h[at + data] = 0;
}
}  // namespace

// Everything that can be wrong with the pack arguments alone, before anything is sized or launched.
void Engine::plan_pack(const mi355vits_pack_args* pack, int B, const PackSettings& set, PackPlan& plan) const {
    if (set.flac()) {
        // FLAC is a layer over the S16LE stream, and a file of its own
        static const char* const enc_names[] = {"s16le", "ulaw", "alaw", "f32le"};  // by PackEncoding
        if (set.enc != PACK_ENC_S16) throw pack_error(-1, std::string("FLAC compresses the s16le stream; output encoding is ") + enc_names[set.enc]);
        if (pack && pack->wav_header != 0) throw pack_error(-1, "a FLAC stream carries its own header (wav_header must be 0)");
    }
    plan.n = pack ? pack->n : B;
    if (plan.n < 1 || plan.n > B) throw pack_error(-1, "n = " + std::to_string(plan.n) + " out of range (1 .. batch = " + std::to_string(B) + ")");
    plan.wav = pack && pack->wav_header != 0;
    plan.set = set;  // the handle's settings are read by the caller: when a pack is made (a streams call brings each stream's own)
    plan.tail = pack ? pack->tail_samples : 0;
    plan.order.resize(plan.n);
    plan.lead.assign(plan.n, 0);
    std::vector<int> at(B, -1);
    int64_t silence = 0;
    for (int i = 0; i < plan.n; ++i) {
        const int row = (pack && pack->order) ? pack->order[i] : i;
        if (row < 0 || row >= B) throw pack_error(i, "row " + std::to_string(row) + " out of range (batch = " + std::to_string(B) + ")");
        if (at[row] >= 0) throw pack_error(i, "row " + std::to_string(row) + " appears twice (also entry " + std::to_string(at[row]) + ")");
        at[row] = i;
        plan.order[i] = row;
        const int64_t lead = (pack && pack->lead_samples) ? pack->lead_samples[i] : 0;
        if (lead < 0) throw pack_error(i, "negative silence (" + std::to_string(lead) + " samples)");
        check_pack_size(i, lead, plan.wav, plan.set.enc);
        plan.lead[i] = lead;
        silence += lead;
        check_pack_size(i, silence, plan.wav, plan.set.enc);  // the silences alone: no row is synthesised for a stream that cannot exist
    }
    if (plan.tail < 0) throw pack_error(-1, "negative tail silence (" + std::to_string(plan.tail) + " samples)");
    check_pack_size(-1, plan.tail, plan.wav, plan.set.enc);
    check_pack_size(-1, silence + plan.tail, plan.wav, plan.set.enc);
}

// Where every entry goes, from the frame counts the host already holds — with trimming on from the edges as well (h_edges_ at the
// plan's ratio: find_edges first); the size limits with the audio counted in.
void Engine::place_pack(PackPlan& plan) const {
    const PackSettings& set = plan.set;
    plan.offsets.resize(plan.n);
    plan.lengths.resize(plan.n);
    plan.skip.assign(set.trimmed() ? plan.n : 0, 0);
    plan.gain.assign(set.normalised() ? plan.n : 0, 0.0);
    int64_t pos = 0;
    plan.audio = 0;
    for (int i = 0; i < plan.n; ++i) {
        const int row = plan.order[i];
        pos += plan.lead[i];
        plan.offsets[i] = pos;
        plan.lengths[i] = h_olen_[row];  // at the run's rate
        if (set.trimmed()) {
            int64_t first, end;
            const std::vector<int>& ed = edges_at(set.trim_ratio);
            trimmed_span(h_olen_[row], ed[row], ed[B_ + row], set.trim_keep, &first, &end);
            plan.skip[i] = (int)first;
            plan.lengths[i] = end - first;
        }
        if (set.normalised()) {
            bool limited;
            loudness_gain(h_loud_[row], ceiling_peak(row, set), set.loud_target, set.loud_ceiling, set.limit_window, &plan.gain[i], &limited);
        }
        pos += plan.lengths[i];
        plan.audio += plan.lengths[i];
        check_pack_size(i, pos, plan.wav, set.enc);
    }
    plan.total = pos + plan.tail;
    check_pack_size(-1, plan.total, plan.wav, set.enc);
}

// A packed call's plan: one stream under the handle's settings, read now.
void Engine::plan_single(const mi355vits_pack_args* pack, int B, OutputPlan& op) const {
    op.single = true;
    op.streams.assign(1, PackPlan());
    plan_pack(pack, B, pack_, op.streams[0]);
    op.entries = op.streams[0].n;
}

void Engine::run_packed(const RunCall& call, const mi355vits_pack_args* pack, mi355vits_packed_result* out) {
    run_output(call, out, [&](OutputPlan& op) { plan_single(pack, call.args.batch, op); });
}

void Engine::fetch_packed(const mi355vits_pack_args* pack, mi355vits_packed_result* out) {
    begin_fetch(out, "fetch_packed", false);
    OutputPlan op;
    plan_single(pack, B_, op);
    output_last_run(op, out);
}

namespace {
// the entry's f32 scale: 32767 * gain in double, rounded once (F32LE: the gain itself)
float entry_scale(const PackSettings& set, double gain) { return set.enc == PACK_ENC_F32 ? (float)gain : (float)(32767.0 * gain); }

// What the host checks of the sizes a FLAC launch reports.  The bytes of `count` frames from frame `first` on, each within what a
// frame of FLAC_BLOCK samples can take ...
size_t flac_frame_bytes(const int* sizes, size_t first, long count) {
    size_t bytes = 0;
    for (size_t f = first; f < first + (size_t)count; ++f) {
        const int sz = sizes[f];
        if (sz < 11 || sz > 16 + 2 * FLAC_BLOCK) throw EngineError(MI355VITS_ERR_INTERNAL, "flac: frame " + std::to_string(f) + " has " + std::to_string(sz) + " bytes");
        bytes += (size_t)sz;
    }
    return bytes;
}
// ... and a total, a place or an end the device made from them against the host's own
void flac_agree(bool same, const std::string& what) {
    if (!same) throw EngineError(MI355VITS_ERR_INTERNAL, "flac: the device's " + what);
}
}  // namespace

void Engine::flac_prof_bytes(double bytes) {
    if (flac_prof_rec_ >= 0 && (size_t)flac_prof_rec_ < prof_.recs.size()) prof_.recs[(size_t)flac_prof_rec_].bytes += bytes;
}

// The result of a single plan: exactly the stream lands behind the header the host writes.  FLAC: the compressed size depends on the
// audio, so the frame sizes and their total come first (4 * (frames + 1) bytes, ONE synchronisation more than an uncompressed
// pack), then exactly the frames land behind the 42 header bytes.
void Engine::copy_out_plan(OutputPlan& op, mi355vits_packed_result* out) {
    const PackPlan& plan = op.streams[0];
    const bool flac = plan.set.flac();
    const int n = plan.n;
    const long frames = op.n_frames;
    Owner* own = new_owner(out);
    out->n = n;
    out->total_samples = plan.total;
    out->offsets = own->alloc<int64_t>(n);
    out->lengths = own->alloc<int64_t>(n);
    out->peaks = own->alloc<float>(n);
    std::vector<unsigned> pk(B_);
    HIP_CHECK(hipMemcpyAsync(pk.data(), o_peaks_, sizeof(unsigned) * B_, hipMemcpyDeviceToHost, stream_));
    if (flac) {
        h_flac_sizes_.assign((size_t)frames + 1, 0);
        if (frames > 0) HIP_CHECK(hipMemcpyAsync(h_flac_sizes_.data(), d_flac_sizes_, 4 * ((size_t)frames + 1), hipMemcpyDeviceToHost, stream_));
    } else {
        const size_t hdr = plan.header_bytes(), data = (size_t)plan.bps() * (size_t)plan.total;
        const size_t pad = (plan.wav && (data & 1)) ? 1 : 0;  // the RIFF pad byte (write_wav_header)
        const size_t lead = hdr == 58 ? 6 : 0;  // the 58-byte header starts 6 bytes into the block: the data behind it keeps the block's alignment
        out->bytes = static_cast<uint8_t*>(own->take_pinned(lead + hdr + data + pad + 16)) + lead;
        out->n_bytes = hdr + data + pad;
        out->pcm = reinterpret_cast<int16_t*>(out->bytes + hdr);  // the first data byte, whatever the encoding
        HIP_CHECK(hipMemcpyAsync(out->pcm, d_pack_, data, hipMemcpyDeviceToHost, stream_));  // exactly the stream: lands behind the header
        if (plan.wav) write_wav_header(out->bytes, plan.set.enc, (uint32_t)run_hz_, plan.total, data);  // the rate the run ran at
    }
    for (int i = 0; i < n; ++i) {
        out->offsets[i] = plan.offsets[i];
        out->lengths[i] = plan.lengths[i];
    }
    HIP_CHECK(hipStreamSynchronize(stream_));
    for (int i = 0; i < n; ++i) memcpy(&out->peaks[i], &pk[plan.order[i]], 4);
    if (!flac) return;
    const size_t data = flac_frame_bytes(h_flac_sizes_.data(), 0, frames);
    flac_agree((unsigned)h_flac_sizes_[(size_t)frames] == (unsigned)data, "total differs from the sum of the frame sizes");
    flac_prof_bytes((double)data);
    const size_t lead = 6;  // the 42-byte header starts 6 bytes into the block: the frames behind it keep the block's alignment
    out->bytes = static_cast<uint8_t*>(own->take_pinned(lead + FLAC_HEADER_BYTES + data + 16)) + lead;
    out->n_bytes = FLAC_HEADER_BYTES + data;
    out->pcm = reinterpret_cast<int16_t*>(out->bytes + FLAC_HEADER_BYTES);  // the first frame
    flac_stream_header(out->bytes, run_hz_, plan.total, h_flac_sizes_.data(), frames);
    if (data) {
        HIP_CHECK(hipMemcpyAsync(out->bytes + FLAC_HEADER_BYTES, d_flac_out_, data, hipMemcpyDeviceToHost, stream_));  // exactly the frames
        HIP_CHECK(hipStreamSynchronize(stream_));
    }
}

// ---------------------------------------------------------------- several streams of one run (mi355vits_run_streams / mi355vits_fetch_streams)
namespace {
std::string fmt_g(double v) {
    char b[64];
    snprintf(b, sizeof b, "%g", v);
    return b;
}
constexpr int64_t STREAMS_MAX_BYTES = 0x7fffffffLL;  // the block's offsets fit the table's words
}  // namespace

// Everything that can be wrong with the arguments alone: each stream's settings by the rules of the setters, its pack by plan_pack's.
std::vector<mi355vits_stream_args2> Engine::streams_v1(const mi355vits_stream_args* streams, int n_streams) const {
    std::vector<mi355vits_stream_args2> v((streams && n_streams > 0) ? (size_t)n_streams : 0);
    for (size_t s = 0; s < v.size(); ++s) {
        memset(&v[s], 0, sizeof(v[s]));
        v[s].base = streams[s];
        v[s].compression = MI355VITS_COMPRESS_NONE;
        v[s].limiter_window_samples = pack_.limit_window;  // the handle settings a v1 streams call reads: mi355vits_stream_args is frozen
        v[s].ceiling_mode = pack_.ceil_mode;
    }
    return v;
}

void Engine::plan_streams(const mi355vits_stream_args2* streams, int n_streams, int B, OutputPlan& op) const {
    if (!streams || n_streams < 1)
        throw EngineError(MI355VITS_ERR_INVALID, "streams: a non-null array of n_streams >= 1 streams is required (n_streams = " + std::to_string(n_streams) + ")");
    op.streams.assign((size_t)n_streams, PackPlan());
    op.entries = 0;
    for (int s = 0; s < n_streams; ++s) {
        const mi355vits_stream_args2& a2 = streams[s];
        const mi355vits_stream_args& a = a2.base;
        const std::string name = "stream " + std::to_string(s) + ": ";
        auto bad = [&](const std::string& what) { return EngineError(MI355VITS_ERR_INVALID, name + what); };
        if (a.encoding != MI355VITS_ENC_S16LE && a.encoding != MI355VITS_ENC_ULAW && a.encoding != MI355VITS_ENC_ALAW && a.encoding != MI355VITS_ENC_F32LE)
            throw bad("unknown encoding " + std::to_string(a.encoding) + " (0 = s16le, 1 = ulaw, 2 = alaw, 3 = f32le)");
        if (!(a.trim_ratio >= 0.0f && a.trim_ratio <= 1.0f)) throw bad("trim ratio " + fmt_g(a.trim_ratio) + " is outside [0, 1]");  // NaN fails both
        if (a.trim_keep_samples < 0) throw bad("trim keep_samples " + std::to_string(a.trim_keep_samples) + " is negative");
        if (!(a.target_lufs == 0.0f || (a.target_lufs >= -70.0f && a.target_lufs < 0.0f)))
            throw bad("loudness target " + fmt_g(a.target_lufs) + " LUFS is neither 0 (off) nor in [-70, 0)");
        if (a.target_lufs != 0.0f && !(std::isfinite(a.ceiling_dbfs) && a.ceiling_dbfs <= 0.0f))
            throw bad("loudness ceiling " + fmt_g(a.ceiling_dbfs) + " dBFS is not a finite value <= 0");
        if (a2.compression != MI355VITS_COMPRESS_NONE && a2.compression != MI355VITS_COMPRESS_FLAC)
            throw bad("unknown compression " + std::to_string(a2.compression) + " (0 = none, 1 = flac)");
        if (a2.limiter_window_samples < 0 || a2.limiter_window_samples > LIMIT_MAX_WINDOW)
            throw bad("limiter window " + std::to_string(a2.limiter_window_samples) + " is outside 0 .. " + std::to_string(LIMIT_MAX_WINDOW));
        if (a2.ceiling_mode != MI355VITS_CEILING_SAMPLE && a2.ceiling_mode != MI355VITS_CEILING_TRUE_PEAK)
            throw bad("unknown ceiling mode " + std::to_string(a2.ceiling_mode) + " (0 = sample peak, 1 = true peak)");
        for (int r : a2.reserved)
            if (r != 0) throw bad("reserved fields must be 0");
        if (a2.compression == MI355VITS_COMPRESS_FLAC) {
            static const char* const enc_names[] = {"s16le", "ulaw", "alaw", "f32le"};  // by PackEncoding
            if (a.encoding != MI355VITS_ENC_S16LE) throw bad(std::string("FLAC compresses the s16le stream; encoding is ") + enc_names[a.encoding]);
            if (a.pack.wav_header != 0) throw bad("a FLAC stream carries its own header (wav_header must be 0)");
        }
        PackSettings set;
        set.enc = a.encoding;
        set.trim_ratio = a.trim_ratio;
        set.trim_keep = a.trim_keep_samples;
        set.loud_target = a.target_lufs;
        if (a.target_lufs != 0.0f) set.loud_ceiling = a.ceiling_dbfs;
        set.limit_window = a2.limiter_window_samples;
        set.ceil_mode = a2.ceiling_mode;
        set.compress = a2.compression;
        try {
            plan_pack(&a.pack, B, set, op.streams[s]);
        } catch (const EngineError& e) {
            throw EngineError(e.code, name + e.what());
        }
        op.entries += op.streams[s].n;
    }
}

// Every stream placed as its own pack, then (block form) the streams in the block: each one's first data byte at the next multiple
// of 16 that leaves room for its header, the header right in front of it, the RIFF pad byte behind an odd data size.
void Engine::place(OutputPlan& op) const {
    const size_t S = op.streams.size();
    op.begin.assign(S, 0);
    op.data.assign(S, 0);
    op.src.assign(S, -1);
    op.frames.assign(S, 0);
    op.dev.clear();
    op.audio = 0;
    op.n_flac = 0;
    op.n_frames = 0;
    std::vector<int> flac;
    int64_t pos = 0;
    for (size_t s = 0; s < S; ++s) {
        PackPlan& p = op.streams[s];
        try {
            place_pack(p);
        } catch (const EngineError& e) {
            if (op.single) throw;
            throw EngineError(e.code, "stream " + std::to_string(s) + ": " + e.what());
        }
        op.audio += p.audio;
        if (op.single) {
            // no block around its one stream: k_pack writes it at d_pack_, where the one FLAC job reads it
            op.dev.push_back(0);
            if (p.set.flac()) {
                op.src[0] = 0;
                op.n_flac = 1;
                op.n_frames = op.frames[0] = flac_frames((long)p.total);
            }
            return;
        }
        if (p.set.flac()) {
            flac.push_back((int)s);  // behind the uncompressed streams, below
            continue;
        }
        const int64_t hdr = (int64_t)p.header_bytes(), bytes = (int64_t)p.bps() * p.total;
        op.data[s] = (pos + hdr + 15) & ~int64_t(15);
        op.begin[s] = op.data[s] - hdr;
        pos = op.data[s] + bytes + ((p.wav && (bytes & 1)) ? 1 : 0);
        op.dev.push_back((int)s);
        if (pos > STREAMS_MAX_BYTES) {
            // (what the remaining streams add only makes it larger: the size named is the block up to this stream)
            throw EngineError(MI355VITS_ERR_INVALID, "streams: block of " + std::to_string(pos) + " bytes exceeds 2^31 - 1");
        }
    }
    op.plain_bytes = op.n_bytes = pos;
    op.flac_base = op.flac_bound = 0;
    if (flac.empty()) return;
    // the compressed streams: their samples behind the uncompressed block, each at a multiple of 16; the block counted with every
    // file at its bound
    op.flac_base = (pos + 15) & ~int64_t(15);
    int64_t at = op.flac_base, bound = op.flac_base;
    for (int s : flac) {
        const PackPlan& p = op.streams[(size_t)s];
        op.src[(size_t)s] = at;
        op.frames[(size_t)s] = flac_frames((long)p.total);
        op.n_frames += op.frames[(size_t)s];
        op.dev.push_back(s);
        op.n_bytes = at + 2 * p.total;
        at = (op.n_bytes + 15) & ~int64_t(15);
        bound += flac_file_bound((long)p.total);
        if (bound > STREAMS_MAX_BYTES || at > STREAMS_MAX_BYTES)
            throw EngineError(MI355VITS_ERR_INVALID, "streams: block of " + std::to_string(std::max(bound, at)) + " bytes exceeds 2^31 - 1 (a FLAC stream counted at its bound)");
    }
    op.n_flac = (int)flac.size();
    op.flac_bound = bound - op.flac_base;
}

void Engine::fill_table(const OutputPlan& op, int* tab) const {
    if (op.single) {
        // k_pack's segment table [seg_rows][n]: only the rows its settings need
        const PackPlan& plan = op.streams[0];
        const PackSettings& set = plan.set;
        const size_t n = plan.n;
        for (size_t i = 0; i < n; ++i) {
            tab[PACK_SEG_OFFSET * n + i] = (int)plan.offsets[i];
            tab[PACK_SEG_ROW * n + i] = plan.order[i];
            tab[PACK_SEG_LENGTH * n + i] = (int)plan.lengths[i];
            if (set.trimmed()) tab[PACK_SEG_SKIP * n + i] = plan.skip[i];
            if (set.normalised()) {
                const float scale = entry_scale(set, plan.gain[i]);
                memcpy(&tab[pack_seg_scale_row(set.trimmed()) * n + i], &scale, 4);
            }
            if (plan.curved()) tab[pack_seg_curve_row(set.trimmed()) * n + i] = plan.curve[i];
        }
        return;
    }
    const size_t n = (size_t)op.entries;
    int* st = tab + pack_ent_rows(op.curved) * n;
    size_t e = 0;
    for (size_t d = 0; d < op.dev.size(); ++d) {
        const size_t s = (size_t)op.dev[d];  // in the order of their places (without a compressed stream: the order given)
        const PackPlan& p = op.streams[s];
        const PackSettings& set = p.set;
        const int64_t bytes = (int64_t)p.bps() * p.total;
        // (a compressed stream: its samples as a headerless S16LE stream, k_flac_frames' source)
        const int64_t data = set.flac() ? op.src[s] : op.data[s], begin = set.flac() ? op.src[s] : op.begin[s];
        for (int i = 0; i < p.n; ++i, ++e) {
            tab[PACK_ENT_OFFSET * n + e] = (int)(data + (int64_t)p.bps() * p.offsets[i]);
            tab[PACK_ENT_ROW * n + e] = p.order[i];
            tab[PACK_ENT_LENGTH * n + e] = (int)p.lengths[i];
            tab[PACK_ENT_SKIP * n + e] = set.trimmed() ? p.skip[i] : 0;
            const bool curved = p.curved() && p.curve[i] >= 0;
            tab[PACK_ENT_ENC * n + e] = set.enc | (set.normalised() ? (int)PACK_ENT_SCALED : 0) | (curved ? (int)PACK_ENT_CURVED : 0);
            if (op.curved) tab[PACK_ENT_CURVE * n + e] = curved ? p.curve[i] : 0;
            const float scale = set.normalised() ? entry_scale(set, p.gain[i]) : 0.0f;
            memcpy(&tab[PACK_ENT_SCALE * n + e], &scale, 4);
        }
        int* r = st + PACK_STREAM_WORDS * d;
        r[PACK_STREAM_BEGIN] = (int)begin;
        r[PACK_STREAM_DATA] = (int)data;
        r[PACK_STREAM_END] = (int)(data + bytes);
        r[PACK_STREAM_ENC] = set.enc;
        uint8_t h[4 * (PACK_STREAM_WORDS - PACK_STREAM_HEADER)] = {0};
        if (p.wav) write_wav_header(h, set.enc, (uint32_t)run_hz_, p.total, (size_t)bytes, false);  // the rate the run ran at
        for (int k = 0; k < PACK_STREAM_WORDS - PACK_STREAM_HEADER; ++k)
            r[PACK_STREAM_HEADER + k] = (int)((uint32_t)h[4 * k] | ((uint32_t)h[4 * k + 1] << 8) | ((uint32_t)h[4 * k + 2] << 16) | ((uint32_t)h[4 * k + 3] << 24));
    }
}

void Engine::launch(const OutputPlan& op) {
    if (op.single) {
        static const char* const labels[] = {"pcm16.pack", "pack.ulaw", "pack.alaw", "pack.f32"};  // by PackEncoding
        const PackPlan& plan = op.streams[0];
        ProfScope ps(prof_, labels[plan.set.enc], 0, 4.0 * (double)plan.audio + (double)plan.bps() * (double)plan.total);
        launch_pack(plan.set.enc, o_audio_, Lo_, o_peaks_, d_vol_, d_pack_seg_, plan.n, d_pack_, (long)plan.total, stream_, plan.set.trimmed(),
                    plan.set.normalised(), plan.curved() ? d_curve_ : nullptr);
    } else {
        ProfScope ps(prof_, "pack.streams", 0, 4.0 * (double)op.audio + (double)op.n_bytes);
        launch_pack_streams(o_audio_, Lo_, o_peaks_, d_vol_, d_pack_seg_, op.entries, (int)op.streams.size(), d_pack_, (long)op.n_bytes, stream_,
                            op.curved ? d_curve_ : nullptr);
    }
    flac_prof_rec_ = -1;
    if (op.compressed()) launch_flac(op);
}

// The compressed streams of a plan: a job per stream over its samples in the pack kernel's buffer, k_flac_frames once over all of
// them (a workgroup per frame); then single: the sizes scanned and the frames gathered (k_flac_scan / k_flac_gather), block form: the
// places and headers (k_flac_place) and the compressed region (k_flac_gather_streams).  One profiler record.
void Engine::launch_flac(const OutputPlan& op) {
    if (op.single && op.n_frames == 0) return;  // an empty stream: the header alone, written by the host
    h_flac_jobs_.clear();
    double samples = 0;
    long slot0 = 0;
    for (int s : op.dev) {
        const PackPlan& p = op.streams[(size_t)s];
        if (!p.set.flac()) continue;
        h_flac_jobs_.push_back(FlacJob{reinterpret_cast<const int16_t*>(d_pack_ + op.src[(size_t)s]), (long)p.total, 0, (int)slot0});
        slot0 += op.frames[(size_t)s];
        samples += (double)p.total;
    }
    HIP_CHECK(hipMemcpyAsync(d_flac_jobs_, h_flac_jobs_.data(), sizeof(FlacJob) * h_flac_jobs_.size(), hipMemcpyHostToDevice, stream_));
    ProfScope ps(prof_, "pack.flac", 0, 2.0 * samples);  // + the frames' bytes once the host knows them (copy_out_plan)
    flac_prof_rec_ = ps.rec;
    launch_flac_frames(d_flac_jobs_, op.n_flac, op.n_frames, run_hz_, d_flac_slots_, d_flac_sizes_, stream_);
    if (op.single) {
        launch_flac_gather(d_flac_slots_, d_flac_sizes_, d_flac_offsets_, op.n_frames, d_flac_out_, stream_);
        return;
    }
    launch_flac_place(d_flac_jobs_, op.n_flac, op.n_frames, run_hz_, (long)op.flac_base, d_flac_sizes_, d_flac_pre_, d_flac_ftab_, d_flac_hdr_,
                      d_flac_items_, d_flac_jtab_, stream_);
    launch_flac_gather_streams(op.n_flac, op.n_frames, d_flac_slots_, d_flac_sizes_, d_flac_ftab_, d_flac_hdr_, d_flac_items_, (long)op.flac_base,
                               (long)op.flac_bound, d_flac_out_, stream_);
}

// The result of a block-form plan: the block's bytes and the arrays of either streams result struct.
template <typename R> void Engine::copy_out_plan(OutputPlan& op, R* out) {
    constexpr bool V2 = std::is_same<R, mi355vits_streams_result2>::value;
    const size_t S = op.streams.size(), E = (size_t)op.entries;
    Owner* own = new_owner(out);
    out->n_streams = (int32_t)S;
    out->n_entries = (int32_t)E;
    out->stream_offset = own->alloc<int64_t>(S);
    out->stream_bytes = own->alloc<int64_t>(S);
    out->data_offset = own->alloc<int64_t>(S);
    out->total_samples = own->alloc<int64_t>(S);
    out->encoding = own->alloc<int32_t>(S);
    out->entry_base = own->alloc<int32_t>(S + 1);
    out->rows = own->alloc<int32_t>(E);
    out->offsets = own->alloc<int64_t>(E);
    out->lengths = own->alloc<int64_t>(E);
    out->peaks = own->alloc<float>(E);
    out->first = own->alloc<int32_t>(E);
    out->lufs = own->alloc<double>(E);
    out->gain = own->alloc<double>(E);
    out->limited = own->alloc<int32_t>(E);
    if constexpr (V2) {
        out->compression = own->alloc<int32_t>(S);
        out->frames = own->alloc<int32_t>(S);
        out->uncompressed_bytes = op.plain_bytes;
    }
    std::vector<unsigned> pk(B_);
    size_t block_bytes = (size_t)op.n_bytes;
    std::vector<int64_t> fbytes(S, 0);  // compressed streams: header + frames
    if (op.compressed()) {
        // The sizes depend on the audio: the frame sizes, four words per compressed stream and the block's end come first — ONE
        // synchronisation more than the same block uncompressed —, then exactly the block's bytes.
        const size_t words = flac_info_words(op.n_frames, op.n_flac);
        h_flac_sizes_.assign(words, 0);
        HIP_CHECK(hipMemcpyAsync(h_flac_sizes_.data(), d_flac_sizes_, 4 * words, hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
        const int* info = h_flac_sizes_.data() + op.n_frames;
        int64_t at = op.flac_base;
        size_t f = 0, frame_bytes = 0;
        int j = 0;
        for (int s : op.dev) {
            if (!op.streams[(size_t)s].set.flac()) continue;
            const int64_t bytes = FLAC_HEADER_BYTES + (int64_t)flac_frame_bytes(h_flac_sizes_.data(), f, op.frames[(size_t)s]);
            f += (size_t)op.frames[(size_t)s];
            flac_agree(info[FLAC_INFO_WORDS * j + FLAC_INFO_BASE] == (int)at && info[FLAC_INFO_WORDS * j + FLAC_INFO_BYTES] == (int)bytes,
                       "place of stream " + std::to_string(s) + " differs from the sum of its frame sizes");
            op.begin[(size_t)s] = at;
            op.data[(size_t)s] = at + FLAC_HEADER_BYTES;
            fbytes[(size_t)s] = bytes;
            frame_bytes += (size_t)(bytes - FLAC_HEADER_BYTES);
            block_bytes = (size_t)(at + bytes);
            at = (at + bytes + 15) & ~int64_t(15);
            ++j;
        }
        flac_agree((int64_t)info[FLAC_INFO_WORDS * op.n_flac] == (int64_t)block_bytes, "block end differs from the host's");
        flac_prof_bytes((double)frame_bytes);
    }
    out->bytes = static_cast<uint8_t*>(own->take_pinned(block_bytes + 16));
    out->n_bytes = block_bytes;
    HIP_CHECK(hipMemcpyAsync(pk.data(), o_peaks_, sizeof(unsigned) * B_, hipMemcpyDeviceToHost, stream_));
    if (!op.compressed()) {
        HIP_CHECK(hipMemcpyAsync(out->bytes, d_pack_, block_bytes, hipMemcpyDeviceToHost, stream_));  // exactly the block: finished files
    } else {
        // the uncompressed part up to where the compressed one starts (the gap's zeros are k_pack_streams'), then the compressed part
        if (op.flac_base > 0) HIP_CHECK(hipMemcpyAsync(out->bytes, d_pack_, (size_t)op.flac_base, hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipMemcpyAsync(out->bytes + op.flac_base, d_flac_out_, block_bytes - (size_t)op.flac_base, hipMemcpyDeviceToHost, stream_));
    }
    size_t e = 0;
    for (size_t s = 0; s < S; ++s) {
        const PackPlan& p = op.streams[s];
        const int64_t bytes = (int64_t)p.bps() * p.total;
        out->stream_offset[s] = op.begin[s];
        out->data_offset[s] = op.data[s];
        out->stream_bytes[s] = p.set.flac() ? fbytes[s] : (op.data[s] - op.begin[s]) + bytes + ((p.wav && (bytes & 1)) ? 1 : 0);
        out->total_samples[s] = p.total;
        out->encoding[s] = p.set.enc;
        if constexpr (V2) {
            out->compression[s] = p.set.compress;
            out->frames[s] = (int32_t)op.frames[s];
        }
        out->entry_base[s] = (int32_t)e;
        for (int i = 0; i < p.n; ++i, ++e) {
            const int row = p.order[i];
            out->rows[e] = row;
            out->offsets[e] = p.offsets[i];
            out->lengths[e] = p.lengths[i];
            out->first[e] = p.set.trimmed() ? p.skip[i] : 0;
            out->lufs[e] = out->gain[e] = 0.0;
            out->limited[e] = 0;
            if (p.set.normalised()) {
                bool lim = false;
                out->lufs[e] = h_loud_[row];
                loudness_gain(h_loud_[row], ceiling_peak(row, p.set), p.set.loud_target, p.set.loud_ceiling, p.set.limit_window, &out->gain[e], &lim);
                out->limited[e] = lim ? 1 : 0;
            }
        }
    }
    out->entry_base[S] = (int32_t)e;
    HIP_CHECK(hipStreamSynchronize(stream_));
    for (size_t i = 0; i < E; ++i) memcpy(&out->peaks[i], &pk[out->rows[i]], 4);
}

// A run with an output plan, which make_plan fills from the form's own arguments (validating them) once the result struct is
// zeroed and the batch known to be one.  No stream trims, normalises or compresses: the places follow from the frame counts, so the table rides
// in the run's own upload and the pack kernel is its last launch.  Else the offsets / the scales depend on the audio and the frames
// are made from the finished stream: synthesise without an early table (and without the padded int16 pass: a packed-form call looks at
// no MI355VITS_WANT_* flag), then what the fetch of the same plan does.  A failure there — a limit exceeded by the trimmed sizes —
// leaves the handle as a failed run does: no result served.
template <typename R, typename F> void Engine::run_output(const RunCall& call, R* out, F&& make_plan) {
    if (!out) throw EngineError(MI355VITS_ERR_INVALID, "result pointer is null");
    memset(out, 0, sizeof(*out));
    if (call.args.batch < 1) throw EngineError(MI355VITS_ERR_INVALID, "batch and tx_max must be >= 1");
    OutputPlan op;
    make_plan(op);
    if (op.compressed()) check_flac_rate(output_rate());  // the rate this run will run at
    if (!op.measured() && !op.compressed()) {
        synthesize(call, &op);
        copy_out_plan(op, out);
        return;
    }
    mi355vits_run_args a = call.args;
    a.flags &= ~(uint32_t)MI355VITS_WANT_PCM16;
    synthesize(RunCall{a, call.rows, call.timing, call.speakers}, nullptr);
    try {
        output_last_run(op, out);
        HIP_CHECK(hipEventRecord(ev_end_, stream_));  // the run's time includes its measurements and its pack
    } catch (...) {
        have_result_ = false;
        throw;
    }
}

void Engine::run_streams(const RunCall& call, const mi355vits_stream_args* streams, int n_streams, mi355vits_streams_result* out) {
    run_output(call, out, [&](OutputPlan& op) {
        const std::vector<mi355vits_stream_args2> v = streams_v1(streams, n_streams);
        plan_streams(v.empty() ? nullptr : v.data(), n_streams, call.args.batch, op);
    });
}

void Engine::fetch_streams(const mi355vits_stream_args* streams, int n_streams, mi355vits_streams_result* out) {
    begin_fetch(out, "fetch_streams");
    OutputPlan op;
    const std::vector<mi355vits_stream_args2> v = streams_v1(streams, n_streams);
    plan_streams(v.empty() ? nullptr : v.data(), n_streams, B_, op);
    output_last_run(op, out);
}

void Engine::run_streams2(const RunCall& call, const mi355vits_stream_args2* streams, int n_streams, mi355vits_streams_result2* out) {
    run_output(call, out, [&](OutputPlan& op) { plan_streams(streams, n_streams, call.args.batch, op); });
}

void Engine::fetch_streams2(const mi355vits_stream_args2* streams, int n_streams, mi355vits_streams_result2* out) {
    begin_fetch(out, "fetch_streams2");
    OutputPlan op;
    plan_streams(streams, n_streams, B_, op);
    output_last_run(op, out);
}

template <typename R> void Engine::output_last_run(OutputPlan& op, R* out) {
    finish_last_run(op);
    copy_out_plan(op, out);
}

void Engine::finish_last_run(OutputPlan& op) {
    if (op.compressed()) check_flac_rate(run_hz_);
    HIP_CHECK(hipSetDevice(device_));
    std::vector<float> ratios;
    bool loud = false, tp = false;
    for (const PackPlan& p : op.streams) {
        ratios.push_back(p.set.trim_ratio);
        loud = loud || p.set.normalised();
        tp = tp || p.set.true_peak();
    }
    // (a block keeps what the host holds at other ratios; a single call at a ratio not held replaces it, as ever)
    measure_last_run(ratios, loud, !op.single, tp);
    place(op);
    {
        // the limiter: one job per distinct (row, target, ceiling, encoding class, window, mode) among the entries the ceiling would
        // hold back; the curves are made before the pack, on the same stream (a single plan has one key: run_limit_jobs itself)
        std::vector<LimitJob> jobs;
        LimitKeys keys;
        for (PackPlan& p : op.streams)
            if (p.set.limiting()) limit_pack(p, jobs, &keys);
        op.curved = !jobs.empty();
        if (op.curved) {
            run_limit_groups(jobs, keys);
            for (PackPlan& p : op.streams) curve_offsets(p, jobs);
        }
    }
    // behind the last run's frame-side layout where the arena has room (its data must stay: a reallocation would lose it),
    // else in an arena of its own
    ArenaCount need;
    layout(need, op);
    if (arena_b_.capacity() >= layout_b_end_ + need.bytes) {
        arena_b_.rewind(layout_b_end_);
        layout(arena_b_, op);
    } else {
        arena_p_.reserve(need.bytes + 4096, stream_);
        arena_p_.reset();
        layout(arena_p_, op);
    }
    h_pack_seg_.assign(op.table_words(), 0);  // a member: it outlives the copy whatever HIP does with pageable sources
    fill_table(op, h_pack_seg_.data());
    HIP_CHECK(hipMemcpyAsync(d_pack_seg_, h_pack_seg_.data(), h_pack_seg_.size() * 4, hipMemcpyHostToDevice, stream_));
    launch(op);
}

// ---------------------------------------------------------------- phoneme timing and levels (mi355vits_fetch_alignment)
void Engine::fetch_alignment(uint32_t want, mi355vits_alignment* out) {
    // (a null `out` is begin_fetch's to name first; unknown bits are named before a missing run)
    if (out && (want & ~MI355VITS_ALIGN_LEVELS)) throw EngineError(MI355VITS_ERR_INVALID, "fetch_alignment: unknown bits in want (" + std::to_string(want) + ")");
    begin_fetch(out, "fetch_alignment");
    const bool levels = (want & MI355VITS_ALIGN_LEVELS) != 0;
    const size_t n = (size_t)B_ * Tx_, arrays = levels ? 5 : 3;
    // one device block, array after array, in an arena of its own: the last run's buffers (phase A: durations, phase B: audio)
    // and whatever a fetch laid out behind them stay where they are
    arena_al_.reserve(5 * n * 4 + 4096, stream_);
    arena_al_.reset();
    int* d = arena_al_.alloc<int>(5 * n);
    float* d_peak = levels ? reinterpret_cast<float*>(d + 3 * n) : nullptr;
    float* d_rms = levels ? reinterpret_cast<float*>(d + 4 * n) : nullptr;
    {
        double audio = 0;
        for (int b = 0; b < B_; ++b) audio += (double)h_olen_[b];
        ProfScope ps(prof_, "align", 0, levels ? 4.0 * audio + 20.0 * (double)n : 12.0 * (double)n);
        launch_align(d_wceil_, d_cum_, d_len_, B_, Tx_, o_audio_, Lo_, o_alen_, cfg_.hop_length, run_L_, run_M_, d, d + n, d + 2 * n,
                     d_peak, d_rms, stream_, pitched_ ? d_wc_ : nullptr);
    }
    int32_t* h = static_cast<int32_t*>(new_owner(out)->take_pinned(arrays * n * 4 + 16));
    HIP_CHECK(hipMemcpyAsync(h, d, arrays * n * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    out->batch = B_;
    out->tx_max = Tx_;
    out->sample_rate = run_hz_;
    out->frames = h;
    out->start = h + n;
    out->samples = h + 2 * n;
    out->peak = levels ? reinterpret_cast<float*>(h + 3 * n) : nullptr;
    out->rms = levels ? reinterpret_cast<float*>(h + 4 * n) : nullptr;
}

// ---------------------------------------------------------------- the quiet edges of a run's rows (mi355vits_set_edge_trim / _fetch_edges)
void Engine::set_edge_trim(float ratio, int keep_samples) {
    if (!(ratio >= 0.0f && ratio <= 1.0f))  // NaN fails both
        throw EngineError(MI355VITS_ERR_INVALID, "set_edge_trim: ratio " + std::to_string(ratio) + " is outside [0, 1]");
    if (keep_samples < 0) throw EngineError(MI355VITS_ERR_INVALID, "set_edge_trim: keep_samples " + std::to_string(keep_samples) + " is negative");
    pack_.trim_ratio = ratio;
    pack_.trim_keep = keep_samples;
}

// The raw first / last loud sample of every row of the last run at `ratio` into h_edges_: one launch in an arena of its own, one
// 8 B byte copy, one synchronisation — or nothing when the host still holds them for this ratio.
void Engine::find_edges(float ratio) { measure_last_run({ratio}, false, false); }

const std::vector<int>& Engine::edges_at(float ratio) const {
    if (have_edges_)
        for (const EdgeSet& e : h_edges_)
            if (e.ready && e.ratio == ratio) return e.edges;
    throw EngineError(MI355VITS_ERR_INTERNAL, "edges of ratio " + std::to_string(ratio) + " were not measured");
}

bool Engine::enqueue_edges(const std::vector<float>& ratios, bool keep) {
    if (!have_edges_) h_edges_.clear();  // of an earlier run
    have_edges_ = true;
    h_edges_.erase(std::remove_if(h_edges_.begin(), h_edges_.end(), [](const EdgeSet& e) { return !e.ready; }), h_edges_.end());  // a copy that failed
    std::vector<float> todo;  // the distinct non-zero ratios the host does not hold
    for (float r : ratios) {
        bool held = r == 0.0f || std::find(todo.begin(), todo.end(), r) != todo.end();
        for (const EdgeSet& e : h_edges_) held = held || e.ratio == r;
        if (!held) todo.push_back(r);
    }
    if (todo.empty()) return false;
    if (!keep) h_edges_.clear();
    const int B = B_;
    arena_ed_.reserve(todo.size() * DeviceArena::padded(2 * (size_t)B * 4) + 4096, stream_);
    arena_ed_.reset();
    double audio = 0;
    for (int b = 0; b < B; ++b) audio += (double)h_olen_[b];
    h_edges_.reserve(h_edges_.size() + todo.size());
    for (float ratio : todo) {
        int* d = arena_ed_.alloc<int>(2 * (size_t)B);
        {
            ProfScope ps(prof_, "edges", 0, 4.0 * audio + 8.0 * (double)B);
            launch_edges(o_audio_, Lo_, o_alen_, o_peaks_, B, Lo_, ratio, d, d + B, stream_);
        }
        h_edges_.push_back(EdgeSet{ratio, std::vector<int>(2 * (size_t)B), false});
        HIP_CHECK(hipMemcpyAsync(h_edges_.back().edges.data(), d, 2 * (size_t)B * 4, hipMemcpyDeviceToHost, stream_));
    }
    return true;  // ready once the caller has synchronised
}

// What a pack needs from the audio before it can be placed: the edges at each of `ratios` (0: none) and / or the loudness, each
// launched only when the host does not hold it, behind ONE synchronisation.
void Engine::measure_last_run(const std::vector<float>& ratios, bool loud, bool keep, bool true_peak) {
    const bool e = enqueue_edges(ratios, keep);
    const bool l = loud && enqueue_loudness();
    const bool t = true_peak && enqueue_true_peak();
    if (!e && !l && !t) return;
    HIP_CHECK(hipStreamSynchronize(stream_));
    if (e)
        for (EdgeSet& s : h_edges_) s.ready = true;
    if (l) have_loud_ = true;
    if (t) have_tp_ = true;
}

// ---------------------------------------------------------------- BS.1770 loudness of a run's rows (mi355vits_set_loudness_target / _fetch_loudness)
void Engine::set_loudness_target(float target_lufs, float ceiling_dbfs) {
    if (!(target_lufs == 0.0f || (target_lufs >= -70.0f && target_lufs < 0.0f)))  // NaN fails all
        throw EngineError(MI355VITS_ERR_INVALID, "set_loudness_target: target " + std::to_string(target_lufs) + " LUFS is neither 0 (off) nor in [-70, 0)");
    if (target_lufs != 0.0f && !(std::isfinite(ceiling_dbfs) && ceiling_dbfs <= 0.0f))
        throw EngineError(MI355VITS_ERR_INVALID, "set_loudness_target: ceiling " + std::to_string(ceiling_dbfs) + " dBFS is not a finite value <= 0");
    pack_.loud_target = target_lufs;
    if (target_lufs != 0.0f) pack_.loud_ceiling = ceiling_dbfs;
}

// The gain rule, in double: g = 10^((T - lufs) / 20) (1 for a row without a gated block), bounded by 10^(c / 20) / peak.
void Engine::loudness_gain(double lufs, double peak, float target, float ceiling, int window, double* gain, bool* limited) {
    const double g = std::isinf(lufs) ? 1.0 : std::pow(10.0, ((double)target - lufs) / 20.0);
    const double p = peak;  // (the sample peak converted exactly, or the oversampled peak: never NaN)
    *gain = g;
    *limited = false;
    if (p != 0.0) {
        const double cap = std::pow(10.0, (double)ceiling / 20.0) / p;
        if (cap < g) {
            if (window <= 0) *gain = cap;  // (the limiter on: the row keeps g and k_limit holds its peaks under the ceiling)
            *limited = true;
        }
    }
}

// k_loud / k_loud_gate over the last run's rows in an arena of their own, and the copy of 16 B bytes + the peaks; nothing when the
// host still holds them.
bool Engine::enqueue_loudness() {
    if (have_loud_) return false;
    const int B = B_;
    LoudnessPlan lp;
    if (!loudness_plan(run_hz_, lp))
        throw EngineError(MI355VITS_ERR_INVALID, "loudness: K-weighting is not offered below " + std::to_string(LOUD_MIN_HZ) + " Hz (the run's rate is " + std::to_string(run_hz_) + " Hz)");
    long l_max = 0;
    double audio = 0, steps = 0;
    for (int b = 0; b < B; ++b) {
        l_max = std::max<long>(l_max, h_olen_[b]);
        audio += (double)h_olen_[b];
        steps += (double)loudness_steps(h_olen_[b], lp.S);
    }
    const size_t ldE = (size_t)std::max<long>(1, loudness_steps(l_max, lp.S));
    arena_ld_.reserve(16 * (size_t)B + 8 * (size_t)B * ldE + 4096, stream_);
    arena_ld_.reset();
    double* d = arena_ld_.alloc<double>(2 * (size_t)B);
    double* dE = arena_ld_.alloc<double>((size_t)B * ldE);
    int* d_blocks = reinterpret_cast<int*>(d + B);
    {
        ProfScope ps(prof_, "loudness", 0, 4.0 * audio + 8.0 * steps + 16.0 * (double)B);
        launch_loudness(run_hz_, o_audio_, Lo_, o_alen_, B, l_max, dE, (long)ldE, d, d_blocks, d_blocks + B, stream_);
    }
    h_loud_.resize(2 * (size_t)B);
    h_loud_peaks_.resize((size_t)B);
    HIP_CHECK(hipMemcpyAsync(h_loud_.data(), d, 16 * (size_t)B, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(h_loud_peaks_.data(), o_peaks_, 4 * (size_t)B, hipMemcpyDeviceToHost, stream_));
    return true;  // have_loud_ once the caller has synchronised
}

void Engine::fetch_loudness(mi355vits_loudness* out) {
    begin_fetch(out, "fetch_loudness");
    const float target = pack_.loud_target, ceiling = pack_.loud_ceiling;
    const int window = pack_.limit_window;
    const PackSettings set = pack_;
    measure_last_run({}, true, false, set.true_peak());
    const size_t B = (size_t)B_;
    out->batch = B_;
    out->sample_rate = run_hz_;
    out->target_lufs = target;
    out->ceiling_dbfs = ceiling;
    out->lufs = static_cast<double*>(new_owner(out)->take_pinned(28 * B + 16));  // lufs, gain: doubles; blocks, gated, limited: int32
    out->gain = out->lufs + B;
    out->blocks = reinterpret_cast<int32_t*>(out->gain + B);
    out->gated = out->blocks + B;
    out->limited = out->gated + B;
    memcpy(out->lufs, h_loud_.data(), 8 * B);
    memcpy(out->blocks, h_loud_.data() + B, 8 * B);  // blocks, then gated
    for (size_t b = 0; b < B; ++b) {
        double g = 0.0;
        bool lim = false;
        if (target != 0.0f) loudness_gain(out->lufs[b], ceiling_peak((int)b, set), target, ceiling, window, &g, &lim);
        out->gain[b] = g;
        out->limited[b] = lim ? 1 : 0;
    }
}

// ---------------------------------------------------------------- the look-ahead peak limiter (mi355vits_set_loudness_limiter / _fetch_limiter)
void Engine::set_loudness_limiter(int window_samples) {
    if (window_samples != 0 && (window_samples < 1 || window_samples > LIMIT_MAX_WINDOW))
        throw EngineError(MI355VITS_ERR_INVALID, "set_loudness_limiter: window of " + std::to_string(window_samples) +
                                                     " samples is neither 0 (off) nor in [1, " + std::to_string(LIMIT_MAX_WINDOW) + "]");
    pack_.limit_window = window_samples;
}

int Engine::limit_job(std::vector<LimitJob>& jobs, int row, const PackSettings& set, double g, LimitKeys* keys) const {
    const std::pair<int, int> key(set.limit_window, set.true_peak() ? 1 : 0);
    const double c = std::pow(10.0, (double)set.loud_ceiling / 20.0);
    const double U = set.enc == PACK_ENC_F32 ? 1.0 : 32767.0;
    // (a linear scan: quadratic in the over entries of a streams call, which a micro-batch keeps to tens; a single pack never repeats a row)
    for (size_t j = 0; j < jobs.size(); ++j)
        if (jobs[j].row == row && jobs[j].g == g && jobs[j].c == c && jobs[j].U == U && (!keys || (*keys)[j] == key)) return (int)j;  // (g is a function of the row and the target)
    LimitJob job;
    job.g = g;
    job.c = c;
    job.U = U;
    job.row = row;
    job.n = (int)h_olen_[row];  // the curve is made on the whole row, as the loudness is measured on it
    job.off = job.tile0 = 0;
    jobs.push_back(job);
    if (keys) keys->push_back(key);
    return (int)jobs.size() - 1;
}

void Engine::limit_pack(PackPlan& plan, std::vector<LimitJob>& jobs, LimitKeys* keys) const {
    const PackSettings& set = plan.set;
    std::vector<int> curve(plan.n, -1);
    bool any = false;
    for (int i = 0; i < plan.n; ++i) {
        const int row = plan.order[i];
        double g;
        bool over;
        loudness_gain(h_loud_[row], ceiling_peak(row, set), set.loud_target, set.loud_ceiling, set.limit_window, &g, &over);
        if (!over || h_olen_[row] < 1) continue;
        curve[i] = limit_job(jobs, row, set, g, keys);
        any = true;
    }
    if (any) plan.curve.swap(curve);
}

void Engine::curve_offsets(PackPlan& plan, const std::vector<LimitJob>& jobs) {
    for (int& c : plan.curve)
        if (c >= 0) c = jobs[(size_t)c].off;
}

// Placed jobs (off / tile0 set; a group's tile0 counts from 0: it is a launch of its own) in ONE layout of jobs, statistics, curves
// and envelopes in `arena`, one upload, and per group k_true_peak_env (true-peak groups) and k_limit over its part of the table.
LimitStat* Engine::launch_limit_groups(const std::vector<LimitJob>& placed, const std::vector<LimitGroup>& groups, long floats, DeviceArena& arena,
                                       bool with_curve) {
    const size_t nj = placed.size();
    bool any_tp = false;
    for (const LimitGroup& g : groups) any_tp = any_tp || g.tp;
    // (reserve waits for the stream when the arena has to grow: "no synchronisation added" holds from the second pack of a size on, as for arena_p_)
    arena.reserve(DeviceArena::padded(sizeof(LimitJob) * nj) + DeviceArena::padded(sizeof(LimitStat) * nj) +
                      (with_curve ? DeviceArena::padded(4 * (size_t)floats) : 0) + (any_tp ? DeviceArena::padded(8 * (size_t)floats) : 0) + 4096,
                  stream_);
    arena.reset();
    LimitJob* d_jobs = arena.alloc<LimitJob>(nj);
    LimitStat* d_stats = arena.alloc<LimitStat>(nj);
    float* curve = with_curve ? arena.alloc<float>((size_t)floats) : nullptr;
    double* env = any_tp ? arena.alloc<double>((size_t)floats) : nullptr;  // e[t] of every job, one behind the other as the curves are
    if (with_curve) d_curve_ = curve;
    h_limit_jobs_ = placed;  // a member: it outlives the copy
    HIP_CHECK(hipMemcpyAsync(d_jobs, h_limit_jobs_.data(), sizeof(LimitJob) * nj, hipMemcpyHostToDevice, stream_));
    for (const LimitGroup& g : groups) {
        if (g.tp) {
            ProfScope ps(prof_, "truepeak.env", 0, 12.0 * (double)g.floats);
            launch_true_peak_env(d_jobs + g.first, (int)g.n, g.tiles, o_audio_, Lo_, env, stream_);
        }
        ProfScope ps(prof_, "limit", 0, 8.0 * (double)g.floats + 16.0 * (double)g.n);
        launch_limit(d_jobs + g.first, (int)g.n, g.tiles, g.window, o_audio_, Lo_, d_stats + g.first, curve, stream_, g.tp ? env : nullptr);
    }
    return d_stats;
}

LimitStat* Engine::run_limit_jobs(std::vector<LimitJob>& jobs, int window, DeviceArena& arena, bool with_curve, bool true_peak) {
    long floats = 0;
    const long tiles = limit_place_jobs(jobs.data(), (int)jobs.size(), &floats);
    if (tiles < 0)
        throw EngineError(MI355VITS_ERR_INVALID, "limiter: the curves of the rows over the ceiling together exceed 2^31 - 1 samples");
    return launch_limit_groups(jobs, {LimitGroup{0, jobs.size(), tiles, floats, window, true_peak}}, floats, arena, with_curve);
}

// The jobs of a streams call, whose streams bring their own window and mode.  One key among them (every v1 call): run_limit_jobs as
// ever.  Several: the jobs sorted by key (stable) and placed group by group in one layout — the curves of all groups coexist until the
// pack has run.  A curve depends on (row, g, c, U, window, mode) alone, so each is what a single pack under that setting makes.
void Engine::run_limit_groups(std::vector<LimitJob>& jobs, const LimitKeys& keys) {
    bool one = true;
    for (const auto& k : keys) one = one && k == keys[0];
    if (one) {
        run_limit_jobs(jobs, keys[0].first, arena_lm_, true, keys[0].second != 0);
        return;
    }
    const size_t nj = jobs.size();
    std::vector<size_t> perm(nj);
    for (size_t j = 0; j < nj; ++j) perm[j] = j;
    std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
    std::vector<LimitGroup> groups;
    std::vector<LimitJob> sorted(nj);
    for (size_t k = 0; k < nj; ++k) {
        sorted[k] = jobs[perm[k]];
        if (k == 0 || keys[perm[k]] != keys[perm[k - 1]]) groups.push_back(LimitGroup{k, 0, 0, 0, keys[perm[k]].first, keys[perm[k]].second != 0});
        ++groups.back().n;
    }
    long floats = 0;
    for (LimitGroup& g : groups) {
        g.tiles = limit_place_jobs(sorted.data() + g.first, (int)g.n, &g.floats);
        if (g.tiles < 0 || floats + g.floats > LIMIT_MAX_CURVE)
            throw EngineError(MI355VITS_ERR_INVALID, "limiter: the curves of the rows over the ceiling together exceed 2^31 - 1 samples");
        for (size_t k = 0; k < g.n; ++k) sorted[g.first + k].off += (int)floats;  // the group's curves behind those of the groups in front
        floats += g.floats;
    }
    for (size_t k = 0; k < nj; ++k) jobs[perm[k]].off = sorted[k].off;  // curve_offsets reads the callers' order
    launch_limit_groups(sorted, groups, floats, arena_lm_, true);
}

void Engine::fetch_limiter(mi355vits_limiter* out) {
    begin_fetch(out, "fetch_limiter");
    const PackSettings set = pack_;
    const size_t B = (size_t)B_;
    Owner* own = new_owner(out);
    out->batch = B_;
    out->sample_rate = run_hz_;
    out->window_samples = set.limit_window;
    out->engaged = own->alloc<int32_t>(B);
    out->reduced_samples = own->alloc<int32_t>(B);
    out->min_scale = own->alloc<double>(B);
    for (size_t b = 0; b < B; ++b) {
        out->engaged[b] = out->reduced_samples[b] = 0;
        out->min_scale[b] = 1.0;
    }
    if (!set.limiting()) return;  // nothing is measured or launched
    measure_last_run({}, true, false, set.true_peak());
    std::vector<LimitJob> jobs;
    for (int b = 0; b < B_; ++b) {
        double g;
        bool over;
        loudness_gain(h_loud_[b], ceiling_peak(b, set), set.loud_target, set.loud_ceiling, set.limit_window, &g, &over);
        if (over && h_olen_[b] >= 1) (void)limit_job(jobs, b, set, g);
    }
    if (jobs.empty()) return;
    const LimitStat* d_stats = run_limit_jobs(jobs, set.limit_window, arena_lf_, false, set.true_peak());
    std::vector<LimitStat> st(jobs.size());
    HIP_CHECK(hipMemcpyAsync(st.data(), d_stats, sizeof(LimitStat) * st.size(), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    const double den = (double)(set.limit_window + 1) * 1073741824.0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        const int b = jobs[j].row;
        out->engaged[b] = 1;
        out->reduced_samples[b] = st[j].reduced;
        out->min_scale[b] = (double)st[j].sq_min / den;
    }
}

// ---------------------------------------------------------------- the 4x oversampled peak (mi355vits_set_loudness_ceiling_mode / _fetch_true_peak)
void Engine::set_loudness_ceiling_mode(int mode) {
    if (mode != MI355VITS_CEILING_SAMPLE && mode != MI355VITS_CEILING_TRUE_PEAK)
        throw EngineError(MI355VITS_ERR_INVALID, "set_loudness_ceiling_mode: mode " + std::to_string(mode) + " unknown (0 = sample peak, 1 = true peak)");
    pack_.ceil_mode = mode;
}

// k_true_peak over the last run's rows in an arena of its own, and the copy of 8 B bytes + the peaks; nothing when the host still
// holds them.
bool Engine::enqueue_true_peak() {
    if (have_tp_) return false;
    const int B = B_;
    long l_max = 0;
    double audio = 0;
    for (int b = 0; b < B; ++b) {
        l_max = std::max<long>(l_max, h_olen_[b]);
        audio += (double)h_olen_[b];
    }
    arena_tp_.reserve(8 * (size_t)B + 4096, stream_);
    arena_tp_.reset();
    double* d = arena_tp_.alloc<double>((size_t)B);
    {
        ProfScope ps(prof_, "truepeak", 0, 4.0 * audio + 8.0 * (double)B);
        launch_true_peak(o_audio_, Lo_, o_alen_, B, l_max, d, stream_);
    }
    h_tp_.resize((size_t)B);
    h_tp_peaks_.resize((size_t)B);
    HIP_CHECK(hipMemcpyAsync(h_tp_.data(), d, 8 * (size_t)B, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(h_tp_peaks_.data(), o_peaks_, 4 * (size_t)B, hipMemcpyDeviceToHost, stream_));
    return true;  // have_tp_ once the caller has synchronised
}

void Engine::fetch_true_peak(mi355vits_true_peak* out) {
    begin_fetch(out, "fetch_true_peak");
    measure_last_run({}, false, false, true);
    const size_t B = (size_t)B_;
    out->batch = B_;
    out->sample_rate = run_hz_;
    out->true_peak = static_cast<double*>(new_owner(out)->take_pinned(12 * B + 16));  // true_peak: doubles; peak: floats
    out->peak = reinterpret_cast<float*>(out->true_peak + B);
    memcpy(out->true_peak, h_tp_.data(), 8 * B);
    memcpy(out->peak, h_tp_peaks_.data(), 4 * B);
}

void Engine::fetch_edges(mi355vits_edges* out) {
    begin_fetch(out, "fetch_edges");
    const float ratio = pack_.trim_ratio;
    const int keep = pack_.trim_keep;
    if (ratio != 0.0f) find_edges(ratio);
    out->batch = B_;
    out->sample_rate = run_hz_;
    out->ratio = ratio;
    out->keep_samples = keep;
    out->first = new_owner(out)->alloc<int32_t>(2 * (size_t)B_);
    out->end = out->first + B_;
    const std::vector<int>* ed = ratio != 0.0f ? &edges_at(ratio) : nullptr;
    for (int b = 0; b < B_; ++b) {
        const int64_t n = h_olen_[b];
        int64_t first = 0, end = n;
        if (ed) trimmed_span(n, (*ed)[b], (*ed)[B_ + b], keep, &first, &end);
        out->first[b] = (int32_t)first;
        out->end[b] = (int32_t)end;
    }
}

}  // namespace m355
