// c_api.cpp — extern "C" surface of libmi355vits.so (include/mi355vits.h).  Exceptions stop here:
// every entry point returns a status code and records a message, never aborts the process.
#include "c_api_internal.h"

namespace {
int create_common(WeightsFile& wf, int device, mi355vits_handle* out) {
    std::unique_ptr<mi355vits_engine> h(new mi355vits_engine());
    h->eng.reset(new Engine(wf, device));  // may throw: `h` is released by the unique_ptr
    *out = h.release();
    return MI355VITS_OK;
}

// mi355vits_free_*: what the struct's owner holds goes back, the struct is zeroed (idempotent; a struct without an owner is left alone)
template <typename R> void free_struct(R* r) {
    if (!r || !r->owner_) return;
    release_result_owner(r->owner_);
    memset(r, 0, sizeof(*r));
}

// A call that fills a result struct: the struct zeroed before anything can fail (its free must never see garbage), the handle
// locked, exceptions fenced, and after a failure whatever was filled freed again — never partial audio.
template <typename R, typename F> int result_call(mi355vits_handle h, R* out, F&& fn) {
    if (out) memset(out, 0, sizeof(*out));
    if (!h) return MI355VITS_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->eng->mu);
    const int rc = guarded(h, fn);
    if (rc != MI355VITS_OK && out) free_struct(out);
    return rc;
}

// A call on a handle that fills no result struct: the handle checked and locked; fn's int is what the call returns ...
template <typename F> int locked(mi355vits_handle h, F&& fn) {
    if (!h) return MI355VITS_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->eng->mu);
    return fn();
}
// ... and with exceptions fenced: fn returns nothing, the call a status
template <typename F> int locked_guarded(mi355vits_handle h, F&& fn) {
    return locked(h, [&] { return guarded(h, fn); });
}

// The run* entry points: a result_call whose `args` must be there; fn receives them with rows, timing, speakers, levels and pitch as
// the engine's RunCall.
template <typename R, typename F>
int run_call(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows, const mi355vits_timing_args* timing,
             const mi355vits_speaker_args* speakers, const mi355vits_level_args* levels, const mi355vits_pitch_args* pitch, R* out,
             F&& fn) {
    return result_call(h, out, [&] {
        if (!args) throw EngineError(MI355VITS_ERR_INVALID, "args must not be null");
        fn(RunCall{*args, rows, timing, speakers, levels, pitch});
    });
}
}  // namespace

extern "C" {

const char* mi355vits_version(void) {
#ifdef MI355_EMU
    return "mi355vits 0.1.0 (hipemu CPU test build)";
#else
    return "mi355vits 0.1.0 (gfx950)";
#endif
}

int mi355vits_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 0) return 0;
    return n;
}

int mi355vits_create(const char* weights_path, int device, mi355vits_handle* out) {
    if (out) *out = nullptr;
    return guarded(nullptr, [&] {
        if (!weights_path || !out) throw EngineError(MI355VITS_ERR_INVALID, "weights_path and out must not be null");
        WeightsFile wf;
        wf.load(weights_path);
        create_common(wf, device, out);
    });
}

int mi355vits_create_from_buffer(const void* blob, size_t blob_bytes, int device, mi355vits_handle* out) {
    if (out) *out = nullptr;
    return guarded(nullptr, [&] {
        if (!blob || !out) throw EngineError(MI355VITS_ERR_INVALID, "blob and out must not be null");
        WeightsFile wf;
        // copy into 64-byte aligned storage so tensor data is float-aligned whatever the caller passed
        wf.storage.resize(blob_bytes + 64);
        unsigned char* base = wf.storage.data();
        base += (64 - reinterpret_cast<uintptr_t>(base) % 64) % 64;
        memcpy(base, blob, blob_bytes);
        wf.parse(base, blob_bytes);
        create_common(wf, device, out);
    });
}

int mi355vits_clone(mi355vits_handle src, mi355vits_handle* out) {
    if (out) *out = nullptr;
    if (!src) return MI355VITS_ERR_INVALID;
    std::lock_guard<std::mutex> lk(src->eng->mu);  // the clone reads the source's math mode / flags: not while a run or set_math is under way
    return guarded(src, [&] {
        if (!out) throw EngineError(MI355VITS_ERR_INVALID, "out must not be null");
        std::unique_ptr<mi355vits_engine> h(new mi355vits_engine());
        h->eng.reset(new Engine(*src->eng));
        *out = h.release();
    });
}

int mi355vits_device_result(mi355vits_handle h, const int16_t** pcm, const float** audio, int64_t* row_stride,
                            int32_t* batch, const int32_t** device_lengths) {
    return locked_guarded(h, [&] {
        long rs = 0;
        int b = 0;
        h->eng->device_buffers(pcm, audio, &rs, &b, device_lengths);
        if (row_stride) *row_stride = rs;
        if (batch) *batch = b;
    });
}

void mi355vits_destroy(mi355vits_handle h) {
    if (!h) return;
    try {
        std::lock_guard<std::mutex> lk(h->eng->mu);
    } catch (...) {
    }
    delete h;
}

int mi355vits_set_math(mi355vits_handle h, int mode) {
    return locked_guarded(h, [&] { h->eng->set_math(mode); });
}
int mi355vits_get_math(mi355vits_handle h) {
    return locked(h, [&] { return h->eng->math(); });
}

int mi355vits_set_output_rate(mi355vits_handle h, int32_t hz) {
    return locked_guarded(h, [&] { h->eng->set_output_rate(hz); });
}
int32_t mi355vits_get_output_rate(mi355vits_handle h) {
    return locked(h, [&] { return h->eng->output_rate(); });
}

int mi355vits_set_output_encoding(mi355vits_handle h, int enc) {
    return locked_guarded(h, [&] { h->eng->set_output_encoding(enc); });
}
int mi355vits_get_output_encoding(mi355vits_handle h) {
    return locked(h, [&] { return h->eng->output_encoding(); });
}

int mi355vits_set_output_compression(mi355vits_handle h, int mode) {
    return locked_guarded(h, [&] { h->eng->set_output_compression(mode); });
}
int mi355vits_get_output_compression(mi355vits_handle h) {
    return locked(h, [&] { return h->eng->output_compression(); });
}

int mi355vits_get_config(mi355vits_handle h, mi355vits_config* out) {
    if (!h) return MI355VITS_ERR_INVALID;
    return guarded(h, [&] {
        if (!out) throw EngineError(MI355VITS_ERR_INVALID, "out must not be null");
        *out = h->eng->config();
    });
}

int mi355vits_run(mi355vits_handle h, const mi355vits_run_args* args, mi355vits_result* out) {
    return mi355vits_run_pitch(h, args, nullptr, nullptr, nullptr, nullptr, nullptr, out);
}

int mi355vits_run_rows(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows,
                       mi355vits_result* out) {
    return mi355vits_run_pitch(h, args, rows, nullptr, nullptr, nullptr, nullptr, out);
}

int mi355vits_run_timed(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows,
                        const mi355vits_timing_args* timing, mi355vits_result* out) {
    return mi355vits_run_pitch(h, args, rows, timing, nullptr, nullptr, nullptr, out);
}

int mi355vits_run_speakers(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows,
                           const mi355vits_timing_args* timing, const mi355vits_speaker_args* speakers, mi355vits_result* out) {
    return mi355vits_run_pitch(h, args, rows, timing, speakers, nullptr, nullptr, out);
}

int mi355vits_run_levels(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows,
                         const mi355vits_timing_args* timing, const mi355vits_speaker_args* speakers,
                         const mi355vits_level_args* levels, mi355vits_result* out) {
    return mi355vits_run_pitch(h, args, rows, timing, speakers, levels, nullptr, out);
}

int mi355vits_run_pitch(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows,
                        const mi355vits_timing_args* timing, const mi355vits_speaker_args* speakers,
                        const mi355vits_level_args* levels, const mi355vits_pitch_args* pitch, mi355vits_result* out) {
    return run_call(h, args, rows, timing, speakers, levels, pitch, out, [&](const RunCall& call) { h->eng->run(call, out); });
}

int mi355vits_get_speaker_embedding(mi355vits_handle h, int64_t sid, float* out, size_t capacity) {
    return locked_guarded(h, [&] { h->eng->speaker_embedding(sid, out, capacity); });
}

int mi355vits_fetch(mi355vits_handle h, uint32_t want_flags, mi355vits_result* out) {
    return result_call(h, out, [&] { h->eng->fetch(want_flags, out); });
}

void mi355vits_free_result(mi355vits_result* r) { free_struct(r); }

int mi355vits_run_packed(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows,
                         const mi355vits_pack_args* pack, mi355vits_packed_result* out) {
    return run_call(h, args, rows, nullptr, nullptr, nullptr, nullptr, out, [&](const RunCall& call) { h->eng->run_packed(call, pack, out); });
}

int mi355vits_fetch_packed(mi355vits_handle h, const mi355vits_pack_args* pack, mi355vits_packed_result* out) {
    return result_call(h, out, [&] { h->eng->fetch_packed(pack, out); });
}

void mi355vits_free_packed(mi355vits_packed_result* r) { free_struct(r); }

int mi355vits_run_streams(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows,
                          const mi355vits_stream_args* streams, int32_t n_streams, mi355vits_streams_result* out) {
    return run_call(h, args, rows, nullptr, nullptr, nullptr, nullptr, out, [&](const RunCall& call) { h->eng->run_streams(call, streams, n_streams, out); });
}

int mi355vits_fetch_streams(mi355vits_handle h, const mi355vits_stream_args* streams, int32_t n_streams, mi355vits_streams_result* out) {
    return result_call(h, out, [&] { h->eng->fetch_streams(streams, n_streams, out); });
}

void mi355vits_free_streams(mi355vits_streams_result* r) { free_struct(r); }

int mi355vits_run_streams2(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows,
                           const mi355vits_stream_args2* streams, int32_t n_streams, mi355vits_streams_result2* out) {
    return run_call(h, args, rows, nullptr, nullptr, nullptr, nullptr, out, [&](const RunCall& call) { h->eng->run_streams2(call, streams, n_streams, out); });
}

int mi355vits_fetch_streams2(mi355vits_handle h, const mi355vits_stream_args2* streams, int32_t n_streams, mi355vits_streams_result2* out) {
    return result_call(h, out, [&] { h->eng->fetch_streams2(streams, n_streams, out); });
}

void mi355vits_free_streams2(mi355vits_streams_result2* r) { free_struct(r); }

int mi355vits_fetch_alignment(mi355vits_handle h, uint32_t want, mi355vits_alignment* out) {
    return result_call(h, out, [&] { h->eng->fetch_alignment(want, out); });
}

void mi355vits_free_alignment(mi355vits_alignment* r) { free_struct(r); }

int mi355vits_set_edge_trim(mi355vits_handle h, float ratio, int32_t keep_samples) {
    return locked_guarded(h, [&] { h->eng->set_edge_trim(ratio, keep_samples); });
}

int mi355vits_get_edge_trim(mi355vits_handle h, float* ratio, int32_t* keep_samples) {
    return locked(h, [&] {
        if (ratio) *ratio = h->eng->edge_trim_ratio();
        if (keep_samples) *keep_samples = h->eng->edge_trim_keep();
        return (int)MI355VITS_OK;
    });
}

int mi355vits_fetch_edges(mi355vits_handle h, mi355vits_edges* out) {
    return result_call(h, out, [&] { h->eng->fetch_edges(out); });
}

void mi355vits_free_edges(mi355vits_edges* r) { free_struct(r); }

int mi355vits_set_loudness_target(mi355vits_handle h, float target_lufs, float ceiling_dbfs) {
    return locked_guarded(h, [&] { h->eng->set_loudness_target(target_lufs, ceiling_dbfs); });
}

int mi355vits_get_loudness_target(mi355vits_handle h, float* target_lufs, float* ceiling_dbfs) {
    return locked(h, [&] {
        if (target_lufs) *target_lufs = h->eng->loudness_target();
        if (ceiling_dbfs) *ceiling_dbfs = h->eng->loudness_ceiling();
        return (int)MI355VITS_OK;
    });
}

int mi355vits_fetch_loudness(mi355vits_handle h, mi355vits_loudness* out) {
    return result_call(h, out, [&] { h->eng->fetch_loudness(out); });
}

void mi355vits_free_loudness(mi355vits_loudness* r) { free_struct(r); }

int mi355vits_set_loudness_limiter(mi355vits_handle h, int32_t window_samples) {
    return locked_guarded(h, [&] { h->eng->set_loudness_limiter(window_samples); });
}

int32_t mi355vits_get_loudness_limiter(mi355vits_handle h) {
    return locked(h, [&] { return h->eng->loudness_limiter(); });
}

int mi355vits_fetch_limiter(mi355vits_handle h, mi355vits_limiter* out) {
    return result_call(h, out, [&] { h->eng->fetch_limiter(out); });
}

void mi355vits_free_limiter(mi355vits_limiter* r) { free_struct(r); }

int mi355vits_set_loudness_ceiling_mode(mi355vits_handle h, int mode) {
    return locked_guarded(h, [&] { h->eng->set_loudness_ceiling_mode(mode); });
}

int mi355vits_get_loudness_ceiling_mode(mi355vits_handle h) {
    return locked(h, [&] { return h->eng->loudness_ceiling_mode(); });
}

int mi355vits_fetch_true_peak(mi355vits_handle h, mi355vits_true_peak* out) {
    return result_call(h, out, [&] { h->eng->fetch_true_peak(out); });
}

void mi355vits_free_true_peak(mi355vits_true_peak* r) { free_struct(r); }

const char* mi355vits_last_error(mi355vits_handle h) { return h ? h->err.c_str() : create_error().c_str(); }

int mi355vits_profile_enable(mi355vits_handle h, int on) {
    return locked(h, [&] {
        h->eng->profiler().enabled = on != 0;
        return (int)MI355VITS_OK;
    });
}
int mi355vits_profile_reset(mi355vits_handle h) {
    return locked_guarded(h, [&] { h->eng->profiler().clear(); });
}
long mi355vits_profile_report(mi355vits_handle h, char* buf, size_t cap) {
    if (!h || !buf || cap == 0) return MI355VITS_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->eng->mu);
    long n = 0;
    int rc = guarded(h, [&] {
        const std::string s = h->eng->profiler().report();
        n = (long)std::min(s.size(), cap - 1);
        memcpy(buf, s.data(), (size_t)n);
        buf[n] = 0;
    });
    return rc == MI355VITS_OK ? n : rc;
}

float mi355vits_last_run_ms(mi355vits_handle h) {
    if (!h) return -1.0f;
    std::lock_guard<std::mutex> lk(h->eng->mu);
    return h->eng->last_run_ms();
}

static long tap_call(mi355vits_handle h, const char* name, long row0, long nrows, float* out, size_t capacity, int64_t dims[4]) {
    if (!h || !name || !dims) return MI355VITS_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->eng->mu);
    long n = 0;
    int rc = guarded(h, [&] { n = h->eng->get_tap(name, out, capacity, dims, row0, nrows); });
    return rc == MI355VITS_OK ? n : rc;
}
long mi355vits_get_tap(mi355vits_handle h, const char* name, float* out, size_t capacity, int64_t dims[4]) {
    return tap_call(h, name, 0, -1, out, capacity, dims);  // every row
}
long mi355vits_get_tap_rows(mi355vits_handle h, const char* name, long row0, long nrows, float* out, size_t capacity, int64_t dims[4]) {
    return tap_call(h, name, row0, nrows < 0 ? 0 : nrows, out, capacity, dims);
}
long mi355vits_list_taps(mi355vits_handle h, char* buf, size_t cap) {
    if (!h || !buf || cap == 0) return MI355VITS_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->eng->mu);
    const std::string s = h->eng->list_taps();
    const size_t n = std::min(s.size(), cap - 1);
    memcpy(buf, s.data(), n);
    buf[n] = 0;
    return (long)n;
}

}  // extern "C"
