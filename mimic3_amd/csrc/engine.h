// engine.h — host side of the MI355X VITS engine: weight container, device arenas, per-kernel
// event profiler and the launch sequence of one synthesis call.
#pragma once
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mi355vits.h"
#include "kernels.h"

namespace m355 {

struct EngineError : std::runtime_error {
    int code;
    EngineError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// ---------------------------------------------------------------- .m355 container (mimic3_amd/weights.py)
struct HostTensor {
    std::vector<int> dims;
    const float* data = nullptr;
    size_t count = 0;
};
struct WeightsFile {
    mi355vits_config cfg{};
    std::map<std::string, HostTensor> tensors;
    std::vector<unsigned char> storage;      // owns the bytes when loaded from a file
    void parse(const void* blob, size_t n);  // tensors point into `blob`
    void load(const std::string& path);
    const HostTensor& get(const std::string& name, std::initializer_list<int> dims) const;
};

// ---------------------------------------------------------------- grow-only bump allocator in HBM
class DeviceArena {
  public:
    ~DeviceArena();
    void reserve(size_t bytes, hipStream_t s);  // may reallocate (synchronises the stream first)
    void reset() { off_ = 0; }
    void rewind(size_t off) { off_ = off; }     // back to an earlier used(): what was allocated after it is given up
    void fill(uint32_t pattern, hipStream_t s);  // every byte of the capacity (tests: mi355vits_test_fill_workspace)
    template <typename T> T* alloc(size_t n) { return reinterpret_cast<T*>(alloc_bytes(n * sizeof(T))); }
    size_t capacity() const { return cap_; }
    size_t used() const { return off_; }
    static size_t padded(size_t bytes) { return (bytes + 255) & ~size_t(255); }

  private:
    void* alloc_bytes(size_t bytes);
    unsigned char* base_ = nullptr;
    size_t cap_ = 0, off_ = 0;
};
struct ArenaCount {  // stand-in that only adds up what a sequence of allocs takes
    size_t bytes = 0;
    template <typename T> T* alloc(size_t n) { bytes += DeviceArena::padded(n * sizeof(T)); return nullptr; }
};

// ---------------------------------------------------------------- HIP-event profiler on the engine stream
struct Profiler {
    struct Rec { int name_id; hipEvent_t a, b; double flops, bytes; };
    bool enabled = false;
    std::vector<std::string> names;
    std::unordered_map<std::string, int> ids;
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipStream_t stream = nullptr;
    ~Profiler();
    int begin(const char* name, double flops, double bytes);
    void end(int rec);
    void clear();
    std::string report();  // synchronises
  private:
    hipEvent_t get_event();
};
struct ProfScope {
    Profiler& p;
    int rec;
    ProfScope(Profiler& prof, const char* name, double flops = 0, double bytes = 0) : p(prof), rec(-1) {
        if (p.enabled) rec = p.begin(name, flops, bytes);
    }
    ~ProfScope() {
        if (rec >= 0) p.end(rec);
    }
};

// ---------------------------------------------------------------- RAII guards of the diagnostic and test calls
// (hipMalloc / hipFree synchronise the device: not for the serving path, which lives in the arenas)
struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes) { HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16)); }
    ~DevBuf() { (void)hipFree(p); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    template <typename T> T* as() { return static_cast<T*>(p); }
};
struct Ev {  // a HIP error between create and destroy must not leak the event
    hipEvent_t e = nullptr;
    Ev() { HIP_CHECK(hipEventCreate(&e)); }
    ~Ev() { if (e) (void)hipEventDestroy(e); }
    Ev(const Ev&) = delete;
    Ev& operator=(const Ev&) = delete;
};
// ms per launch between two events on `stream`: `warm` untimed launches, then `reps` timed ones
template <typename F>
double timed(F&& launch, int warm, int reps, hipStream_t stream = nullptr) {
    Ev e0, e1;
    for (int i = 0; i < warm; ++i) launch();
    HIP_CHECK(hipEventRecord(e0.e, stream));
    for (int i = 0; i < reps; ++i) launch();
    HIP_CHECK(hipEventRecord(e1.e, stream));
    HIP_CHECK(hipEventSynchronize(e1.e));
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0.e, e1.e));
    return (double)ms / reps;
}

struct Tap {
    std::string name;
    float* dev;
    std::vector<int64_t> dims;
    size_t count;
};

constexpr size_t NO_OFF = ~size_t(0);

// one dense Conv1d's parameters, as offsets (floats) into the device weight arena
struct ConvW {
    size_t raw = NO_OFF;     // [Cout,Cin,K]
    size_t packed = NO_OFF;  // MFMA fragment order (absent when Cin is odd)
    size_t packed4 = NO_OFF; // same records regrouped [tile][tap][4 pairs][lane][4] for 16-byte A loads (fused MRF stage)
    size_t packed_b3 = NO_OFF;  // three bf16 planes in bf16-MFMA fragment order (pack_conv_weights_bf16x3), 32-bit words
    size_t packed_b3s = NO_OFF; // the same for the staged split-bf16 conv kernel (layout 1, this conv's tile map)
    size_t packed_w16 = NO_OFF; // WaveNet layer convs (Cin = 192): pack_conv_weights_w16, the fused split-bf16 layer kernel on 16x16x32 tiles
    size_t packed_b3w = NO_OFF; // WaveNet in-layer convs: layout 1, 32-row tiles of (16 tanh rows, their 16 sigmoid rows) (lab build / CPU model: MI355VITS_WN_SHAPE=32)
    size_t packed_h2 = NO_OFF;    // fused-MRF convs: two fp16 planes, weights x 2^13 (MATH_F16X2), when every |w| < 7.99
    size_t packed_p = NO_OFF;     // fused-MRF convs (Cin = Cout, taps 3 / 5 / 7): pack_conv_weights_p16 fragments (k_mrf_p)
    size_t packed_h2s = NO_OFF;   // WaveNet layer convs: the same in plane order (layout 1), plain rows (gate convs: packed_b3w's tile order)
    size_t bias = NO_OFF;
    int Cout = 0, Cin = 0, K = 1;
    int epi = EPI_STD;  // tile map the packed copy was built for
};
// what a conv is in the graph, declared by whoever adds it: decides which of the copies above are packed (Engine::add_conv_data)
enum ConvRole { ROLE_PLAIN, ROLE_RESBLOCK, ROLE_UPSAMPLER };
// the kernel one dense conv runs on, in the order Engine::pick_conv tries them
enum ConvKernel { UPS_PL, RB_CONV, ENC_B3, STAGED_B3, STAGED_F16X2, MFMA_F32, GENERIC };

// ---------------------------------------------------------------- lab switches (MI355VITS_* through lab_getenv: tests, A/B runs)
// Read once when a handle is created; a cloned lane takes lane 0's.  The product build's lab_getenv returns null: all defaults.
struct LabSwitches {
    bool force_generic = false;    // FORCE_GENERIC=1: every layer on its generic kernel
    bool no_fused_wn = false;      // NO_FUSED_WN=1: in-layer + res/skip as two launches (A/B + fallback)
    bool no_fused_mrf = false;     // NO_FUSED_MRF=1: conv-by-conv resblocks (A/B + fallback)
    int b3_min_work = 256;         // B3_MIN_WORK: MATH_BF16X3: smallest K * Cin routed to the staged split-bf16 conv kernel
    bool wn_b3 = false;            // WN_B3: MATH_BF16X3: WaveNet layers as two staged split-bf16 convs instead of the fused f32 layer
    bool no_mrf_p = false;         // NO_MRF_P: keep the on-the-fly split MRF kernel (A/B against k_mrf_p)
    bool no_rbc = false;           // NO_RBC: the 128-channel stage on k_mrf_fused + the staged conv (A/B against k_rb_conv)
    bool no_fused_dds = false;     // NO_FUSED_DDS: DDS layers as three launches (A/B + fallback)
    bool no_dds_stack = false;     // NO_DDS_STACK: one launch per DDS layer / pre / proj / spline (A/B + fallback)
    bool no_dds_stack_b3 = false;  // NO_DDS_STACK_B3: the f32-MFMA form of the stack in every math mode (A/B)
    bool no_enc_gemm = false;      // NO_ENC_GEMM: phoneme-sized convs on the general conv kernels (A/B + fallback)
    bool no_enc_o_ln = false;      // NO_ENC_O_LN: o-proj and its LayerNorm as two launches (A/B + fallback)
    bool no_flow_gemm = false;     // NO_FLOW_GEMM: flow.pre / flow.post on the general conv kernels (A/B + fallback)
    bool no_f16x2_convs = false;   // F16X2_NO_CONVS: in MATH_F16X2 keep the staged convs / upsamplers on bf16x3
    static LabSwitches from_env();
};

// ---------------------------------------------------------------- one weight replica on one device
// Uploaded once per (voice, device); every engine handle ("lane") created on that device through mi355vits_clone shares
// it, so N lanes cost N workspaces but ONE copy of the weights.
struct Model {
    int device = 0;
    float* dev_weights = nullptr;
    std::unordered_map<std::string, ConvW> convs;
    std::unordered_map<std::string, size_t> vecs;
    float ea_m[2] = {0, 0}, ea_logs[2] = {0, 0};
    std::vector<float> emb_g;  // host copy of emb_g.weight [n_speakers, gin] (empty for a single-speaker voice)
    int dp_filter = 0;  // deterministic duration predictor (dp_n_flows == 0): its filter width F; 0 for the stochastic one
    bool flow_reversed_out = false;
    size_t bytes = 0;
    ~Model();
};

// ---------------------------------------------------------------- the handle's settings of the packed streams
// Written by the setters (which validate), copied whole into a pack's plan when it is made and into a cloned lane.
struct PackSettings {
    int enc = PACK_ENC_S16;      // mi355vits_set_output_encoding: MI355VITS_ENC_* = PackEncoding
    float trim_ratio = 0.0f;     // mi355vits_set_edge_trim: 0 = off
    int trim_keep = 0;
    float loud_target = 0.0f, loud_ceiling = -1.0f;  // mi355vits_set_loudness_target: target 0 = off
    int limit_window = 0;        // mi355vits_set_loudness_limiter: samples at the run's rate, 0 = off; acts on packs with a target only
    int ceil_mode = 0;           // mi355vits_set_loudness_ceiling_mode: MI355VITS_CEILING_*; acts on packs with a target only
    int compress = 0;            // mi355vits_set_output_compression: MI355VITS_COMPRESS_*; single packs (a v1 streams call never reads it; a v2 stream brings its own)
    bool trimmed() const { return trim_ratio != 0.0f; }
    bool normalised() const { return loud_target != 0.0f; }
    bool limiting() const { return normalised() && limit_window > 0; }
    bool true_peak() const { return normalised() && ceil_mode == MI355VITS_CEILING_TRUE_PEAK; }
    bool flac() const { return compress == MI355VITS_COMPRESS_FLAC; }
};

// ---------------------------------------------------------------- one run's inputs
// What a run* entry point was called with, unchecked: the one form every run call of the engine takes.
struct RunCall {
    const mi355vits_run_args& args;
    const mi355vits_row_args* rows = nullptr;          // per-row scales / volume / noise keys (mi355vits_run_rows), or NULL: args' own for every row
    const mi355vits_timing_args* timing = nullptr;     // per-phoneme stretch / minimum frames / a target per row (mi355vits_run_timed), or NULL: the plain run
    const mi355vits_speaker_args* speakers = nullptr;  // a blend of speakers or a vector per row in place of args.sid (mi355vits_run_speakers), or NULL: args.sid
    const mi355vits_level_args* levels = nullptr;      // a gain per phoneme and a ramp per row (mi355vits_run_levels), or NULL: the waveform as it is
    const mi355vits_pitch_args* pitch = nullptr;       // a pitch ratio per phoneme (mi355vits_run_pitch), or NULL: the waveform as it is
};
// What validation leaves of a RunCall: everything the rest of the call reads.  The pointers are the caller's arrays; one that is null
// is an input the run does not have.
struct RunInputs {
    int B = 0, Tx = 0;
    uint64_t seed = 0;
    uint32_t flags = 0;
    const int64_t* ids = nullptr;
    const int64_t* sid = nullptr;           // null when not read: a single-speaker voice, a speakers run
    std::vector<int> len32;                 // [B] the lengths in 32 bits
    // per-row settings: rows->* where given, else args' value for every row (row b keyed utterance_base + b)
    std::vector<float> sc3;                 // [B,3] noise_scale, length_scale, noise_w
    std::vector<double> vol;                // [B] PCM volume (0 or less: 1)
    std::vector<unsigned long long> utt;    // [B] Philox keys
    const int32_t* forced_durations = nullptr;
    const float* noise_w = nullptr;
    const float* noise_z = nullptr;
    int noise_z_frames = 0;
    bool any_noise_z = false;               // some row samples the prior noise (the only case that reads injected noise_z)
    // timing: the caller's struct (all null without one); each of stretch, min_frames and target_frames is there or not, and without
    // any of them the run is the plain one, launch for launch
    mi355vits_timing_args timing{};
    bool timed() const { return timing.stretch || timing.min_frames || timing.target_frames; }
    // speakers: args.sid (NONE), spk.n_terms terms per row of spk.mix_sid / mix_weight (MIX), or spk.vectors, one per row (VECTORS)
    enum Speakers { SPK_NONE, SPK_MIX, SPK_VECTORS };
    Speakers speakers = SPK_NONE;
    mi355vits_speaker_args spk{};  // the caller's struct (all null without one)
    // levels: the caller's struct (all null without one); without a gain the run is the plain one, launch for launch
    mi355vits_level_args lvl{};
    bool levelled() const { return lvl.gain != nullptr; }
    // pitch: the caller's struct (null without one); without a ratio the run is the levels run, launch for launch.  Without
    // forced_durations such a run is a timed run whose stretch is pitch_stretch = fl(stretch * ratio): timing.stretch points into it
    mi355vits_pitch_args pit{};
    std::vector<float> pitch_stretch;
    bool pitched() const { return pit.ratio != nullptr; }
    // the frames of injected noise_z the frame side holds: none unless some row reads it
    size_t noise_z_held() const { return (noise_z && any_noise_z) ? (size_t)noise_z_frames : 0; }
};
// A call's checks, in the order a caller sees their errors; pure host code: no engine state, no HIP call.  Throws EngineError.
// (What only the frame counts can tell — a timing status, too few noise_z frames — is checked where they are read.)
RunInputs check_inputs(const mi355vits_config& c, const RunCall& call);

// ---------------------------------------------------------------- the engine
class Engine {
  public:
    Engine(const WeightsFile& wf, int device);
    explicit Engine(const Engine& lane0);  // another lane on lane0's device, sharing its weight replica
    ~Engine();
    // diagnostics (mi355vits_probe_weights): how fast every CU together streams 2.6 MB windows of THIS replica's weight arena out of
    // the L2 — eight loads in flight per lane (bandwidth) and one (latency per fragment); min / median / max over the windows
    void probe_weights(double out[8]);
    // test hook (mi355vits_test_fill_workspace): both workspace arenas filled with a 32-bit pattern, synchronised
    void fill_workspace(uint32_t pattern);
    const std::shared_ptr<Model>& model() const { return model_; }
    // device pointers of the last run's results (valid until the next run on this handle); for device-side gathers
    void device_buffers(const int16_t** pcm, const float** audio, long* row_stride, int* batch, const int** dev_lengths);
    void run(const RunCall& call, mi355vits_result* out);
    // row `sid` of emb_g from the host copy kept with the weight replica (mi355vits_get_speaker_embedding): no stream work
    void speaker_embedding(int64_t sid, float* out, size_t capacity) const;
    void fetch(uint32_t want, mi355vits_result* out);
    // the packed stream (mi355vits_run_packed / mi355vits_fetch_packed): pack == NULL = every row, in order, no silence, no header
    void run_packed(const RunCall& call, const mi355vits_pack_args* pack, mi355vits_packed_result* out);
    void fetch_packed(const mi355vits_pack_args* pack, mi355vits_packed_result* out);
    // several streams out of one run (mi355vits_run_streams / mi355vits_fetch_streams): each with its own pack, encoding, trim and
    // loudness target; the handle's own settings are neither read nor changed
    void run_streams(const RunCall& call, const mi355vits_stream_args* streams, int n_streams, mi355vits_streams_result* out);
    void fetch_streams(const mi355vits_stream_args* streams, int n_streams, mi355vits_streams_result* out);
    // the same with compression, limiter window and ceiling mode per stream (mi355vits_run_streams2 / mi355vits_fetch_streams2): NONE
    // of the handle's pack settings is read
    void run_streams2(const RunCall& call, const mi355vits_stream_args2* streams, int n_streams, mi355vits_streams_result2* out);
    void fetch_streams2(const mi355vits_stream_args2* streams, int n_streams, mi355vits_streams_result2* out);
    // phoneme timing (and, with MI355VITS_ALIGN_LEVELS, levels) of the last completed run (mi355vits_fetch_alignment)
    void fetch_alignment(uint32_t want, mi355vits_alignment* out);
    // edge trimming of the packed streams (mi355vits_set_edge_trim): ratio 0 = off.  Read when a pack is made and at fetch_edges.
    void set_edge_trim(float ratio, int keep_samples);
    float edge_trim_ratio() const { return pack_.trim_ratio; }
    int edge_trim_keep() const { return pack_.trim_keep; }
    // first / end of every row of the last completed run under the current setting (mi355vits_fetch_edges)
    void fetch_edges(mi355vits_edges* out);
    // loudness target of the packed streams (mi355vits_set_loudness_target): target 0 = off.  Read when a pack is made and at
    // fetch_loudness.
    void set_loudness_target(float target_lufs, float ceiling_dbfs);
    float loudness_target() const { return pack_.loud_target; }
    float loudness_ceiling() const { return pack_.loud_ceiling; }
    // BS.1770 integrated loudness of every row of the last completed run, and the gains of the current setting (mi355vits_fetch_loudness)
    void fetch_loudness(mi355vits_loudness* out);
    // look-ahead peak limiter of the packed streams with a target (mi355vits_set_loudness_limiter): window 0 = off.  Read when a pack
    // is made (a streams call reads it too: its one handle setting), at fetch_loudness and at fetch_limiter.
    void set_loudness_limiter(int window_samples);
    int loudness_limiter() const { return pack_.limit_window; }
    // which rows of the last completed run the limiter engages on under the current target, ceiling and window, and how far
    void fetch_limiter(mi355vits_limiter* out);
    // what the ceiling of the loudness target bounds (mi355vits_set_loudness_ceiling_mode): the row's sample peak or its 4x
    // oversampled peak.  Read where the limiter window is read.
    void set_loudness_ceiling_mode(int mode);
    int loudness_ceiling_mode() const { return pack_.ceil_mode; }
    // the 4x oversampled peak of every row of the last completed run, whatever the mode (mi355vits_fetch_true_peak)
    void fetch_true_peak(mi355vits_true_peak* out);
    const mi355vits_config& config() const { return cfg_; }
    void set_math(int mode);
    int math() const { return math_; }
    // the rate of every result (mi355vits_set_output_rate): 0 or the voice's own = native.  Read when a run starts.
    void set_output_rate(int hz);
    int output_rate() const { return out_hz_ ? out_hz_ : cfg_.sample_rate; }
    // the sample encoding of the packed streams (mi355vits_set_output_encoding).  Read when a pack is made.
    void set_output_encoding(int enc);
    int output_encoding() const { return pack_.enc; }
    // the compression of the packed stream (mi355vits_set_output_compression): FLAC frames of the S16LE stream.  Read when a pack is made.
    void set_output_compression(int mode);
    int output_compression() const { return pack_.compress; }
    Profiler& profiler() { return prof_; }
    float last_run_ms();
    long get_tap(const std::string& name, float* out, size_t cap, int64_t dims[4], long row0 = 0, long nrows = -1);
    std::string list_taps() const;
    std::string last_error;
    std::mutex mu;

  private:
    void construct(const WeightsFile& wf, int device);
    void open_device(int device);
    void release() noexcept;
    // weight staging
    size_t stage(const float* p, size_t n);
    const ConvW& add_conv(const WeightsFile& wf, const std::string& key, const std::string& tensor, int Cout, int Cin,
                          int K, bool bias, int epi = EPI_STD, ConvRole role = ROLE_PLAIN);
    const ConvW& add_conv_data(const std::string& key, const std::vector<float>& w, const std::vector<float>* bias,
                               int Cout, int Cin, int K, int epi = EPI_STD, ConvRole role = ROLE_PLAIN);
    void add_vec(const WeightsFile& wf, const std::string& name, std::initializer_list<int> dims);
    const float* vec(const std::string& name) const;
    const float* P(size_t off) const { return off == NO_OFF ? nullptr : model_->dev_weights + off; }
    const ConvW& cw(const std::string& key) const;

    // launch helpers
    void conv(const char* label, const ConvW& w, ConvArgs a);
    void fill_conv(const ConvW& w, ConvArgs& a) const;             // the shape fields of `a` from w (Cin, Cout, K, bias, default pad, fixed_rule)
    ConvKernel pick_conv(const ConvW& w, const ConvArgs& a) const;  // the kernel conv() runs the filled-in `a` on (callers may ask ahead)
    // row_len / factor: frame-resolution taps of a ragged batch are zeroed past len[b] * factor (those columns are not computed)
    void tap(const char* name, const float* dev, std::initializer_list<int64_t> dims, const int* row_len = nullptr, int factor = 1);
    void tap_ints(const char* name, const int* dev, std::initializer_list<int64_t> dims);  // an int32 array as floats (synchronises)
    Tap* new_tap(const char* name, std::initializer_list<int64_t> dims);  // what both start with; null: taps off, or the name taken
    void text_encoder(int B, int Tx);
    void duration_predictor(const RunInputs& in);
    void duration_predictor_det(const RunInputs& in);
    void dds(const std::string& key, float* X, float* Y1, float* Y2, int B, int T);
    void flow_and_decoder(const RunInputs& in);
    void coupling_layer(int j, int B, int Ty);
    void decoder_stage(int i, int B, int ch, long T);  // upsampler i on bufC [B,ch,T] -> bufA, its resblocks -> bufC
    int mrf_stage(int i, int B, int ch, long T);       // the stage's leading resblocks in one launch; how many it took
    ConvArgs rb2_conv_args(int i, int j, int m, int B, int ch, long T) const;
    // the workspace layouts: run against ArenaCount for the size, then against the arena (engine.cpp)
    // in: the run whose inputs head the layout (the input block, copied into h_in_ as it is laid out); widest: every optional input
    // there, at its largest, and nothing copied (sizing)
    template <typename A> void layout_a(A& ar, const RunInputs& in, bool widest);
    // Lr: the row stride of the resampled audio, 0 in a native run (which lays out nothing for it)
    template <typename A> void layout_b(A& ar, size_t B, size_t Ty, size_t noise_z_frames, size_t Lr, size_t Lw);
    // what a packed call puts where (mi355vits_pack_args, validated; then the offsets made from the frame counts)
    struct PackPlan {
        int n = 0;
        bool wav = false;
        std::vector<int> order;
        std::vector<int64_t> lead;
        int64_t tail = 0;
        PackSettings set;  // the handle's settings when the pack was planned
        // made by place_pack from the frame counts (trimmed: and the edges; normalised: and the loudness)
        std::vector<int64_t> offsets, lengths;
        int64_t total = 0, audio = 0;
        std::vector<int> skip;     // trimmed only: the first sample of its row each entry starts at
        std::vector<double> gain;  // normalised only: each entry's linear gain
        // limiting only, and only when the limiter engages on some entry (else empty): per entry -1, or first its job and, once
        // the jobs are placed, its offset into the curves
        std::vector<int> curve;
        bool curved() const { return !curve.empty(); }
        int seg_rows() const { return pack_seg_rows(set.trimmed(), set.normalised(), curved()); }
        int bps() const { return pack_bytes_per_sample(set.enc); }
        size_t header_bytes() const { return !wav ? 0 : set.enc == PACK_ENC_S16 ? 44 : 58; }  // PCM form / non-PCM form (fmt 18 + fact)
    };
    // What a packed-form call puts where: one PackPlan per stream (with that stream's settings), then the streams' places in the block.
    // single: a packed call (run_packed / fetch_packed) — exactly one stream, k_pack's segment table, no block and no header on the
    // device, its FLAC frames by k_flac_gather.  Else the block form of a streams call: k_pack_streams, k_flac_place,
    // k_flac_gather_streams.  The two device forms differ for a measured reason; everything around them is one.
    struct OutputPlan {
        bool single = false;
        std::vector<PackPlan> streams;
        std::vector<int64_t> begin, data;  // block byte offset of each stream's first byte (its header) / first data byte (16-byte aligned)
        int64_t n_bytes = 0, audio = 0;    // what k_pack_streams writes (without a compressed stream: the block); the audio samples in it
        int entries = 0;
        bool curved = false;               // the limiter engages on some entry: the block's table has its curve row
        // Compressed streams.  k_pack_streams' buffer holds the uncompressed streams exactly as v1 lays them
        // out — [0, plain_bytes) —, then from the next multiple of 16 every compressed stream's samples as a headerless S16LE stream
        // (src[s], 16-byte aligned): the streams in `dev` order.  begin / data of a compressed stream are known once its sizes are.
        // (single: its one stream is k_pack's, src 0)
        std::vector<int> dev;              // the streams in the order of their places in the pack kernel's buffer
        std::vector<int64_t> src;          // compressed streams: where their samples sit in that buffer (else -1)
        std::vector<long> frames;          // compressed streams: their FLAC frames (else 0)
        int64_t plain_bytes = 0;           // R: the v1 block of the uncompressed streams
        int64_t flac_base = 0, flac_bound = 0;  // (R + 15) & ~15; the bound of the bytes behind it
        long n_frames = 0;                 // of all compressed streams
        int n_flac = 0;
        bool compressed() const {          // some stream asks for FLAC
            for (const PackPlan& p : streams)
                if (p.set.flac()) return true;
            return false;
        }
        bool measured() const {            // some stream trims or normalises: the places depend on the audio
            for (const PackPlan& p : streams)
                if (p.set.trimmed() || p.set.normalised()) return true;
            return false;
        }
        // the words of the kernel's table: the segment table [seg_rows][n], or the entry rows and a record per stream
        size_t table_words() const {
            return single ? (size_t)streams[0].seg_rows() * streams[0].n : pack_streams_table_words(entries, (int)streams.size(), curved);
        }
    };
    // Packed-form calls only: the plan's table and its stream or block, behind everything layout_b placed — no other pointer moves,
    // so a call that packs nothing runs on the layout it always had.  Behind them, with a compressed stream, what the FLAC launches of
    // the form need.  Run against ArenaCount for the size, then against the arena.
    template <typename A> void layout(A& ar, const OutputPlan& op) {
        d_pack_seg_ = ar.template alloc<int>(op.table_words());
        if (op.single) {
            const PackPlan& plan = op.streams[0];
            d_pack_ = ar.template alloc<uint8_t>(pack_capacity_bytes(plan.set.enc, (long)plan.total));  // in bytes, the last store's overrun included
            if (!op.compressed()) return;
            // the one job (the S16LE stream k_pack wrote), a slot and a size word per frame (+ the total), the frames' offsets, and
            // the frames back to back — what the host copies
            const size_t frames = (size_t)op.n_frames;
            d_flac_jobs_ = ar.template alloc<FlacJob>(1);
            d_flac_slots_ = ar.template alloc<uint8_t>(frames * FLAC_SLOT_BYTES);
            d_flac_sizes_ = ar.template alloc<int>(frames + 1);
            d_flac_offsets_ = ar.template alloc<long long>(frames);
            d_flac_out_ = ar.template alloc<uint8_t>(flac_out_capacity((long)frames, (long)plan.total));
            return;
        }
        d_pack_ = ar.template alloc<uint8_t>(pack_streams_capacity((long)op.n_bytes));
        if (!op.compressed()) return;
        // a job per compressed stream, a slot per frame, the words the host reads (sizes, FLAC_INFO_* per job, the block's end), the
        // scan and the frames' places, the headers, and the compressed region of the block
        d_flac_jobs_ = ar.template alloc<FlacJob>((size_t)op.n_flac);
        d_flac_slots_ = ar.template alloc<uint8_t>((size_t)op.n_frames * FLAC_SLOT_BYTES + 16);
        d_flac_sizes_ = ar.template alloc<int>(flac_info_words(op.n_frames, op.n_flac));
        d_flac_pre_ = ar.template alloc<unsigned>((size_t)op.n_frames + 1);
        d_flac_ftab_ = ar.template alloc<int2>((size_t)op.n_frames + 1);
        d_flac_hdr_ = ar.template alloc<unsigned>((size_t)FLAC_HDR_WORDS * op.n_flac);
        d_flac_items_ = ar.template alloc<int>(flac_gather_items((long)op.flac_bound));
        d_flac_jtab_ = ar.template alloc<int>((size_t)FLAC_JTAB_ROWS * op.n_flac);
        d_flac_out_ = ar.template alloc<uint8_t>((size_t)op.flac_bound + 16);
    }
    // ---- everything behind the waveform: engine_results.cpp
    // what every fetch starts with: a result struct to fill, zeroed; a completed run to serve; its device current
    template <typename R> void begin_fetch(R* out, const char* call, bool call_in_null_text = true);
    void copy_out(uint32_t want, mi355vits_result* out);
    // one synthesis call up to the finished float audio (+ the padded int16 pass when the flags ask for it); with an output plan
    // the packed stream or block instead (its places made from the frame counts, its table uploaded with the per-stage lengths)
    void synthesize(const RunCall& call, OutputPlan* plan);
    // its steps, in order (text_encoder, duration_predictor and flow_and_decoder above among them)
    void begin_run(const RunInputs& in);       // the last run's caches dropped, its taps freed
    void upload_inputs(const RunInputs& in);   // the text side sized and laid out, the inputs in ONE copy
    // the k_speaker_cond launches, or in a speakers run k_speaker_cond_mix in their place
    void conditioning(const RunInputs& in);
    // k_durations, or in a timed run k_durations_timed in its place (the one call of both predictors)
    void durations(const RunInputs& in, int ch, float ea_m, float ea_logs);
    // the run's one sizing synchronisation: the frame counts (a timed run: its statuses, factor_out), Ty_ / L_, h_olen_ at the run's rate
    void read_frame_counts(const RunInputs& in);
    void size_frame_side(const RunInputs& in, const OutputPlan* plan);  // layout_b, and behind it the plan's layout
    // injected noise_z, then per-stage lengths, audio lengths, a resampled run's table (rs_items_) and an early plan's table in ONE copy
    void upload_stage_table(const RunInputs& in, const OutputPlan* plan);
    // a levels run: k_levels shapes d_audio_ in place and takes the row peaks again (kernels_level.cpp); else nothing
    void levels(const RunInputs& in);
    // a pitch run: k_pitch_plan behind the duration kernel (its wlen rides in read_frame_counts' copy), k_pitch from d_audio_ into
    // d_waudio_ behind levels() (kernels_pitch.cpp); else nothing
    void pitch_plan(const RunInputs& in);
    void pitch(const RunInputs& in);
    void resample();
    void output(const RunInputs& in, const OutputPlan* plan);  // the plan's pack kernel, or the padded int16 pass when the flags ask
    void plan_pack(const mi355vits_pack_args* pack, int B, const PackSettings& set, PackPlan& plan) const;  // validates; nothing sized or launched yet
    void plan_single(const mi355vits_pack_args* pack, int B, OutputPlan& op) const;  // a packed call's plan: plan_pack under the handle's settings
    // validates every stream, naming it (v1's streams arrive as v2 ones carrying the handle's window and mode, uncompressed)
    void plan_streams(const mi355vits_stream_args2* streams, int n_streams, int B, OutputPlan& op) const;
    std::vector<mi355vits_stream_args2> streams_v1(const mi355vits_stream_args* streams, int n_streams) const;
    // The one pipeline over a plan; each step branches on `single` only where the device form differs.
    void place_pack(PackPlan& plan) const;         // a stream's offsets / total from h_olen_ (and the edges, the loudness); the size limits
    void place(OutputPlan& op) const;              // place_pack per stream, then (block form) the block's layout and its limit
    void fill_table(const OutputPlan& op, int* tab) const;  // kernels.h: PACK_SEG_*, or PACK_ENT_* / PACK_STREAM_*
    void launch(const OutputPlan& op);             // the pack kernel of the form, then launch_flac with a compressed stream
    void launch_flac(const OutputPlan& op);        // the compressed streams' samples in d_pack_ -> frames, sizes / places, d_flac_out_
    // Behind a fetch's checks, and the second half of a measured or compressed run: measure (ONE synchronisation, or none), place,
    // the limiter's curves, the buffers behind the run's layout or in arena_p_, the table's upload, launch.
    void finish_last_run(OutputPlan& op);
    // R: mi355vits_packed_result (single plans), mi355vits_streams_result or mi355vits_streams_result2
    template <typename R> void output_last_run(OutputPlan& op, R* out);  // finish_last_run, then the copy-out
    // what the three packed-form run calls are: the result struct zeroed, make_plan(op) (the form's validation), then the run
    template <typename R, typename F> void run_output(const RunCall& call, R* out, F&& make_plan);
    // FLAC: the sizes first (ONE synchronisation more than uncompressed), then exactly the frames behind the header the host writes
    void copy_out_plan(OutputPlan& op, mi355vits_packed_result* out);
    template <typename R> void copy_out_plan(OutputPlan& op, R* out);  // the block of a streams call
    void flac_prof_bytes(double bytes);  // the frames' bytes onto the pack.flac record under way, once the host knows them
    void find_edges(float ratio);                                      // h_edges_ of the last run at `ratio` (k_edges, 8 B bytes, one synchronisation) unless held
    // k_edges and its copy on the stream for each of the distinct non-zero `ratios` the host does not hold; true: a synchronisation is
    // owed.  keep: what the host holds at other ratios stays (a streams call); else the ratio measured replaces it, as ever
    bool enqueue_edges(const std::vector<float>& ratios, bool keep);
    const std::vector<int>& edges_at(float ratio) const;  // [2][B] of the last run at a ratio the host holds
    bool enqueue_loudness();          // k_loud / k_loud_gate and their copy likewise (throws below LOUD_MIN_HZ)
    bool enqueue_true_peak();         // k_true_peak and its copy likewise
    // what a pack needs from the audio: every launch, then ONE synchronisation (or none)
    void measure_last_run(const std::vector<float>& ratios, bool loud, bool keep, bool true_peak = false);
    // the peak the ceiling bounds, in double: the row's sample peak, or in true-peak mode its oversampled peak (measured before)
    double ceiling_peak(int row, const PackSettings& set) const { return set.true_peak() ? h_tp_[(size_t)row] : (double)h_loud_peaks_[(size_t)row]; }
    // window > 0 (the limiter on): a limited row keeps its uncapped gain — k_limit holds its peaks under the ceiling instead
    static void loudness_gain(double lufs, double peak, float target, float ceiling, int window, double* gain, bool* limited);
    // The limiter's jobs of a pack / a block / a fetch_limiter.  limit_job: the job of (row, set's target, ceiling and encoding
    // class) among `jobs`, appended when new.  run_limit_jobs: the jobs placed (their offsets checked before anything is sized),
    // uploaded and k_limit launched in `arena`; with_curve: d_curve_ = the curves, else statistics only.  Returns the device statistics.
    // keys (a streams call): the (window, true-peak mode) of every job, part of its identity
    using LimitKeys = std::vector<std::pair<int, int>>;
    int limit_job(std::vector<LimitJob>& jobs, int row, const PackSettings& set, double g, LimitKeys* keys = nullptr) const;
    // the jobs of a streams call: one k_limit launch per distinct key over one layout of curves (one key: run_limit_jobs itself)
    void run_limit_groups(std::vector<LimitJob>& jobs, const LimitKeys& keys);
    // what both end in: the placed jobs in one layout in `arena`, one upload, the launches of every group
    struct LimitGroup { size_t first, n; long tiles, floats; int window; bool tp; };
    LimitStat* launch_limit_groups(const std::vector<LimitJob>& placed, const std::vector<LimitGroup>& groups, long floats, DeviceArena& arena,
                                   bool with_curve);
    // true_peak: k_true_peak_env writes the jobs' envelopes into the same arena first and k_limit reads them instead of the samples
    LimitStat* run_limit_jobs(std::vector<LimitJob>& jobs, int window, DeviceArena& arena, bool with_curve, bool true_peak);
    void limit_pack(PackPlan& plan, std::vector<LimitJob>& jobs, LimitKeys* keys = nullptr) const;  // plan.curve = each over entry's job (after place_pack)
    static void curve_offsets(PackPlan& plan, const std::vector<LimitJob>& jobs);  // plan.curve: jobs -> their placed offsets

    mi355vits_config cfg_{};
    int device_ = 0;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_start_ = nullptr, ev_end_ = nullptr;
    bool end_recorded_ = false;  // ev_end_ of a completed run is on the stream: last_run_ms has something to read
    bool phase_b_ = false;       // inside flow_and_decoder (see Engine::fill_conv, pick_conv)
    LabSwitches sw_;
    int math_ = MATH_BF16X3;     // which matrix-core path the dense convs take (include/mi355vits.h: MI355VITS_MATH_*)
    // the math mode of the kernels that have no fp16 form of their own: in F16X2 they run as BF16X3 (the kernels that do —
    // fused MRF stages, fused WaveNet layers, staged convs, upsamplers — are switched where they are launched)
    int kmath() const { return math_ == MATH_F16X2 ? (int)MATH_BF16X3 : math_; }
    // the text side (phase A: encoder, duration predictor) never rounds its weights: ceil(exp(logw) * length_scale) is
    // discontinuous, so in MATH_BF16W it runs the exact three-term split and utterance lengths equal the default mode's
    int tmath() const { return kmath() == MATH_BF16W ? (int)MATH_BF16X3 : kmath(); }
    int pmath() const { return phase_b_ ? kmath() : tmath(); }  // math of the launch helpers shared by both phases
    Profiler prof_;

    std::vector<float> host_stage_;
    std::shared_ptr<Model> model_;

    DeviceArena arena_a_, arena_b_;
    DeviceArena arena_p_;  // mi355vits_fetch_packed only: the packed stream of a run whose frame-side arena has no room left for it
    DeviceArena arena_al_;  // mi355vits_fetch_alignment only: its five arrays, outside everything a run or a fetch lays out
    DeviceArena arena_ed_;  // k_edges' two words per row, likewise
    DeviceArena arena_ld_;  // k_loud's step energies and k_loud_gate's 16 bytes per row, likewise
    DeviceArena arena_lm_;  // k_limit's jobs, statistics and curves of the pack being made: no fetch serves from it
    DeviceArena arena_lf_;  // mi355vits_fetch_limiter only: k_limit's jobs and statistics
    DeviceArena arena_tp_;  // k_true_peak's 8 bytes per row, outside everything a run or another fetch lays out
    std::vector<Tap> taps_;
    bool taps_on_ = false;
    int B_ = 0, Tx_ = 0, Ty_ = 0;
    long L_ = 0;
    bool have_result_ = false, have_pcm_ = false;
    // phase-A buffers (sized by B, Tx)
    long long *d_ids_ = nullptr, *d_sid_ = nullptr;
    // per-row settings, uploaded with the inputs: [B,3] noise_scale, length_scale, noise_w; [B] PCM volume; [B] Philox keys
    float* d_scales_ = nullptr;
    double* d_vol_ = nullptr;
    unsigned long long* d_utt_ = nullptr;
    int *d_len_ = nullptr, *d_wceil_ = nullptr, *d_cum_ = nullptr, *d_ylen_ = nullptr, *d_alen_ = nullptr,
        *d_forced_ = nullptr;
    // a timed run's inputs (in the one upload, like d_forced_) and, right behind d_ylen_ (the same copy brings all three to the
    // host), its status and factor per row; d_durf_ = the u[t] the fit ran on (the dur_float tap)
    float *d_stretch_ = nullptr, *d_tfactor_ = nullptr, *d_durf_ = nullptr;
    int *d_minf_ = nullptr, *d_target_ = nullptr, *d_tstatus_ = nullptr;
    // a speakers run's tables (in the one upload, like d_sid_) and the g [B, gin] its kernel leaves (the "g" tap)
    long long* d_mix_sid_ = nullptr;
    float *d_mix_w_ = nullptr, *d_spk_vec_ = nullptr, *d_g_ = nullptr;
    // a levels run's gain [B, Tx] and ramp [B] (in the one upload)
    float* d_gain_ = nullptr;
    int* d_ramp_ = nullptr;
    // a pitch run's ratio [B, Tx] (in the one upload), k_pitch_plan's time map tq [B, Tx] and warped boundaries wc [B, Tx], and
    // wlen [B] (the fourth group of d_ylen_'s block)
    float* d_ratio_ = nullptr;
    long long* d_tq_ = nullptr;
    int *d_wc_ = nullptr, *d_wlen_ = nullptr;
    float *d_x_ = nullptr, *d_x2_ = nullptr, *d_qkv_ = nullptr, *d_att_ = nullptr, *d_ffn_ = nullptr, *d_part_ = nullptr,
          *d_stats_ = nullptr;
    float *d_h_ = nullptr, *d_d0_ = nullptr, *d_d1_ = nullptr, *d_d2_ = nullptr, *d_theta_ = nullptr, *d_z2_ = nullptr,
          *d_logw_ = nullptr, *d_noise_w_ = nullptr;
    float *d_cond_dp_ = nullptr, *d_cond_dec_ = nullptr;
    std::vector<float*> d_cond_flow_;
    // phase-B buffers (sized by B, Ty)
    float* d_fh2_ = nullptr;  // second h buffer of the fused WaveNet layers (ping-pong)
    float *d_z_ = nullptr, *d_fh_ = nullptr, *d_fu_ = nullptr, *d_fskip_ = nullptr, *d_noise_z_ = nullptr;
    float *d_bufA_ = nullptr, *d_bufB_ = nullptr, *d_bufT_ = nullptr, *d_bufC_ = nullptr;
    float* d_audio_ = nullptr;
    int16_t* d_pcm_ = nullptr;
    unsigned* d_peaks_ = nullptr;
    // output rate (mi355vits_set_output_rate).  The filter of the handle's setting, its table on the device; a run at another
    // rate than the voice's resamples d_audio_ into d_raudio_ (k_resample) and everything behind the waveform works on the o_*
    // view: the resampled rows, or in a native run d_audio_ / d_peaks_ / d_alen_ / L_ themselves.
    int out_hz_ = 0;               // the setting: 0 = native
    ResampleFilter rs_;
    float* d_rs_coef_ = nullptr;   // rs_.table (an allocation of its own: it outlives the runs)
    int run_hz_ = 0;               // the rate the last run ran at
    int run_L_ = 1, run_M_ = 1;    // its reduced ratio to the voice's rate (1 / 1 native): the handle's setting may have moved on
    PackSettings pack_;            // encoding, edge trimming and loudness target of the packed streams
    // edge trimming: the last run's raw first / last loud sample per row at each ratio measured so far (kept on the host so a
    // repeated fetch_packed / fetch_streams / fetch_edges does not launch again; dropped when a run starts).  A single-stream call
    // at a ratio not held replaces them by that one; a streams call adds its distinct ratios.
    struct EdgeSet {
        float ratio;
        std::vector<int> edges;  // [2][B]: s_first (n when none), s_last (-1)
        bool ready;              // the copy has been synchronised
    };
    std::vector<EdgeSet> h_edges_;
    bool have_edges_ = false;      // false: a run has started since, h_edges_ is of an earlier run
    // loudness: the last run's raw measurement (lufs [B] doubles, blocks [B], gated [B]) with its peaks, kept on the host so that
    // a fetch at any target launches nothing; dropped when a run starts
    std::vector<double> h_loud_;  // 2 B doubles: lufs, then blocks / gated as int32 pairs
    std::vector<float> h_loud_peaks_;
    bool have_loud_ = false;
    // true peak: the last run's tp [B] with the peaks [B] of the run, kept on the host likewise; dropped when a run starts
    std::vector<double> h_tp_;
    std::vector<float> h_tp_peaks_;
    bool have_tp_ = false;
    // pitch (mi355vits_run_pitch): k_pitch warps d_audio_ into d_waudio_, which takes the native waveform's place for every consumer:
    // the n_* view is the warped rows, or without pitch d_audio_ / d_peaks_ / d_alen_ / L_ themselves; the resampler reads it
    bool pitched_ = false;         // the last run was a pitch run (fetch_alignment: boundaries from d_wc_)
    float* d_waudio_ = nullptr;    // [B][Ln_] in the frame-side arena, pitch runs only
    unsigned* d_wpeaks_ = nullptr;
    int* d_walen_ = nullptr;       // pitch_fill_tab's table (the warped lengths, then k_pitch's first items), behind d_alen_ in the stage table (the same upload)
    long pitch_items_ = 0;         // the work items of that table, for k_pitch
    const float* n_audio_ = nullptr;
    unsigned* n_peaks_ = nullptr;
    const int* n_alen_ = nullptr;
    long Ln_ = 0;                  // row stride of the n_* view
    std::vector<int64_t> h_nlen_;  // [B] valid native-rate samples of a row of it
    float* d_raudio_ = nullptr;    // [B][Lo_] in the frame-side arena, resampled runs only
    unsigned* d_rpeaks_ = nullptr;
    int* d_rtab_ = nullptr;        // resample_fill_tab's table, behind the audio lengths in d_slen_'s block (the same upload)
    const float* o_audio_ = nullptr;
    const unsigned* o_peaks_ = nullptr;
    const int* o_alen_ = nullptr;
    long Lo_ = 0;                  // row stride and l_max of the results
    long rs_items_ = 0;            // a resampled run: the work items of its table (resample_fill_tab), for k_resample
    std::vector<int64_t> h_olen_;  // [B] valid samples of a row at the run's rate
    int* d_slen_ = nullptr;  // [n_upsamples + 1][B] valid frames per decoder stage
    // packed calls only, at the END of layout_b (every other pointer keeps its offset): the segment table right behind
    // d_slen_ (one upload brings both) and the stream itself
    int* d_pack_seg_ = nullptr;
    uint8_t* d_pack_ = nullptr;  // pack_capacity_bytes(encoding, total) bytes
    size_t layout_b_end_ = 0;  // arena_b_.used() behind d_slen_: where fetch_packed puts its buffers when there is room
    std::vector<int> h_ylen_;
    std::vector<unsigned char> h_in_;  // the call's host inputs, laid out like their device block (one upload)
    std::vector<int> h_slen_;         // per-stage valid lengths + audio lengths (one upload; packed calls: + the segment table)
    std::vector<int> h_pack_seg_;     // finish_last_run's table (its own upload)
    std::vector<LimitJob> h_limit_jobs_;  // k_limit's job table (its own upload)
    float* d_curve_ = nullptr;        // the curves of the pack being made (arena_lm_), nullptr when the limiter engages on no entry
    // plans with a compressed stream only (layout)
    FlacJob* d_flac_jobs_ = nullptr;
    uint8_t *d_flac_slots_ = nullptr, *d_flac_out_ = nullptr;
    int* d_flac_sizes_ = nullptr;
    long long* d_flac_offsets_ = nullptr;
    std::vector<FlacJob> h_flac_jobs_;  // the jobs' own upload: a member outlives the copy
    unsigned *d_flac_pre_ = nullptr, *d_flac_hdr_ = nullptr;  // the block form only
    int2* d_flac_ftab_ = nullptr;
    int *d_flac_items_ = nullptr, *d_flac_jtab_ = nullptr;
    std::vector<int> h_flac_sizes_;   // the frame sizes and their total, as copied
    int flac_prof_rec_ = -1;          // the profiler's record of the pack.flac launches under way: its bytes are known after the sizes
};

// what the owner_ of any of the five result structs points to goes back: pinned blocks to the pool, heap blocks freed (engine_results.cpp)
void release_result_owner(void* owner);

}  // namespace m355
