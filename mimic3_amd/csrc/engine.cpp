// engine.cpp — weight upload (with the load-time repacks the kernels want) and the launch sequence of one
// synthesis call: text encoder -> stochastic duration predictor -> length regulator -> flow^-1 -> HiFi-GAN
// -> tanh / peak / int16.  Everything runs on one HIP stream; the only host round trip inside a call is
// the 4*B-byte read of the frame counts that size the second half of the graph.  What is done with the finished
// waveform — copy-outs, packed streams, alignment, edges, loudness — is engine_results.cpp.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <type_traits>

namespace m355 {

// =================================================================================================
// .m355 container
// =================================================================================================
namespace {
struct Reader {
    const unsigned char* p;
    size_t n, pos = 0;
    void need(size_t k) const {
        if (pos + k > n) throw EngineError(MI355VITS_ERR_FORMAT, "weight container truncated");
    }
    template <typename T> T get() {
        need(sizeof(T));
        T v;
        memcpy(&v, p + pos, sizeof(T));
        pos += sizeof(T);
        return v;
    }
};
}  // namespace

void WeightsFile::parse(const void* blob, size_t n) {
    Reader r{static_cast<const unsigned char*>(blob), n};
    r.need(8);
    if (memcmp(r.p, "M355VITS", 8) != 0) throw EngineError(MI355VITS_ERR_FORMAT, "not an M355VITS weight container");
    r.pos = 8;
    const uint32_t version = r.get<uint32_t>();
    const uint32_t clen = r.get<uint32_t>();
    if (version != 1) throw EngineError(MI355VITS_ERR_FORMAT, "unsupported container version");
    if (clen != sizeof(mi355vits_config)) throw EngineError(MI355VITS_ERR_FORMAT, "config block size mismatch");
    r.need(clen);
    memcpy(&cfg, r.p + r.pos, clen);
    r.pos += clen;
    const uint32_t nt = r.get<uint32_t>();
    struct Ent { std::string name; std::vector<int> dims; uint64_t off; };
    std::vector<Ent> ents;
    for (uint32_t i = 0; i < nt; ++i) {
        const uint16_t nl = r.get<uint16_t>();
        r.need(nl);
        Ent e;
        e.name.assign(reinterpret_cast<const char*>(r.p + r.pos), nl);
        r.pos += nl;
        const uint32_t nd = r.get<uint32_t>();
        if (nd > 8) throw EngineError(MI355VITS_ERR_FORMAT, "tensor rank too large");
        for (uint32_t d = 0; d < nd; ++d) {
            const uint32_t v = r.get<uint32_t>();
            if (v > (1u << 28)) throw EngineError(MI355VITS_ERR_FORMAT, "implausible tensor dimension in " + e.name);
            e.dims.push_back((int)v);
        }
        e.off = r.get<uint64_t>();
        ents.push_back(std::move(e));
    }
    const uint64_t dbytes = r.get<uint64_t>();
    r.pos += (64 - r.pos % 64) % 64;
    if (r.pos > n || dbytes > n - r.pos) throw EngineError(MI355VITS_ERR_FORMAT, "weight container truncated (data section)");
    for (auto& e : ents) {
        size_t cnt = 1;
        for (int d : e.dims) {
            cnt *= (size_t)d;
            if (cnt > (size_t(1) << 34)) throw EngineError(MI355VITS_ERR_FORMAT, "tensor " + e.name + " too large");
        }
        if ((e.off & 3) || e.off > dbytes || cnt * 4 > dbytes - e.off)
            throw EngineError(MI355VITS_ERR_FORMAT, "tensor " + e.name + " out of bounds");
        HostTensor t;
        t.dims = e.dims;
        t.count = cnt;
        t.data = reinterpret_cast<const float*>(r.p + r.pos + e.off);
        tensors[e.name] = t;
    }
}

void WeightsFile::load(const std::string& path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw EngineError(MI355VITS_ERR_IO, "cannot open weight file: " + path);
    const std::streamsize sz = f.tellg();
    f.seekg(0);
    storage.resize((size_t)sz + 64);
    // keep float data 4-byte aligned: the data section starts on a 64-byte file offset
    unsigned char* base = storage.data();
    base += (64 - reinterpret_cast<uintptr_t>(base) % 64) % 64;
    if (!f.read(reinterpret_cast<char*>(base), sz)) throw EngineError(MI355VITS_ERR_IO, "cannot read weight file: " + path);
    parse(base, (size_t)sz);
}

const HostTensor& WeightsFile::get(const std::string& name, std::initializer_list<int> dims) const {
    auto it = tensors.find(name);
    if (it == tensors.end()) throw EngineError(MI355VITS_ERR_FORMAT, "missing tensor: " + name);
    if (it->second.dims != std::vector<int>(dims)) {
        std::ostringstream os;
        os << "tensor " << name << " has shape [";
        for (int d : it->second.dims) os << d << ",";
        os << "] expected [";
        for (int d : dims) os << d << ",";
        os << "]";
        throw EngineError(MI355VITS_ERR_FORMAT, os.str());
    }
    return it->second;
}

// =================================================================================================
// arena / profiler
// =================================================================================================
DeviceArena::~DeviceArena() {
    if (base_) (void)hipFree(base_);
}
void DeviceArena::reserve(size_t bytes, hipStream_t s) {
    if (bytes <= cap_) return;
    HIP_CHECK(hipStreamSynchronize(s));
    if (base_) HIP_CHECK(hipFree(base_));
    base_ = nullptr;
    cap_ = 0;
    const size_t want = bytes + bytes / 8 + (1 << 20);
    void* p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) throw EngineError(MI355VITS_ERR_NOMEM, "out of device memory (workspace)");
    base_ = static_cast<unsigned char*>(p);
    cap_ = want;
    // zero-filled once per (re)allocation: the decoder / flow kernels never compute items past a row's length in a ragged batch
    // (kernels_mrfp.cpp), so those columns keep whatever an earlier run left there — consumers mask by select, never by multiply
    // (a NaN or Inf there must reach no valid sample); tests/test_grid_geometry_and_poison.py is the guard
    HIP_CHECK(hipMemsetAsync(base_, 0, want, s));
}
void DeviceArena::fill(uint32_t pattern, hipStream_t s) {
    if (!base_) return;
#ifdef MI355_EMU
    (void)s;  // the CPU model's device memory is host memory
    std::fill_n(reinterpret_cast<uint32_t*>(base_), cap_ / 4, pattern);
#else
    HIP_CHECK(hipMemsetD32Async(base_, (int)pattern, cap_ / 4, s));
#endif
}
void* DeviceArena::alloc_bytes(size_t bytes) {
    const size_t need = padded(bytes);
    if (off_ + need > cap_) throw EngineError(MI355VITS_ERR_INTERNAL, "workspace arena overflow (sizing bug)");
    void* p = base_ + off_;
    off_ += need;
    return p;
}

Profiler::~Profiler() {
    for (auto e : pool) (void)hipEventDestroy(e);
    for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
}
hipEvent_t Profiler::get_event() {
    if (!pool.empty()) {
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
    }
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    return e;
}
int Profiler::begin(const char* name, double flops, double bytes) {
    auto it = ids.find(name);
    int id;
    if (it == ids.end()) {
        id = (int)names.size();
        names.emplace_back(name);
        ids[name] = id;
    } else {
        id = it->second;
    }
    Rec r{id, get_event(), get_event(), flops, bytes};
    HIP_CHECK(hipEventRecord(r.a, stream));
    recs.push_back(r);
    return (int)recs.size() - 1;
}
void Profiler::end(int rec) { (void)hipEventRecord(recs[rec].b, stream); }
void Profiler::clear() {
    (void)hipStreamSynchronize(stream);
    for (auto& r : recs) { pool.push_back(r.a); pool.push_back(r.b); }
    recs.clear();
}
std::string Profiler::report() {
    HIP_CHECK(hipStreamSynchronize(stream));
    struct Agg { long calls = 0; double ms = 0, flops = 0, bytes = 0; };
    std::vector<Agg> agg(names.size());
    for (auto& r : recs) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) ms = 0;
        Agg& a = agg[r.name_id];
        a.calls++;
        a.ms += ms;
        a.flops += r.flops;
        a.bytes += r.bytes;
    }
    std::ostringstream os;
    os.precision(9);
    for (size_t i = 0; i < names.size(); ++i)
        if (agg[i].calls) os << names[i] << " " << agg[i].calls << " " << agg[i].ms << " " << agg[i].flops << " " << agg[i].bytes << "\n";
    return os.str();
}

// =================================================================================================
// engine: construction / weight upload
// =================================================================================================
size_t Engine::stage(const float* p, size_t n) {
    const size_t off = (host_stage_.size() + 63) & ~size_t(63);
    host_stage_.resize(off + n);
    if (n) memcpy(host_stage_.data() + off, p, n * sizeof(float));
    return off;
}

const ConvW& Engine::add_conv_data(const std::string& key, const std::vector<float>& w, const std::vector<float>* bias,
                                   int Cout, int Cin, int K, int epi, ConvRole role) {
    if (w.size() != (size_t)Cout * Cin * K) throw EngineError(MI355VITS_ERR_INTERNAL, "add_conv_data size: " + key);
    ConvW c;
    c.Cout = Cout; c.Cin = Cin; c.K = K; c.epi = epi;
    c.raw = stage(w.data(), w.size());
    if (bias) c.bias = stage(bias->data(), bias->size());
    static_assert(sizeof(uint32_t) == sizeof(float), "bit patterns travel in the float arena");
    auto stage_words = [&](const std::vector<uint32_t>& p) { return stage(reinterpret_cast<const float*>(p.data()), p.size()); };
    if (conv1d_mfma_supported(Cin, Cout, K, 1)) {
        const int pe = epi == EPI_GATE ? EPI_GATE : EPI_STD;
        const std::vector<float> pk = conv_weights_mfma(w.data(), Cout, Cin, K, pe);
        c.packed = stage(pk.data(), pk.size());
        const bool rb = role == ROLE_RESBLOCK && epi == EPI_STD;
        if (rb && Cin % 8 == 0 && Cout % 32 == 0) {  // fused MRF stage
            const std::vector<float> p4 = conv_weights_mfma_x4(pk);
            c.packed4 = stage(p4.data(), p4.size());
        }
        if (rb && Cin % 16 == 0 && Cout % 32 == 0) {
            // the same weights as three bf16 planes for the split-operand path (MATH_BF16X3)
            c.packed_b3 = stage_words(conv_weights_bf16x3(w.data(), Cout, Cin, K));
            // ... and as two fp16 planes (MATH_F16X2, experimental), unless a weight is too large for the fixed scale
            const std::vector<uint32_t> h2 = conv_weights_f16x2(w.data(), Cout, Cin, K, 0);
            if (!h2.empty()) c.packed_h2 = stage_words(h2);
        }
        // ... and in the fragment order of k_mrf_p (16-row tiles, 32-channel k-groups)
        if (rb && Cin == Cout && Cin % 32 == 0 && (K == 3 || K == 5 || K == 7)) c.packed_p = stage_words(conv_weights_p16(w.data(), Cout, Cin, K));
        // polyphase upsamplers 128 -> 64 / 64 -> 32: fragments of 16-row tiles in natural row order (k_ups_pl)
        if (role == ROLE_UPSAMPLER && epi == EPI_STD && (Cin == 64 || Cin == 128 || Cin == 256) && Cout % 128 == 0 && K == 2)
            c.packed_p = stage_words(conv_weights_p16n(w.data(), Cout, Cin, K));
        if (Cin % 32 == 0 && (epi == EPI_GATE ? (Cout / 2) % 32 == 0 : true)) {
            // ... and for the staged split-bf16 kernel (every dense conv with a multiple of 32 input channels)
            c.packed_b3s = stage_words(conv_weights_bf16x3_staged(w.data(), Cout, Cin, K, pe));
            // k_wn_layer_b3 gates in registers: a gate conv's rows in tile order (kernels.h, conv_weights_gate_tiles)
            std::vector<float> wg;
            if (epi == EPI_GATE && Cout % 32 == 0) {
                wg = conv_weights_gate_tiles(w.data(), Cout, Cin, K);
#if defined(MI355_LAB) || defined(MI355_EMU)
                // (the split-bf16 form on these tiles is the lab build's and the CPU model's MI355VITS_WN_SHAPE=32 only; MATH_F16X2 below
                // keeps the tile order in every build)
                c.packed_b3w = stage_words(conv_weights_bf16x3_staged(wg.data(), Cout, Cin, K));
#endif
            }
            // the two convs of a coupling's WaveNet layer ("flow.<j>.in.<l>", "flow.<j>.rs.<l>") as k_wn_layer_b3 reads them on 16x16x32
            // tiles (kernels.h, pack_conv_weights_w16)
            const bool wn_conv = key.compare(0, 5, "flow.") == 0 && (epi == EPI_GATE ? key.find(".in.") != std::string::npos && Cout == 2 * Cin
                                                                                     : key.find(".rs.") != std::string::npos && K == 1 && epi == EPI_STD &&
                                                                                           (Cout == Cin || Cout == 2 * Cin));
            if (wn_conv && wn_layer_b3_supported(Cin, 1, 1)) c.packed_w16 = stage_words(conv_weights_w16(w.data(), Cout, Cin, K, epi == EPI_GATE));
            if (Cin % 16 == 0 && Cout % 32 == 0) {  // MATH_F16X2: WaveNet layers (gate convs: the tile order above), staged convs, polyphase upsamplers (plain rows)
                const std::vector<uint32_t> h2 = conv_weights_f16x2(wg.empty() ? w.data() : wg.data(), Cout, Cin, K, 1);
                if (!h2.empty()) c.packed_h2s = stage_words(h2);
            }
        }
    }
    return model_->convs[key] = c;
}

const ConvW& Engine::add_conv(const WeightsFile& wf, const std::string& key, const std::string& tensor, int Cout, int Cin,
                              int K, bool bias, int epi, ConvRole role) {
    const HostTensor& w = wf.get(tensor + ".weight", {Cout, Cin, K});
    std::vector<float> wv(w.data, w.data + w.count), bv;
    if (bias) {
        const HostTensor& b = wf.get(tensor + ".bias", {Cout});
        bv.assign(b.data, b.data + b.count);
    }
    return add_conv_data(key, wv, bias ? &bv : nullptr, Cout, Cin, K, epi, role);
}

void Engine::add_vec(const WeightsFile& wf, const std::string& name, std::initializer_list<int> dims) {
    const HostTensor& t = wf.get(name, dims);
    model_->vecs[name] = stage(t.data, t.count);
}
const float* Engine::vec(const std::string& name) const {
    auto it = model_->vecs.find(name);
    if (it == model_->vecs.end()) throw EngineError(MI355VITS_ERR_INTERNAL, "unknown tensor: " + name);
    return model_->dev_weights + it->second;
}
const ConvW& Engine::cw(const std::string& key) const {
    auto it = model_->convs.find(key);
    if (it == model_->convs.end()) throw EngineError(MI355VITS_ERR_INTERNAL, "unknown conv: " + key);
    return it->second;
}

static std::string S(const char* fmt, int a = 0, int b = 0, int c = 0) {
    char buf[160];
    snprintf(buf, sizeof(buf), fmt, a, b, c);
    return buf;
}

static void validate_config(const mi355vits_config& c) {
    auto bad = [](const std::string& m) { throw EngineError(MI355VITS_ERR_FORMAT, "invalid voice config: " + m); };
    if (c.num_symbols < 1 || c.n_speakers < 1) bad("num_symbols / n_speakers");
    if (c.hidden_channels < 2 || c.hidden_channels % 2 || c.inter_channels < 2 || c.inter_channels % 2) bad("channel counts must be even");
    if (c.n_heads < 1 || c.hidden_channels % c.n_heads) bad("hidden_channels % n_heads");
    if (c.resblock != 1 && c.resblock != 2) bad("resblock must be 1 or 2");
    if (c.n_upsamples < 1 || c.n_upsamples > MI355VITS_MAX_STAGES) bad("n_upsamples");
    if (c.n_resblock_kernels < 1 || c.n_resblock_kernels > MI355VITS_MAX_STAGES) bad("n_resblock_kernels");
    long hop = 1;
    int ch = c.upsample_initial_channel;
    for (int i = 0; i < c.n_upsamples; ++i) {
        if (c.upsample_rates[i] < 1 || c.upsample_kernel_sizes[i] < c.upsample_rates[i]) bad("upsample stage");
        if ((c.upsample_kernel_sizes[i] - c.upsample_rates[i]) % 2) bad("upsample kernel - rate must be even");
        if (ch % 2) bad("upsample channels must halve evenly");
        ch /= 2;
        hop *= c.upsample_rates[i];
    }
    if (ch % 2) bad("decoder channel counts must be even");
    if (hop != c.hop_length) bad("hop_length must equal the product of upsample_rates");
    for (int j = 0; j < c.n_resblock_kernels; ++j) {
        if (c.resblock_kernel_sizes[j] < 1 || c.resblock_kernel_sizes[j] % 2 == 0) bad("resblock kernel sizes must be odd");
        if (c.resblock_n_dilations[j] < 1 || c.resblock_n_dilations[j] > MI355VITS_MAX_STAGES) bad("resblock dilations");
    }
    if (c.n_speakers > 1 && c.gin_channels < 1) bad("multi-speaker voice needs gin_channels");
    // dp_n_flows == 0 marks the deterministic duration predictor (include/mi355vits.h); it has no DDS layers and no spline
    const bool det_dp = c.dp_n_flows == 0;
    if (det_dp ? (c.dp_num_bins != 0 || c.dp_dds_layers != 0) : (c.dp_num_bins < 2 || c.dp_num_bins > 16)) bad("dp_num_bins");
    if ((!det_dp && c.dp_n_flows < 2) || c.flow_n_flows < 1 || c.flow_wn_layers < 1) bad("flow depth");
    if (c.flow_wn_kernel % 2 == 0 || c.dp_kernel_size % 2 == 0) bad("flow / dp kernels must be odd");
    if (c.window_size < 0 || c.n_layers < 1 || c.kernel_size < 1) bad("encoder");
    // plausibility caps: a corrupted header must not turn into absurd loops or allocations
    if (c.num_symbols > (1 << 20) || c.n_speakers > (1 << 20) || c.hidden_channels > 8192 || c.inter_channels > 8192 ||
        c.filter_channels < 1 || c.filter_channels > 32768 || c.upsample_initial_channel < 2 || c.upsample_initial_channel > 8192 ||
        c.gin_channels < 0 || c.gin_channels > 8192)
        bad("channel / symbol counts out of range");
    if (c.n_layers > 64 || c.kernel_size > 63 || c.window_size > 15 || c.flow_n_flows > 32 || c.flow_wn_layers > 32 ||
        c.flow_wn_kernel < 1 || c.flow_wn_kernel > 63 || c.flow_wn_dilation_rate < 1 || c.flow_wn_dilation_rate > 8 ||
        c.dp_n_flows > 16 || (!det_dp && c.dp_dds_layers < 1) || c.dp_dds_layers > 8 || c.dp_kernel_size < 1 || c.dp_kernel_size > 63 ||
        !(c.dp_tail_bound > 0.0f) || c.hop_length > (1 << 16))
        bad("depth / kernel sizes out of range");
    for (int i = 0; i < c.n_upsamples; ++i)
        if (c.upsample_rates[i] > 64 || c.upsample_kernel_sizes[i] > 256) bad("upsample stage out of range");
    for (int j = 0; j < c.n_resblock_kernels; ++j) {
        if (c.resblock_kernel_sizes[j] > 63) bad("resblock kernel size out of range");
        for (int m = 0; m < c.resblock_n_dilations[j]; ++m)
            if (c.resblock_dilations[j * MI355VITS_MAX_STAGES + m] < 1 || c.resblock_dilations[j * MI355VITS_MAX_STAGES + m] > 256)
                bad("resblock dilation out of range");
    }
}

Engine::Engine(const WeightsFile& wf, int device) : cfg_(wf.cfg), device_(device) {
    // a throwing constructor never runs the destructor: stream, events and the weight arena are released here
    try {
        construct(wf, device);
    } catch (...) {
        release();
        throw;
    }
}

Model::~Model() {
    if (dev_weights) {
        (void)hipSetDevice(device);
        (void)hipFree(dev_weights);
    }
}

Engine::Engine(const Engine& lane0) : cfg_(lane0.cfg_), device_(lane0.device_) {
    try {
        open_device(device_);
        model_ = lane0.model_;
        math_ = lane0.math_;
        sw_ = lane0.sw_;
        if (lane0.out_hz_) set_output_rate(lane0.out_hz_);
        pack_ = lane0.pack_;
    } catch (...) {
        release();
        throw;
    }
}

LabSwitches LabSwitches::from_env() {
    auto one = [](const char* name) { const char* v = lab_getenv(name); return v && v[0] == '1'; };
    auto set = [](const char* name) { return lab_getenv(name) != nullptr; };
    LabSwitches s;
    s.force_generic = one("MI355VITS_FORCE_GENERIC");
    s.no_fused_wn = one("MI355VITS_NO_FUSED_WN");
    s.no_fused_mrf = one("MI355VITS_NO_FUSED_MRF");
    if (const char* bw = lab_getenv("MI355VITS_B3_MIN_WORK")) s.b3_min_work = atoi(bw);
    s.wn_b3 = set("MI355VITS_WN_B3");
    s.no_mrf_p = set("MI355VITS_NO_MRF_P");
    s.no_rbc = set("MI355VITS_NO_RBC");
    s.no_fused_dds = set("MI355VITS_NO_FUSED_DDS");
    s.no_dds_stack = set("MI355VITS_NO_DDS_STACK");
    s.no_dds_stack_b3 = set("MI355VITS_NO_DDS_STACK_B3");
    s.no_enc_gemm = set("MI355VITS_NO_ENC_GEMM");
    s.no_enc_o_ln = set("MI355VITS_NO_ENC_O_LN");
    s.no_flow_gemm = set("MI355VITS_NO_FLOW_GEMM");
    s.no_f16x2_convs = set("MI355VITS_F16X2_NO_CONVS");
    return s;
}

void Engine::open_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        throw EngineError(MI355VITS_ERR_DEVICE, "no HIP device available (the MI355X engine has no CPU fallback)");
    if (device < 0 || device >= ndev) throw EngineError(MI355VITS_ERR_INVALID, "device index out of range");
    HIP_CHECK(hipSetDevice(device_));
    HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreate(&ev_start_));
    HIP_CHECK(hipEventCreate(&ev_end_));
    prof_.stream = stream_;
    sw_ = LabSwitches::from_env();
    math_ = MATH_BF16X3;  // default (see include/mi355vits.h: f32-grade results; MI355VITS_MATH=f32 for v_mfma_f32_*)
    const char* mm = getenv("MI355VITS_MATH");
    if (mm && mm[0]) {
        if (!strcmp(mm, "bf16x3")) math_ = MATH_BF16X3;
        else if (!strcmp(mm, "f32")) math_ = MATH_F32;
        else if (!strcmp(mm, "bf16w")) math_ = MATH_BF16W;
        else if (!strcmp(mm, "f16x2")) math_ = MATH_F16X2;
        else throw EngineError(MI355VITS_ERR_INVALID, std::string("MI355VITS_MATH: unknown mode '") + mm + "' (f32 | bf16x3 | bf16w | f16x2)");
    }
}

void Engine::set_math(int mode) {
    if (mode != MATH_F32 && mode != MATH_BF16X3 && mode != MATH_BF16W && mode != MATH_F16X2) throw EngineError(MI355VITS_ERR_INVALID, "unknown math mode");
    math_ = mode;
}

// The rate of every result of the runs that start after this.  Nothing of the handle changes unless the whole setting succeeds.
void Engine::set_output_rate(int hz) {
    if (hz == 0 || hz == cfg_.sample_rate) {  // native: no kernel, no buffer (the table of an earlier setting stays where it is, unused)
        out_hz_ = 0;
        return;
    }
    if (d_rs_coef_ && hz == rs_.out_hz) {  // the table of this rate is still on the device (set, then native, then set again)
        out_hz_ = hz;
        return;
    }
    ResampleFilter f;
    if (!resample_design(cfg_.sample_rate, hz, f)) {
        std::string ratio;
        if (hz >= 1) {
            int a = hz, b = cfg_.sample_rate;
            while (b) { const int t = a % b; a = b; b = t; }
            ratio = " = " + std::to_string(hz / a) + " / " + std::to_string(cfg_.sample_rate / a) + " of the voice's " + std::to_string(cfg_.sample_rate) + " Hz";
        }
        throw EngineError(MI355VITS_ERR_INVALID, "output rate " + std::to_string(hz) + " Hz" + ratio + " not supported: the rate must be >= 1 and both terms of the reduced ratio <= " +
                                                     std::to_string(RESAMPLE_MAX_RATIO));
    }
    HIP_CHECK(hipSetDevice(device_));
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, f.table.size() * 4));
    if (hipMemcpy(p, f.table.data(), f.table.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p);
        throw EngineError(MI355VITS_ERR_DEVICE, "output rate: the filter upload failed");
    }
    HIP_CHECK(hipStreamSynchronize(stream_));  // no run of this handle still reads the table about to be freed
    if (d_rs_coef_) (void)hipFree(d_rs_coef_);
    d_rs_coef_ = static_cast<float*>(p);
    rs_ = std::move(f);
    out_hz_ = hz;
}

void Engine::construct(const WeightsFile& wf, int device) {
    validate_config(cfg_);
    open_device(device);
    model_ = std::make_shared<Model>();
    model_->device = device;

    const mi355vits_config& c = cfg_;
    const int H = c.hidden_channels, F = c.filter_channels, I = c.inter_channels, half = I / 2;
    const int hd = H / c.n_heads, nrel = 2 * c.window_size + 1;
    const int gin = c.n_speakers > 1 ? c.gin_channels : 0;

    auto add_dds = [&](const std::string& p, int C) {
        for (int i = 0; i < c.dp_dds_layers; ++i) {
            add_vec(wf, p + S(".convs_sep.%d.weight", i), {C, 1, c.dp_kernel_size});
            add_vec(wf, p + S(".convs_sep.%d.bias", i), {C});
            add_conv(wf, p + S(".convs_1x1.%d", i), p + S(".convs_1x1.%d", i), C, C, 1, true);
            add_vec(wf, p + S(".norms_1.%d.gamma", i), {C});
            add_vec(wf, p + S(".norms_1.%d.beta", i), {C});
            add_vec(wf, p + S(".norms_2.%d.gamma", i), {C});
            add_vec(wf, p + S(".norms_2.%d.beta", i), {C});
        }
    };

    // ---- k_pitch's filter table (mi355vits_run_pitch): made on the host in double, staged with the weights
    model_->vecs["pitch.table"] = stage(pitch_table().data(), pitch_table().size());

    // ---- text encoder
    add_vec(wf, "enc_p.emb.weight", {c.num_symbols, H});
    for (int i = 0; i < c.n_layers; ++i) {
        const std::string a = S("enc_p.encoder.attn_layers.%d", i);
        std::vector<float> wq(3 * (size_t)H * H), bq(3 * (size_t)H);
        const char* names[3] = {".conv_q", ".conv_k", ".conv_v"};
        for (int q = 0; q < 3; ++q) {
            const HostTensor& w = wf.get(a + names[q] + ".weight", {H, H, 1});
            const HostTensor& b = wf.get(a + names[q] + ".bias", {H});
            memcpy(wq.data() + (size_t)q * H * H, w.data, sizeof(float) * H * H);
            memcpy(bq.data() + (size_t)q * H, b.data, sizeof(float) * H);
        }
        add_conv_data(S("enc.%d.qkv", i), wq, &bq, 3 * H, H, 1);
        add_conv(wf, S("enc.%d.o", i), a + ".conv_o", H, H, 1, true);
        add_vec(wf, a + ".emb_rel_k", {1, nrel, hd});
        add_vec(wf, a + ".emb_rel_v", {1, nrel, hd});
        add_vec(wf, S("enc_p.encoder.norm_layers_1.%d.gamma", i), {H});
        add_vec(wf, S("enc_p.encoder.norm_layers_1.%d.beta", i), {H});
        add_conv(wf, S("enc.%d.ffn1", i), S("enc_p.encoder.ffn_layers.%d.conv_1", i), F, H, c.kernel_size, true);
        add_conv(wf, S("enc.%d.ffn2", i), S("enc_p.encoder.ffn_layers.%d.conv_2", i), H, F, c.kernel_size, true);
        add_vec(wf, S("enc_p.encoder.norm_layers_2.%d.gamma", i), {H});
        add_vec(wf, S("enc_p.encoder.norm_layers_2.%d.beta", i), {H});
    }
    add_conv(wf, "enc.proj", "enc_p.proj", 2 * I, H, 1, true);

    // ---- deterministic duration predictor (dp_n_flows == 0): F from the container's tensor table
    if (c.dp_n_flows == 0) {
        const auto it = wf.tensors.find("dp.conv_1.bias");
        if (it == wf.tensors.end() || it->second.dims.size() != 1)
            throw EngineError(MI355VITS_ERR_FORMAT, "missing tensor dp.conv_1.bias (deterministic duration predictor)");
        const int DF = it->second.dims[0], K = c.dp_kernel_size;
        if (!dp_det_supported(H, DF, K))
            throw EngineError(MI355VITS_ERR_FORMAT, S("deterministic duration predictor: hidden %d / filter %d / kernel %d not supported "
                                                           "(multiples of 32 up to 256, odd kernel up to 7)", H, DF, K));
        model_->dp_filter = DF;
        add_conv(wf, "dp.conv_1", "dp.conv_1", DF, H, K, true);
        add_conv(wf, "dp.conv_2", "dp.conv_2", DF, DF, K, true);
        for (const char* n : {"dp.norm_1.gamma", "dp.norm_1.beta", "dp.norm_2.gamma", "dp.norm_2.beta"}) add_vec(wf, n, {DF});
        add_vec(wf, "dp.proj.weight", {1, DF, 1});
        add_vec(wf, "dp.proj.bias", {1});
        if (gin) {
            add_vec(wf, "dp.cond.weight", {H, gin, 1});
            add_vec(wf, "dp.cond.bias", {H});
        }
    } else {
    // ---- stochastic duration predictor (inference half)
    add_conv(wf, "dp.pre", "dp.pre", H, H, 1, true);
    add_conv(wf, "dp.proj", "dp.proj", H, H, 1, true);
    add_dds("dp.convs", H);
    if (gin) {
        add_vec(wf, "dp.cond.weight", {H, gin, 1});
        add_vec(wf, "dp.cond.bias", {H});
    }
    {
        const HostTensor& m = wf.get("dp.flows.0.m", {2, 1});
        const HostTensor& l = wf.get("dp.flows.0.logs", {2, 1});
        model_->ea_m[0] = m.data[0]; model_->ea_m[1] = m.data[1];
        model_->ea_logs[0] = l.data[0]; model_->ea_logs[1] = l.data[1];
    }
    for (int j = 1; j < c.dp_n_flows; ++j) {
        const std::string p = S("dp.flows.%d", 1 + 2 * j);
        add_vec(wf, p + ".pre.weight", {H, 1, 1});
        add_vec(wf, p + ".pre.bias", {H});
        add_dds(p + ".convs", H);
        add_conv(wf, p + ".proj", p + ".proj", 3 * c.dp_num_bins - 1, H, 1, true);
    }
    }

    // ---- residual coupling flow.  The channel flips between couplings are folded into the weights:
    // after an odd number of flips the logical tensor is the physical one reversed, so that coupling reads
    // its x0 from the physical upper half through a channel-reversed `pre` and writes its x1 into the
    // physical lower half through a channel-reversed `post`; after an even number it is the identity.
    for (int j = 0; j < c.flow_n_flows; ++j) {
        const int e = c.flow_n_flows - 1 - j;  // execution index (reverse order)
        const bool rev = (e % 2) == 0;
        const std::string f = S("flow.flows.%d", 2 * j);
        {
            const HostTensor& w = wf.get(f + ".pre.weight", {H, half, 1});
            const HostTensor& b = wf.get(f + ".pre.bias", {H});
            std::vector<float> wv(w.count), bv(b.data, b.data + b.count);
            for (int co = 0; co < H; ++co)
                for (int q = 0; q < half; ++q) wv[(size_t)co * half + q] = w.data[(size_t)co * half + (rev ? half - 1 - q : q)];
            add_conv_data(S("flow.%d.pre", j), wv, &bv, H, half, 1);
        }
        for (int l = 0; l < c.flow_wn_layers; ++l) {
            add_conv(wf, S("flow.%d.in.%d", j, l), f + S(".enc.in_layers.%d", l), 2 * H, H, c.flow_wn_kernel, true, EPI_GATE);
            const int rs = l < c.flow_wn_layers - 1 ? 2 * H : H;
            add_conv(wf, S("flow.%d.rs.%d", j, l), f + S(".enc.res_skip_layers.%d", l), rs, H, 1, true);
        }
        if (gin) {
            add_vec(wf, f + ".enc.cond_layer.weight", {2 * H * c.flow_wn_layers, gin, 1});
            add_vec(wf, f + ".enc.cond_layer.bias", {2 * H * c.flow_wn_layers});
        }
        {
            const HostTensor& w = wf.get(f + ".post.weight", {half, H, 1});
            const HostTensor& b = wf.get(f + ".post.bias", {half});
            std::vector<float> wv(w.count), bv(b.count);
            for (int p = 0; p < half; ++p) {
                const int src = rev ? half - 1 - p : p;
                memcpy(wv.data() + (size_t)p * H, w.data + (size_t)src * H, sizeof(float) * H);
                bv[p] = b.data[src];
            }
            add_conv_data(S("flow.%d.post", j), wv, &bv, half, H, 1);
        }
    }
    model_->flow_reversed_out = (c.flow_n_flows % 2) == 1;

    // ---- HiFi-GAN decoder
    const int C0 = c.upsample_initial_channel;
    {
        const HostTensor& w = wf.get("dec.conv_pre.weight", {C0, I, 7});
        const HostTensor& b = wf.get("dec.conv_pre.bias", {C0});
        std::vector<float> wv(w.count), bv(b.data, b.data + b.count);
        for (int co = 0; co < C0; ++co)
            for (int ci = 0; ci < I; ++ci)
                memcpy(wv.data() + ((size_t)co * I + ci) * 7, w.data + ((size_t)co * I + (model_->flow_reversed_out ? I - 1 - ci : ci)) * 7,
                       sizeof(float) * 7);
        add_conv_data("dec.conv_pre", wv, &bv, C0, I, 7);
    }
    int ch = C0;
    for (int i = 0; i < c.n_upsamples; ++i) {
        add_vec(wf, S("dec.ups.%d.weight", i), {ch, ch / 2, c.upsample_kernel_sizes[i]});
        add_vec(wf, S("dec.ups.%d.bias", i), {ch / 2});
        {
            // the transposed conv as `rate` polyphase stride-1 filters on the matrix cores (kernels.h: shuf_*)
            const int uk = c.upsample_kernel_sizes[i], ur = c.upsample_rates[i], taps = convt_taps(uk, ur);
            const HostTensor& w = wf.get(S("dec.ups.%d.weight", i), {ch, ch / 2, uk});
            const HostTensor& b = wf.get(S("dec.ups.%d.bias", i), {ch / 2});
            std::vector<float> wv((size_t)ur * (ch / 2) * ch * taps), bv((size_t)ur * (ch / 2));
            convt_to_polyphase(w.data, b.data, ch, ch / 2, uk, ur, wv.data(), bv.data());
            add_conv_data(S("dec.ups.%d.poly", i), wv, &bv, ur * (ch / 2), ch, taps, EPI_STD, ROLE_UPSAMPLER);
        }
        ch /= 2;
        for (int j = 0; j < c.n_resblock_kernels; ++j) {
            const int n = i * c.n_resblock_kernels + j;
            const int rk = c.resblock_kernel_sizes[j];
            for (int m = 0; m < c.resblock_n_dilations[j]; ++m) {
                if (c.resblock == 2) {
                    add_conv(wf, S("dec.rb.%d.c.%d", n, m), S("dec.resblocks.%d.convs.%d", n, m), ch, ch, rk, true, EPI_STD, ROLE_RESBLOCK);
                } else {
                    add_conv(wf, S("dec.rb.%d.c1.%d", n, m), S("dec.resblocks.%d.convs1.%d", n, m), ch, ch, rk, true, EPI_STD, ROLE_RESBLOCK);
                    add_conv(wf, S("dec.rb.%d.c2.%d", n, m), S("dec.resblocks.%d.convs2.%d", n, m), ch, ch, rk, true, EPI_STD, ROLE_RESBLOCK);
                }
            }
        }
    }
    add_vec(wf, "dec.conv_post.weight", {1, ch, 7});
    if (gin) {
        add_vec(wf, "dec.cond.weight", {C0, gin, 1});
        add_vec(wf, "dec.cond.bias", {C0});
        add_vec(wf, "emb_g.weight", {c.n_speakers, gin});
        const HostTensor& e = wf.get("emb_g.weight", {c.n_speakers, gin});
        model_->emb_g.assign(e.data, e.data + e.count);  // mi355vits_get_speaker_embedding serves table rows without stream work
    }

    // ---- one upload
    void* p = nullptr;
    if (hipMalloc(&p, host_stage_.size() * sizeof(float) + 256) != hipSuccess)
        throw EngineError(MI355VITS_ERR_NOMEM, "out of device memory (weights)");
    model_->dev_weights = static_cast<float*>(p);
    model_->bytes = host_stage_.size() * sizeof(float);
    HIP_CHECK(hipMemcpy(model_->dev_weights, host_stage_.data(), host_stage_.size() * sizeof(float), hipMemcpyHostToDevice));
    std::vector<float>().swap(host_stage_);
}

void Engine::fill_workspace(uint32_t pattern) {
    HIP_CHECK(hipSetDevice(device_));
    arena_a_.fill(pattern, stream_);
    arena_b_.fill(pattern, stream_);
    arena_p_.fill(pattern, stream_);
    arena_al_.fill(pattern, stream_);
    arena_ed_.fill(pattern, stream_);
    arena_ld_.fill(pattern, stream_);
    arena_lm_.fill(pattern, stream_);
    arena_lf_.fill(pattern, stream_);
    arena_tp_.fill(pattern, stream_);
    HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::probe_weights(double out[8]) {
    HIP_CHECK(hipSetDevice(device_));
    const int cus = current_device_cu_count();
    const int n16 = 256 * 8 * 80;  // 2.62 MB windows
    const size_t win = (size_t)n16 * 16;
    const int nwin = (int)std::min<size_t>(model_->bytes / win, 24);
    if (nwin < 1) throw EngineError(MI355VITS_ERR_INVALID, "weight arena smaller than one probe window");
    // (diagnostics of include/mi355vits_lab.h: hipMalloc / hipFree synchronise the device — not for a handle that is serving.)
    DevBuf sk((size_t)cus * 4 + 16);
    unsigned* sink = sk.as<unsigned>();
    std::vector<double> g8, g1;
    for (int wdx = 0; wdx < nwin; ++wdx) {
        const char* base = reinterpret_cast<const char*>(model_->dev_weights) + (size_t)wdx * win;
        for (int mode = 0; mode < 2; ++mode) {
            auto go = [&] {
                if (mode == 0) launch_probe_l2_stream(base, n16, 4, sink, cus, stream_);
                else launch_probe_l2_stream1(base, n16, 1, sink, cus, stream_);
            };
            const double ms = timed(go, 1, 2, stream_);
            const double gbs = (double)cus * (mode == 0 ? 4 : 1) * win / (ms * 1e-3) / 1e9;
            (mode == 0 ? g8 : g1).push_back(gbs);
        }
    }
    std::sort(g8.begin(), g8.end());
    std::sort(g1.begin(), g1.end());
    out[0] = g8.front(); out[1] = g8[g8.size() / 2]; out[2] = g8.back();
    out[3] = g1.front(); out[4] = g1[g1.size() / 2]; out[5] = g1.back();
    out[6] = (double)nwin;
    out[7] = (double)(reinterpret_cast<uintptr_t>(model_->dev_weights) & 0xfffffffffULL);  // low bits of the arena's virtual address
}

void Engine::release() noexcept {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (auto& t : taps_) (void)hipFree(t.dev);
    taps_.clear();
    if (d_rs_coef_) (void)hipFree(d_rs_coef_);
    d_rs_coef_ = nullptr;
    model_.reset();  // the replica is freed with its last lane
    if (ev_start_) (void)hipEventDestroy(ev_start_);
    if (ev_end_) (void)hipEventDestroy(ev_end_);
    ev_start_ = ev_end_ = nullptr;
    if (stream_) (void)hipStreamDestroy(stream_);
    stream_ = nullptr;
}

Engine::~Engine() { release(); }

// =================================================================================================
// launch helpers
// =================================================================================================
void Engine::fill_conv(const ConvW& w, ConvArgs& a) const {
    // frames-sized tensors: the kernel is a function of the layer, not of the batch's padding.  Phoneme-sized ones (the text
    // encoder) stay on the f32 kernels except the wide FFN conv (192 -> 768, k3: K Cin >= 512 and >= 4 row blocks), whose
    // grid fills most of the chip even at one column tile per row — again a rule of the layer alone
    const bool wide_enc = !phase_b_ && w.K * w.Cin >= 512 && w.Cout >= 512 && a.epi == EPI_STD;
    a.fixed_rule = (phase_b_ || wide_enc) ? 1 : 0;
    a.Cin = w.Cin;
    a.Cout = w.Cout;
    a.K = w.K;
    a.bias = P(w.bias);
    if (a.pad < 0) a.pad = (w.K * a.dil - a.dil) / 2;
}

// The one place that decides which kernel a dense conv runs on; `a` is filled in (fill_conv).
ConvKernel Engine::pick_conv(const ConvW& w, const ConvArgs& a) const {
    // every input channel resident in LDS (kernels_rbc.cpp), MATH_BF16X3 only: the other modes keep their kernels
    const bool resident = phase_b_ && !sw_.force_generic && !sw_.no_rbc && math_ == MATH_BF16X3 && w.packed_p != NO_OFF;
    if (resident && a.shuf_s && ups_pl_supported(a)) return UPS_PL;  // polyphase upsamplers 128 -> 64, 64 -> 32 (k_ups_pl)
    if (resident && rb_conv_supported(a)) return RB_CONV;            // 128-channel resblock convs, one launch per conv (k_rb_conv)
    // phoneme-sized convs, and the pointwise convs around the coupling layers' WaveNet stacks (frames: K = 1 only): one 192-channel
    // slice per workgroup, staged once (k_enc_b3); a split conv only where the caller adds up the slices
    if (!sw_.force_generic && !sw_.no_enc_gemm && (!phase_b_ || (w.K == 1 && !sw_.no_flow_gemm)) && math_on_bf16(pmath()) &&
        w.packed_b3s != NO_OFF && a.epi == EPI_STD && w.epi == EPI_STD && !a.shuf_s && a.Tin < 0 && !a.accumulate &&
        enc_conv_b3_supported(w.Cin, w.Cout, w.K, a.dil) && a.ksplit == enc_conv_b3_slices(w.Cin) && (a.ksplit == 1 || a.part))
        return ENC_B3;
    if (sw_.force_generic || w.packed == NO_OFF) return GENERIC;
    // split-bf16 staged kernel where it pays: convs with little work per staged chunk (1x1 convs, the last
    // upsampler: K * Cin < 256) spend more on splitting the chunk than the faster matrix-core loop saves
    // (measured: flow.pre / post, res_skip, upsample 64 -> 32); MI355VITS_B3_MIN_WORK overrides the threshold (tests).
    // math_on_bf16(a.math): the caller's opt-in (MI355VITS_WN_B3)
    if (math_on_bf16(pmath()) && w.packed_b3s != NO_OFF &&
        (math_on_bf16(a.math) || ((w.K * w.Cin >= sw_.b3_min_work || (a.shuf_s && w.Cin % 64 == 0)) && a.epi == EPI_STD)))
        return (math_ == MATH_F16X2 && w.packed_h2s != NO_OFF && a.epi == EPI_STD && !sw_.no_f16x2_convs) ? STAGED_F16X2 : STAGED_B3;
    return MFMA_F32;
}

void Engine::conv(const char* label, const ConvW& w, ConvArgs a) {
    fill_conv(w, a);
    if ((a.epi == EPI_GATE) != (w.epi == EPI_GATE)) throw EngineError(MI355VITS_ERR_INTERNAL, "conv epilogue / packing mismatch");
    const double flops = 2.0 * a.B * (double)a.T * w.Cout * w.Cin * w.K;
    double ch_io = (double)w.Cin + (a.epi == EPI_GATE ? a.H : w.Cout);
    if (a.res) ch_io += w.Cout;
    if (a.accumulate) ch_io += w.Cout;
    if (a.epi == EPI_RESSKIP) ch_io += w.Cout;  // h and skip are read-modify-write
    const double bytes = 4.0 * a.B * (double)a.T * ch_io + 4.0 * (double)w.Cout * w.Cin * w.K;
    ProfScope ps(prof_, label, flops, bytes);
    const ConvKernel kernel = pick_conv(w, a);
    switch (kernel) {  // the weights in the kernel's format, its math
    case UPS_PL:
    case RB_CONV:
        a.w = P(w.packed_p); a.math = MATH_BF16X3;
        // the host's copy of the row lengths (the per-stage lengths are made on the host and uploaded as one table): the launcher
        // counts the (row, column block) items that have work from it
        if (d_slen_ && a.in_len >= d_slen_ && a.in_len < d_slen_ + h_slen_.size()) a.in_len_host = h_slen_.data() + (a.in_len - d_slen_);
        break;
    case ENC_B3: a.wb3 = P(w.packed_b3s); a.math = pmath(); break;
    case STAGED_B3: a.w = P(w.packed); a.wb3 = P(w.packed_b3s); a.math = pmath(); break;
    case STAGED_F16X2: a.w = P(w.packed); a.wb3 = P(w.packed_h2s); a.math = MATH_F16X2; break;  // two fp16 terms per operand
    case MFMA_F32: a.w = P(w.packed); a.math = MATH_F32; break;
    case GENERIC: a.w = P(w.raw); break;
    }
    if (kernel == UPS_PL) launch_ups_pl(a, stream_);
    else if (kernel == RB_CONV) launch_rb_conv(a, stream_);
    else if (kernel == ENC_B3) launch_enc_conv_b3(a, stream_);
    else if (kernel == GENERIC) launch_conv1d_generic(a, stream_);
    else launch_conv1d_mfma(a, stream_);
}

// a named buffer for the copy of an intermediate, or null: taps are off, or the name is taken (the first tap of a name stays)
Tap* Engine::new_tap(const char* name, std::initializer_list<int64_t> dims) {
    if (!taps_on_) return nullptr;
    for (auto& t : taps_)
        if (t.name == name) return nullptr;
    Tap t;
    t.name = name;
    t.dims.assign(dims.begin(), dims.end());
    t.count = 1;
    for (auto d : dims) t.count *= (size_t)d;
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, t.count * sizeof(float) + 16));
    t.dev = static_cast<float*>(p);
    taps_.push_back(std::move(t));
    return &taps_.back();
}

void Engine::tap(const char* name, const float* dev, std::initializer_list<int64_t> dims, const int* row_len, int factor) {
    Tap* t = new_tap(name, dims);
    if (!t) return;
    HIP_CHECK(hipMemcpyAsync(t->dev, dev, t->count * sizeof(float), hipMemcpyDeviceToDevice, stream_));
    if (row_len && t->dims.size() == 3) launch_zero_row_tails(t->dev, (int)t->dims[0], (int)t->dims[1], (long)t->dims[2], row_len, factor, stream_);
}

// an int32 array as floats for the tap interface (w_ceil): through the host, with copies that synchronise
void Engine::tap_ints(const char* name, const int* dev, std::initializer_list<int64_t> dims) {
    Tap* t = new_tap(name, dims);
    if (!t) return;
    std::vector<int> v(t->count);
    HIP_CHECK(hipMemcpy(v.data(), dev, t->count * 4, hipMemcpyDeviceToHost));
    const std::vector<float> f32(v.begin(), v.end());
    HIP_CHECK(hipMemcpy(t->dev, f32.data(), t->count * 4, hipMemcpyHostToDevice));
}

// rows [row0, row0 + nrows) of the leading (batch) extent; nrows < 0: all rows (a batch-256 stage tap is 6.4 GB: the tests fetch the rows they check)
long Engine::get_tap(const std::string& name, float* out, size_t cap, int64_t dims[4], long row0, long nrows) {
    for (auto& t : taps_)
        if (t.name == name) {
            for (int i = 0; i < 4; ++i) dims[i] = i < (int)t.dims.size() ? t.dims[i] : 1;
            const long rows = t.dims.empty() ? 1 : (long)t.dims[0];
            if (nrows < 0) { row0 = 0; nrows = rows; }
            if (row0 < 0 || nrows < 0 || row0 + nrows > rows) throw EngineError(MI355VITS_ERR_INVALID, "tap rows out of range");
            const size_t per_row = rows > 0 ? t.count / (size_t)rows : 0, cnt = per_row * (size_t)nrows;
            dims[0] = nrows;
            if (out) {
                if (cap < cnt) throw EngineError(MI355VITS_ERR_INVALID, "tap buffer too small");
                HIP_CHECK(hipStreamSynchronize(stream_));
                if (cnt) HIP_CHECK(hipMemcpy(out, t.dev + per_row * (size_t)row0, cnt * sizeof(float), hipMemcpyDeviceToHost));
            }
            return (long)cnt;
        }
    throw EngineError(MI355VITS_ERR_INVALID, "no such tap: " + name);
}
std::string Engine::list_taps() const {
    std::string s;
    for (auto& t : taps_) s += t.name + "\n";
    return s;
}

float Engine::last_run_ms() {
    if (!end_recorded_) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ev_start_, ev_end_) != hipSuccess) return -1.0f;
    return ms;
}

// =================================================================================================
// K1-K4 text encoder
// =================================================================================================
void Engine::text_encoder(int B, int Tx) {
    const mi355vits_config& c = cfg_;
    const int H = c.hidden_channels, F = c.filter_channels, I = c.inter_channels;
    const long xbs = (long)H * Tx;
    {
        ProfScope ps(prof_, "embed", 0, 4.0 * B * H * Tx);
        launch_embed(d_ids_, d_len_, vec("enc_p.emb.weight"), B, Tx, H, c.num_symbols, sqrtf((float)H), d_x_, stream_);
    }
    for (int i = 0; i < c.n_layers; ++i) {
        const std::string a = S("enc_p.encoder.attn_layers.%d", i);
        ConvArgs q;
        q.x = d_x_; q.x_bs = xbs; q.x_ld = Tx;
        q.y = d_qkv_; q.y_bs = 3 * xbs; q.y_ld = Tx;
        q.B = B; q.T = Tx;
        conv("enc.qkv", cw(S("enc.%d.qkv", i)), q);
        if (Tx > rel_attention_valu_cap(H, c.n_heads, c.window_size)) {
            // beyond the VALU kernel's LDS row buffer: keys streamed (lengths up to the cap keep their kernels and bits)
            const double fl = 4.0 * B * (double)Tx * Tx * H;
            ProfScope ps(prof_, "enc.attention.stream", fl, 4.0 * B * 4 * H * Tx);
            launch_rel_attention_stream(d_qkv_, vec(a + ".emb_rel_k"), vec(a + ".emb_rel_v"), d_len_, B, Tx, H, c.n_heads,
                                        c.window_size, d_att_, stream_);
        } else {
            const double fl = 4.0 * B * (double)Tx * Tx * H;
            ProfScope ps(prof_, "enc.attention", fl, 4.0 * B * 4 * H * Tx);
            if (!sw_.force_generic && rel_attention_mfma_supported(Tx, H, c.n_heads, c.window_size))
                launch_rel_attention_mfma(d_qkv_, vec(a + ".emb_rel_k"), vec(a + ".emb_rel_v"), d_len_, B, Tx, H, c.n_heads,
                                          c.window_size, d_att_, stream_);
            else
                launch_rel_attention(d_qkv_, vec(a + ".emb_rel_k"), vec(a + ".emb_rel_v"), d_len_, B, Tx, H, c.n_heads,
                                     c.window_size, d_att_, stream_);
        }
        ConvArgs o;
        o.x = d_att_; o.x_bs = xbs; o.x_ld = Tx;
        o.y = d_x2_; o.y_bs = xbs; o.y_ld = Tx;
        o.res = d_x_; o.res_bs = xbs; o.res_ld = Tx;
        o.B = B; o.T = Tx;
        const ConvW& wo = cw(S("enc.%d.o", i));
        fill_conv(wo, o);
        if (pick_conv(wo, o) == ENC_B3 && !sw_.no_enc_o_ln && enc_o_ln_supported(wo.Cin, wo.Cout, wo.K)) {
            // o-proj + residual + LayerNorm in one launch, in place on x (k_enc_o_ln)
            o.y = d_x_;
            o.wb3 = P(wo.packed_b3s);
            o.math = tmath();
            ProfScope ps(prof_, "enc.o_ln", 2.0 * B * (double)Tx * H * H, 4.0 * B * 3 * H * Tx);
            launch_enc_o_ln(o, vec(S("enc_p.encoder.norm_layers_1.%d.gamma", i)), vec(S("enc_p.encoder.norm_layers_1.%d.beta", i)), nullptr,
                            1e-5f, stream_);
        } else {
            conv("enc.o", wo, o);
            LNArgs ln;
            ln.x = d_x2_; ln.y = d_x_; ln.B = B; ln.C = H; ln.T = Tx;
            ln.gamma = vec(S("enc_p.encoder.norm_layers_1.%d.gamma", i));
            ln.beta = vec(S("enc_p.encoder.norm_layers_1.%d.beta", i));
            ProfScope ps(prof_, "layernorm", 0, 8.0 * B * H * Tx);
            launch_layernorm(ln, stream_);
        }
        ConvArgs f1;
        f1.x = d_x_; f1.x_bs = xbs; f1.x_ld = Tx;
        f1.y = d_ffn_; f1.y_bs = (long)F * Tx; f1.y_ld = Tx;
        f1.in_len = d_len_; f1.relu = 1;
        f1.B = B; f1.T = Tx;
        conv("enc.ffn1", cw(S("enc.%d.ffn1", i)), f1);
        ConvArgs f2;
        f2.x = d_ffn_; f2.x_bs = (long)F * Tx; f2.x_ld = Tx;
        f2.y = d_x2_; f2.y_bs = xbs; f2.y_ld = Tx;
        f2.in_len = d_len_; f2.out_len = d_len_; f2.mask_before_res = 1;
        f2.res = d_x_; f2.res_bs = xbs; f2.res_ld = Tx;
        f2.B = B; f2.T = Tx;
        const ConvW& w2 = cw(S("enc.%d.ffn2", i));
        bool split2 = false;  // conv_2 as 192-channel slices: raw sums, added up by the LayerNorm launch below
        if (d_part_ && w2.Cout == H && enc_conv_b3_slices(w2.Cin) > 1 && enc_conv_b3_slices(w2.Cin) * 192 == F) {
            f2.ksplit = enc_conv_b3_slices(w2.Cin);
            f2.part = d_part_;
            fill_conv(w2, f2);
            split2 = pick_conv(w2, f2) == ENC_B3;
            if (!split2) { f2.ksplit = 1; f2.part = nullptr; }
        }
        conv("enc.ffn2", w2, f2);
        {
            LNArgs ln;
            ln.x = d_x2_; ln.y = d_x_; ln.B = B; ln.C = H; ln.T = Tx;
            if (split2) {
                ln.x = d_part_; ln.nparts = f2.ksplit; ln.part_stride = (long)B * xbs;
                ln.bias = P(w2.bias); ln.premask_len = d_len_;
                ln.res = d_x_;
            }
            ln.gamma = vec(S("enc_p.encoder.norm_layers_2.%d.gamma", i));
            ln.beta = vec(S("enc_p.encoder.norm_layers_2.%d.beta", i));
            if (i == c.n_layers - 1) ln.out_len = d_len_;  // x = x * x_mask after the last layer
            ProfScope ps(prof_, "layernorm", 0, 8.0 * B * H * Tx);
            launch_layernorm(ln, stream_);
        }
    }
    tap("x", d_x_, {B, H, Tx});
    ConvArgs p;
    p.x = d_x_; p.x_bs = xbs; p.x_ld = Tx;
    p.y = d_stats_; p.y_bs = 2L * I * Tx; p.y_ld = Tx;
    p.out_len = d_len_;
    p.B = B; p.T = Tx;
    conv("enc.proj", cw("enc.proj"), p);
    tap("stats", d_stats_, {B, 2 * I, Tx});
}

// =================================================================================================
// K5 stochastic duration predictor (reverse) + K6 durations
// =================================================================================================
void Engine::dds(const std::string& key, float* X, float* Y1, float* Y2, int B, int T) {
    const mi355vits_config& c = cfg_;
    const int C = c.hidden_channels;
    const long bs = (long)C * T;
    int dil = 1;
    if (!sw_.force_generic && !sw_.no_fused_dds && c.dp_dds_layers >= 2 && dds_layer_fused_supported(C) &&
        cw(key + S(".convs_1x1.%d", 0)).packed != NO_OFF) {
        // one launch per layer; x ping-pongs through the scratch buffers and the last layer lands in X again
        const float* src = X;
        for (int i = 0; i < c.dp_dds_layers; ++i) {
            float* dst = (i == c.dp_dds_layers - 1) ? X : ((i & 1) ? Y2 : Y1);
            const ConvW& w = cw(key + S(".convs_1x1.%d", i));
            ProfScope ps(prof_, "dds.layer", 2.0 * B * (double)T * C * C, 8.0 * B * C * T);
            launch_dds_layer(src, dst, vec(key + S(".convs_sep.%d.weight", i)), vec(key + S(".convs_sep.%d.bias", i)),
                             vec(key + S(".norms_1.%d.gamma", i)), vec(key + S(".norms_1.%d.beta", i)), P(w.packed), P(w.bias),
                             vec(key + S(".norms_2.%d.gamma", i)), vec(key + S(".norms_2.%d.beta", i)), d_len_, B, C, T,
                             c.dp_kernel_size, dil, stream_);
            src = dst;
            dil *= c.dp_kernel_size;
        }
        return;
    }
    for (int i = 0; i < c.dp_dds_layers; ++i) {
        {
            ProfScope ps(prof_, "dds.dwconv_ln_gelu", 0, 8.0 * B * C * T);
            launch_dds_dwconv_ln_gelu(X, vec(key + S(".convs_sep.%d.weight", i)), vec(key + S(".convs_sep.%d.bias", i)),
                                      vec(key + S(".norms_1.%d.gamma", i)), vec(key + S(".norms_1.%d.beta", i)), d_len_,
                                      B, C, T, c.dp_kernel_size, dil, Y1, stream_);
        }
        ConvArgs a;
        a.x = Y1; a.x_bs = bs; a.x_ld = T;
        a.y = Y2; a.y_bs = bs; a.y_ld = T;
        a.B = B; a.T = T;
        conv("dds.1x1", cw(key + S(".convs_1x1.%d", i)), a);
        {
            LNArgs ln;
            ln.x = Y2; ln.y = X; ln.add_to = X; ln.gelu = 1;
            ln.B = B; ln.C = C; ln.T = T;
            ln.gamma = vec(key + S(".norms_2.%d.gamma", i));
            ln.beta = vec(key + S(".norms_2.%d.beta", i));
            ProfScope ps(prof_, "layernorm", 0, 12.0 * B * C * T);
            launch_layernorm(ln, stream_);
        }
        dil *= c.dp_kernel_size;
    }
}

// deterministic predictor (dp_n_flows == 0): k_dp_det writes logw into channel 0 of z2, and k_durations reads it back through an
// identity ElementwiseAffine ((z - 0) * expf(-0) * m: exact).  noise_w is not used, as in upstream VITS.
void Engine::duration_predictor_det(const RunInputs& in) {
    const mi355vits_config& c = cfg_;
    const int B = in.B, Tx = in.Tx, H = c.hidden_channels, DF = model_->dp_filter, K = c.dp_kernel_size;
    DpDetArgs a;
    a.x = d_x_;
    a.cond = d_cond_dp_;
    a.cond_bs = H;
    const bool f32 = tmath() == MATH_F32;  // every other mode: the exact three-term split (durations must not move)
    auto wt = [&](const ConvW& w) { return P(f32 ? w.packed : w.packed_b3s); };
    const ConvW& c1 = cw("dp.conv_1");
    const ConvW& c2 = cw("dp.conv_2");
    if ((f32 ? c1.packed : c1.packed_b3s) == NO_OFF || (f32 ? c2.packed : c2.packed_b3s) == NO_OFF)
        throw EngineError(MI355VITS_ERR_INTERNAL, "dp.det: conv without packed weights");
    a.w1 = wt(c1); a.b1 = P(c1.bias); a.g1 = vec("dp.norm_1.gamma"); a.be1 = vec("dp.norm_1.beta");
    a.w2 = wt(c2); a.b2 = P(c2.bias); a.g2 = vec("dp.norm_2.gamma"); a.be2 = vec("dp.norm_2.beta");
    a.pw = vec("dp.proj.weight");
    a.pb = vec("dp.proj.bias");
    a.len = d_len_;
    a.out = d_z2_;
    a.out_bs = 2L * Tx;
    a.B = B; a.T = Tx; a.H = H; a.F = DF; a.K = K;
    a.math = f32 ? (int)MATH_F32 : (int)MATH_BF16X3;
    {
        const double flops = 2.0 * B * (double)Tx * ((double)K * H * DF + (double)K * DF * DF + DF);
        ProfScope ps(prof_, "dp.det", flops, 4.0 * B * (double)Tx * (H + 1));
        launch_dp_det(a, stream_);
    }
    durations(in, 0, 0.0f, 0.0f);
}

// The durations of both predictors: k_durations, or in a timed run k_durations_timed IN ITS PLACE (the same EA^-1 and logw, then
// the fit: kernels_timing.cpp), which also leaves status and factor of every row right behind d_ylen_.
void Engine::durations(const RunInputs& in, int ch, float ea_m, float ea_logs) {
    const int B = in.B, Tx = in.Tx;
    if (!in.timed()) {
        ProfScope ps(prof_, "durations");
        launch_durations(d_z2_, ch, ea_m, ea_logs, d_len_, d_forced_, B, Tx, d_scales_, d_logw_, d_wceil_, d_cum_, d_ylen_, stream_);
    } else {
        DurTimedArgs a;
        a.z = d_z2_; a.ch = ch; a.ea_m = ea_m; a.ea_logs = ea_logs;
        a.len = d_len_; a.B = B; a.T = Tx;
        a.scales = d_scales_;
        a.stretch = d_stretch_; a.min_frames = d_minf_; a.target = d_target_;
        a.logw = d_logw_; a.u = d_durf_;
        a.w_ceil = d_wceil_; a.cum = d_cum_; a.ylen = d_ylen_;
        a.factor = d_tfactor_; a.status = d_tstatus_;
        ProfScope ps(prof_, "durations.timed");
        launch_durations_timed(a, stream_);
    }
    tap("logw", d_logw_, {B, 1, Tx});
    if (in.timed()) tap("dur_float", d_durf_, {B, 1, Tx});
}

void Engine::duration_predictor(const RunInputs& in) {
    if (model_->dp_filter) {
        duration_predictor_det(in);
        return;
    }
    const mi355vits_config& c = cfg_;
    const int B = in.B, Tx = in.Tx, H = c.hidden_channels;
    const long bs = (long)H * Tx;
    const int nth = 3 * c.dp_num_bins - 1;
    // the whole stack in one launch each (k_dds_stack): pre + DDS layers + proj, and for a ConvFlow the spline too
    const bool stack = !sw_.force_generic && !sw_.no_fused_dds && !sw_.no_dds_stack &&
                       dds_stack_supported(H, c.dp_kernel_size, c.dp_dds_layers, H) && nth <= H && c.dp_num_bins <= 16 &&
                       cw("dp.pre").packed != NO_OFF && cw("dp.proj").packed != NO_OFF && cw("dp.pre").packed_b3s != NO_OFF &&
                       cw("dp.proj").packed_b3s != NO_OFF;
    // the stack's 1x1 convs: bf16 planes in the split-bf16 math modes (k_dds_stack_b3), f32 A fragments in MATH_F32
    const bool stack_b3 = math_on_bf16(tmath()) && !sw_.no_dds_stack_b3;
    auto stack_w = [&](const ConvW& w) -> const float* {
        const size_t off = stack_b3 ? w.packed_b3s : w.packed;
        return off == NO_OFF ? nullptr : P(off);
    };
    auto stack_layers = [&](DdsStackArgs& a, const std::string& key) {
        a.math = stack_b3 ? tmath() : (int)MATH_F32;  // exact in MATH_BF16W too: durations must not move
        a.n_layers = c.dp_dds_layers;
        a.K = c.dp_kernel_size;
        for (int i = 0; i < c.dp_dds_layers; ++i) {
            const ConvW& w = cw(key + S(".convs_1x1.%d", i));
            if (stack_w(w) == nullptr) throw EngineError(MI355VITS_ERR_INTERNAL, "dds stack: 1x1 conv without packed weights");
            a.dw_w[i] = vec(key + S(".convs_sep.%d.weight", i));
            a.dw_b[i] = vec(key + S(".convs_sep.%d.bias", i));
            a.g1[i] = vec(key + S(".norms_1.%d.gamma", i));
            a.b1[i] = vec(key + S(".norms_1.%d.beta", i));
            a.w1x1[i] = stack_w(w);
            a.bias1x1[i] = P(w.bias);
            a.g2[i] = vec(key + S(".norms_2.%d.gamma", i));
            a.b2[i] = vec(key + S(".norms_2.%d.beta", i));
        }
        a.len = d_len_;
        a.B = B;
        a.T = Tx;
    };
    const double stack_flops = 2.0 * B * (double)Tx * H * H;
    if (stack) {
        DdsStackArgs a;
        a.src = d_x_;
        a.pre_mode = DDS_PRE_CONV;
        a.pre_w = stack_w(cw("dp.pre"));
        a.pre_b = P(cw("dp.pre").bias);
        a.cond = d_cond_dp_;
        a.cond_bs = H;
        stack_layers(a, "dp.convs");
        a.proj_w = stack_w(cw("dp.proj"));
        a.proj_b = P(cw("dp.proj").bias);
        a.proj_cout = H;
        a.out = d_h_;
        ProfScope ps(prof_, "dp.stack", stack_flops * (c.dp_dds_layers + 2), 8.0 * B * H * Tx);
        launch_dds_stack(a, H, stream_);
    }
    // h = proj(DDS(pre(x) [+ cond(g)])) * mask
    ConvArgs pre;
    pre.x = d_x_; pre.x_bs = bs; pre.x_ld = Tx;
    pre.y = d_d0_; pre.y_bs = bs; pre.y_ld = Tx;
    pre.cond = d_cond_dp_; pre.cond_bs = H;
    pre.B = B; pre.T = Tx;
    if (!stack) {
        conv("dp.pre", cw("dp.pre"), pre);
        dds("dp.convs", d_d0_, d_d1_, d_d2_, B, Tx);
    }
    ConvArgs pr;
    pr.x = d_d0_; pr.x_bs = bs; pr.x_ld = Tx;
    pr.y = d_h_; pr.y_bs = bs; pr.y_ld = Tx;
    pr.in_len = d_len_; pr.out_len = d_len_;
    pr.B = B; pr.T = Tx;
    if (!stack) conv("dp.proj", cw("dp.proj"), pr);
    tap("dp.h", d_h_, {B, H, Tx});

    {
        ProfScope ps(prof_, "sdp.noise");
        launch_sdp_noise(d_z2_, d_noise_w_, B, Tx, d_scales_, in.seed, d_utt_, stream_);
    }
    int ch0 = 0;  // physical channel that is logical channel 0
    for (int j = c.dp_n_flows - 1; j >= 1; --j) {
        ch0 ^= 1;  // Flip
        const std::string p = S("dp.flows.%d", 1 + 2 * j);
        if (stack && stack_w(cw(p + ".proj")) != nullptr) {
            DdsStackArgs a;
            a.src = d_h_;
            a.pre_mode = DDS_PRE_AFFINE;
            a.pre_w = vec(p + ".pre.weight");
            a.pre_b = vec(p + ".pre.bias");
            a.z = d_z2_;
            a.zch = ch0;
            stack_layers(a, p + ".convs");
            a.proj_w = stack_w(cw(p + ".proj"));
            a.proj_b = P(cw(p + ".proj").bias);
            a.proj_cout = nth;
            a.spline = 1;
            a.nb = c.dp_num_bins;
            a.tail = c.dp_tail_bound;
            a.inv_sqrt_fc = 1.0f / sqrtf((float)H);
            ProfScope ps(prof_, "convflow.stack", stack_flops * c.dp_dds_layers + 2.0 * B * (double)Tx * H * nth, 12.0 * B * H * Tx);
            launch_dds_stack(a, H, stream_);
            continue;
        }
        {
            ProfScope ps(prof_, "convflow.pre", 0, 12.0 * B * H * Tx);
            launch_convflow_pre(d_z2_, ch0, vec(p + ".pre.weight"), vec(p + ".pre.bias"), d_h_, B, H, Tx, d_d0_, stream_);
        }
        dds(p + ".convs", d_d0_, d_d1_, d_d2_, B, Tx);
        ConvArgs a;
        a.x = d_d0_; a.x_bs = bs; a.x_ld = Tx;
        a.y = d_theta_; a.y_bs = (long)nth * Tx; a.y_ld = Tx;
        a.in_len = d_len_; a.out_len = d_len_;
        a.B = B; a.T = Tx;
        conv("convflow.proj", cw(p + ".proj"), a);
        {
            ProfScope ps(prof_, "spline");
            launch_spline_inverse(d_z2_, ch0, d_theta_, d_len_, B, Tx, c.dp_num_bins, c.dp_tail_bound,
                                  1.0f / sqrtf((float)H), stream_);
        }
    }
    ch0 ^= 1;  // Flip before the ElementwiseAffine
    durations(in, ch0, model_->ea_m[0], model_->ea_logs[0]);  // logical channel 0 uses EA parameters [0]
}

// =================================================================================================
// K6/K7 expand + K8 flow^-1 + K9-K12 decoder
// =================================================================================================
// stage i's profile label out of {stage 0, 1, 2, later}: tests and bench.py key their kernel tables by these strings
static const char* stage_label(int i, const char* const (&t)[4]) { return t[std::min(i, 3)]; }

// one residual coupling layer, inverted: x1 = (x1 - post(WN(pre(x0)))) * mask
void Engine::coupling_layer(int j, int B, int Ty) {
    const mi355vits_config& c = cfg_;
    const int H = c.hidden_channels, I = c.inter_channels, half = I / 2;
    const long zbs = (long)I * Ty, hbs = (long)H * Ty;
    const bool rev = ((c.flow_n_flows - 1 - j) % 2) == 0;
    float* x0 = d_z_ + (rev ? (long)half * Ty : 0);
    float* x1 = d_z_ + (rev ? 0 : (long)half * Ty);
    ConvArgs pre;
    pre.x = x0; pre.x_bs = zbs; pre.x_ld = Ty;
    pre.y = d_fh_; pre.y_bs = hbs; pre.y_ld = Ty;
    pre.out_len = d_ylen_;
    pre.B = B; pre.T = Ty;
    conv("flow.pre", cw(S("flow.%d.pre", j)), pre);
    float* hcur = d_fh_;
    float* hnext = d_fh2_;
    for (int l = 0; l < c.flow_wn_layers; ++l) {
        int dil = 1;
        for (int q = 0; q < l; ++q) dil *= c.flow_wn_dilation_rate;
        const ConvW& win = cw(S("flow.%d.in.%d", j, l));
        const ConvW& wrs = cw(S("flow.%d.rs.%d", j, l));
        const float* cond_l = d_cond_flow_.empty() ? nullptr : d_cond_flow_[j] + (long)l * 2 * H;
        // in-layer + res/skip through the staged split-bf16 kernel (two launches, `u` through HBM: 38 MB per layer, nothing next
        // to the matrix-core time saved) instead of a fused layer: measured 2.09 + 1.70 ms vs 3.65 ms per step for the fused f32
        // layer — no gain (small grids, scalar res/skip epilogue); opt-in for A/B and for the tests
        const bool wn_b3 = sw_.wn_b3 && math_on_bf16(kmath()) && win.packed_b3s != NO_OFF && wrs.packed_b3s != NO_OFF &&
                           conv1d_b3_supported(win.Cin, win.Cout, win.K, dil, Ty) && !sw_.force_generic;
        const bool fused = !sw_.force_generic && !sw_.no_fused_wn && !wn_b3;
        // fused layer on the bf16 matrix cores (k_wn_layer_b3), else on the f32 ones (k_wn_layer).  Chosen by the layer shape
        // alone (never by the grid size), so a row's bits do not depend on what it is batched with.
        const int wn_shape = wn_layer_b3_shape();  // 16; the lab build's A/B switch: 32
        const bool b3 = fused && math_on_bf16(kmath()) && wn_layer_b3_supported(H, win.K, dil) &&
                        (wn_shape == 32 ? win.packed_b3w != NO_OFF && wrs.packed_b3s != NO_OFF : win.packed_w16 != NO_OFF && wrs.packed_w16 != NO_OFF);
        if (b3 || (fused && wn_layer_fused_supported(H, win.K, dil))) {
            const bool h2 = b3 && math_ == MATH_F16X2 && win.packed_h2s != NO_OFF && wrs.packed_h2s != NO_OFF;  // two fp16 terms per operand
            WnArgs w;
            w.h_in = hcur; w.h_out = hnext; w.h_bs = hbs; w.h_ld = Ty;
            w.skip = d_fskip_; w.s_bs = hbs; w.s_ld = Ty;
            const bool s16 = b3 && !h2 && wn_shape != 32;
            w.w_in = P(h2 ? win.packed_h2s : (s16 ? win.packed_w16 : (b3 ? win.packed_b3w : win.packed))); w.b_in = P(win.bias);
            w.w_rs = P(h2 ? wrs.packed_h2s : (s16 ? wrs.packed_w16 : (b3 ? wrs.packed_b3s : wrs.packed))); w.b_rs = P(wrs.bias);
            w.shape = s16 ? 16 : 32;
            w.cond = cond_l; w.cond_bs = 2L * H * c.flow_wn_layers;
            w.len = d_ylen_;
            w.B = B; w.H = H; w.T = Ty; w.K = win.K; w.dil = dil; w.Crs = wrs.Cout; w.skip_init = (l == 0);
            if (b3) w.math = h2 ? (int)MATH_F16X2 : kmath();
            const double fl = 2.0 * B * (double)Ty * H * ((double)win.Cout * win.K + wrs.Cout);
            ProfScope ps(prof_, b3 ? "flow.wn_layer_b3" : "flow.wn_layer", fl, 4.0 * B * (double)Ty * H * 4);
            if (b3) launch_wn_layer_b3(w, stream_);
            else launch_wn_layer(w, stream_);
            if (wrs.Cout == 2 * H) std::swap(hcur, hnext);  // the last layer leaves h untouched
            continue;
        }
        ConvArgs in;
        in.x = hcur; in.x_bs = hbs; in.x_ld = Ty;
        in.y = d_fu_; in.y_bs = hbs; in.y_ld = Ty;
        in.epi = EPI_GATE; in.H = H; in.dil = dil;
        if (cond_l) {
            in.cond = cond_l;
            in.cond_bs = 2L * H * c.flow_wn_layers;
        }
        in.B = B; in.T = Ty;
        if (wn_b3) in.math = kmath();
        conv("flow.in_gate", win, in);
        ConvArgs rs;
        rs.x = d_fu_; rs.x_bs = hbs; rs.x_ld = Ty;
        rs.y = hcur; rs.y_bs = hbs; rs.y_ld = Ty;
        rs.y2 = d_fskip_; rs.y2_bs = hbs; rs.y2_ld = Ty;
        rs.epi = EPI_RESSKIP; rs.H = H; rs.skip_init = (l == 0);
        rs.out_len = d_ylen_;
        rs.B = B; rs.T = Ty;
        if (wn_b3) rs.math = kmath();
        conv("flow.res_skip", wrs, rs);
    }
    ConvArgs post;
    post.x = d_fskip_; post.x_bs = hbs; post.x_ld = Ty;
    post.y = x1; post.y_bs = zbs; post.y_ld = Ty;
    post.res = x1; post.res_bs = zbs; post.res_ld = Ty; post.res_sub = 1;
    post.in_len = d_ylen_; post.out_len = d_ylen_;
    post.B = B; post.T = Ty;
    conv("flow.post_couple", cw(S("flow.%d.post", j)), post);
}

// conv m of ResBlock2 j in stage i, conv by conv: x = x + conv_{k,d}(lrelu(x)), from bufA through bufB / bufT, the block's last
// conv scaled and accumulated onto the stage output bufC
ConvArgs Engine::rb2_conv_args(int i, int j, int m, int B, int ch, long T) const {
    const mi355vits_config& c = cfg_;
    float* const pp[2] = {d_bufB_, d_bufT_};
    const bool last = (m == c.resblock_n_dilations[j] - 1);
    const float* src = m == 0 ? d_bufA_ : pp[(m - 1) & 1];
    ConvArgs a;
    a.x = src; a.x_bs = (long)ch * T; a.x_ld = (int)T;
    a.y = last ? d_bufC_ : pp[m & 1]; a.y_bs = (long)ch * T; a.y_ld = (int)T;
    a.res = src; a.res_bs = (long)ch * T; a.res_ld = (int)T;
    a.in_slope = 0.1f; a.dil = c.resblock_dilations[j * MI355VITS_MAX_STAGES + m];
    a.in_len = d_slen_ + (long)(i + 1) * B;  // rows end at their own length (batched == unbatched)
    if (last) { a.out_scale = 1.0f / c.n_resblock_kernels; a.accumulate = (j > 0); }
    a.B = B; a.T = (int)T;
    return a;
}

// ResBlock2 stages: the leading resblocks of stage i (input bufA [B,ch,T], output bufC) in one launch where a fused kernel takes
// them.  Returns how many it took; decoder_stage runs the rest conv by conv.
int Engine::mrf_stage(int i, int B, int ch, long T) {
    const mi355vits_config& c = cfg_;
    const int nk = c.n_resblock_kernels;
    if (sw_.force_generic || sw_.no_fused_mrf || c.resblock != 2 || nk > MRF_MAX_RB) return 0;
    MrfArgs m;
    for (int j = 0; j < nk; ++j) {
        if (c.resblock_n_dilations[j] != 2) return 0;
        m.k[j] = c.resblock_kernel_sizes[j];
        m.d1[j] = c.resblock_dilations[j * MI355VITS_MAX_STAGES + 0];
        m.d2[j] = c.resblock_dilations[j * MI355VITS_MAX_STAGES + 1];
    }
    m.x = d_bufA_; m.x_bs = (long)ch * T; m.x_ld = (int)T;
    m.y = d_bufC_; m.y_bs = (long)ch * T; m.y_ld = (int)T;
    m.len = d_slen_ + (long)(i + 1) * B; m.B = B; m.C = ch; m.T = (int)T;
    m.len_host = h_slen_.data() + (size_t)(i + 1) * B;
    auto rb = [&](int j, int q) -> const ConvW& { return cw(S("dec.rb.%d.c.%d", i * nk + j, q)); };
    // resblocks 0 .. n - 1 with their weights in format fmt, and their flops; false if a conv has no such copy
    double flops = 0;
    auto take = [&](int n, size_t ConvW::*fmt) {
        flops = 0;
        for (int j = 0; j < n; ++j) {
            for (int q = 0; q < 2; ++q) {
                const ConvW& w = rb(j, q);
                if (w.*fmt == NO_OFF) return false;
                m.w[j][q] = P(w.*fmt);
                m.bias[j][q] = P(w.bias);
            }
            flops += 2.0 * 2.0 * B * (double)T * ch * ch * m.k[j];
        }
        m.nrb = n;
        return true;
    };
    const double bytes = 8.0 * B * (double)T * ch;
    // MATH_BF16X3: the whole stage on planes split once, weights in registers (k_mrf_p)
    if (math_ == MATH_BF16X3 && !sw_.no_mrf_p && mrf_p_supported(ch, nk, m.k, m.d1, m.d2) && take(nk, &ConvW::packed_p)) {
        m.math = MATH_BF16X3;
        // large grids: the row sweep (k_mrf_s: fragments register-resident per segment, no halo recompute); small ones:
        // (row, column block) items (k_mrf_p).  The two agree bit for bit, so the choice may follow the grid.
        // 64 channels: one pass per resblock (k_mrf_s).  32 channels: k_mrf_p (its single-pass sweep, k_mrf_s1, measured equal in
        // round 4 — 2.33 vs 2.34 ms, 2.37 vs 2.36 with 48-column steps — and was deleted in round 5: DESIGN.md §6)
        const bool sw_ok = ch != 32 && mrf_s_supported(ch, nk, m.k, m.d1, m.d2);
        int seg = !sw_ok ? 0 : mrf_s_segment(ch, B, (int)T, current_device_cu_count(), m.len_host);
        if (const char* f = lab_getenv("MI355VITS_MRF_SWEEP_SEG")) seg = sw_ok ? atoi(f) : 0;  // lab / tests (read per call)
        if (seg > 0) {
            m.seg = seg;
            ProfScope ps(prof_, stage_label(i, {"dec.mrf_s", "dec.mrf_s.s1", "dec.mrf_s.s2", "dec.mrf_s"}), flops, bytes);
            launch_mrf_s(m, stream_);
        } else {
            ProfScope ps(prof_, stage_label(i, {"dec.mrf_p", "dec.mrf_p.s1", "dec.mrf_p.s2", "dec.mrf_p"}), flops, bytes);
            launch_mrf_p(m, stream_);
        }
        return nk;
    }
    // 128 channels in MATH_BF16X3: conv by conv on k_rb_conv (every input channel resident in LDS, kernels_rbc.cpp)
    bool rbc_stage = true;
    for (int j = 0; j < nk && rbc_stage; ++j)
        for (int q = 0; q < 2 && rbc_stage; ++q) {
            const ConvW& w = rb(j, q);
            ConvArgs a = rb2_conv_args(i, j, q, B, ch, T);  // what decoder_stage launches if nothing is fused
            fill_conv(w, a);
            rbc_stage = pick_conv(w, a) == RB_CONV;
        }
    if (rbc_stage) return 0;
    // the longest prefix of resblocks whose tiles fit LDS together (128 channels: only the narrow ones)
    int p = nk;
    while (p > 0 && !(mrf_fused_supported(ch, p, m.k, m.d1, m.d2) && rb(0, 0).packed4 != NO_OFF)) --p;
    if (p == 0) return 0;
    if (math_ == MATH_F16X2 && take(p, &ConvW::packed_h2)) m.math = MATH_F16X2;
    else if (math_on_bf16(kmath()) && take(p, &ConvW::packed_b3)) m.math = kmath();
    else if (take(p, &ConvW::packed4)) m.math = MATH_F32;
    else return 0;
    if (p < nk) m.out_scale = 1.0f / nk;
    ProfScope ps(prof_, stage_label(i, {"dec.mrf_fused.s0", "dec.mrf_fused.s1", "dec.mrf_fused.s2", "dec.mrf_fused"}), flops, bytes);
    launch_mrf_fused(m, stream_);
    return p;
}

void Engine::decoder_stage(int i, int B, int ch, long T) {
    const mi355vits_config& c = cfg_;
    const int r = c.upsample_rates[i], k = c.upsample_kernel_sizes[i], nk = c.n_resblock_kernels;
    const ConvW& up = cw(S("dec.ups.%d.poly", i));
    if (!sw_.force_generic && up.packed != NO_OFF) {
        ConvArgs u;
        u.x = d_bufC_; u.x_bs = (long)ch * T; u.x_ld = (int)T;
        u.y = d_bufA_; u.y_bs = (long)(ch / 2) * T * r; u.y_ld = (int)(T * r);
        u.in_slope = 0.1f; u.in_len = d_slen_ + (long)i * B;
        u.pad = up.K - 1; u.Tin = (int)T;
        u.shuf_s = r; u.shuf_p = (k - r) / 2; u.shuf_cout = ch / 2; u.shuf_T = (int)(T * r);
        u.B = B; u.T = (int)T + up.K - 1;
        conv(stage_label(i, {"dec.upsample.s0", "dec.upsample.s1", "dec.upsample.s2+", "dec.upsample.s2+"}), up, u);
    } else {
        ConvTArgs u;
        u.x = d_bufC_; u.x_bs = (long)ch * T; u.x_ld = (int)T;
        u.y = d_bufA_; u.y_bs = (long)(ch / 2) * T * r; u.y_ld = (int)(T * r);
        u.w = vec(S("dec.ups.%d.weight", i)); u.bias = vec(S("dec.ups.%d.bias", i));
        u.B = B; u.Cin = ch; u.Cout = ch / 2; u.Tin = (int)T; u.K = k; u.stride = r; u.pad = (k - r) / 2;
        u.in_slope = 0.1f;
        u.in_len = d_slen_ + (long)i * B;
        const int taps = (k + r - 1) / r;
        ProfScope ps(prof_, "dec.upsample", 2.0 * B * (double)T * r * ch * (ch / 2) * taps,
                     4.0 * B * ((double)ch * T + (double)(ch / 2) * T * r));
        launch_conv_transpose1d(u, stream_);
    }
    ch /= 2;
    T *= r;
    const long sbs = (long)ch * T;
    const int* slen = d_slen_ + (long)(i + 1) * B;  // rows end at their own length (batched == unbatched)
    tap(S("dec.ups.%d", i).c_str(), d_bufA_, {B, ch, T}, d_ylen_, (int)(T / Ty_));
    // resblocks 0 .. n_fused-1 of this stage run in the fused kernel, the rest conv by conv
    for (int j = mrf_stage(i, B, ch, T); j < nk; ++j) {
        const int n = i * nk + j;
        const int nd = c.resblock_n_dilations[j];
        const float* src = d_bufA_;
        for (int m = 0; m < nd; ++m) {
            if (c.resblock == 2) {
                conv(stage_label(i, {"dec.rb.s0", "dec.rb.s1", "dec.rb.s2+", "dec.rb.s2+"}), cw(S("dec.rb.%d.c.%d", n, m)),
                     rb2_conv_args(i, j, m, B, ch, T));
                continue;
            }
            // xt = c2(lrelu(c1(lrelu(x)))); x = xt + x
            // the pair's output may overwrite its own residual source in place (c2 reads `mid`, and each
            // thread reads res[co,t] before writing y[co,t]); only the stage input bufA must survive.
            const bool last = (m == nd - 1);
            float* mid = d_bufT_;
            float* dst = last ? d_bufC_ : d_bufB_;
            ConvArgs a1;
            a1.x = src; a1.x_bs = sbs; a1.x_ld = (int)T;
            a1.y = mid; a1.y_bs = sbs; a1.y_ld = (int)T;
            a1.in_slope = 0.1f; a1.dil = c.resblock_dilations[j * MI355VITS_MAX_STAGES + m]; a1.in_len = slen;
            a1.B = B; a1.T = (int)T;
            conv("dec.rb1.c1", cw(S("dec.rb.%d.c1.%d", n, m)), a1);
            ConvArgs a2;
            a2.x = mid; a2.x_bs = sbs; a2.x_ld = (int)T;
            a2.y = dst; a2.y_bs = sbs; a2.y_ld = (int)T;
            a2.res = src; a2.res_bs = sbs; a2.res_ld = (int)T;
            a2.in_slope = 0.1f; a2.dil = 1; a2.in_len = slen;
            if (last) { a2.out_scale = 1.0f / nk; a2.accumulate = (j > 0); }
            a2.B = B; a2.T = (int)T;
            conv("dec.rb1.c2", cw(S("dec.rb.%d.c2.%d", n, m)), a2);
            src = dst;
        }
    }
    tap(S("dec.mrf.%d", i).c_str(), d_bufC_, {B, ch, T}, d_ylen_, (int)(T / Ty_));
}

// expand, flows, conv_pre, stages, conv_post
void Engine::flow_and_decoder(const RunInputs& in) {
    struct PhaseB { bool& f; explicit PhaseB(bool& r) : f(r) { f = true; } ~PhaseB() { f = false; } } phase_guard(phase_b_);
    const mi355vits_config& c = cfg_;
    const int B = in.B, Ty = Ty_, I = c.inter_channels, C0 = c.upsample_initial_channel;
    {
        ProfScope ps(prof_, "expand_prior", 0, 4.0 * B * I * Ty * 3);
        launch_expand_prior(d_stats_, d_cum_, d_ylen_, d_noise_z_, in.noise_z_frames, B, I, Tx_, Ty, d_scales_,
                            in.seed, d_utt_, d_z_, stream_);
    }
    tap("z_p", d_z_, {B, I, Ty}, d_ylen_, 1);
    for (int j = c.flow_n_flows - 1; j >= 0; --j) coupling_layer(j, B, Ty);
    tap("z", d_z_, {B, I, Ty}, d_ylen_, 1);

    ConvArgs cp;
    cp.x = d_z_; cp.x_bs = (long)I * Ty; cp.x_ld = Ty;
    cp.y = d_bufC_; cp.y_bs = (long)C0 * Ty; cp.y_ld = Ty;
    cp.in_len = d_ylen_;
    cp.cond = d_cond_dec_; cp.cond_bs = C0;
    cp.B = B; cp.T = Ty;
    conv("dec.conv_pre", cw("dec.conv_pre"), cp);
    tap("dec.conv_pre", d_bufC_, {B, C0, Ty}, d_ylen_, 1);

    int ch = C0;
    long T = Ty;
    HIP_CHECK(hipMemsetAsync(d_peaks_, 0, sizeof(unsigned) * B, stream_));
    for (int i = 0; i < c.n_upsamples; ++i) {
        decoder_stage(i, B, ch, T);
        ch /= 2;
        T *= c.upsample_rates[i];
    }
    {
        ProfScope ps(prof_, "dec.conv_post_tanh", 2.0 * B * (double)T * ch * 7, 4.0 * B * (double)T * (ch + 1));
        launch_conv_post_tanh(d_bufC_, (long)ch * T, (int)T, vec("dec.conv_post.weight"), ch, 7, B, (int)T, d_alen_, d_audio_,
                              T, d_peaks_, stream_);
    }
}

// =================================================================================================
// one synthesis call
// =================================================================================================
// The sequence of alloc calls below IS the workspace layout: a run plays it against an ArenaCount for the size to reserve, then
// against the arena for the pointers.
// Its head is the input block: the call's host inputs sit side by side so that ONE host-to-device copy brings them all (each copy
// from pageable memory is a staging pass + a copy kernel: ~35 us apiece in the stream of a single utterance).  Each input is named
// in ONE `field` line, which says whether it is allocated, where (the order of the lines) and what lands there: h_in_ grows by
// every allocated field — its source where it has one, zeros else, padded as the arena pads — so h_in_ is the block byte for byte
// and h_in_.size() its extent.  widest: the same list with every optional field there, the mix at MI355VITS_MAX_SPEAKER_TERMS
// terms, whatever `in` brings, and nothing copied — what the sizing pass asks: a handle that served a call without them does not
// reallocate when the next call brings them.
template <typename A> void Engine::layout_a(A& ar, const RunInputs& in, bool widest) {
    const mi355vits_config& c = cfg_;
    const size_t B = in.B, Tx = in.Tx, H = c.hidden_channels, F = c.filter_channels, I = c.inter_channels, fBT = B * Tx, gin = c.gin_channels;
    const size_t nth = std::max(3 * c.dp_num_bins - 1, 0);  // 0: the deterministic predictor has no spline parameters
    const bool cond = c.n_speakers > 1 && gin;  // only such a voice takes a speakers run
    // a field is there when the run brings `src`, or `anyway` (then left zero)
    auto field = [&](auto*& dev, size_t n, const void* src, bool anyway) {
        using T = std::remove_reference_t<decltype(*dev)>;
        dev = (src || anyway) ? ar.template alloc<T>(n) : nullptr;
        if (widest || !dev) return;
        const size_t at = h_in_.size();
        h_in_.resize(at + DeviceArena::padded(n * sizeof(T)), 0);
        if (src) memcpy(h_in_.data() + at, src, n * sizeof(T));
    };
    const size_t K = widest ? MI355VITS_MAX_SPEAKER_TERMS : in.spk.n_terms;
    h_in_.clear();
    field(d_ids_, fBT, in.ids, true);
    field(d_sid_, B, in.sid, true);
    field(d_len_, B, in.len32.data(), true);
    field(d_scales_, B * 3, in.sc3.data(), true);
    field(d_vol_, B, in.vol.data(), true);
    field(d_utt_, B, in.utt.data(), true);
    field(d_forced_, fBT, in.forced_durations, widest);
    field(d_noise_w_, fBT * 2, in.noise_w, widest);
    field(d_stretch_, fBT, in.timing.stretch, widest);
    field(d_minf_, fBT, in.timing.min_frames, widest);
    field(d_target_, B, in.timing.target_frames, widest);
    field(d_mix_sid_, B * K, in.spk.mix_sid, widest && cond);
    field(d_mix_w_, B * K, in.spk.mix_weight, widest && cond);
    field(d_spk_vec_, B * gin, in.spk.vectors, widest && cond);
    field(d_gain_, fBT, in.lvl.gain, widest);
    field(d_ramp_, B, in.lvl.ramp_samples, widest || in.levelled());  // a levels run without ramps: zeros
    field(d_ratio_, fBT, in.pit.ratio, widest);
    // what the host reads at the run's one sizing synchronisation: ylen, of a timed run status and factor, and of a pitch run the
    // warped lengths, in ONE copy (4-byte words side by side: each of the four is B words)
    d_ylen_ = ar.template alloc<int>(4 * B);
    d_tstatus_ = d_ylen_ + B;
    d_tfactor_ = reinterpret_cast<float*>(d_ylen_ + 2 * B);
    d_wlen_ = d_ylen_ + 3 * B;
    d_tq_ = ar.template alloc<long long>(fBT);
    d_wc_ = ar.template alloc<int>(fBT);
    d_durf_ = ar.template alloc<float>(fBT);
    d_peaks_ = ar.template alloc<unsigned>(B);
    d_wceil_ = ar.template alloc<int>(fBT);
    d_cum_ = ar.template alloc<int>(fBT);
    d_x_ = ar.template alloc<float>(fBT * H);
    d_x2_ = ar.template alloc<float>(fBT * H);
    d_att_ = ar.template alloc<float>(fBT * H);
    d_qkv_ = ar.template alloc<float>(fBT * 3 * H);
    d_ffn_ = ar.template alloc<float>(fBT * F);
    // slice sums of the FFN's second conv
    d_part_ = (F % 192 == 0 && F / 192 > 1 && H <= 256) ? ar.template alloc<float>(fBT * H * (F / 192)) : nullptr;
    d_stats_ = ar.template alloc<float>(fBT * 2 * I);
    d_h_ = ar.template alloc<float>(fBT * H);
    d_d0_ = ar.template alloc<float>(fBT * H);
    d_d1_ = ar.template alloc<float>(fBT * H);
    d_d2_ = ar.template alloc<float>(fBT * H);
    d_theta_ = ar.template alloc<float>(fBT * nth);
    d_z2_ = ar.template alloc<float>(fBT * 2);
    d_logw_ = ar.template alloc<float>(fBT);
    d_g_ = (cond && (widest || in.speakers != RunInputs::SPK_NONE)) ? ar.template alloc<float>(B * gin) : nullptr;
    d_cond_dp_ = cond ? ar.template alloc<float>(B * H) : nullptr;
    d_cond_dec_ = cond ? ar.template alloc<float>(B * c.upsample_initial_channel) : nullptr;
    d_cond_flow_.clear();
    for (int j = 0; cond && j < c.flow_n_flows; ++j) d_cond_flow_.push_back(ar.template alloc<float>(B * 2 * H * c.flow_wn_layers));
}

template <typename A> void Engine::layout_b(A& ar, size_t B, size_t Ty, size_t noise_z_frames, size_t Lr, size_t Lw) {
    const mi355vits_config& c = cfg_;
    const size_t H = c.hidden_channels, I = c.inter_channels, fBTy = B * Ty;
    size_t ch = c.upsample_initial_channel, T = Ty, max_stage = ch * T;  // the widest decoder tensor of a row
    for (int i = 0; i < c.n_upsamples; ++i) {
        ch /= 2;
        T *= c.upsample_rates[i];
        max_stage = std::max(max_stage, ch * T);
    }
    d_z_ = ar.template alloc<float>(fBTy * I);
    d_fh_ = ar.template alloc<float>(fBTy * H);
    d_fh2_ = ar.template alloc<float>(fBTy * H);
    d_fskip_ = ar.template alloc<float>(fBTy * H);
    d_fu_ = ar.template alloc<float>(fBTy * H);
    d_noise_z_ = noise_z_frames ? ar.template alloc<float>(B * I * noise_z_frames) : nullptr;
    d_bufA_ = ar.template alloc<float>(B * max_stage);
    d_bufB_ = ar.template alloc<float>(B * max_stage);
    d_bufT_ = ar.template alloc<float>(B * max_stage);
    d_bufC_ = ar.template alloc<float>(B * max_stage);
    d_audio_ = ar.template alloc<float>(B * L_);
    d_pcm_ = ar.template alloc<int16_t>(B * (Lr ? Lr : (Lw ? Lw : (size_t)L_)));  // of the rows the caller receives
    d_waudio_ = Lw ? ar.template alloc<float>(B * Lw) : nullptr;  // a pitch run: the warped rows (Lw: their stride)
    d_wpeaks_ = Lw ? ar.template alloc<unsigned>(B) : nullptr;
    d_raudio_ = Lr ? ar.template alloc<float>(B * Lr) : nullptr;
    d_rpeaks_ = Lr ? ar.template alloc<unsigned>(B) : nullptr;
    // per-stage valid lengths and (last row) the audio lengths; a pitch run's table (the warped lengths, k_pitch's first items), then
    // a resampled run's table behind them
    d_slen_ = ar.template alloc<int>((size_t)(c.n_upsamples + 2) * B + (Lw ? pitch_tab_ints((int)B) : 0) + (Lr ? resample_tab_ints((int)B) : 0));
    d_alen_ = d_slen_ + (size_t)(c.n_upsamples + 1) * B;
    d_walen_ = Lw ? d_alen_ + B : nullptr;
    d_rtab_ = Lr ? d_alen_ + B + (Lw ? pitch_tab_ints((int)B) : 0) : nullptr;
}

void Engine::run(const RunCall& call, mi355vits_result* out) {
    if (!out) throw EngineError(MI355VITS_ERR_INVALID, "result pointer is null");
    memset(out, 0, sizeof(*out));
    synthesize(call, nullptr);
    copy_out(call.args.flags, out);
}

void Engine::speaker_embedding(int64_t sid, float* out, size_t capacity) const {
    const mi355vits_config& c = cfg_;
    if (c.n_speakers <= 1 || model_->emb_g.empty()) throw EngineError(MI355VITS_ERR_INVALID, "voice has no speaker embedding");
    if (!out) throw EngineError(MI355VITS_ERR_INVALID, "out must not be null");
    if (sid < 0 || sid >= c.n_speakers)
        throw EngineError(MI355VITS_ERR_INVALID, "speaker id " + std::to_string(sid) + " out of range (the voice has " + std::to_string(c.n_speakers) + " speakers)");
    if (capacity < (size_t)c.gin_channels)
        throw EngineError(MI355VITS_ERR_INVALID, "capacity of " + std::to_string(capacity) + " floats is below gin_channels = " + std::to_string(c.gin_channels));
    memcpy(out, model_->emb_g.data() + (size_t)sid * c.gin_channels, (size_t)c.gin_channels * sizeof(float));
}

// A speakers run's part of check_inputs: in.spk = the caller's struct, in.speakers = which of the two forms it is
static void check_speakers(const mi355vits_config& c, const mi355vits_speaker_args& sp, RunInputs& in) {
    const int B = in.B;
    in.spk = sp;
    for (int i = 0; i < 6; ++i)
        if (sp.reserved[i] != 0) throw EngineError(MI355VITS_ERR_INVALID, "speakers: reserved fields must be 0");
    if (c.n_speakers <= 1 || c.gin_channels < 1) throw EngineError(MI355VITS_ERR_INVALID, "speakers: voice has no speaker embedding");
    const bool mix = sp.mix_sid || sp.mix_weight;
    if (mix && sp.vectors) throw EngineError(MI355VITS_ERR_INVALID, "speakers: mix_sid / mix_weight and vectors exclude each other");
    if (!mix && !sp.vectors) throw EngineError(MI355VITS_ERR_INVALID, "speakers: give mix_sid and mix_weight, or vectors");
    const int gin = c.gin_channels;
    if (!mix) {
        if (sp.n_terms != 0) throw EngineError(MI355VITS_ERR_INVALID, "speakers: n_terms must be 0 with vectors");
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < gin; ++i)
                if (!std::isfinite(sp.vectors[(size_t)b * gin + i]))
                    throw EngineError(MI355VITS_ERR_INVALID, "row " + std::to_string(b) + ": speaker vector must be finite (channel " + std::to_string(i) + ")");
        in.speakers = RunInputs::SPK_VECTORS;
        return;
    }
    if (!sp.mix_sid || !sp.mix_weight) throw EngineError(MI355VITS_ERR_INVALID, "speakers: mix_sid and mix_weight go together");
    const int K = sp.n_terms;
    if (K < 1 || K > MI355VITS_MAX_SPEAKER_TERMS)
        throw EngineError(MI355VITS_ERR_INVALID, "speakers: n_terms must be within 1 .. " + std::to_string(MI355VITS_MAX_SPEAKER_TERMS));
    for (int b = 0; b < B; ++b) {
        bool any = false;
        for (int k = 0; k < K; ++k) {
            const float w = sp.mix_weight[(size_t)b * K + k];
            const std::string where = "row " + std::to_string(b) + ", term " + std::to_string(k);
            if (!std::isfinite(w) || std::fabs(w) > 1024.0f) throw EngineError(MI355VITS_ERR_INVALID, where + ": speaker weight must be finite and within -1024 .. 1024");
            if (w == 0.0f) continue;  // a skipped term: its sid is not looked at
            any = true;
            const int64_t s = sp.mix_sid[(size_t)b * K + k];
            if (s < 0 || s >= c.n_speakers)
                throw EngineError(MI355VITS_ERR_INVALID, where + ": speaker id " + std::to_string(s) + " out of range (the voice has " + std::to_string(c.n_speakers) + " speakers)");
        }
        if (!any) throw EngineError(MI355VITS_ERR_INVALID, "row " + std::to_string(b) + ": every speaker weight is 0");
    }
    in.speakers = RunInputs::SPK_MIX;
}

// Every consumer's projection of the speaker vector g of each row (a multi-speaker voice only): a k_speaker_cond launch per consumer
// from emb_g[sid], or in a speakers run k_speaker_cond_mix for all of them, which makes g from the mix tables or takes the vectors.
void Engine::conditioning(const RunInputs& in) {
    const mi355vits_config& c = cfg_;
    const int B = in.B, H = c.hidden_channels, gin = c.n_speakers > 1 ? c.gin_channels : 0;
    if (!gin) return;
    std::vector<SpeakerMixJob> jobs;
    auto job = [&](const std::string& name, int Cout, float* out) {
        SpeakerMixJob j;
        j.w = vec(name + ".weight"); j.bias = vec(name + ".bias"); j.Cout = Cout; j.out = out;
        jobs.push_back(j);
    };
    job("dp.cond", H, d_cond_dp_);
    job("dec.cond", c.upsample_initial_channel, d_cond_dec_);
    for (int j = 0; j < c.flow_n_flows; ++j) job(S("flow.flows.%d", 2 * j) + ".enc.cond_layer", 2 * H * c.flow_wn_layers, d_cond_flow_[j]);
    if (in.speakers == RunInputs::SPK_NONE) {
        ProfScope ps(prof_, "speaker_cond");
        for (const SpeakerMixJob& j : jobs) launch_speaker_cond(vec("emb_g.weight"), d_sid_, j.w, j.bias, B, gin, j.Cout, j.out, stream_);
        return;
    }
    const bool mix = in.speakers == RunInputs::SPK_MIX;
    SpeakerMixArgs m;
    m.B = B; m.gin = gin; m.g = d_g_;
    if (mix) {
        m.emb_g = vec("emb_g.weight"); m.sid = d_mix_sid_; m.weight = d_mix_w_; m.K = in.spk.n_terms;
    } else {
        m.vectors = d_spk_vec_;
    }
    // one launch (a voice with more than SPEAKER_MIX_MAX_JOBS - 2 flows: one per table-full)
    for (size_t q0 = 0; q0 < jobs.size(); q0 += SPEAKER_MIX_MAX_JOBS) {
        m.n_jobs = (int)std::min<size_t>(SPEAKER_MIX_MAX_JOBS, jobs.size() - q0);
        double couts = 0;
        for (int q = 0; q < m.n_jobs; ++q) {
            m.jobs[q] = jobs[q0 + q];
            couts += m.jobs[q].Cout;
        }
        // the weights once, the tables (K gin table values or gin vector values per row), the outputs
        const double bytes = 4.0 * couts * (gin + 1) + 4.0 * B * (double)(mix ? in.spk.n_terms : 1) * gin + 4.0 * B * couts;
        ProfScope ps(prof_, "speaker_cond.mix", 2.0 * B * couts * gin, bytes);
        launch_speaker_cond_mix(m, stream_);
    }
    tap("g", d_g_, {B, gin, 1});
}

RunInputs check_inputs(const mi355vits_config& c, const RunCall& call) {
    const mi355vits_run_args& args = call.args;
    if (args.batch < 1 || args.tx_max < 1) throw EngineError(MI355VITS_ERR_INVALID, "batch and tx_max must be >= 1");
    const float* row_scales = call.rows ? call.rows->scales : nullptr;
    if (!args.ids || !args.lengths || (!args.scales && !row_scales))
        throw EngineError(MI355VITS_ERR_INVALID, "input, input_lengths and scales are required");
    const bool multi = c.n_speakers > 1;
    if (multi && !args.sid && !call.speakers) throw EngineError(MI355VITS_ERR_INVALID, "multi-speaker voice: feed 'sid' is required");
    const int B = args.batch, Tx = args.tx_max;
    if ((long)B * Tx > (1L << 26)) throw EngineError(MI355VITS_ERR_INVALID, "batch * tx_max too large");
    if (Tx > rel_attention_valu_cap(c.hidden_channels, c.n_heads, c.window_size) &&
        !rel_attention_stream_supported(c.hidden_channels, c.n_heads, c.window_size))
        throw EngineError(MI355VITS_ERR_INVALID, "tx_max above " + std::to_string(rel_attention_valu_cap(c.hidden_channels, c.n_heads, c.window_size)) +
                                                 " ids needs the streamed attention kernel, which supports an even head width <= 128 and a "
                                                 "relative window <= 15 only");
    RunInputs in;
    in.B = B;
    in.Tx = Tx;
    in.seed = args.seed;
    in.flags = args.flags;
    in.ids = args.ids;
    in.sid = (multi && !call.speakers) ? args.sid : nullptr;
    in.forced_durations = args.forced_durations;
    in.noise_w = args.noise_w;
    in.noise_z = args.noise_z;
    in.noise_z_frames = args.noise_z_frames;
    in.sc3.resize((size_t)B * 3);
    in.vol.resize(B);
    in.utt.resize(B);
    for (int b = 0; b < B; ++b) {
        const float* sc = row_scales ? row_scales + (size_t)b * 3 : args.scales;
        auto bad = [&](const char* what) {  // a per-row message names the row
            return EngineError(MI355VITS_ERR_INVALID, (row_scales ? "row " + std::to_string(b) + ": " : std::string()) + what);
        };
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(sc[i])) throw bad("scales must be finite");
        if (sc[0] < 0 || sc[2] < 0) throw bad("noise scales must be >= 0");
        if (!(sc[1] > 0)) throw bad("length_scale must be > 0");
        for (int i = 0; i < 3; ++i) in.sc3[(size_t)b * 3 + i] = sc[i];
        in.any_noise_z = in.any_noise_z || sc[0] != 0.0f;
        const double v = (call.rows && call.rows->pcm_volume) ? call.rows->pcm_volume[b] : args.pcm_volume;
        in.vol[b] = (v > 0.0) ? v : 1.0;
        in.utt[b] = (call.rows && call.rows->utterance) ? call.rows->utterance[b] : args.utterance_base + (unsigned long long)b;
    }
    in.len32.resize(B);
    for (int b = 0; b < B; ++b) {
        if (args.lengths[b] < 0 || args.lengths[b] > Tx) throw EngineError(MI355VITS_ERR_INVALID, "input_lengths out of range");
        in.len32[b] = (int)args.lengths[b];
        for (int t = 0; t < in.len32[b]; ++t) {
            const int64_t id = args.ids[(long)b * Tx + t];
            if (id < 0 || id >= c.num_symbols) throw EngineError(MI355VITS_ERR_INVALID, "phoneme id out of range");
        }
        if (in.sid && (in.sid[b] < 0 || in.sid[b] >= c.n_speakers)) throw EngineError(MI355VITS_ERR_INVALID, "speaker id out of range");
    }
    if (args.noise_z && args.noise_z_frames < 1) throw EngineError(MI355VITS_ERR_INVALID, "noise_z_frames must be >= 1");
    // timing (mi355vits_run_timed)
    if (call.timing) {
        const mi355vits_timing_args& tm = in.timing = *call.timing;
        for (int i = 0; i < 6; ++i)
            if (tm.reserved[i] != 0) throw EngineError(MI355VITS_ERR_INVALID, "timing: reserved fields must be 0");
        if (in.timed() && args.forced_durations) throw EngineError(MI355VITS_ERR_INVALID, "timing and forced_durations exclude each other");
        for (int b = 0; b < B; ++b) {
            const std::string rowname = "row " + std::to_string(b);
            for (int t = 0; t < in.len32[b]; ++t) {
                const size_t i = (size_t)b * Tx + t;
                if (tm.stretch && !(std::isfinite(tm.stretch[i]) && tm.stretch[i] >= 0.0f && tm.stretch[i] <= 1048576.0f))
                    throw EngineError(MI355VITS_ERR_INVALID, rowname + ", phoneme " + std::to_string(t) + ": stretch must be finite and within 0 .. 2^20");
                if (tm.min_frames && (tm.min_frames[i] < 0 || tm.min_frames[i] > DURATION_FRAME_CAP))
                    throw EngineError(MI355VITS_ERR_INVALID, rowname + ", phoneme " + std::to_string(t) + ": min_frames must be within 0 .. " + std::to_string(DURATION_FRAME_CAP));
            }
            if (tm.target_frames && (tm.target_frames[b] < 0 || tm.target_frames[b] > DURATION_FRAME_CAP))
                throw EngineError(MI355VITS_ERR_INVALID, rowname + ": target_frames must be 0 (none) or within 1 .. " + std::to_string(DURATION_FRAME_CAP));
        }
    }
    // speakers (mi355vits_run_speakers): a blend or a vector per row in place of args.sid, which is then not read
    if (call.speakers) check_speakers(c, *call.speakers, in);
    // levels (mi355vits_run_levels): a gain per phoneme, a ramp per row; without a gain the struct's ramps are not looked at
    if (call.levels) {
        const mi355vits_level_args& lv = *call.levels;
        for (int i = 0; i < 6; ++i)
            if (lv.reserved[i] != 0) throw EngineError(MI355VITS_ERR_INVALID, "levels: reserved fields must be 0");
        if (lv.gain) {
            in.lvl = lv;
            for (int b = 0; b < B; ++b) {
                const std::string rowname = "row " + std::to_string(b);
                for (int t = 0; t < in.len32[b]; ++t) {
                    const float g = lv.gain[(size_t)b * Tx + t];
                    if (!(std::isfinite(g) && g >= 0.0f && g <= 1024.0f))
                        throw EngineError(MI355VITS_ERR_INVALID, rowname + ", phoneme " + std::to_string(t) + ": gain must be finite and within 0 .. 1024");
                }
                if (lv.ramp_samples && (lv.ramp_samples[b] < 0 || lv.ramp_samples[b] > LEVELS_MAX_RAMP))
                    throw EngineError(MI355VITS_ERR_INVALID, rowname + ": ramp_samples must be within 0 .. " + std::to_string(LEVELS_MAX_RAMP));
            }
        }
    }
    // pitch (mi355vits_run_pitch): a ratio per phoneme; the duration half of the change is the stretch of a timed run
    if (call.pitch) {
        const mi355vits_pitch_args& pa = *call.pitch;
        for (int i = 0; i < 7; ++i)
            if (pa.reserved[i] != 0) throw EngineError(MI355VITS_ERR_INVALID, "pitch: reserved fields must be 0");
        if (pa.ratio) {
            in.pit = pa;
            for (int b = 0; b < B; ++b)
                for (int t = 0; t < in.len32[b]; ++t) {
                    const float p = pa.ratio[(size_t)b * Tx + t];
                    if (!(std::isfinite(p) && p >= 0.5f && p <= 2.0f))
                        throw EngineError(MI355VITS_ERR_INVALID, "row " + std::to_string(b) + ", phoneme " + std::to_string(t) + ": pitch ratio must be finite and within 0.5 .. 2");
                    if (p != 1.0f && in.timing.target_frames && in.timing.target_frames[b] != 0)
                        throw EngineError(MI355VITS_ERR_INVALID, "row " + std::to_string(b) + ": a fitted length and a pitch ratio exclude each other");
                }
            if (!args.forced_durations) {  // (with forced_durations the table IS the synthesized frames: no compensation)
                in.pitch_stretch.assign((size_t)B * Tx, 1.0f);
                for (int b = 0; b < B; ++b)
                    for (int t = 0; t < in.len32[b]; ++t) {
                        const size_t i = (size_t)b * Tx + t;
                        volatile float prod = (in.timing.stretch ? in.timing.stretch[i] : 1.0f) * pa.ratio[i];  // one f32 product
                        if (!(prod <= 1048576.0f))
                            throw EngineError(MI355VITS_ERR_INVALID, "row " + std::to_string(b) + ", phoneme " + std::to_string(t) + ": stretch times pitch ratio is above 2^20");
                        in.pitch_stretch[i] = prod;
                    }
                in.timing.stretch = in.pitch_stretch.data();  // (the vector's storage moves with `in`)
            }
        }
    }
    return in;
}

void Engine::begin_run(const RunInputs& in) {
    HIP_CHECK(hipSetDevice(device_));
    have_result_ = false;
    have_edges_ = false;
    have_loud_ = false;
    have_tp_ = false;
    taps_on_ = (in.flags & MI355VITS_DEBUG_TAPS) != 0;
    for (auto& t : taps_) (void)hipFree(t.dev);
    taps_.clear();
}

void Engine::upload_inputs(const RunInputs& in) {
    ArenaCount size_a;
    layout_a(size_a, in, true);
    arena_a_.reserve(size_a.bytes + 4096, stream_);
    arena_a_.reset();
    HIP_CHECK(hipEventRecord(ev_start_, stream_));
    end_recorded_ = false;
    layout_a(arena_a_, in, false);
    // h_in_ is a member: it outlives the copy whatever HIP does with pageable sources
    HIP_CHECK(hipMemcpyAsync(d_ids_, h_in_.data(), h_in_.size(), hipMemcpyHostToDevice, stream_));
}

// The one host round trip: frame counts size the rest of the graph (a timed run: status and factor of every row sit right behind
// ylen and come in the same copy).  Here, too, the two checks that need them.
void Engine::read_frame_counts(const RunInputs& in) {
    const int B = in.B;
    const size_t nread = in.pitched() ? 4 : (in.timed() ? 3 : 1);
    h_ylen_.resize(nread * B);
    HIP_CHECK(hipMemcpyAsync(h_ylen_.data(), d_ylen_, nread * B * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    if (in.timed()) {
        for (int b = 0; b < B; ++b) {
            const int st = h_ylen_[(size_t)B + b];
            const std::string what = "row " + std::to_string(b) + ": target of " + std::to_string(in.timing.target_frames ? in.timing.target_frames[b] : 0) + " frames ";
            if (st == TIMING_BELOW_FLOOR) throw EngineError(MI355VITS_ERR_INVALID, what + "is below the " + std::to_string(h_ylen_[b]) + " the row needs at least");
            if (st == TIMING_UNREACHABLE) throw EngineError(MI355VITS_ERR_INVALID, what + "cannot be reached: at the largest factor, 2^30, the row has " + std::to_string(h_ylen_[b]) + " (is every stretched duration 0?)");
            if (st != TIMING_OK) throw EngineError(MI355VITS_ERR_INTERNAL, "row " + std::to_string(b) + ": timing status " + std::to_string(st));
        }
        if (in.timing.factor_out) memcpy(in.timing.factor_out, h_ylen_.data() + 2 * (size_t)B, (size_t)B * 4);
    } else if (in.timing.factor_out) {
        std::fill(in.timing.factor_out, in.timing.factor_out + B, 1.0f);
    }
    int Ty = 1;
    for (int b = 0; b < B; ++b) {
        if (h_ylen_[b] < 1 || h_ylen_[b] > DURATION_FRAME_CAP) throw EngineError(MI355VITS_ERR_INVALID, "predicted duration out of range (bad weights or length_scale?)");
        Ty = std::max(Ty, h_ylen_[b]);
    }
    if (in.noise_z && in.any_noise_z && in.noise_z_frames < Ty)
        throw EngineError(MI355VITS_ERR_INVALID, "noise_z has fewer frames than the utterance needs");
    tap_ints("w_ceil", d_wceil_, {B, 1, in.Tx});
    Ty_ = Ty;
    const long hop = cfg_.hop_length;
    L_ = (long)Ty * hop;
    // the rows the caller receives: the waveform itself, or with an output rate set what the resampler makes of it — lengths from
    // the frame counts, so its table rides in the stage table's upload
    const bool rs = out_hz_ != 0;
    run_hz_ = rs ? out_hz_ : cfg_.sample_rate;
    run_L_ = rs ? rs_.L : 1;
    run_M_ = rs ? rs_.M : 1;
    // the native-rate rows everything behind the waveform reads: the waveform itself, or in a pitch run its warp
    pitched_ = in.pitched();
    h_nlen_.resize(B);
    Ln_ = pitched_ ? 1 : L_;
    for (int b = 0; b < B; ++b) {
        h_nlen_[b] = pitched_ ? (int64_t)h_ylen_[3 * (size_t)B + b] : (int64_t)h_ylen_[b] * hop;
        if (pitched_ && (h_nlen_[b] < 1 || h_nlen_[b] >= 0x7fffffffLL))  // (k_pitch_plan saturates)
            throw EngineError(MI355VITS_ERR_INVALID, "row " + std::to_string(b) + ": the warped row does not fit 32 bits");
        if (pitched_) Ln_ = std::max<long>(Ln_, (long)h_nlen_[b]);
    }
    h_olen_.resize(B);
    Lo_ = rs ? 0 : Ln_;
    for (int b = 0; b < B; ++b) {
        const int64_t n = h_nlen_[b];
        h_olen_[b] = rs ? (int64_t)resample_out_len(n, rs_.L, rs_.M) : n;
        if (h_olen_[b] > 0x7fffffffLL)
            throw EngineError(MI355VITS_ERR_INVALID, "row " + std::to_string(b) + ": " + std::to_string(h_olen_[b]) + " samples at " + std::to_string(run_hz_) + " Hz do not fit 32 bits");
        if (rs) Lo_ = std::max<long>(Lo_, (long)h_olen_[b]);
    }
}

void Engine::size_frame_side(const RunInputs& in, const OutputPlan* plan) {
    const bool rs = out_hz_ != 0;
    const size_t B = in.B, Lr = rs ? Lo_ : 0, Lw = pitched_ ? Ln_ : 0;
    ArenaCount size_b;
    layout_b(size_b, B, Ty_, in.noise_z_held(), Lr, Lw);
    if (plan) layout(size_b, *plan);
    arena_b_.reserve(size_b.bytes + 4096, stream_);
    arena_b_.reset();
    layout_b(arena_b_, B, Ty_, in.noise_z_held(), Lr, Lw);
    layout_b_end_ = arena_b_.used();
    n_audio_ = pitched_ ? d_waudio_ : d_audio_;
    n_peaks_ = pitched_ ? d_wpeaks_ : d_peaks_;
    n_alen_ = pitched_ ? d_walen_ : d_alen_;
    o_audio_ = rs ? d_raudio_ : n_audio_;
    o_peaks_ = rs ? d_rpeaks_ : n_peaks_;
    o_alen_ = rs ? d_rtab_ : n_alen_;
    d_pack_seg_ = nullptr;
    d_pack_ = nullptr;
    if (plan) layout(arena_b_, *plan);
}

void Engine::upload_stage_table(const RunInputs& in, const OutputPlan* plan) {
    const mi355vits_config& c = cfg_;
    const int B = in.B;
    const long hop = c.hop_length;
    const bool rs = out_hz_ != 0;
    if (d_noise_z_) HIP_CHECK(hipMemcpyAsync(d_noise_z_, in.noise_z, (size_t)B * c.inter_channels * in.noise_z_held() * 4, hipMemcpyHostToDevice, stream_));
    // per-stage valid lengths and (last row) the audio lengths: one copy
    // (a plan's table sits right behind d_slen_ in the arena: the same copy brings it; no early block has a curve row)
    h_slen_.assign(plan ? (size_t)(d_pack_seg_ - d_slen_) + plan->table_words() : (size_t)(c.n_upsamples + 2) * B + (pitched_ ? pitch_tab_ints(B) : 0) + (rs ? resample_tab_ints(B) : 0), 0);
    if (plan) fill_table(*plan, h_slen_.data() + (d_pack_seg_ - d_slen_));
    long f = 1;
    for (int i = 0; i <= c.n_upsamples; ++i) {
        for (int b = 0; b < B; ++b) h_slen_[(size_t)i * B + b] = (int)(h_ylen_[b] * f);
        if (i < c.n_upsamples) f *= c.upsample_rates[i];
    }
    for (int b = 0; b < B; ++b) h_slen_[(size_t)(c.n_upsamples + 1) * B + b] = (int)(h_ylen_[b] * hop);
    pitch_items_ = !pitched_ ? 0 : pitch_fill_tab(h_nlen_.data(), B, h_slen_.data() + (d_walen_ - d_slen_));
    rs_items_ = !rs ? 0 : resample_fill_tab(rs_, h_slen_.data() + (n_alen_ - d_slen_), B, h_slen_.data() + (d_rtab_ - d_slen_));
    HIP_CHECK(hipMemcpyAsync(d_slen_, h_slen_.data(), h_slen_.size() * 4, hipMemcpyHostToDevice, stream_));
}

// a levels run: the envelope of the gains over the phoneme boundaries in d_cum_ onto the native waveform, in place, in front of
// everything that reads it; the row peaks are taken again from the shaped samples
void Engine::levels(const RunInputs& in) {
    if (!in.levelled()) return;
    double n = 0;
    for (int b = 0; b < in.B; ++b) n += (double)h_ylen_[b] * cfg_.hop_length;
    ProfScope ps(prof_, "levels", 0, 8.0 * n + 4.0 * in.B * (double)(in.Tx + 1));
    HIP_CHECK(hipMemsetAsync(d_peaks_, 0, sizeof(unsigned) * in.B, stream_));
    launch_levels(d_cum_, d_len_, d_gain_, d_ramp_, in.B, in.Tx, cfg_.hop_length, d_audio_, L_, d_alen_, L_, d_peaks_, stream_);
}

// a pitch run: the warped boundaries of every row from the frames the duration kernel just left, in front of the run's one sizing
// copy, which brings wlen with the frame counts
void Engine::pitch_plan(const RunInputs& in) {
    if (!in.pitched()) return;
    ProfScope ps(prof_, "pitch.plan", 0, 20.0 * in.B * (double)in.Tx);
    launch_pitch_plan(d_cum_, d_len_, d_ratio_, in.B, in.Tx, cfg_.hop_length, d_tq_, d_wc_, d_wlen_, stream_);
}

// a pitch run: the band-limited warp of the (shaped) native waveform along d_tq_ into d_waudio_, which every consumer reads in
// d_audio_'s place; the row peaks are taken from the warped samples
void Engine::pitch(const RunInputs& in) {
    if (!in.pitched()) return;
    tap("audio_synth", d_audio_, {in.B, 1, L_}, d_alen_, 1);
    double n = 0, w = 0;
    for (int b = 0; b < in.B; ++b) {
        n += (double)h_ylen_[b] * cfg_.hop_length;
        w += (double)h_nlen_[b];
    }
    ProfScope ps(prof_, "pitch", 0, 4.0 * (n + w) + 20.0 * in.B * (double)in.Tx);
    HIP_CHECK(hipMemsetAsync(d_wpeaks_, 0, sizeof(unsigned) * in.B, stream_));
    launch_pitch(d_audio_, L_, d_alen_, d_cum_, d_len_, d_ratio_, d_tq_, d_wc_, d_walen_, pitch_items_, vec("pitch.table"), in.B, in.Tx, cfg_.hop_length,
                 d_waudio_, Ln_, (int)Ln_, d_wpeaks_, stream_);
}

// a run at another rate than the voice's: the native rows -> d_raudio_ over the rs_items_ of the table uploaded with the stage lengths
void Engine::resample() {
    if (!out_hz_) return;
    double n_in = 0, n_out = 0;
    for (int b = 0; b < B_; ++b) {
        n_in += (double)h_nlen_[b];
        n_out += (double)h_olen_[b];
    }
    ProfScope ps(prof_, "resample", 2.0 * rs_.tpp * n_out, 4.0 * n_in + 4.0 * n_out);
    HIP_CHECK(hipMemsetAsync(d_rpeaks_, 0, sizeof(unsigned) * B_, stream_));
    launch_resample(rs_, d_rs_coef_, n_audio_, Ln_, n_alen_, B_, d_rtab_, rs_items_, d_raudio_, Lo_, (int)Lo_, d_rpeaks_, stream_);
}

void Engine::output(const RunInputs& in, const OutputPlan* plan) {
    have_pcm_ = false;
    if (plan) {
        launch(*plan);  // the packed stream or block and nothing else (the pack kernel alone: no early plan is compressed): MI355VITS_WANT_* / DEVICE_ONLY are not looked at
    } else if (in.flags & MI355VITS_WANT_PCM16) {
        ProfScope ps(prof_, "pcm16", 0, 6.0 * in.B * (double)Lo_);
        launch_pcm16(o_audio_, Lo_, o_peaks_, o_alen_, in.B, (int)Lo_, d_pcm_, Lo_, stream_, d_vol_);
        have_pcm_ = true;
    }
    HIP_CHECK(hipEventRecord(ev_end_, stream_));
    end_recorded_ = true;
    have_result_ = true;
}

void Engine::synthesize(const RunCall& call, OutputPlan* plan) {
    const RunInputs in = check_inputs(cfg_, call);  // invalid input is refused here: nothing of the last run has been touched
    begin_run(in);
    upload_inputs(in);
    conditioning(in);
    B_ = in.B;
    Tx_ = in.Tx;
    text_encoder(in.B, in.Tx);
    duration_predictor(in);
    pitch_plan(in);
    read_frame_counts(in);
    if (plan) place(*plan);  // places from the frame counts just read (no early plan trims, normalises or compresses); the size limits, before the frame side is sized
    size_frame_side(in, plan);
    upload_stage_table(in, plan);
    flow_and_decoder(in);
    levels(in);
    pitch(in);
    resample();
    output(in, plan);
}

}  // namespace m355
