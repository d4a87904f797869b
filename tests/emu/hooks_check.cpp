// hooks_check.cpp — a stand-alone bounds check of the hooks of include/mi355vits_lab.h on the CPU model (tests/test_hooks_sanitized.py
// compiles it with the model's sources under the address and undefined-behaviour sanitizers and runs it once).  The model's hipMalloc
// is malloc, so the sanitizer sees every byte a hook or a kernel touches outside a "device" buffer.
//   (a) HookScope itself (csrc/c_api_internal.h): a NULL input stays NULL, inout() returns what the device holds at finish() in the
//       order of registration, a zero-element upload gets a pointer, a throw before finish() copies nothing back, filled() fills.
//   (b) every device hook once through the C ABI at the smallest shape its kernel takes (B = 2, T = 37, lengths {37, 18}), every impl
//       and math mode, every optional pointer given once and withheld once; then, for every hook that takes lengths, one call with a
//       length of T + 1: MI355VITS_ERR_INVALID and nothing written.
// Results are not compared (the pytest suites do that).  One line per call, then "N failures".  -DHOOKS_CHECK_ABI_ONLY builds (b) alone,
// which needs nothing but the C ABI and so runs against any earlier state of the library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#ifndef HOOKS_CHECK_ABI_ONLY
#include "../../mimic3_amd/csrc/c_api_internal.h"
#endif
#include "mi355vits_lab.h"

namespace {

int failures = 0;
const int B = 2, T = 37;
const int32_t LEN[B] = {37, 18}, BAD[B] = {T + 1, 18};
const int F32 = MI355VITS_MATH_F32, X3 = MI355VITS_MATH_BF16X3, BW = MI355VITS_MATH_BF16W;

uint32_t rng_state = 1u;
float rnd() {  // [-0.5, 0.5)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((rng_state >> 8) & 0xffff) / 65536.0f - 0.5f;
}
std::vector<float> F(size_t n, float scale = 1.0f, float offset = 0.0f) {
    std::vector<float> v(n);
    for (float& x : v) x = rnd() * scale + offset;
    return v;
}

void check(const char* what, bool ok) {
    printf("%-72s %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) ++failures;
}
void ok(const char* what, int rc) {
    printf("%-72s rc %d%s\n", what, rc, rc == MI355VITS_OK ? "" : "  FAILED");
    if (rc != MI355VITS_OK) { ++failures; printf("    %s\n", mi355vits_last_error(nullptr)); }
}
// the outputs of a call that must be refused: as they were
struct Watch {
    std::vector<std::pair<const void*, std::vector<uint8_t>>> w;
    template <typename V> void add(const V& v) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(v.data());
        w.emplace_back(v.data(), std::vector<uint8_t>(p, p + v.size() * sizeof(v[0])));
    }
    bool same() const {
        for (const auto& e : w)
            if (memcmp(e.first, e.second.data(), e.second.size()) != 0) return false;
        return true;
    }
};
void refused(const char* what, int rc, const Watch& w) {
    const bool good = rc == MI355VITS_ERR_INVALID && w.same();
    printf("%-72s rc %d%s\n", what, rc, good ? " (refused, nothing written)" : "  FAILED");
    if (!good) ++failures;
}

// ---------------------------------------------------------------- (a) HookScope
#ifdef HOOKS_CHECK_ABI_ONLY
void scope_checks() {}
#else
void scope_checks() {
    {
        HookScope s(0);
        check("scope: a NULL in() stays NULL", s.in(static_cast<const float*>(nullptr), 5) == nullptr);
        check("scope: a NULL inout() stays NULL", s.inout(static_cast<float*>(nullptr), 5) == nullptr);
        float one = 1.0f;
        check("scope: a zero-element in() of a non-NULL pointer gets a pointer", s.in(&one, 0) != nullptr);
        const std::vector<float> none;
        check("scope: an empty vector gets a pointer", s.in(none) != nullptr);
        const uint8_t* f = s.filled<uint8_t>(33, 0x5a);
        bool all = true;
        for (int i = 0; i < 33; ++i) all = all && f[i] == 0x5a;
        check("scope: filled() writes its byte", all);
        s.finish();
    }
    {
        // both host ranges overlap: the later registration is the one that stays
        float host[6] = {1, 2, 3, 4, 5, 6};
        HookScope s(0);
        float* a = s.inout(host, 4);
        float* b = s.inout(host + 2, 4);
        check("scope: inout() sends the prior contents up", a[0] == 1 && a[3] == 4 && b[0] == 3 && b[3] == 6);
        for (int i = 0; i < 4; ++i) { a[i] = 10.0f + i; b[i] = 20.0f + i; }
        check("scope: nothing comes back before finish()", host[0] == 1 && host[5] == 6);
        s.finish();
        check("scope: finish() copies back in the order of registration",
              host[0] == 10 && host[1] == 11 && host[2] == 20 && host[3] == 21 && host[4] == 22 && host[5] == 23);
        float got[2] = {0, 0};
        s.fetch(got, b + 2, 2);
        check("scope: fetch() reads a device range", got[0] == 22 && got[1] == 23);
    }
    {
        float host[4] = {1, 2, 3, 4};
        try {
            HookScope s(0);
            float* d = s.inout(host, 4);
            for (int i = 0; i < 4; ++i) d[i] = -1.0f;
            throw std::runtime_error("before finish");
        } catch (const std::runtime_error&) {
        }
        check("scope: a throw before finish() copies nothing back (and frees: the leak check)", host[0] == 1 && host[3] == 4);
    }
}
#endif

// ---------------------------------------------------------------- (b) the hooks
enum { BIAS = 1, RES = 2, COND = 4, INL = 8, OUTL = 16, ALL = 31 };

void conv1d(const char* what, int impl, int math, int Cin, int Cout, int K, int dil, int fixed, int opts, const int32_t* len = LEN,
            bool expect_refusal = false) {
    auto x = F((size_t)B * Cin * T), w = F((size_t)Cout * Cin * K, 0.1f), bias = F(Cout), res = F((size_t)B * Cout * T), cond = F((size_t)B * Cout);
    auto y = F((size_t)B * Cout * T);
    mi355vits_conv_test t{};
    t.impl = impl; t.B = B; t.Cin = Cin; t.Cout = Cout; t.T = T; t.K = K; t.dilation = dil;
    t.x = x.data(); t.w = w.data(); t.y = y.data();
    t.bias = opts & BIAS ? bias.data() : nullptr;
    t.res = opts & RES ? res.data() : nullptr;
    t.cond = opts & COND ? cond.data() : nullptr;
    t.in_len = opts & INL ? len : nullptr;
    t.out_len = opts & OUTL ? len : nullptr;
    t.in_slope = 1.0f; t.out_scale = 1.0f; t.math = math; t.fixed_rule = fixed;
    Watch wt;
    wt.add(y);
    const int rc = mi355vits_test_conv1d(0, &t);
    if (expect_refusal) refused(what, rc, wt);
    else ok(what, rc);
}

void conv_hooks() {
    conv1d("conv1d impl 0, every option", 0, F32, 3, 5, 3, 1, 0, ALL);
    conv1d("conv1d impl 0, no option", 0, F32, 3, 5, 3, 1, 0, 0);
    conv1d("conv1d impl 1, every option", 1, F32, 4, 5, 3, 1, 0, ALL);
    conv1d("conv1d impl 1, no option, fixed_rule", 1, F32, 4, 5, 3, 1, 1, 0);
    conv1d("conv1d impl 2 bf16x3, every option", 2, X3, 32, 32, 3, 1, 1, ALL);
    conv1d("conv1d impl 2 bf16x3, no option", 2, X3, 32, 32, 3, 1, 1, 0);
    conv1d("conv1d impl 2 bf16w, every option", 2, BW, 32, 32, 3, 1, 1, ALL);
    conv1d("conv1d impl 3 bf16x3, every option", 3, X3, 96, 32, 3, 1, 0, ALL);
    conv1d("conv1d impl 3 bf16x3, no option", 3, X3, 96, 32, 3, 1, 0, 0);
    conv1d("conv1d impl 3 bf16w, every option", 3, BW, 96, 32, 1, 1, 0, ALL);
    conv1d("conv1d impl 3, two slices, in_len", 3, X3, 384, 32, 1, 1, 0, INL);
    conv1d("conv1d impl 3, two slices, no option", 3, X3, 384, 32, 3, 1, 0, 0);
    conv1d("conv1d impl 4, bias", 4, X3, 128, 128, 3, 1, 0, BIAS | RES | INL);
    conv1d("conv1d impl 4, no bias", 4, X3, 128, 128, 3, 1, 0, RES | INL);
    conv1d("conv1d, in_len T + 1", 0, F32, 3, 5, 3, 1, 0, ALL, BAD, true);

    auto convt = [&](const char* what, int impl, int Cin, int Cout, int K, int stride, bool with_bias, const int32_t* len, bool expect_refusal = false) {
        auto x = F((size_t)B * Cin * T), w = F((size_t)Cin * Cout * K, 0.1f), bias = F(Cout), y = F((size_t)B * Cout * T * stride);
        Watch wt;
        wt.add(y);
        const int rc = mi355vits_test_conv_transpose1d(0, impl, B, Cin, Cout, T, K, stride, x.data(), w.data(), with_bias ? bias.data() : nullptr, 0.1f, len, y.data());
        if (expect_refusal) refused(what, rc, wt);
        else ok(what, rc);
    };
    convt("conv_transpose1d impl 0, bias", 0, 3, 2, 4, 2, true, nullptr);
    convt("conv_transpose1d impl 0, no bias", 0, 3, 2, 4, 2, false, nullptr);
    convt("conv_transpose1d impl 1, bias", 1, 4, 2, 4, 2, true, nullptr);
    convt("conv_transpose1d impl 1, no bias", 1, 4, 2, 4, 2, false, nullptr);
    convt("conv_transpose1d impl 2, bias", 2, 32, 16, 4, 2, true, nullptr);
    convt("conv_transpose1d impl 2, no bias", 2, 32, 16, 4, 2, false, nullptr);
    convt("conv_transpose1d impl 3, bias, in_len", 3, 64, 32, 8, 4, true, LEN);
    convt("conv_transpose1d impl 3, no bias, no in_len", 3, 64, 32, 8, 4, false, nullptr);
    convt("conv_transpose1d, in_len T + 1", 3, 64, 32, 8, 4, true, BAD, true);

    auto enc_o_ln = [&](const char* what, int math, bool opts, int in_place, const int32_t* len, bool expect_refusal = false) {
        const int C = 192;
        auto x = F((size_t)B * C * T), w = F((size_t)C * C, 0.1f), bias = F(C), res = F((size_t)B * C * T), g = F(C, 1.0f, 1.0f), be = F(C), y = F((size_t)B * C * T);
        Watch wt;
        wt.add(y);
        const int rc = mi355vits_test_enc_o_ln(0, math, B, T, x.data(), w.data(), opts ? bias.data() : nullptr, res.data(), g.data(), be.data(), 1e-5f,
                                               opts ? len : nullptr, opts ? len : nullptr, in_place, y.data());
        if (expect_refusal) refused(what, rc, wt);
        else ok(what, rc);
    };
    enc_o_ln("enc_o_ln bf16x3, every option, out of place", X3, true, 0, LEN);
    enc_o_ln("enc_o_ln bf16x3, no option, in place", X3, false, 1, LEN);
    enc_o_ln("enc_o_ln bf16w, every option, in place", BW, true, 1, LEN);
    enc_o_ln("enc_o_ln bf16w, no option, out of place", BW, false, 0, LEN);
    enc_o_ln("enc_o_ln, in_len T + 1", X3, true, 0, BAD, true);

    auto conv_post = [&](const char* what, bool opts, const int32_t* len, bool expect_refusal = false) {
        const int Cin = 4, K = 7;
        auto x = F((size_t)B * Cin * T), w = F((size_t)Cin * K), audio = F((size_t)B * T), peaks = F(B);
        std::vector<double> vol = {0.5, 2.0};
        std::vector<int16_t> pcm((size_t)B * T, 77);
        int32_t kernel = -1;
        Watch wt;
        wt.add(audio); wt.add(peaks); wt.add(pcm);
        const int rc = mi355vits_test_conv_post(0, B, Cin, K, T, x.data(), w.data(), len, opts ? vol.data() : nullptr, audio.data(), peaks.data(), pcm.data(),
                                                opts ? &kernel : nullptr);
        if (expect_refusal) refused(what, rc, wt);
        else ok(what, rc);
    };
    conv_post("conv_post, volumes and kernel", true, LEN);
    conv_post("conv_post, neither", false, LEN);
    conv_post("conv_post, valid_len T + 1", true, BAD, true);
}

void audio_hooks() {
    {
        const int ys = 40;
        auto x = F((size_t)B * T), y = F((size_t)B * ys), peaks = F(B);
        std::vector<int32_t> yl(B, -7);
        ok("resample 22050 -> 16000", mi355vits_test_resample(0, B, T, x.data(), LEN, 22050, 16000, ys, y.data(), yl.data(), peaks.data()));
        Watch wt;
        wt.add(y); wt.add(yl); wt.add(peaks);
        refused("resample, length T + 1", mi355vits_test_resample(0, B, T, x.data(), BAD, 22050, 16000, ys, y.data(), yl.data(), peaks.data()), wt);
    }
    {
        const int hop = 4, rs = T * hop;
        std::vector<int32_t> frames((size_t)B * T, 1), alen = {LEN[0] * hop, LEN[1] * hop}, of((size_t)B * T, -7), os_((size_t)B * T, -7), on((size_t)B * T, -7);
        auto audio = F((size_t)B * rs), pk = F((size_t)B * T), rms = F((size_t)B * T);
        ok("alignment, peak and rms", mi355vits_test_alignment(0, B, T, frames.data(), LEN, rs, audio.data(), alen.data(), hop, 1, 1, of.data(), os_.data(),
                                                               on.data(), pk.data(), rms.data()));
        ok("alignment, timing only", mi355vits_test_alignment(0, B, T, frames.data(), LEN, rs, audio.data(), alen.data(), hop, 1, 1, of.data(), os_.data(),
                                                              on.data(), nullptr, nullptr));
        Watch wt;
        wt.add(of); wt.add(os_); wt.add(on); wt.add(pk); wt.add(rms);
        refused("alignment, len T + 1", mi355vits_test_alignment(0, B, T, frames.data(), BAD, rs, audio.data(), alen.data(), hop, 1, 1, of.data(), os_.data(),
                                                                 on.data(), pk.data(), rms.data()), wt);
    }
    {
        std::vector<int16_t> in(T);
        for (int i = 0; i < T; ++i) in[i] = (int16_t)(i * 1771 - 32768);
        std::vector<uint8_t> out(T);
        ok("g711 mu-law", mi355vits_lab_g711_encode(MI355VITS_ENC_ULAW, in.data(), T, out.data()));
        ok("g711 A-law", mi355vits_lab_g711_encode(MI355VITS_ENC_ALAW, in.data(), T, out.data()));
    }
    {
        // two frames; the source starts 2 bytes behind a 16-byte boundary
        const long n = 5000;
        alignas(16) static int16_t store[5008];
        int16_t* pcm = store + 1;
        for (long i = 0; i < n; ++i) pcm[i] = (int16_t)((i * 37) % 2001 - 1000);
        std::vector<uint8_t> out(64 * 1024);
        size_t nb = 0;
        int32_t sizes[2] = {0, 0};
        ok("flac, source at offset 2, frame sizes", mi355vits_lab_flac(pcm, n, 22050, 0, out.data(), out.size(), &nb, sizes));
        ok("flac, no frame sizes", mi355vits_lab_flac(pcm, n, 22050, 126, out.data(), out.size(), &nb, nullptr));
        ok("flac, an empty stream", mi355vits_lab_flac(nullptr, 0, 22050, 0, out.data(), out.size(), &nb, nullptr));
        alignas(16) static int16_t second[40];
        for (int i = 0; i < T; ++i) second[i] = (int16_t)(i - 18);
        const int16_t* arrays[2] = {pcm, second};
        const long counts[2] = {n, T};
        int64_t offsets[2], fsizes[2];
        ok("flac_jobs, two files", mi355vits_lab_flac_jobs(arrays, counts, 2, 22050, out.data(), out.size(), &nb, offsets, fsizes));
    }
    {
        auto audio = F((size_t)B * T), peaks = F(B, 0.0f, 0.4f);
        std::vector<int32_t> first(B, -7), last(B, -7);
        ok("edges", mi355vits_lab_edges(audio.data(), T, LEN, peaks.data(), B, 0.5f, first.data(), last.data()));
        Watch wt;
        wt.add(first); wt.add(last);
        refused("edges, length T + 1", mi355vits_lab_edges(audio.data(), T, BAD, peaks.data(), B, 0.5f, first.data(), last.data()), wt);
    }
    {
        const int rate = 4000, n = 2 * rate;  // rows of 2 s and 1 s: a few gating blocks
        const int32_t len[B] = {n, rate}, bad[B] = {n + 1, rate};
        auto audio = F((size_t)B * n);
        std::vector<double> lufs(B, -7.0);
        std::vector<int32_t> blocks(B, -7), gated(B, -7);
        ok("loudness", mi355vits_lab_loudness(audio.data(), n, len, B, rate, lufs.data(), blocks.data(), gated.data()));
        Watch wt;
        wt.add(lufs); wt.add(blocks); wt.add(gated);
        refused("loudness, length stride + 1", mi355vits_lab_loudness(audio.data(), n, bad, B, rate, lufs.data(), blocks.data(), gated.data()), wt);
    }
    {
        auto audio = F((size_t)B * T, 2.0f), scale = F((size_t)B * T);
        std::vector<double> g = {1.0, 1.5}, env((size_t)B * T);
        for (size_t i = 0; i < env.size(); ++i) env[i] = audio[i] < 0 ? -audio[i] : audio[i];
        std::vector<int64_t> sq(B, -7);
        std::vector<int32_t> red(B, -7);
        ok("limit", mi355vits_lab_limit(audio.data(), T, LEN, B, g.data(), 0.5, 1.0, 4, scale.data(), sq.data(), red.data()));
        ok("limit_env, envelope", mi355vits_lab_limit_env(audio.data(), T, LEN, B, g.data(), 0.5, 1.0, 4, env.data(), scale.data(), sq.data(), red.data()));
        Watch wt;
        wt.add(scale); wt.add(sq); wt.add(red);
        refused("limit, length T + 1", mi355vits_lab_limit(audio.data(), T, BAD, B, g.data(), 0.5, 1.0, 4, scale.data(), sq.data(), red.data()), wt);
        refused("limit_env, length T + 1", mi355vits_lab_limit_env(audio.data(), T, BAD, B, g.data(), 0.5, 1.0, 4, env.data(), scale.data(), sq.data(), red.data()), wt);
    }
    {
        auto audio = F((size_t)B * T);
        std::vector<double> tp(B, -7.0), env((size_t)B * T, -7.0);
        for (int off = 0; off < 4; ++off) {
            char what[64];
            snprintf(what, sizeof what, "true_peak, offset %d, %s", off, off & 1 ? "envelope" : "measurement only");
            ok(what, mi355vits_lab_true_peak(audio.data(), T, LEN, B, off, tp.data(), off & 1 ? env.data() : nullptr));
        }
        Watch wt;
        wt.add(tp); wt.add(env);
        refused("true_peak, length T + 1", mi355vits_lab_true_peak(audio.data(), T, BAD, B, 0, tp.data(), env.data()), wt);
    }
}

void attention_and_flow_hooks() {
    {
        const int H = 4, nh = 2, W = 4;
        auto qkv = F((size_t)B * 3 * H * T), ek = F((size_t)(2 * W + 1) * (H / nh)), ev = F((size_t)(2 * W + 1) * (H / nh)), out = F((size_t)B * H * T);
        const char* names[3] = {"rel_attention impl 0", "rel_attention impl 1", "rel_attention impl 2"};
        for (int impl = 0; impl < 3; ++impl) ok(names[impl], mi355vits_test_rel_attention(0, impl, B, T, H, nh, W, qkv.data(), ek.data(), ev.data(), LEN, out.data()));
        Watch wt;
        wt.add(out);
        refused("rel_attention, len T + 1", mi355vits_test_rel_attention(0, 2, B, T, H, nh, W, qkv.data(), ek.data(), ev.data(), BAD, out.data()), wt);
    }
    auto wn = [&](const char* what, int impl, int math, int H, int Crs, bool with_cond, const int32_t* len, bool expect_refusal = false) {
        const int K = 3;
        auto h = F((size_t)B * H * T), w_in = F((size_t)2 * H * H * K, 0.1f), b_in = F(2 * H), w_rs = F((size_t)Crs * H, 0.1f), b_rs = F(Crs), cond = F((size_t)B * 2 * H);
        auto h_out = F((size_t)B * H * T), skip = F((size_t)B * H * T);
        for (int b = 0; b < B; ++b)  // impl 0 reads h past a row's length: zero there, as the engine keeps it
            for (int c = 0; c < H; ++c)
                for (int t = LEN[b]; t < T; ++t) h[((size_t)b * H + c) * T + t] = 0.0f;
        mi355vits_wn_test t{};
        t.impl = impl; t.B = B; t.H = H; t.T = T; t.K = K; t.dilation = 2; t.Crs = Crs; t.skip_init = 0; t.math = math;
        t.h_in = h.data(); t.w_in = w_in.data(); t.b_in = b_in.data(); t.w_rs = w_rs.data(); t.b_rs = b_rs.data();
        t.cond = with_cond ? cond.data() : nullptr; t.len = len; t.h_out = h_out.data(); t.skip = skip.data();
        Watch wt;
        wt.add(h_out); wt.add(skip);
        const int rc = mi355vits_test_wn_layer(0, &t);
        if (expect_refusal) refused(what, rc, wt);
        else ok(what, rc);
    };
    wn("wn_layer impl 0, generic convs, cond", 0, F32, 3, 6, true, LEN);
    wn("wn_layer impl 0, MFMA convs, last layer, no cond", 0, F32, 32, 32, false, LEN);
    wn("wn_layer impl 1, cond", 1, F32, 32, 64, true, LEN);
    wn("wn_layer impl 1, last layer, no cond", 1, F32, 32, 32, false, LEN);
    wn("wn_layer impl 2, cond", 2, X3, 192, 384, true, LEN);
    wn("wn_layer impl 2, last layer, no cond", 2, X3, 192, 192, false, LEN);
    setenv("MI355VITS_WN_SHAPE", "32", 1);  // read at every call: the 32x32x16 form, the gate conv packed in tile order
    wn("wn_layer impl 2 on 32-row tiles, cond", 2, X3, 192, 384, true, LEN);
    wn("wn_layer impl 2 on 32-row tiles, last layer, no cond", 2, X3, 192, 192, false, LEN);
    unsetenv("MI355VITS_WN_SHAPE");
    wn("wn_layer, len T + 1", 1, F32, 32, 64, true, BAD, true);

    auto mrf = [&](const char* what, int impl, int math, int C, int nrb, const int32_t* len, bool expect_refusal = false) {
        const int32_t k3[4] = {3, 5, 7, 0}, a3[4] = {1, 2, 3, 0}, b3[4] = {2, 6, 12, 0}, k1[4] = {3, 0, 0, 0}, a1[4] = {1, 0, 0, 0};
        const int32_t *k = nrb == 3 ? k3 : k1, *d1 = nrb == 3 ? a3 : a1, *d2 = nrb == 3 ? b3 : a1;
        auto x = F((size_t)B * C * T), y = F((size_t)B * C * T), bias = F(C);
        std::vector<std::vector<float>> w;
        mi355vits_mrf_test t{};
        t.impl = impl; t.B = B; t.C = C; t.T = T; t.nrb = nrb; t.math = math;
        for (int j = 0; j < nrb; ++j) {
            t.k[j] = k[j]; t.d1[j] = d1[j]; t.d2[j] = d2[j];
            for (int q = 0; q < 2; ++q) {
                w.push_back(F((size_t)C * C * k[j], 0.05f));
                t.bias[j][q] = bias.data();
            }
        }
        for (int j = 0; j < nrb; ++j)
            for (int q = 0; q < 2; ++q) t.w[j][q] = w[(size_t)2 * j + q].data();
        if (impl == 2) {
            int32_t width = 0;
            if (mi355vits_lab_mrf_plan(2, C, nrb, k, d1, d2, &width, nullptr, nullptr, nullptr) != MI355VITS_OK) width = 0;
            t.seg = width;
        }
        t.x = x.data(); t.len = len; t.out_scale = 0.0f; t.y = y.data();
        Watch wt;
        wt.add(y);
        const int rc = mi355vits_test_mrf_stage(0, &t);
        if (expect_refusal) refused(what, rc, wt);
        else ok(what, rc);
    };
    mrf("mrf_stage impl 0 f32", 0, F32, 32, 1, LEN);
    mrf("mrf_stage impl 0 bf16x3", 0, X3, 32, 1, LEN);
    mrf("mrf_stage impl 1", 1, X3, 32, 3, LEN);
    mrf("mrf_stage impl 2", 2, X3, 64, 3, LEN);
    mrf("mrf_stage, len T + 1", 0, F32, 32, 1, BAD, true);
}

void sdp_hooks() {
    // impl, math, C, pre_mode, cond, z, proj, spline
    auto dds = [&](const char* what, int impl, int math, int C, int pre_mode, bool with_cond, bool with_z, bool proj, bool spline, const int32_t* len,
                   bool expect_refusal = false) {
        const int K = 3, NL = 2, nb = 4, PC = 3 * nb - 1;
        auto src = F((size_t)B * C * T), pre_w = F(pre_mode ? (size_t)C : (size_t)C * C, 0.1f), vec = F(C), gamma = F(C, 1.0f, 1.0f), cond = F((size_t)B * C);
        auto dw = F((size_t)C * K), w1 = F((size_t)C * C, 0.1f), pw = F((size_t)PC * C, 0.1f), pb = F(PC);
        auto z = F((size_t)B * 2 * T), out = F((size_t)B * PC * T), x_out = F((size_t)B * C * T);
        mi355vits_dds_stack_test t{};
        t.impl = impl; t.math = math; t.B = B; t.C = C; t.T = T; t.K = K; t.n_layers = NL; t.pre_mode = pre_mode; t.zch = 0;
        t.proj_cout = proj ? PC : 0; t.spline = spline; t.nb = nb; t.tail = 5.0f; t.inv_sqrt_fc = 0.1f;
        t.src = src.data(); t.pre_w = pre_w.data(); t.pre_b = vec.data(); t.cond = with_cond ? cond.data() : nullptr;
        for (int i = 0; i < NL; ++i) {
            t.dw_w[i] = dw.data(); t.dw_b[i] = vec.data(); t.g1[i] = gamma.data(); t.b1[i] = vec.data();
            t.w1x1[i] = w1.data(); t.bias1x1[i] = vec.data(); t.g2[i] = gamma.data(); t.b2[i] = vec.data();
        }
        t.proj_w = proj ? pw.data() : nullptr; t.proj_b = proj ? pb.data() : nullptr;
        t.len = len; t.z = with_z ? z.data() : nullptr; t.out = proj ? out.data() : nullptr; t.x_out = x_out.data();
        Watch wt;
        wt.add(z); wt.add(out); wt.add(x_out);
        const int rc = mi355vits_test_dds_stack(0, &t);
        if (expect_refusal) refused(what, rc, wt);
        else ok(what, rc);
    };
    dds("dds_stack impl 0, generic convs, conv pre, cond, no z, no proj", 0, F32, 3, 0, true, false, false, false, LEN);
    dds("dds_stack impl 0, affine pre, proj, spline", 0, F32, 4, 1, false, true, true, true, LEN);
    dds("dds_stack impl 1, conv pre, z, proj", 1, F32, 32, 0, false, true, true, false, LEN);
    dds("dds_stack impl 1, affine pre, spline", 1, F32, 32, 1, false, true, true, true, LEN);
    dds("dds_stack impl 2, conv pre, cond, no z, no proj", 2, F32, 192, 0, true, false, false, false, LEN);
    dds("dds_stack impl 2, affine pre, spline", 2, F32, 192, 1, false, true, true, true, LEN);
    dds("dds_stack impl 3 bf16x3, affine pre, spline", 3, X3, 192, 1, false, true, true, true, LEN);
    dds("dds_stack impl 3 bf16w, conv pre, cond, proj", 3, BW, 192, 0, true, false, true, false, LEN);
    dds("dds_stack, len T + 1", 1, F32, 32, 1, false, true, true, true, BAD, true);
    {
        const int nb = 4;
        auto theta = F((size_t)B * (3 * nb - 1) * T), z = F((size_t)B * 2 * T);
        ok("spline_inverse", mi355vits_test_spline_inverse(0, B, T, nb, 0, 5.0f, 0.1f, theta.data(), LEN, z.data()));
        Watch wt;
        wt.add(z);
        refused("spline_inverse, len T + 1", mi355vits_test_spline_inverse(0, B, T, nb, 0, 5.0f, 0.1f, theta.data(), BAD, z.data()), wt);
    }
    {
        auto z = F((size_t)B * 2 * T), scales = F((size_t)B * 3, 0.0f, 1.0f), logw = F((size_t)B * T);
        std::vector<int32_t> forced((size_t)B * T, 2), w((size_t)B * T, -7), cum((size_t)B * T, -7), ylen(B, -7);
        ok("durations, forced", mi355vits_test_durations(0, B, T, 0, 0.1f, 0.2f, z.data(), LEN, forced.data(), scales.data(), logw.data(), w.data(), cum.data(), ylen.data()));
        ok("durations, free", mi355vits_test_durations(0, B, T, 1, 0.1f, 0.2f, z.data(), LEN, nullptr, scales.data(), logw.data(), w.data(), cum.data(), ylen.data()));
        Watch wt;
        wt.add(logw); wt.add(w); wt.add(cum); wt.add(ylen);
        refused("durations, len T + 1", mi355vits_test_durations(0, B, T, 0, 0.1f, 0.2f, z.data(), BAD, forced.data(), scales.data(), logw.data(), w.data(), cum.data(), ylen.data()), wt);
    }
    {
        auto u = F((size_t)B * T, 1.0f, 2.0f), factor = F(B);
        std::vector<int32_t> minf((size_t)B * T, 1), target = {100, 0}, fr((size_t)B * T, -7), cum((size_t)B * T, -7), ylen(B, -7), status(B, -7);
        ok("fit_durations, floors and targets", mi355vits_test_fit_durations(0, B, T, u.data(), LEN, minf.data(), target.data(), fr.data(), cum.data(), ylen.data(), factor.data(), status.data()));
        ok("fit_durations, neither", mi355vits_test_fit_durations(0, B, T, u.data(), LEN, nullptr, nullptr, fr.data(), cum.data(), ylen.data(), factor.data(), status.data()));
        Watch wt;
        wt.add(fr); wt.add(cum); wt.add(ylen); wt.add(factor); wt.add(status);
        refused("fit_durations, len T + 1", mi355vits_test_fit_durations(0, B, T, u.data(), BAD, minf.data(), target.data(), fr.data(), cum.data(), ylen.data(), factor.data(), status.data()), wt);
    }
    {
        const int I = 2, Tx = 5;
        auto stats = F((size_t)B * 2 * I * Tx), inj = F((size_t)B * I * T), z = F((size_t)B * I * T);
        std::vector<float> noisy = {0.5f, 1.0f, 0.8f, 0.5f, 1.0f, 0.8f}, quiet = {0.0f, 1.0f, 0.8f, 0.0f, 1.0f, 0.8f};
        std::vector<int32_t> cum((size_t)B * Tx);
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < Tx; ++j) cum[(size_t)b * Tx + j] = (j + 1) * LEN[b] / Tx;
        const uint64_t utt[B] = {3, 0x100000002ull};
        ok("expand_prior, injected noise", mi355vits_test_expand_prior(0, B, I, Tx, T, stats.data(), cum.data(), LEN, inj.data(), T, noisy.data(), z.data()));
        ok("expand_prior, no noise", mi355vits_test_expand_prior(0, B, I, Tx, T, stats.data(), cum.data(), LEN, nullptr, 0, quiet.data(), z.data()));
        ok("expand_prior_keyed", mi355vits_test_expand_prior_keyed(0, B, I, Tx, T, stats.data(), cum.data(), LEN, noisy.data(), 11, utt, z.data()));
        Watch wt;
        wt.add(z);
        refused("expand_prior, ylen T + 1", mi355vits_test_expand_prior(0, B, I, Tx, T, stats.data(), cum.data(), BAD, inj.data(), T, noisy.data(), z.data()), wt);
        refused("expand_prior_keyed, ylen T + 1", mi355vits_test_expand_prior_keyed(0, B, I, Tx, T, stats.data(), cum.data(), BAD, noisy.data(), 11, utt, z.data()), wt);
        auto zn = F((size_t)B * 2 * T);
        ok("sdp_noise", mi355vits_test_sdp_noise(0, B, T, 11, utt, noisy.data(), zn.data()));
    }
    auto dp_det = [&](const char* what, int math, bool with_cond, const int32_t* len, bool expect_refusal = false) {
        const int H = 32, Fc = 32, K = 3;
        auto x = F((size_t)B * H * T), cond = F((size_t)B * H), w1 = F((size_t)Fc * H * K, 0.1f), w2 = F((size_t)Fc * Fc * K, 0.1f), vec = F(Fc), gamma = F(Fc, 1.0f, 1.0f);
        auto logw = F((size_t)B * T);
        mi355vits_dp_det_test t{};
        t.B = B; t.H = H; t.F = Fc; t.K = K; t.T = T; t.math = math;
        t.x = x.data(); t.cond = with_cond ? cond.data() : nullptr; t.len = len;
        t.w1 = w1.data(); t.b1 = vec.data(); t.g1 = gamma.data(); t.be1 = vec.data();
        t.w2 = w2.data(); t.b2 = vec.data(); t.g2 = gamma.data(); t.be2 = vec.data();
        t.proj_w = vec.data(); t.proj_b = vec.data(); t.logw = logw.data();
        Watch wt;
        wt.add(logw);
        const int rc = mi355vits_test_dp_det(0, &t);
        if (expect_refusal) refused(what, rc, wt);
        else ok(what, rc);
    };
    dp_det("dp_det f32, cond", F32, true, LEN);
    dp_det("dp_det bf16x3, no cond", X3, false, LEN);
    dp_det("dp_det, len T + 1", F32, true, BAD, true);
}

void text_and_speaker_hooks() {
    {
        const int H = 5, NS = 7;
        std::vector<int64_t> ids((size_t)B * T);
        for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int64_t)(i % NS);
        auto emb = F((size_t)NS * H), y = F((size_t)B * H * T);
        ok("embed", mi355vits_test_embed(0, B, T, H, NS, ids.data(), LEN, emb.data(), 2.0f, y.data()));
        Watch wt;
        wt.add(y);
        refused("embed, len T + 1", mi355vits_test_embed(0, B, T, H, NS, ids.data(), BAD, emb.data(), 2.0f, y.data()), wt);
    }
    auto layernorm = [&](const char* what, int alias, bool opts, int nparts, const int32_t* len, bool expect_refusal = false) {
        const int C = 5;
        const size_t n = (size_t)B * C * T, stride = n + 3;
        auto x = F((nparts - 1) * stride + n), bias = F(C), res = F(n), add = F(n), gamma = F(C, 1.0f, 1.0f), beta = F(C), y = F(n);
        mi355vits_layernorm_test t{};
        t.B = B; t.C = C; t.T = T; t.nparts = nparts; t.gelu = opts; t.alias = alias; t.eps = 1e-5f; t.part_stride = (int64_t)stride;
        t.x = x.data(); t.gamma = gamma.data(); t.beta = beta.data(); t.y = y.data();
        t.bias = opts ? bias.data() : nullptr;
        t.premask_len = opts ? len : nullptr;
        t.out_len = opts ? len : nullptr;
        t.res = opts || alias == 2 ? res.data() : nullptr;
        t.add_to = opts || alias == 3 ? add.data() : nullptr;
        Watch wt;
        wt.add(y);
        const int rc = mi355vits_test_layernorm(0, &t);
        if (expect_refusal) refused(what, rc, wt);
        else ok(what, rc);
    };
    layernorm("layernorm alias 0, every option, two slices", 0, true, 2, LEN);
    layernorm("layernorm alias 0, no option", 0, false, 1, LEN);
    layernorm("layernorm alias 1", 1, false, 1, LEN);
    layernorm("layernorm alias 2", 2, false, 1, LEN);
    layernorm("layernorm alias 3, every option", 3, true, 1, LEN);
    layernorm("layernorm, out_len T + 1", 0, true, 1, BAD, true);
    {
        const int gin = 6, NS = 3, Cout = 5;
        auto emb = F((size_t)NS * gin), w = F((size_t)Cout * gin), bias = F(Cout), out = F((size_t)B * Cout + 3);
        const int64_t sid[B] = {2, 0};
        ok("speaker_cond, bias", mi355vits_test_speaker_cond(0, B, gin, NS, Cout, emb.data(), sid, w.data(), bias.data(), out.data(), out.size()));
        ok("speaker_cond, no bias", mi355vits_test_speaker_cond(0, B, gin, NS, Cout, emb.data(), sid, w.data(), nullptr, out.data(), out.size()));
        const int K = 2;
        const int64_t msid[B * K] = {2, 0, 1, 1};
        const float mw[B * K] = {0.25f, 0.75f, 1.0f, 0.0f};
        auto w2 = F((size_t)3 * gin), out2 = F((size_t)B * 3), g = F((size_t)B * gin + 1), vectors = F((size_t)B * gin);
        mi355vits_speaker_mix_test t{};
        t.B = B; t.gin = gin; t.n_speakers = NS; t.n_terms = K; t.n_jobs = 2;
        t.emb_g = emb.data(); t.mix_sid = msid; t.mix_weight = mw;
        t.w[0] = w.data(); t.bias[0] = bias.data(); t.Cout[0] = Cout; t.out[0] = out.data(); t.out_floats[0] = out.size();
        t.w[1] = w2.data(); t.bias[1] = nullptr; t.Cout[1] = 3; t.out[1] = out2.data(); t.out_floats[1] = out2.size();
        t.g = g.data(); t.g_floats = g.size();
        ok("speaker_cond_mix, a mix, bias given and withheld", mi355vits_test_speaker_cond_mix(0, &t));
        t.emb_g = nullptr; t.mix_sid = nullptr; t.mix_weight = nullptr; t.n_terms = 0; t.vectors = vectors.data();
        ok("speaker_cond_mix, vectors", mi355vits_test_speaker_cond_mix(0, &t));
    }
    {
        const int hop = 4, bs = T * hop + 1;
        std::vector<int32_t> cum((size_t)B * T), alen = {LEN[0] * hop, LEN[1] * hop}, ramp = {8, 0};
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < T; ++t) cum[(size_t)b * T + t] = t + 1;
        auto gain = F((size_t)B * T, 1.0f, 1.0f), ratio = F((size_t)B * T, 0.5f, 1.0f), audio = F((size_t)B * bs + 5), peaks = F(B);
        ok("levels, ramp", mi355vits_test_levels(0, B, T, hop, cum.data(), LEN, gain.data(), ramp.data(), alen.data(), bs, audio.data(), audio.size(), peaks.data()));
        ok("levels, no ramp", mi355vits_test_levels(0, B, T, hop, cum.data(), LEN, gain.data(), nullptr, alen.data(), bs, audio.data(), audio.size(), peaks.data()));
        {
            Watch wt;
            wt.add(audio); wt.add(peaks);
            refused("levels, len T + 1", mi355vits_test_levels(0, B, T, hop, cum.data(), BAD, gain.data(), ramp.data(), alen.data(), bs, audio.data(), audio.size(), peaks.data()), wt);
        }
        std::vector<int64_t> tq((size_t)B * T, -7);
        std::vector<int32_t> wc((size_t)B * T, -7), wlen(B, -7);
        ok("pitch_plan, ratio", mi355vits_test_pitch_plan(0, B, T, hop, cum.data(), LEN, ratio.data(), tq.data(), wc.data(), wlen.data()));
        ok("pitch_plan, no ratio", mi355vits_test_pitch_plan(0, B, T, hop, cum.data(), LEN, nullptr, tq.data(), wc.data(), wlen.data()));
        const int y_ld = 2 * T * hop + 8, y_bs = y_ld + 1;
        auto x = F((size_t)B * bs + 5), y = F((size_t)B * y_bs + 5);
        ok("pitch, ratio", mi355vits_test_pitch(0, B, T, hop, cum.data(), LEN, ratio.data(), x.data(), bs, x.size(), y.data(), y_bs, y_ld, y.size(), peaks.data(), wlen.data()));
        ok("pitch, no ratio", mi355vits_test_pitch(0, B, T, hop, cum.data(), LEN, nullptr, x.data(), bs, x.size(), y.data(), y_bs, y_ld, y.size(), peaks.data(), wlen.data()));
        Watch wt;
        wt.add(tq); wt.add(wc); wt.add(wlen); wt.add(y); wt.add(peaks);
        refused("pitch_plan, len T + 1", mi355vits_test_pitch_plan(0, B, T, hop, cum.data(), BAD, ratio.data(), tq.data(), wc.data(), wlen.data()), wt);
        refused("pitch, len T + 1", mi355vits_test_pitch(0, B, T, hop, cum.data(), BAD, ratio.data(), x.data(), bs, x.size(), y.data(), y_bs, y_ld, y.size(), peaks.data(), wlen.data()), wt);
    }
}

void timing_hooks() {
    float err = -1.0f, ms = -1.0f;
    ok("mfma_layout", mi355vits_test_mfma_layout(0, &err));
    ok("bench_conv1d, standard epilogue", mi355vits_bench_conv1d(0, 1, 2, 32, T, 3, 1, 0, 1, &ms));
    ok("bench_conv1d, gate", mi355vits_bench_conv1d(0, 1, 2, 64, T, 3, 1, 1, 1, &ms));
    ok("bench_conv1d, res / skip", mi355vits_bench_conv1d(0, 1, 2, 64, T, 1, 1, 2, 1, &ms));
    double probe[8];
    ok("probe_device", mi355vits_probe_device(0, probe));
}

}  // namespace

int main() {
    scope_checks();
    conv_hooks();
    audio_hooks();
    attention_and_flow_hooks();
    sdp_hooks();
    text_and_speaker_hooks();
    timing_hooks();
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
