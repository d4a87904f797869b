// lab_api.cpp — the hooks of include/mi355vits_lab.h: kernel unit tests, a conv micro-benchmark, the box probes, the MFMA layout
// self test.  NOT part of the product library (libmi355vits.so exports include/mi355vits.h only): linked into
//   libmi355vits_hooks.so   the product's own objects + this file (the kernel-level GPU tests run the product's kernels through it),
//   libmi355vits_lab.so     the -DMI355_LAB build (A/B switches, tools/), and the CPU model of the kernels (tests/emu).
#include "c_api_internal.h"
#include "mi355vits_lab.h"

#include <algorithm>

extern "C" {

int mi355vits_probe_weights(mi355vits_handle h, double out[8]) {
    if (!h || !out) return MI355VITS_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->eng->mu);
    return guarded(h, [&] { h->eng->probe_weights(out); });
}

// ---- the conv hooks (include/mi355vits_lab.h says what each impl reads and writes at and past a row's lengths)
}  // extern "C"

namespace {
const float* const ALIGNED = reinterpret_cast<const float*>(uintptr_t(4096));  // a stand-in for a 16-byte aligned buffer (plan call: never read)

struct ConvHookOpts { bool bias, res, cond, in_len, out_len, relu, res_sub, accumulate, mask_before_res; float out_scale; };

// the launch arguments of mi355vits_test_conv1d without its buffers, after the checks the hook makes before any launch
ConvArgs conv_hook_args(int impl, int B, int Cin, int Cout, int T, int K, int dil, int math, int fixed_rule, const ConvHookOpts& o) {
    if (impl < 0 || impl > 4) throw EngineError(MI355VITS_ERR_INVALID, "impl must be 0 .. 4");
    if (B < 1 || Cin < 1 || Cout < 1 || T < 1 || K < 1 || dil < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
    if ((size_t)B * std::max(Cin, Cout) * T >= 0x7fffffffull / 4) throw EngineError(MI355VITS_ERR_INVALID, "tensor too large for the hook");
    const bool ok_math = impl <= 1 ? math == MATH_F32 : impl == 4 ? math == MATH_BF16X3 : (math == MATH_BF16X3 || math == MATH_BF16W);
    if (!ok_math) throw EngineError(MI355VITS_ERR_INVALID, "math mode: MATH_F32 for impl 0 and 1, MATH_BF16X3 or MATH_BF16W for impl 2 and 3, MATH_BF16X3 for impl 4");
    if (fixed_rule && impl != 1 && impl != 2) throw EngineError(MI355VITS_ERR_INVALID, "fixed_rule: impl 1 and 2 only");
    ConvArgs a;
    a.x_bs = (long)Cin * T; a.x_ld = T;
    a.y_bs = (long)Cout * T; a.y_ld = T;
    a.B = B; a.Cin = Cin; a.Cout = Cout; a.T = T; a.K = K; a.dil = dil;
    a.pad = (K * dil - dil) / 2;
    a.relu = o.relu; a.out_scale = o.out_scale; a.res_sub = o.res_sub; a.accumulate = o.accumulate; a.mask_before_res = o.mask_before_res;
    a.math = math;
    a.fixed_rule = fixed_rule ? 1 : 0;
    if (o.res) { a.res_bs = a.y_bs; a.res_ld = T; }
    if (o.cond) a.cond_bs = Cout;
    if (impl == 3) {  // the encoder's slice kernel (k_enc_b3); split convs: the raw slice sums added up by the hook, no epilogue
        if (!enc_conv_b3_supported(Cin, Cout, K, dil)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the encoder slice kernel");
        a.ksplit = enc_conv_b3_slices(Cin);
        if (a.ksplit > 1 && (o.bias || o.res || o.relu || o.accumulate || o.cond || o.res_sub || o.mask_before_res || o.out_len || o.out_scale != 1.0f))
            throw EngineError(MI355VITS_ERR_INVALID, "split conv: raw sums only");
    } else if (impl == 4) {  // the 128-channel resblock conv with every input channel resident (k_rb_conv / k_rb_conv_pw)
        ConvArgs c = a;
        c.res = o.res ? ALIGNED : nullptr; c.in_len = o.in_len ? reinterpret_cast<const int*>(ALIGNED) : nullptr;
        c.cond = o.cond ? ALIGNED : nullptr; c.out_len = o.out_len ? reinterpret_cast<const int*>(ALIGNED) : nullptr;
        if (!rb_conv_supported(c)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the resident-input kernel");
    } else if (impl == 1 || impl == 2) {
        if (!conv1d_mfma_supported(Cin, Cout, K, dil)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the MFMA kernel");
        if (impl == 2 && !conv1d_b3_supported(Cin, Cout, K, dil, fixed_rule ? 1 << 30 : T))
            throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the split-bf16 kernel");
    }
    return a;
}

// the polyphase view of mi355vits_test_conv_transpose1d impl 1 - 3 (ConvArgs::shuf_*), without its buffers
ConvArgs convt_hook_args(int impl, int B, int Cin, int Cout, int Tin, int K, int stride) {
    const int taps = convt_taps(K, stride);
    ConvArgs u;
    u.x_bs = (long)Cin * Tin; u.x_ld = Tin;
    u.y_bs = (long)Cout * Tin * stride; u.y_ld = Tin * stride;
    u.Cin = Cin; u.Cout = stride * Cout; u.K = taps; u.dil = 1;
    u.pad = taps - 1; u.Tin = Tin;
    u.shuf_s = stride; u.shuf_p = (K - stride) / 2; u.shuf_cout = Cout; u.shuf_T = Tin * stride;
    u.B = B; u.T = Tin + taps - 1;
    if (impl >= 2) u.math = MATH_BF16X3;
    if (impl == 2) u.fixed_rule = 1;
    return u;
}

void convt_hook_check(int impl, int B, int Cin, int Cout, int Tin, int K, int stride, bool has_len) {
    if (impl < 0 || impl > 3) throw EngineError(MI355VITS_ERR_INVALID, "impl must be 0 .. 3");
    if (B < 1 || Cin < 1 || Cout < 1 || Tin < 1 || K < 1 || stride < 1 || K < stride || ((K - stride) & 1))
        throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
    if ((size_t)B * std::max(Cin, Cout * stride) * Tin >= 0x7fffffffull / 4) throw EngineError(MI355VITS_ERR_INVALID, "tensor too large for the hook");
    if (has_len && impl != 3) throw EngineError(MI355VITS_ERR_INVALID, "per-row lengths: impl 3 only");
    if ((impl == 1 || impl == 2) && !conv1d_mfma_supported(Cin, stride * Cout, convt_taps(K, stride), 1))
        throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the MFMA kernel");
    if (impl == 2 && !conv1d_b3_supported(Cin, stride * Cout, convt_taps(K, stride), 1, 1 << 30))
        throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the split-bf16 kernel");
}

void check_lens(const int32_t* len, int B, long T, const char* what) {
    for (int b = 0; len && b < B; ++b)
        if (len[b] < 0 || len[b] > T) throw EngineError(MI355VITS_ERR_INVALID, what);
}

// packed bit patterns travel as floats (ConvArgs::w / wb3 and the like)
const float* in_words(HookScope& s, const std::vector<uint32_t>& p) { return reinterpret_cast<const float*>(s.in(p)); }
}  // namespace

extern "C" {

int mi355vits_test_conv1d(int device, const mi355vits_conv_test* t) {
    return guarded(nullptr, [&] {
        if (!t || !t->x || !t->w || !t->y) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        const ConvHookOpts o{t->bias != nullptr, t->res != nullptr, t->cond != nullptr, t->in_len != nullptr, t->out_len != nullptr, t->relu != 0,
                             t->res_sub != 0, t->accumulate != 0, t->mask_before_res != 0, t->out_scale};
        ConvArgs a = conv_hook_args(t->impl, t->B, t->Cin, t->Cout, t->T, t->K, t->dilation, t->math, t->fixed_rule, o);
        check_lens(t->in_len, t->B, t->T, "in_len out of range");
        check_lens(t->out_len, t->B, t->T, "out_len out of range");
        HookScope s(device);
        const size_t nx = (size_t)t->B * t->Cin * t->T, ny = (size_t)t->B * t->Cout * t->T;
        a.x = s.in(t->x, nx);
        a.y = s.in<float>(t->y, ny);  // a position no kernel writes keeps the caller's value
        a.in_slope = t->in_slope;
        a.bias = s.in(t->bias, (size_t)t->Cout);
        a.res = s.in(t->res, ny);
        a.cond = s.in(t->cond, (size_t)t->B * t->Cout);
        a.in_len = s.in(t->in_len, (size_t)t->B);
        a.out_len = s.in(t->out_len, (size_t)t->B);
        if (t->impl == 3) {
            a.wb3 = in_words(s, conv_weights_bf16x3_staged(t->w, t->Cout, t->Cin, t->K));
            if (a.ksplit > 1) a.part = s.scratch<float>(ny * (size_t)a.ksplit);
            launch_enc_conv_b3(a, nullptr);
        } else if (t->impl == 4) {
            a.w = in_words(s, conv_weights_p16(t->w, t->Cout, t->Cin, t->K));
            a.in_len_host = t->in_len;
            launch_rb_conv(a, nullptr);
        } else if (t->impl == 1 || t->impl == 2) {
            a.w = s.in(conv_weights_mfma(t->w, t->Cout, t->Cin, t->K));
            // impl 2: the split-bf16 staged kernel (MATH_BF16X3 / MATH_BF16W)
            if (t->impl == 2) a.wb3 = in_words(s, conv_weights_bf16x3_staged(t->w, t->Cout, t->Cin, t->K));
            launch_conv1d_mfma(a, nullptr);
        } else {
            a.w = s.in(t->w, (size_t)t->Cout * t->Cin * t->K);
            launch_conv1d_generic(a, nullptr);
        }
        s.finish();
        if (t->impl == 3 && a.ksplit > 1) {
            std::vector<float> parts(ny * (size_t)a.ksplit);
            s.fetch(parts.data(), a.part, parts.size());
            for (size_t i = 0; i < ny; ++i) {
                float v = parts[i];
                for (int sl = 1; sl < a.ksplit; ++sl) v += parts[(size_t)sl * ny + i];
                t->y[i] = v;
            }
            return;
        }
        s.fetch(t->y, a.y, ny);
    });
}

int mi355vits_lab_conv_plan(int impl, int B, int Cin, int Cout, int T, int K, int dilation, int stride, int math, int fixed_rule,
                            int has_res, int has_cond, const int32_t* len, mi355vits_conv_plan* out) {
    return guarded(nullptr, [&] {
        if (!out) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        ConvPlan p;
        if (stride > 0) {
            convt_hook_check(impl, B, Cin, Cout, T, K, stride, len != nullptr);
            check_lens(len, B, T, "in_len out of range");
            if (impl == 0) {
                ConvTArgs a;
                a.B = B; a.Cin = Cin; a.Cout = Cout; a.Tin = T; a.K = K; a.stride = stride; a.pad = (K - stride) / 2;
                p = conv_transpose1d_plan(a);
            } else {
                ConvArgs u = convt_hook_args(impl, B, Cin, Cout, T, K, stride);
                u.x = u.w = u.bias = ALIGNED;
                u.y = const_cast<float*>(ALIGNED);
                if (impl == 2) u.wb3 = ALIGNED;
                if (impl == 3) {
                    std::vector<int> lens = len ? std::vector<int>(len, len + B) : std::vector<int>((size_t)B, T);
                    u.in_len = reinterpret_cast<const int*>(ALIGNED);
                    u.in_len_host = lens.data();
                    if (!ups_pl_supported(u)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the resident-input polyphase kernels");
                    p = ups_pl_plan(u);
                } else {
                    p = conv1d_mfma_plan(u);
                }
            }
        } else {
            const ConvHookOpts o{false, has_res != 0, has_cond != 0, len != nullptr, false, false, false, false, false, 1.0f};
            ConvArgs a = conv_hook_args(impl, B, Cin, Cout, T, K, dilation, math, fixed_rule, o);
            check_lens(len, B, T, "in_len out of range");
            a.x = a.w = ALIGNED;
            a.y = const_cast<float*>(ALIGNED);
            if (has_res) a.res = ALIGNED;
            if (has_cond) a.cond = ALIGNED;
            if (impl >= 2) a.wb3 = ALIGNED;
            if (len) { a.in_len = reinterpret_cast<const int*>(ALIGNED); a.in_len_host = len; }
            p = impl == 0 ? conv1d_generic_plan(a) : impl <= 2 ? conv1d_mfma_plan(a) : impl == 3 ? enc_conv_b3_plan(a) : rb_conv_plan(a);
        }
        out->kernel = p.kernel; out->cols = p.cols; out->rows = p.rows;
        out->MT = p.MT; out->NT = p.NT; out->WM = p.WM; out->WN = p.WN;
        out->chunk = p.chunk; out->ring = p.ring; out->rb_loop = p.rb_loop;
        out->vec = p.vec; out->yvec = p.yvec; out->ovec = p.ovec;
        out->grid[0] = (int32_t)p.gx; out->grid[1] = (int32_t)p.gy; out->grid[2] = (int32_t)p.gz;
        out->lds_bytes = (int32_t)p.shmem;
    });
}

int mi355vits_test_enc_o_ln(int device, int math, int B, int T, const float* x, const float* w, const float* bias, const float* res,
                            const float* gamma, const float* beta, float eps, const int32_t* in_len, const int32_t* ln_out_len,
                            int in_place, float* y) {
    return guarded(nullptr, [&] {
        if (!x || !w || !res || !gamma || !beta || !y) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1 || (size_t)B * 192 * T >= 0x7fffffffull / 4) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        if (math != MATH_BF16X3 && math != MATH_BF16W) throw EngineError(MI355VITS_ERR_INVALID, "math mode: MATH_BF16X3 or MATH_BF16W");
        check_lens(in_len, B, T, "in_len out of range");
        check_lens(ln_out_len, B, T, "ln_out_len out of range");
        const int C = 192;
        if (!enc_o_ln_supported(C, C, 1)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported");
        HookScope s(device);
        const size_t n = (size_t)B * C * T;
        float* dres = s.in(res, n);
        float* dy = in_place ? dres : s.in<float>(y, n);  // in place: the one device pointer serves as residual and as output
        ConvArgs c;
        c.x = s.in(x, n); c.x_bs = (long)C * T; c.x_ld = T;
        c.res = dres; c.res_bs = (long)C * T; c.res_ld = T;
        c.y = dy; c.y_bs = (long)C * T; c.y_ld = T;
        c.wb3 = in_words(s, conv_weights_bf16x3_staged(w, C, C, 1));
        c.math = math;
        c.B = B; c.Cin = C; c.Cout = C; c.T = T; c.K = 1; c.dil = 1; c.pad = 0;
        c.bias = s.in(bias, (size_t)C);
        c.in_len = s.in(in_len, (size_t)B);
        launch_enc_o_ln(c, s.in(gamma, (size_t)C), s.in(beta, (size_t)C), s.in(ln_out_len, (size_t)B), eps, nullptr);
        s.finish();
        s.fetch(y, dy, n);
    });
}

int mi355vits_test_conv_post(int device, int B, int Cin, int K, int L, const float* x, const float* w, const int32_t* valid_len,
                             const double* volumes, float* audio, float* peaks, int16_t* pcm, int32_t* kernel) {
    return guarded(nullptr, [&] {
        if (!x || !w || !valid_len || !audio || !peaks || !pcm) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || Cin < 1 || K < 1 || !(K & 1) || L < 1 || (size_t)B * Cin * L >= 0x7fffffffull / 4) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        check_lens(valid_len, B, L, "valid_len out of range");
        HookScope s(device);
        const size_t nx = (size_t)B * Cin * L, na = (size_t)B * L;
        const float* dx = s.in(x, nx);
        const float* dw = s.in(w, (size_t)Cin * K);
        const int* dl = s.in(valid_len, (size_t)B);
        const double* dv = s.in(volumes, (size_t)B);
        float* da = s.inout(audio, na);
        unsigned* dp = s.filled<unsigned>((size_t)B, 0);  // the peaks are an atomic maximum over bit patterns: zeroed before the launch, as the engine does
        int16_t* dq = s.inout(pcm, na);
        if (kernel) *kernel = conv_post_kernel(dx, (long)Cin * L, L, Cin, K, da, L);
        launch_conv_post_tanh(dx, (long)Cin * L, L, dw, Cin, K, B, L, dl, da, L, dp, nullptr);
        launch_pcm16(da, L, dp, dl, B, L, dq, L, nullptr, dv);
        s.finish();
        s.fetch(peaks, dp, (size_t)B);
    });
}

int mi355vits_test_resample(int device, int B, int64_t row_stride, const float* x, const int32_t* lengths, int32_t in_hz,
                            int32_t out_hz, int64_t y_stride, float* y, int32_t* y_lengths, float* peaks) {
    return guarded(nullptr, [&] {
        if (!x || !lengths || !y || !y_lengths || !peaks || B < 1 || row_stride < 1 || y_stride < 1 || y_stride > 0x7fffffffLL)
            throw EngineError(MI355VITS_ERR_INVALID, "null or empty argument");
        ResampleFilter f;
        if (!resample_design(in_hz, out_hz, f)) throw EngineError(MI355VITS_ERR_INVALID, "rate pair not supported");
        std::vector<int> tab(resample_tab_ints(B));
        check_lens(lengths, B, row_stride, "row length out of range");
        for (int b = 0; b < B; ++b)
            if (resample_out_len(lengths[b], f.L, f.M) > y_stride) throw EngineError(MI355VITS_ERR_INVALID, "row length out of range");
        const long items = resample_fill_tab(f, lengths, B, tab.data());
        HookScope s(device);
        const size_t ny = (size_t)B * y_stride;
        float* dy = s.filled<float>(ny, 0xff);  // NaNs: the kernel writes every sample of y
        unsigned* dp = s.filled<unsigned>((size_t)B, 0);
        launch_resample(f, s.in(f.table), s.in(x, (size_t)B * row_stride), (long)row_stride, s.in(lengths, (size_t)B), B, s.in(tab), items, dy,
                        (long)y_stride, (int)y_stride, dp, nullptr);
        s.finish();
        s.fetch(y, dy, ny);
        s.fetch(peaks, dp, (size_t)B);
        for (int b = 0; b < B; ++b) y_lengths[b] = tab[b];
    });
}

int mi355vits_test_alignment(int device, int B, int T, const int32_t* frames, const int32_t* len, int64_t row_stride, const float* audio,
                             const int32_t* alen, int32_t hop, int32_t L, int32_t M, int32_t* out_frames, int32_t* out_start,
                             int32_t* out_samples, float* out_peak, float* out_rms) {
    return guarded(nullptr, [&] {
        if (!frames || !len || !audio || !alen || !out_frames || !out_start || !out_samples || B < 1 || T < 1 || row_stride < 1)
            throw EngineError(MI355VITS_ERR_INVALID, "null or empty argument");
        if ((out_peak == nullptr) != (out_rms == nullptr)) throw EngineError(MI355VITS_ERR_INVALID, "peak and rms: both or neither");
        if (hop < 1 || L < 1 || M < 1 || L > RESAMPLE_MAX_RATIO || M > RESAMPLE_MAX_RATIO) throw EngineError(MI355VITS_ERR_INVALID, "hop, L, M out of range");
        const size_t n = (size_t)B * T;
        // cum = the inclusive scan of the frames a row's phonemes have (k_durations' d_cum_); behind a row's count it is left as
        // a pattern: the kernel must not look there
        std::vector<int> cum(n, 0x7f7f7f7f);
        for (int b = 0; b < B; ++b) {
            if (len[b] < 0 || len[b] > T || alen[b] < 0 || alen[b] > row_stride) throw EngineError(MI355VITS_ERR_INVALID, "row length out of range");
            long long acc = 0;
            for (int t = 0; t < len[b]; ++t) {
                const int f = frames[(size_t)b * T + t];
                if (f < 0 || f > DURATION_FRAME_CAP) throw EngineError(MI355VITS_ERR_INVALID, "frames out of range");
                acc += f;
                if (acc > DURATION_FRAME_CAP) throw EngineError(MI355VITS_ERR_INVALID, "a row's frames exceed the duration cap");
                cum[(size_t)b * T + t] = (int)acc;
            }
            if (resample_out_len(acc * hop, L, M) > 0x7fffffffLL) throw EngineError(MI355VITS_ERR_INVALID, "row does not fit 32 bits");
        }
        HookScope s(device);
        int* d = s.filled<int>(5 * n, 0xff);  // five planes; the kernel writes every element it is asked for
        launch_align(s.in(frames, n), s.in(cum), s.in(len, (size_t)B), B, T, s.in(audio, (size_t)B * row_stride), (long)row_stride,
                     s.in(alen, (size_t)B), hop, L, M, d, d + n, d + 2 * n, out_peak ? reinterpret_cast<float*>(d + 3 * n) : nullptr,
                     out_peak ? reinterpret_cast<float*>(d + 4 * n) : nullptr, nullptr);
        s.finish();
        s.fetch(out_frames, d, n);
        s.fetch(out_start, d + n, n);
        s.fetch(out_samples, d + 2 * n, n);
        if (out_peak) {
            s.fetch(out_peak, d + 3 * n, n);
            s.fetch(out_rms, d + 4 * n, n);
        }
    });
}

int mi355vits_lab_g711_encode(int law, const int16_t* in, long n, uint8_t* out) {
    return guarded(nullptr, [&] {
        if (!in || !out || n < 1) throw EngineError(MI355VITS_ERR_INVALID, "null or empty argument");
        if (law != MI355VITS_ENC_ULAW && law != MI355VITS_ENC_ALAW) throw EngineError(MI355VITS_ERR_INVALID, "law must be MI355VITS_ENC_ULAW or MI355VITS_ENC_ALAW");
        HookScope s;
        uint8_t* dout = s.scratch<uint8_t>((size_t)n);
        launch_g711_encode(law, s.in(in, (size_t)n), n, dout, nullptr);
        s.finish();
        s.fetch(out, dout, (size_t)n);
    });
}

int mi355vits_lab_flac(const int16_t* pcm, long n, int32_t rate, int32_t first_frame, uint8_t* out, size_t cap, size_t* n_bytes,
                       int32_t* frame_sizes) {
    return guarded(nullptr, [&] {
        if (n_bytes) *n_bytes = 0;
        if ((!pcm && n > 0) || !out || !n_bytes || n < 0 || n > 0x7fffffffL) throw EngineError(MI355VITS_ERR_INVALID, "null argument or n out of range");
        if (rate < 1 || rate > FLAC_MAX_RATE) throw EngineError(MI355VITS_ERR_INVALID, "rate must be in [1, 1048575]");
        const long frames = flac_frames(n);
        if (first_frame < 0 || (long)first_frame + frames > FLAC_MAX_FRAME_NUMBER + 1) throw EngineError(MI355VITS_ERR_INVALID, "frame numbers must stay below 2^21");
        const size_t lead = n > 0 ? (reinterpret_cast<uintptr_t>(pcm) & 15) : 0;  // the host pointer's place behind a 16-byte boundary, kept
        HookScope s;
        int16_t* src = reinterpret_cast<int16_t*>(s.scratch<uint8_t>(lead + (size_t)n * 2 + 16) + lead);
        if (n > 0) s.put(src, pcm, (size_t)n);
        const FlacJob job = {src, n, first_frame, 0};
        uint8_t* dslots = s.scratch<uint8_t>((size_t)frames * FLAC_SLOT_BYTES);
        int* dsizes = s.scratch<int>((size_t)frames + 1);
        uint8_t* dout = s.scratch<uint8_t>(flac_out_capacity(frames, n));
        launch_flac_frames(s.in(&job, 1), 1, frames, rate, dslots, dsizes, nullptr);
        launch_flac_gather(dslots, dsizes, s.scratch<long long>((size_t)frames), frames, dout, nullptr);
        s.finish();
        std::vector<int> sizes((size_t)frames + 1, 0);
        if (frames > 0) s.fetch(sizes.data(), dsizes, sizes.size());
        size_t data = 0;
        for (long f = 0; f < frames; ++f) {
            if (sizes[f] < 11 || sizes[f] > 16 + 2 * FLAC_BLOCK) throw EngineError(MI355VITS_ERR_INTERNAL, "flac: frame " + std::to_string(f) + " has " + std::to_string(sizes[f]) + " bytes");
            data += (size_t)sizes[f];
        }
        if ((unsigned)sizes[frames] != (unsigned)data) throw EngineError(MI355VITS_ERR_INTERNAL, "flac: the device's total differs from the sum of the frame sizes");
        *n_bytes = FLAC_HEADER_BYTES + data;
        if (cap < *n_bytes) throw EngineError(MI355VITS_ERR_INVALID, "flac: the file has " + std::to_string(*n_bytes) + " bytes, out holds " + std::to_string(cap));
        flac_stream_header(out, rate, n, sizes.data(), frames);
        s.fetch(out + FLAC_HEADER_BYTES, dout, data);
        if (frame_sizes)
            for (long f = 0; f < frames; ++f) frame_sizes[f] = sizes[f];
    });
}

int mi355vits_lab_flac_jobs(const int16_t* const* pcm, const long* n, int32_t n_jobs, int32_t rate, uint8_t* out, size_t cap,
                            size_t* n_bytes, int64_t* offsets, int64_t* sizes_out) {
    return guarded(nullptr, [&] {
        if (n_bytes) *n_bytes = 0;
        if (!pcm || !n || !out || !n_bytes || !offsets || !sizes_out || n_jobs < 1) throw EngineError(MI355VITS_ERR_INVALID, "null argument or no job");
        if (rate < 1 || rate > FLAC_MAX_RATE) throw EngineError(MI355VITS_ERR_INVALID, "rate must be in [1, 1048575]");
        long frames = 0, bound = 0;
        size_t src_bytes = 0;
        std::vector<size_t> at((size_t)n_jobs);
        for (int j = 0; j < n_jobs; ++j) {
            if (n[j] < 0 || n[j] > 0x7fffffffL || (!pcm[j] && n[j] > 0)) throw EngineError(MI355VITS_ERR_INVALID, "job " + std::to_string(j) + ": null array or n out of range");
            if (flac_frames(n[j]) > FLAC_MAX_FRAME_NUMBER + 1) throw EngineError(MI355VITS_ERR_INVALID, "frame numbers must stay below 2^21");
            at[(size_t)j] = src_bytes + (n[j] > 0 ? (reinterpret_cast<uintptr_t>(pcm[j]) & 15) : 0);  // the host pointer's place behind a 16-byte boundary, kept
            src_bytes = (at[(size_t)j] + (size_t)n[j] * 2 + 15) & ~size_t(15);
            frames += flac_frames(n[j]);
            bound += flac_file_bound(n[j]);
            if (bound > 0x7fffffffL) throw EngineError(MI355VITS_ERR_INVALID, "the block's bound exceeds 2^31 - 1 bytes");
        }
        HookScope s;
        uint8_t* din = s.scratch<uint8_t>(src_bytes + 16);
        uint8_t* dslots = s.scratch<uint8_t>((size_t)frames * FLAC_SLOT_BYTES + 16);
        int* dsizes = s.scratch<int>(flac_info_words(frames, n_jobs));
        int2* dftab = s.scratch<int2>((size_t)frames + 1);
        unsigned* dhdr = s.scratch<unsigned>((size_t)FLAC_HDR_WORDS * n_jobs);
        int* ditems = s.scratch<int>(flac_gather_items(bound));
        uint8_t* dout = s.filled<uint8_t>((size_t)bound + 16, 0xa5);  // the gather writes every byte of the block
        std::vector<FlacJob> jobs((size_t)n_jobs);
        long slot0 = 0;
        for (int j = 0; j < n_jobs; ++j) {
            int16_t* src = reinterpret_cast<int16_t*>(din + at[(size_t)j]);
            if (n[j] > 0) s.put(src, pcm[j], (size_t)n[j]);
            jobs[(size_t)j] = FlacJob{src, n[j], 0, (int)slot0};
            slot0 += flac_frames(n[j]);
        }
        const FlacJob* djobs = s.in(jobs);
        launch_flac_frames(djobs, n_jobs, frames, rate, dslots, dsizes, nullptr);
        launch_flac_place(djobs, n_jobs, frames, rate, 0, dsizes, s.scratch<unsigned>((size_t)frames + 1), dftab, dhdr, ditems,
                          s.scratch<int>((size_t)FLAC_JTAB_ROWS * n_jobs), nullptr);
        launch_flac_gather_streams(n_jobs, frames, dslots, dsizes, dftab, dhdr, ditems, 0, bound, dout, nullptr);
        s.finish();
        std::vector<int> info(flac_info_words(frames, n_jobs));
        s.fetch(info.data(), dsizes, info.size());
        const int* in = info.data() + frames;
        for (int j = 0; j < n_jobs; ++j) {
            offsets[j] = in[FLAC_INFO_WORDS * j + FLAC_INFO_BASE];
            sizes_out[j] = in[FLAC_INFO_WORDS * j + FLAC_INFO_BYTES];
            if (offsets[j] < 0 || (offsets[j] & 15) || sizes_out[j] < FLAC_HEADER_BYTES || offsets[j] + sizes_out[j] > bound)
                throw EngineError(MI355VITS_ERR_INTERNAL, "flac: job " + std::to_string(j) + " placed outside the bound");
        }
        const long end = in[FLAC_INFO_WORDS * n_jobs];
        if (end != offsets[n_jobs - 1] + sizes_out[n_jobs - 1]) throw EngineError(MI355VITS_ERR_INTERNAL, "flac: the block's end differs from the last file's");
        *n_bytes = (size_t)end;
        if (cap < *n_bytes) throw EngineError(MI355VITS_ERR_INVALID, "flac: the block has " + std::to_string(*n_bytes) + " bytes, out holds " + std::to_string(cap));
        s.fetch(out, dout, (size_t)end);
    });
}

int mi355vits_lab_edges(const float* audio, long stride, const int32_t* lens, const float* peaks, int B, float ratio, int32_t* s_first,
                        int32_t* s_last) {
    return guarded(nullptr, [&] {
        if (!audio || !lens || !peaks || !s_first || !s_last || B < 1 || stride < 1) throw EngineError(MI355VITS_ERR_INVALID, "null or empty argument");
        if (!(ratio > 0.0f && ratio <= 1.0f)) throw EngineError(MI355VITS_ERR_INVALID, "ratio must be in (0, 1]");
        check_lens(lens, B, stride, "row length out of range");
        const long l_max = *std::max_element(lens, lens + B);
        HookScope s;
        int* d = s.filled<int>((size_t)B * 2, 0x5a);  // the launch initialises its words itself
        launch_edges(s.in(audio, (size_t)B * stride), stride, s.in(lens, (size_t)B), reinterpret_cast<const unsigned*>(s.in(peaks, (size_t)B)), B, l_max,
                     ratio, d, d + B, nullptr);
        s.finish();
        s.fetch(s_first, d, (size_t)B);
        s.fetch(s_last, d + B, (size_t)B);
    });
}

int mi355vits_lab_loudness(const float* audio, long stride, const int32_t* lens, int B, int32_t rate, double* lufs, int32_t* blocks,
                           int32_t* gated) {
    return guarded(nullptr, [&] {
        if (!audio || !lens || !lufs || !blocks || !gated || B < 1 || stride < 1) throw EngineError(MI355VITS_ERR_INVALID, "null or empty argument");
        LoudnessPlan lp;
        if (!loudness_plan(rate, lp)) throw EngineError(MI355VITS_ERR_INVALID, "rate " + std::to_string(rate) + " Hz is below " + std::to_string(LOUD_MIN_HZ) + " Hz");
        check_lens(lens, B, stride, "row length out of range");
        const long l_max = *std::max_element(lens, lens + B);
        const long ldE = std::max<long>(1, loudness_steps(l_max, lp.S));
        HookScope s;
        double* dE = s.filled<double>((size_t)B * ldE, 0xff);  // NaN: the launch writes every energy it reads
        double* d_lufs = s.filled<double>((size_t)B * 2, 0x5a);  // B doubles, then 2 B ints
        int* d_blocks = reinterpret_cast<int*>(d_lufs + B);
        launch_loudness(rate, s.in(audio, (size_t)B * stride), stride, s.in(lens, (size_t)B), B, l_max, dE, ldE, d_lufs, d_blocks, d_blocks + B, nullptr);
        s.finish();
        s.fetch(lufs, d_lufs, (size_t)B);
        s.fetch(blocks, d_blocks, (size_t)B);
        s.fetch(gated, d_blocks + B, (size_t)B);
    });
}

int mi355vits_lab_limit(const float* audio, long stride, const int32_t* lens, int B, const double* g, double c, double U, int32_t L,
                        float* scale_out, int64_t* sq_min, int32_t* reduced) {
    return mi355vits_lab_limit_env(audio, stride, lens, B, g, c, U, L, nullptr, scale_out, sq_min, reduced);
}

int mi355vits_lab_limit_env(const float* audio, long stride, const int32_t* lens, int B, const double* g, double c, double U, int32_t L,
                            const double* env, float* scale_out, int64_t* sq_min, int32_t* reduced) {
    return guarded(nullptr, [&] {
        if (!audio || !lens || !g || !scale_out || !sq_min || !reduced || B < 1 || stride < 1) throw EngineError(MI355VITS_ERR_INVALID, "null or empty argument");
        if (L < 1 || L > LIMIT_MAX_WINDOW) throw EngineError(MI355VITS_ERR_INVALID, "window " + std::to_string(L) + " is outside [1, " + std::to_string(LIMIT_MAX_WINDOW) + "]");
        if (!(c > 0.0 && std::isfinite(c)) || !(U > 0.0 && std::isfinite(U))) throw EngineError(MI355VITS_ERR_INVALID, "c and U must be finite and > 0");
        // one job per non-empty row; its curve goes where the row's samples are: scale_out has the audio's shape
        std::vector<LimitJob> jobs;
        for (int b = 0; b < B; ++b) {
            if (lens[b] < 0 || lens[b] > stride) throw EngineError(MI355VITS_ERR_INVALID, "row length out of range");
            if (!(g[b] > 0.0 && std::isfinite(g[b]))) throw EngineError(MI355VITS_ERR_INVALID, "g must be finite and > 0");
            sq_min[b] = (int64_t)(L + 1) << 30;
            reduced[b] = 0;
            if (lens[b] < 1) continue;
            LimitJob j;
            j.g = g[b]; j.c = c; j.U = U; j.row = b; j.n = lens[b]; j.off = j.tile0 = 0;
            jobs.push_back(j);
        }
        const size_t na = (size_t)B * stride;
        for (size_t i = 0; i < na; ++i) scale_out[i] = 0.0f;
        if (jobs.empty()) return;
        long floats = 0;
        const long tiles = limit_place_jobs(jobs.data(), (int)jobs.size(), &floats);
        if (tiles < 0) throw EngineError(MI355VITS_ERR_INVALID, "the curves together exceed 2^31 - 1 samples");
        HookScope s;
        LimitStat* ds = s.filled<LimitStat>(jobs.size(), 0x5a);  // the launch initialises its words itself
        float* dc = s.filled<float>((size_t)floats, 0xff);       // NaN: the launch writes every curve element
        double* de = env ? s.scratch<double>((size_t)floats) : nullptr;
        if (env)  // the jobs' envelopes one behind the other, as k_true_peak_env leaves them
            for (const LimitJob& j : jobs) s.put(de + j.off, env + (size_t)j.row * stride, (size_t)j.n);
        launch_limit(s.in(jobs), (int)jobs.size(), tiles, L, s.in(audio, na), stride, ds, dc, nullptr, de);
        s.finish();
        std::vector<LimitStat> st(jobs.size());
        std::vector<float> cv((size_t)floats);
        s.fetch(st.data(), ds, st.size());
        s.fetch(cv.data(), dc, cv.size());
        for (size_t j = 0; j < jobs.size(); ++j) {
            const int b = jobs[j].row;
            memcpy(scale_out + (size_t)b * stride, cv.data() + jobs[j].off, (size_t)jobs[j].n * 4);
            sq_min[b] = (int64_t)st[j].sq_min;
            reduced[b] = st[j].reduced;
        }
    });
}

int mi355vits_lab_true_peak(const float* audio, long stride, const int32_t* lens, int B, int32_t offset_floats, double* tp, double* env_out) {
    return guarded(nullptr, [&] {
        if (!audio || !lens || !tp || B < 1 || stride < 1) throw EngineError(MI355VITS_ERR_INVALID, "null or empty argument");
        if (offset_floats < 0 || offset_floats > 3) throw EngineError(MI355VITS_ERR_INVALID, "offset_floats must be 0 .. 3");
        check_lens(lens, B, stride, "row length out of range");
        const long l_max = *std::max_element(lens, lens + B);
        std::vector<LimitJob> jobs;  // the envelope form: one job per non-empty row
        for (int b = 0; b < B; ++b) {
            if (lens[b] < 1) continue;
            LimitJob j;
            j.g = j.c = j.U = 1.0; j.row = b; j.n = lens[b]; j.off = j.tile0 = 0;
            jobs.push_back(j);
        }
        const size_t na = (size_t)B * stride;
        HookScope s;
        float* d_audio = s.filled<float>(na + 4, 0xff) + offset_floats;  // NaN in front of the first row and behind the last
        s.put(d_audio, audio, na);
        double* dt = s.filled<double>((size_t)B, 0x5a);  // the launch initialises its words itself
        launch_true_peak(d_audio, stride, s.in(lens, (size_t)B), B, l_max, dt, nullptr);
        s.finish();
        s.fetch(tp, dt, (size_t)B);
        if (!env_out) return;
        for (size_t i = 0; i < na; ++i) env_out[i] = 0.0;
        if (jobs.empty()) return;
        long floats = 0;
        const long tiles = limit_place_jobs(jobs.data(), (int)jobs.size(), &floats);
        if (tiles < 0) throw EngineError(MI355VITS_ERR_INVALID, "the envelopes together exceed 2^31 - 1 samples");
        double* de = s.filled<double>((size_t)floats, 0xff);  // NaN: the launch writes every element
        launch_true_peak_env(s.in(jobs), (int)jobs.size(), tiles, d_audio, stride, de, nullptr);
        s.finish();
        for (const LimitJob& j : jobs) s.fetch(env_out + (size_t)j.row * stride, de + j.off, (size_t)j.n);
    });
}

int mi355vits_lab_true_peak_plan(double* taps, int32_t* tile) {
    return guarded(nullptr, [&] {
        if (taps) memcpy(taps, true_peak_taps(), sizeof(double) * TRUE_PEAK_TAPS);
        if (tile) *tile = TRUE_PEAK_TILE;
    });
}

int mi355vits_lab_loudness_plan(int32_t rate, int32_t* step, int32_t* warmup, int32_t* steps_per_item) {
    return guarded(nullptr, [&] {
        LoudnessPlan lp;
        if (!loudness_plan(rate, lp)) throw EngineError(MI355VITS_ERR_INVALID, "rate " + std::to_string(rate) + " Hz is below " + std::to_string(LOUD_MIN_HZ) + " Hz");
        if (step) *step = lp.S;
        if (warmup) *warmup = lp.W;
        if (steps_per_item) *steps_per_item = lp.K;
    });
}

int mi355vits_test_fill_workspace(mi355vits_handle h, uint32_t pattern) {
    if (!h) return MI355VITS_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->eng->mu);
    return guarded(h, [&] { h->eng->fill_workspace(pattern); });
}

int mi355vits_test_conv_transpose1d(int device, int impl, int B, int Cin, int Cout, int Tin, int K, int stride,
                                    const float* x, const float* w, const float* bias, float in_slope, const int32_t* in_len, float* y) {
    return guarded(nullptr, [&] {
        if (!x || !w || !y) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        convt_hook_check(impl, B, Cin, Cout, Tin, K, stride, in_len != nullptr);
        check_lens(in_len, B, Tin, "in_len out of range");
        HookScope s(device);
        const size_t nx = (size_t)B * Cin * Tin, ny = (size_t)B * Cout * Tin * stride;
        const float* dx = s.in(x, nx);
        float* dy = s.inout(y, ny);  // a position no kernel writes keeps the caller's value
        if (impl == 0) {
            ConvTArgs a;
            a.x = dx; a.x_bs = (long)Cin * Tin; a.x_ld = Tin;
            a.y = dy; a.y_bs = (long)Cout * Tin * stride; a.y_ld = Tin * stride;
            a.w = s.in(w, (size_t)Cin * Cout * K);
            a.bias = s.in(bias, (size_t)Cout);
            a.B = B; a.Cin = Cin; a.Cout = Cout; a.Tin = Tin; a.K = K; a.stride = stride; a.pad = (K - stride) / 2;
            a.in_slope = in_slope;
            launch_conv_transpose1d(a, nullptr);
        } else {
            // the polyphase filters [stride * Cout, Cin, taps] and their bias
            const int taps = convt_taps(K, stride), PC = stride * Cout;
            std::vector<float> wv((size_t)PC * Cin * taps), bv((size_t)PC);
            convt_to_polyphase(w, bias, Cin, Cout, K, stride, wv.data(), bv.data());
            ConvArgs u = convt_hook_args(impl, B, Cin, Cout, Tin, K, stride);
            u.x = dx;
            u.y = dy;
            u.bias = s.in(bv);
            u.in_slope = in_slope;
            if (impl == 3) {
                // the resident-input polyphase kernels (k_ups_pl: 256 -> 128, 128 -> 64; k_ups64: 64 -> 32), MATH_BF16X3; a valid length per
                // row is part of their contract (the engine always has one): in_len, or every row at full length
                const std::vector<int> lens = in_len ? std::vector<int>(in_len, in_len + B) : std::vector<int>((size_t)B, Tin);
                u.w = in_words(s, conv_weights_p16n(wv.data(), PC, Cin, taps));
                u.in_len = s.in(lens); u.in_len_host = lens.data();
                if (!ups_pl_supported(u)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the resident-input polyphase kernels");
                launch_ups_pl(u, nullptr);
            } else {
                // polyphase filters on the MFMA conv kernel (the path Engine uses); impl 2: the split-bf16 staged kernels
                // (MATH_BF16X3; 64-channel chunks run the persistent producer / consumer form)
                u.w = s.in(conv_weights_mfma(wv.data(), PC, Cin, taps));
                if (impl == 2) u.wb3 = in_words(s, conv_weights_bf16x3_staged(wv.data(), PC, Cin, taps));
                launch_conv1d_mfma(u, nullptr);
            }
        }
        s.finish();
    });
}

int mi355vits_test_rel_attention(int device, int impl, int B, int T, int H, int n_heads, int W, const float* qkv,
                                 const float* emb_rel_k, const float* emb_rel_v, const int32_t* len, float* out) {
    return guarded(nullptr, [&] {
        if (!qkv || !emb_rel_k || !emb_rel_v || !len || !out) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1 || n_heads < 1 || H % n_heads || W < 0) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        check_lens(len, B, T, "len out of range");
        const int d = H / n_heads, nrel = 2 * W + 1;
        if (impl == 0 && T > rel_attention_valu_cap(H, n_heads, W)) throw EngineError(MI355VITS_ERR_INVALID, "T beyond the VALU kernel's LDS row buffer");
        if (impl == 1 && !rel_attention_mfma_supported(T, H, n_heads, W)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the MFMA kernel");
        if (impl == 2 && !rel_attention_stream_supported(H, n_heads, W)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the streamed kernel");
        if (impl < 0 || impl > 2) throw EngineError(MI355VITS_ERR_INVALID, "impl must be 0, 1 or 2");
        HookScope s(device);
        const float* dq = s.in(qkv, (size_t)B * 3 * H * T);
        const float *dk = s.in(emb_rel_k, (size_t)nrel * d), *dv = s.in(emb_rel_v, (size_t)nrel * d);
        const int* dl = s.in(len, (size_t)B);
        float* dout = s.inout(out, (size_t)B * H * T);
        if (impl == 0) launch_rel_attention(dq, dk, dv, dl, B, T, H, n_heads, W, dout, nullptr);
        else if (impl == 1) launch_rel_attention_mfma(dq, dk, dv, dl, B, T, H, n_heads, W, dout, nullptr);
        else launch_rel_attention_stream(dq, dk, dv, dl, B, T, H, n_heads, W, dout, nullptr);
        s.finish();
    });
}

// one WaveNet layer through a chosen path (include/mi355vits_lab.h says what each reads and writes at and past len[b])
int mi355vits_test_wn_layer(int device, const mi355vits_wn_test* t) {
    return guarded(nullptr, [&] {
        if (!t || !t->h_in || !t->w_in || !t->b_in || !t->w_rs || !t->b_rs || !t->len || !t->h_out || !t->skip) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        const int B = t->B, H = t->H, T = t->T, K = t->K, dil = t->dilation, Crs = t->Crs;
        if (B < 1 || H < 1 || T < 1 || K < 1 || (K % 2) == 0 || dil < 1 || (Crs != H && Crs != 2 * H)) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        if ((long)B * H * T >= 0x7fffffffL / 4) throw EngineError(MI355VITS_ERR_INVALID, "tensor too large for the hook");
        check_lens(t->len, B, T, "len out of range");
        if (t->impl < 0 || t->impl > 2) throw EngineError(MI355VITS_ERR_INVALID, "impl must be 0, 1 or 2");
        if (t->impl == 2 ? t->math != MATH_BF16X3 : t->math != MATH_F32) throw EngineError(MI355VITS_ERR_INVALID, "math mode: MATH_F32 for impl 0 and 1, MATH_BF16X3 for impl 2");
        if (t->impl == 1 && !wn_layer_fused_supported(H, K, dil)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the fused f32 layer");
        if (t->impl == 2 && !wn_layer_b3_supported(H, K, dil)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the fused split-bf16 layer");
        HookScope s(device);
        const size_t n = (size_t)B * H * T;
        const long hbs = (long)H * T;
        float* dh = s.in(t->h_in, n);
        float* dho = s.in<float>(t->h_out, n);
        float* dsk = s.inout(t->skip, n);
        const float *dbi = s.in(t->b_in, (size_t)2 * H), *dbr = s.in(t->b_rs, (size_t)Crs), *dc = s.in(t->cond, (size_t)B * 2 * H);
        const int* dl = s.in(t->len, (size_t)B);
        const float* h_result = dho;
        if (t->impl == 0) {
            // Engine::coupling_layer's two launches: the gate conv h -> u (no input mask: the engine's h is zero past a row), then the
            // res/skip conv u -> (h in place, skip); weights in the forms Engine::pick_conv's MFMA_F32 / GENERIC read (each conv on its
            // own, as Engine::add_conv_data decides per conv: packed fragments where the MFMA kernel takes it, raw weights else)
            const bool mfma_in = conv1d_mfma_supported(H, 2 * H, K, 1), mfma_rs = conv1d_mfma_supported(H, Crs, 1, 1);
            float* du = s.scratch<float>(n);
            ConvArgs in;
            in.x = dh; in.x_bs = hbs; in.x_ld = T;
            in.y = du; in.y_bs = hbs; in.y_ld = T;
            in.epi = EPI_GATE; in.H = H; in.dil = dil;
            if (dc) { in.cond = dc; in.cond_bs = 2L * H; }
            in.B = B; in.T = T;
            in.fixed_rule = 1; in.Cin = H; in.Cout = 2 * H; in.K = K; in.bias = dbi; in.pad = (K * dil - dil) / 2;
            in.w = mfma_in ? s.in(conv_weights_mfma(t->w_in, 2 * H, H, K, EPI_GATE)) : s.in(t->w_in, (size_t)2 * H * H * K);
            in.math = MATH_F32;
            ConvArgs rs;
            rs.x = du; rs.x_bs = hbs; rs.x_ld = T;
            rs.y = dh; rs.y_bs = hbs; rs.y_ld = T;
            rs.y2 = dsk; rs.y2_bs = hbs; rs.y2_ld = T;
            rs.epi = EPI_RESSKIP; rs.H = H; rs.skip_init = t->skip_init != 0;
            rs.out_len = dl;
            rs.B = B; rs.T = T;
            rs.fixed_rule = 1; rs.Cin = H; rs.Cout = Crs; rs.K = 1; rs.bias = dbr; rs.pad = 0;
            rs.w = mfma_rs ? s.in(conv_weights_mfma(t->w_rs, Crs, H, 1)) : s.in(t->w_rs, (size_t)Crs * H);
            rs.math = MATH_F32;
            if (mfma_in) launch_conv1d_mfma(in, nullptr);
            else launch_conv1d_generic(in, nullptr);
            if (mfma_rs) launch_conv1d_mfma(rs, nullptr);
            else launch_conv1d_generic(rs, nullptr);
            h_result = dh;  // in place
        } else {
            WnArgs w;
            w.h_in = dh; w.h_out = dho; w.h_bs = hbs; w.h_ld = T;
            w.skip = dsk; w.s_bs = hbs; w.s_ld = T;
            w.b_in = dbi; w.b_rs = dbr;
            if (dc) { w.cond = dc; w.cond_bs = 2L * H; }
            w.len = dl;
            w.B = B; w.H = H; w.T = T; w.K = K; w.dil = dil; w.Crs = Crs; w.skip_init = t->skip_init != 0;
            if (t->impl == 1) {
                w.w_in = s.in(conv_weights_mfma(t->w_in, 2 * H, H, K, EPI_GATE));
                w.w_rs = s.in(conv_weights_mfma(t->w_rs, Crs, H, 1));
                launch_wn_layer(w, nullptr);
            } else {
                w.math = MATH_BF16X3;
                w.shape = wn_layer_b3_shape();
                if (w.shape != 32) {  // ConvW::packed_w16 of both convs (16x16x32 tiles)
                    w.w_in = in_words(s, conv_weights_w16(t->w_in, 2 * H, H, K, true));
                    w.w_rs = in_words(s, conv_weights_w16(t->w_rs, Crs, H, 1, false));
                } else {  // MI355VITS_WN_SHAPE=32 (lab build, CPU model): ConvW::packed_b3w of the gate conv, packed_b3s of the res/skip conv
                    w.w_in = in_words(s, conv_weights_bf16x3_staged(conv_weights_gate_tiles(t->w_in, 2 * H, H, K).data(), 2 * H, H, K));
                    w.w_rs = in_words(s, conv_weights_bf16x3_staged(t->w_rs, Crs, H, 1));
                }
                launch_wn_layer_b3(w, nullptr);
            }
        }
        s.finish();
        // impl 1 and 2: whatever the device's h_out holds now (Crs = H: the launch must have left it as it was); impl 0 works in place
        // on its copy of h, which a last layer leaves untouched: nothing to report then
        if (t->impl != 0 || Crs == 2 * H) s.fetch(t->h_out, h_result, n);
    });
}

// one DDS stack of the stochastic duration predictor through a chosen path (include/mi355vits_lab.h says what each reads and writes
// at and past len[b])
int mi355vits_test_dds_stack(int device, const mi355vits_dds_stack_test* t) {
    return guarded(nullptr, [&] {
        if (!t || !t->src || !t->pre_w || !t->pre_b || !t->len || !t->x_out) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        const int B = t->B, C = t->C, T = t->T, K = t->K, NL = t->n_layers, PC = t->proj_w ? t->proj_cout : 0;
        if (B < 1 || C < 1 || T < 1 || K < 1 || (K % 2) == 0 || NL < 1 || NL > DDS_STACK_MAX_LAYERS) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        if ((long)B * C * T >= 0x7fffffffL / 4) throw EngineError(MI355VITS_ERR_INVALID, "tensor too large for the hook");
        if (t->pre_mode != DDS_PRE_CONV && t->pre_mode != DDS_PRE_AFFINE) throw EngineError(MI355VITS_ERR_INVALID, "pre_mode must be 0 or 1");
        if (t->zch != 0 && t->zch != 1) throw EngineError(MI355VITS_ERR_INVALID, "zch must be 0 or 1");
        for (int i = 0; i < NL; ++i)
            if (!t->dw_w[i] || !t->dw_b[i] || !t->g1[i] || !t->b1[i] || !t->w1x1[i] || !t->bias1x1[i] || !t->g2[i] || !t->b2[i])
                throw EngineError(MI355VITS_ERR_INVALID, "null layer argument");
        if (t->proj_w && (!t->proj_b || !t->out || PC < 1)) throw EngineError(MI355VITS_ERR_INVALID, "proj needs proj_b, out and proj_cout >= 1");
        if (t->pre_mode == DDS_PRE_AFFINE && !t->z) throw EngineError(MI355VITS_ERR_INVALID, "the affine pre needs z");
        if (t->pre_mode == DDS_PRE_AFFINE && t->cond) throw EngineError(MI355VITS_ERR_INVALID, "cond goes with the conv pre only");
        if (t->spline && (!t->proj_w || !t->z)) throw EngineError(MI355VITS_ERR_INVALID, "the spline needs proj and z");
        if (t->spline && (t->nb < 2 || t->nb > 16)) throw EngineError(MI355VITS_ERR_INVALID, "spline: 2 <= nb <= 16");
        if (t->spline && PC != 3 * t->nb - 1) throw EngineError(MI355VITS_ERR_INVALID, "spline: proj_cout must be 3 nb - 1");
        check_lens(t->len, B, T, "len out of range");
        if (t->impl < 0 || t->impl > 3) throw EngineError(MI355VITS_ERR_INVALID, "impl must be 0, 1, 2 or 3");
        if (t->impl == 3 ? !math_on_bf16(t->math) : t->math != MATH_F32)
            throw EngineError(MI355VITS_ERR_INVALID, "math mode: MATH_F32 for impl 0, 1 and 2, MATH_BF16X3 or MATH_BF16W for impl 3");
        if (t->impl == 1 && !dds_layer_fused_supported(C)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the fused DDS layer");
        if (t->impl >= 2 && !dds_stack_supported(C, K, NL, PC)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the DDS stack kernels");
        HookScope s(device);
        const size_t n = (size_t)B * C * T, nz = (size_t)B * 2 * T, no = (size_t)B * PC * T;
        // a dense 1x1 conv's weights [Cout, C, 1] in the form the chosen path reads (ConvW::packed_b3s, packed, raw)
        auto conv_mfma = [&](int Cout) { return conv1d_mfma_supported(C, Cout, 1, 1); };
        auto dense = [&](const float* w, int Cout) -> const float* {
            if (t->impl == 3) return in_words(s, conv_weights_bf16x3_staged(w, Cout, C, 1));
            if (t->impl != 0 || conv_mfma(Cout)) return s.in(conv_weights_mfma(w, Cout, C, 1));
            return s.in(w, (size_t)Cout * C);
        };
        const float* dsrc = s.in(t->src, n);
        float* dxo = s.inout(t->x_out, n);
        float* dout = PC ? s.inout(t->out, no) : nullptr;
        float* dz = s.inout(t->z, nz);
        const int* dl = s.in(t->len, (size_t)B);
        const float* dcond = s.in(t->cond, (size_t)B * C);
        const float* pre_w = t->pre_mode == DDS_PRE_AFFINE ? s.in(t->pre_w, (size_t)C) : dense(t->pre_w, C);
        const float* pre_b = s.in(t->pre_b, (size_t)C);
        const float *dw_w[DDS_STACK_MAX_LAYERS], *dw_b[DDS_STACK_MAX_LAYERS], *g1[DDS_STACK_MAX_LAYERS], *b1[DDS_STACK_MAX_LAYERS];
        const float *w1[DDS_STACK_MAX_LAYERS], *bb[DDS_STACK_MAX_LAYERS], *g2[DDS_STACK_MAX_LAYERS], *b2[DDS_STACK_MAX_LAYERS];
        for (int i = 0; i < NL; ++i) {
            dw_w[i] = s.in(t->dw_w[i], (size_t)C * K); dw_b[i] = s.in(t->dw_b[i], (size_t)C);
            g1[i] = s.in(t->g1[i], (size_t)C); b1[i] = s.in(t->b1[i], (size_t)C);
            w1[i] = dense(t->w1x1[i], C); bb[i] = s.in(t->bias1x1[i], (size_t)C);
            g2[i] = s.in(t->g2[i], (size_t)C); b2[i] = s.in(t->b2[i], (size_t)C);
        }
        const float* proj_w = PC ? dense(t->proj_w, PC) : nullptr;
        const float* proj_b = PC ? s.in(t->proj_b, (size_t)PC) : nullptr;
        if (t->impl >= 2) {
            DdsStackArgs a;
            a.src = dsrc; a.pre_mode = t->pre_mode; a.pre_w = pre_w; a.pre_b = pre_b;
            if (dcond) { a.cond = dcond; a.cond_bs = C; }
            a.z = dz; a.zch = t->zch;
            a.n_layers = NL; a.K = K;
            for (int i = 0; i < NL; ++i) {
                a.dw_w[i] = dw_w[i]; a.dw_b[i] = dw_b[i]; a.g1[i] = g1[i]; a.b1[i] = b1[i];
                a.w1x1[i] = w1[i]; a.bias1x1[i] = bb[i]; a.g2[i] = g2[i]; a.b2[i] = b2[i];
            }
            a.x_out = dxo;
            a.proj_w = proj_w; a.proj_b = proj_b; a.proj_cout = PC;
            a.out = dout;
            a.spline = t->spline ? 1 : 0; a.nb = t->nb; a.tail = t->tail; a.inv_sqrt_fc = t->inv_sqrt_fc;
            a.len = dl; a.B = B; a.T = T; a.math = t->math;
            launch_dds_stack(a, C, nullptr);
        } else {
            // Engine::duration_predictor's launches without the stack kernels: x lives in d0 (d1 / d2: Engine::dds's scratch)
            float *d0 = s.scratch<float>(n), *d1 = s.scratch<float>(n), *d2 = s.scratch<float>(n);
            const long bs = (long)C * T;
            auto conv1x1 = [&](const float* x, float* y, const float* w, const float* bias, int Cout, bool masked) {
                ConvArgs a;
                a.x = x; a.x_bs = bs; a.x_ld = T;
                a.y = y; a.y_bs = (long)Cout * T; a.y_ld = T;
                a.B = B; a.T = T; a.Cin = C; a.Cout = Cout; a.K = 1; a.bias = bias; a.pad = 0; a.w = w; a.math = MATH_F32;
                if (masked) { a.in_len = dl; a.out_len = dl; }
                return a;
            };
            auto run_conv = [&](const ConvArgs& a) {
                if (conv_mfma(a.Cout)) launch_conv1d_mfma(a, nullptr);
                else launch_conv1d_generic(a, nullptr);
            };
            float* X = d0;
            if (t->pre_mode == DDS_PRE_AFFINE) {
                launch_convflow_pre(dz, t->zch, pre_w, pre_b, dsrc, B, C, T, X, nullptr);
            } else {
                ConvArgs a = conv1x1(dsrc, X, pre_w, pre_b, C, false);
                if (dcond) { a.cond = dcond; a.cond_bs = C; }
                run_conv(a);
            }
            int dil = 1;
            for (int i = 0; i < NL; ++i) {
                if (t->impl == 1) {  // x ping-pongs (k_dds_layer reads its neighbours' OLD columns)
                    float* dst = X == d0 ? d1 : d0;
                    launch_dds_layer(X, dst, dw_w[i], dw_b[i], g1[i], b1[i], w1[i], bb[i], g2[i], b2[i], dl, B, C, T, K, dil, nullptr);
                    X = dst;
                } else {
                    launch_dds_dwconv_ln_gelu(X, dw_w[i], dw_b[i], g1[i], b1[i], dl, B, C, T, K, dil, d1, nullptr);
                    run_conv(conv1x1(d1, d2, w1[i], bb[i], C, false));
                    LNArgs ln;
                    ln.x = d2; ln.y = X; ln.add_to = X; ln.gelu = 1;
                    ln.B = B; ln.C = C; ln.T = T; ln.gamma = g2[i]; ln.beta = b2[i];
                    launch_layernorm(ln, nullptr);
                }
                dil *= K;
            }
            HIP_CHECK(hipMemcpyAsync(dxo, X, n * 4, hipMemcpyDeviceToDevice, nullptr));
            if (PC) run_conv(conv1x1(X, dout, proj_w, proj_b, PC, true));
            if (t->spline)
                launch_spline_inverse(dz, t->zch, dout, dl, B, T, t->nb, t->tail, t->inv_sqrt_fc, nullptr);
        }
        s.finish();
    });
}

int mi355vits_test_spline_inverse(int device, int B, int T, int nb, int ch_x0, float tail, float inv_sqrt_fc, const float* theta,
                                  const int32_t* len, float* z) {
    return guarded(nullptr, [&] {
        if (!theta || !len || !z) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1 || nb < 2 || nb > 16 || (ch_x0 != 0 && ch_x0 != 1)) throw EngineError(MI355VITS_ERR_INVALID, "bad shape (2 <= nb <= 16)");
        check_lens(len, B, T, "len out of range");
        HookScope s(device);
        launch_spline_inverse(s.inout(z, (size_t)B * 2 * T), ch_x0, s.in(theta, (size_t)B * (3 * nb - 1) * T), s.in(len, (size_t)B), B, T, nb, tail,
                              inv_sqrt_fc, nullptr);
        s.finish();
    });
}

int mi355vits_test_durations(int device, int B, int T, int ch, float ea_m, float ea_logs, const float* z, const int32_t* len,
                             const int32_t* forced, const float* scales, float* logw, int32_t* w_ceil, int32_t* cum, int32_t* ylen) {
    return guarded(nullptr, [&] {
        if (!z || !len || !scales || !logw || !w_ceil || !cum || !ylen) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1 || (ch != 0 && ch != 1)) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        check_lens(len, B, T, "len out of range");
        HookScope s(device);
        const size_t nt = (size_t)B * T;
        // the outputs' prior contents go up: a missing write shows
        float* dlw = s.inout(logw, nt);
        int *dw = s.inout(w_ceil, nt), *dc = s.inout(cum, nt), *dy = s.inout(ylen, (size_t)B);
        launch_durations(s.in(z, (size_t)B * 2 * T), ch, ea_m, ea_logs, s.in(len, (size_t)B), s.in(forced, nt), B, T, s.in(scales, (size_t)B * 3), dlw, dw,
                         dc, dy, nullptr);
        s.finish();
    });
}

int mi355vits_test_fit_durations(int device, int B, int T, const float* u, const int32_t* len, const int32_t* min_frames,
                                 const int32_t* target, int32_t* frames, int32_t* cum, int32_t* ylen, float* factor, int32_t* status) {
    return guarded(nullptr, [&] {
        if (!u || !len || !frames || !cum || !ylen || !factor || !status) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        for (int b = 0; b < B; ++b) {
            if (len[b] < 0 || len[b] > T) throw EngineError(MI355VITS_ERR_INVALID, "len out of range");
            if (target && (target[b] < 0 || target[b] > DURATION_FRAME_CAP)) throw EngineError(MI355VITS_ERR_INVALID, "target out of range");
        }
        HookScope s(device);
        const size_t nt = (size_t)B * T;
        DurTimedArgs a;
        a.u_in = s.in(u, nt);
        a.len = s.in(len, (size_t)B); a.B = B; a.T = T;
        a.min_frames = s.in(min_frames, nt);
        a.target = s.in(target, (size_t)B);
        a.u = s.scratch<float>(nt);
        // the outputs' prior contents go up: a missing write shows
        a.w_ceil = s.inout(frames, nt); a.cum = s.inout(cum, nt); a.ylen = s.inout(ylen, (size_t)B);
        a.factor = s.inout(factor, (size_t)B); a.status = s.inout(status, (size_t)B);
        launch_durations_timed(a, nullptr);
        s.finish();
    });
}

int mi355vits_test_speaker_cond(int device, int B, int gin, int n_speakers, int Cout, const float* emb_g, const int64_t* sid,
                                const float* w, const float* bias, float* out, size_t out_floats) {
    return guarded(nullptr, [&] {
        if (!emb_g || !sid || !w || !out) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || gin < 1 || gin > 8192 || n_speakers < 1 || Cout < 1 || out_floats < (size_t)B * Cout) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        for (int b = 0; b < B; ++b)
            if (sid[b] < 0 || sid[b] >= n_speakers) throw EngineError(MI355VITS_ERR_INVALID, "sid out of range");
        HookScope s(device);
        float* dout = s.inout(out, out_floats);  // the prior contents: a missing or stray write shows
        launch_speaker_cond(s.in(emb_g, (size_t)n_speakers * gin), reinterpret_cast<const long long*>(s.in(sid, (size_t)B)), s.in(w, (size_t)Cout * gin),
                            s.in(bias, (size_t)Cout), B, gin, Cout, dout, nullptr);
        s.finish();
    });
}

int mi355vits_test_speaker_cond_mix(int device, const mi355vits_speaker_mix_test* t) {
    return guarded(nullptr, [&] {
        if (!t || !t->g) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        const int B = t->B, gin = t->gin, K = t->n_terms, nj = t->n_jobs;
        if (B < 1 || gin < 1 || gin > 8192 || nj < 1 || nj > SPEAKER_MIX_MAX_JOBS || t->g_floats < (size_t)B * gin) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        const bool mix = t->vectors == nullptr;
        if (mix) {
            if (!t->emb_g || !t->mix_sid || !t->mix_weight || t->n_speakers < 1 || K < 1 || K > SPEAKER_MIX_MAX_TERMS)
                throw EngineError(MI355VITS_ERR_INVALID, "a mix needs emb_g, mix_sid, mix_weight and n_terms 1 .. 8");
            for (size_t i = 0; i < (size_t)B * K; ++i)
                if (t->mix_weight[i] != 0.0f && (t->mix_sid[i] < 0 || t->mix_sid[i] >= t->n_speakers)) throw EngineError(MI355VITS_ERR_INVALID, "sid out of range");
        } else if (t->emb_g || t->mix_sid || t->mix_weight || K != 0) {
            throw EngineError(MI355VITS_ERR_INVALID, "vectors exclude emb_g, mix_sid, mix_weight and n_terms");
        }
        for (int q = 0; q < nj; ++q)
            if (!t->w[q] || !t->out[q] || t->Cout[q] < 1 || t->out_floats[q] < (size_t)B * t->Cout[q]) throw EngineError(MI355VITS_ERR_INVALID, "bad job");
        HookScope s(device);
        SpeakerMixArgs a;
        a.B = B; a.gin = gin; a.K = K; a.n_jobs = nj;
        a.g = s.inout(t->g, t->g_floats);  // the prior contents: a missing or stray write shows
        if (mix) {
            a.emb_g = s.in(t->emb_g, (size_t)t->n_speakers * gin);
            a.sid = reinterpret_cast<const long long*>(s.in(t->mix_sid, (size_t)B * K));
            a.weight = s.in(t->mix_weight, (size_t)B * K);
        } else {
            a.vectors = s.in(t->vectors, (size_t)B * gin);
        }
        for (int q = 0; q < nj; ++q) {
            a.jobs[q].w = s.in(t->w[q], (size_t)t->Cout[q] * gin);
            a.jobs[q].bias = s.in(t->bias[q], (size_t)t->Cout[q]);
            a.jobs[q].Cout = t->Cout[q];
            a.jobs[q].out = s.inout(t->out[q], t->out_floats[q]);
        }
        launch_speaker_cond_mix(a, nullptr);
        s.finish();
    });
}

int mi355vits_test_levels(int device, int B, int T, int hop, const int32_t* cum, const int32_t* len, const float* gain,
                          const int32_t* ramp, const int32_t* alen, int64_t audio_bs, float* audio, size_t audio_floats, float* peaks) {
    return guarded(nullptr, [&] {
        if (!cum || !len || !gain || !alen || !audio || !peaks) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1 || hop < 1 || audio_bs < 1 || audio_floats < (size_t)B * (size_t)audio_bs) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        long l_max = 0;
        for (int b = 0; b < B; ++b) {
            const int L = len[b];
            if (L < 0 || L > T) throw EngineError(MI355VITS_ERR_INVALID, "len out of range");
            for (int t = 0; t < L; ++t) {
                const float g = gain[(size_t)b * T + t];
                if (cum[(size_t)b * T + t] < (t ? cum[(size_t)b * T + t - 1] : 0)) throw EngineError(MI355VITS_ERR_INVALID, "cum must be non-negative and non-decreasing");
                if (!(std::isfinite(g) && g >= 0.0f && g <= 1024.0f)) throw EngineError(MI355VITS_ERR_INVALID, "gain out of range");
            }
            const long long frames = L > 0 ? cum[(size_t)b * T + L - 1] : 0;
            const long long n = (long long)hop * (frames < 1 ? 1 : frames);
            if (n > audio_bs || n > 0x7fffffffLL || alen[b] != n) throw EngineError(MI355VITS_ERR_INVALID, "alen must be hop * max(1, c[len - 1]) and fit the row");
            if (ramp && (ramp[b] < 0 || ramp[b] > LEVELS_MAX_RAMP)) throw EngineError(MI355VITS_ERR_INVALID, "ramp out of range");
            l_max = std::max<long>(l_max, (long)n);
        }
        HookScope s(device);
        const size_t nbt = (size_t)B * T;
        float* dx = s.inout(audio, audio_floats);  // everything: a stray write shows
        unsigned* dp = s.filled<unsigned>((size_t)B, 0);
        launch_levels(s.in(cum, nbt), s.in(len, (size_t)B), s.in(gain, nbt), s.in(ramp, (size_t)B), B, T, hop, dx, (long)audio_bs, s.in(alen, (size_t)B),
                      l_max, dp, nullptr);
        s.finish();
        s.fetch(peaks, dp, (size_t)B);
    });
}

int mi355vits_test_pitch_table(float* out, size_t capacity) {
    return guarded(nullptr, [&] {
        const std::vector<float>& h = pitch_table();
        if (!out || capacity < h.size()) throw EngineError(MI355VITS_ERR_INVALID, "pitch table: out must take " + std::to_string(h.size()) + " floats");
        memcpy(out, h.data(), h.size() * sizeof(float));
    });
}

namespace {
// what both pitch hooks check of their inputs; returns the longest native row
long check_pitch_inputs(int B, int T, int hop, const int32_t* cum, const int32_t* len, const float* ratio, int64_t x_bs) {
    if (!cum || !len) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
    if (B < 1 || T < 1 || hop < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
    long n_max = 0;
    for (int b = 0; b < B; ++b) {
        const int L = len[b];
        if (L < 0 || L > T) throw EngineError(MI355VITS_ERR_INVALID, "len out of range");
        for (int t = 0; t < L; ++t) {
            if (cum[(size_t)b * T + t] < (t ? cum[(size_t)b * T + t - 1] : 0)) throw EngineError(MI355VITS_ERR_INVALID, "cum must be non-negative and non-decreasing");
            if (ratio) {
                const float p = ratio[(size_t)b * T + t];
                if (!(std::isfinite(p) && p >= 0.5f && p <= 2.0f)) throw EngineError(MI355VITS_ERR_INVALID, "ratio out of range");
            }
        }
        const long long frames = L > 0 ? cum[(size_t)b * T + L - 1] : 0;
        const long long n = (long long)hop * (frames < 1 ? 1 : frames);
        if (n > 0x7fffffffLL || (x_bs > 0 && n > x_bs)) throw EngineError(MI355VITS_ERR_INVALID, "hop * max(1, c[len - 1]) must fit the row");
        n_max = std::max<long>(n_max, (long)n);
    }
    return n_max;
}
}  // namespace

int mi355vits_test_pitch_plan(int device, int B, int T, int hop, const int32_t* cum, const int32_t* len, const float* ratio,
                              int64_t* tq, int32_t* wc, int32_t* wlen) {
    return guarded(nullptr, [&] {
        if (!tq || !wc || !wlen) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        check_pitch_inputs(B, T, hop, cum, len, ratio, 0);
        HookScope s(device);
        const size_t nbt = (size_t)B * T;
        long long* dq = s.scratch<long long>(nbt);
        int *dw = s.scratch<int>(nbt), *dn = s.scratch<int>((size_t)B);
        launch_pitch_plan(s.in(cum, nbt), s.in(len, (size_t)B), s.in(ratio, nbt), B, T, hop, dq, dw, dn, nullptr);
        s.finish();
        s.fetch(tq, dq, nbt);
        s.fetch(wc, dw, nbt);
        s.fetch(wlen, dn, (size_t)B);
    });
}

int mi355vits_test_pitch(int device, int B, int T, int hop, const int32_t* cum, const int32_t* len, const float* ratio,
                         const float* x, int64_t x_bs, size_t x_floats, float* y, int64_t y_bs, int32_t y_ld, size_t y_floats,
                         float* peaks, int32_t* wlen) {
    return guarded(nullptr, [&] {
        if (!x || !y || !peaks || !wlen) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (x_bs < 1 || y_bs < 1 || y_ld < 1 || y_ld > y_bs || B < 1 || x_floats < (size_t)B * (size_t)x_bs || y_floats < (size_t)B * (size_t)y_bs)
            throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        check_pitch_inputs(B, T, hop, cum, len, ratio, x_bs);
        HookScope s(device);
        const size_t nbt = (size_t)B * T;
        std::vector<int> alen(B);
        for (int b = 0; b < B; ++b) {
            const int frames = len[b] > 0 ? cum[(size_t)b * T + len[b] - 1] : 0;
            alen[b] = hop * (frames < 1 ? 1 : frames);
        }
        const int *dc = s.in(cum, nbt), *dl = s.in(len, (size_t)B);
        const float* dratio = s.in(ratio, nbt);
        long long* dq = s.scratch<long long>(nbt);
        int *dw = s.scratch<int>(nbt), *dn = s.scratch<int>((size_t)B);
        float* dy = s.in<float>(y, y_floats);  // everything: a stray write shows
        unsigned* dp = s.filled<unsigned>((size_t)B, 0);
        launch_pitch_plan(dc, dl, dratio, B, T, hop, dq, dw, dn, nullptr);
        s.finish();
        s.fetch(wlen, dn, (size_t)B);
        for (int b = 0; b < B; ++b)
            if (wlen[b] < 1 || wlen[b] == 0x7fffffff || wlen[b] > y_ld) throw EngineError(MI355VITS_ERR_INVALID, "row " + std::to_string(b) + ": the warped row of " + std::to_string(wlen[b]) + " samples does not fit y_ld");
        std::vector<int64_t> w64(wlen, wlen + B);
        std::vector<int> tab(pitch_tab_ints(B));
        const long items = pitch_fill_tab(w64.data(), B, tab.data());
        launch_pitch(s.in(x, x_floats), (long)x_bs, s.in(alen), dc, dl, dratio, dq, dw, s.in(tab), items, s.in(pitch_table()), B, T, hop, dy, (long)y_bs,
                     y_ld, dp, nullptr);
        s.finish();
        s.fetch(y, dy, y_floats);
        s.fetch(peaks, dp, (size_t)B);
    });
}

int mi355vits_test_expand_prior(int device, int B, int I, int Tx, int Ty, const float* stats, const int32_t* cum, const int32_t* ylen,
                                const float* injected, int injected_frames, const float* scales, float* z) {
    return guarded(nullptr, [&] {
        if (!stats || !cum || !ylen || !scales || !z) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || I < 1 || Tx < 1 || Ty < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        if (injected && injected_frames < Ty) throw EngineError(MI355VITS_ERR_INVALID, "injected_frames must cover Ty");
        for (int b = 0; b < B; ++b) {
            if (ylen[b] < 0 || ylen[b] > Ty) throw EngineError(MI355VITS_ERR_INVALID, "ylen out of range");
            if (!injected && scales[3 * b] != 0.0f) throw EngineError(MI355VITS_ERR_INVALID, "noise_scale != 0 needs injected noise (no Philox path here)");
            for (int j = 0; j < Tx; ++j)
                if (cum[(size_t)b * Tx + j] < (j ? cum[(size_t)b * Tx + j - 1] : 0)) throw EngineError(MI355VITS_ERR_INVALID, "cum must be non-negative and non-decreasing");
        }
        HookScope s(device);
        const size_t ni = injected ? (size_t)B * I * injected_frames : 0;
        launch_expand_prior(s.in(stats, (size_t)B * 2 * I * Tx), s.in(cum, (size_t)B * Tx), s.in(ylen, (size_t)B), s.in(injected, ni), injected_frames, B, I,
                            Tx, Ty, s.in(scales, (size_t)B * 3), 0ull, s.filled<unsigned long long>((size_t)B, 0), s.inout(z, (size_t)B * I * Ty), nullptr);
        s.finish();
    });
}

// ---- the text side's small kernels and the Philox noise (include/mi355vits_lab.h says what each reads and writes at and past the lengths)
int mi355vits_test_expand_prior_keyed(int device, int B, int I, int Tx, int Ty, const float* stats, const int32_t* cum, const int32_t* ylen,
                                      const float* scales, uint64_t seed, const uint64_t* utt, float* z) {
    return guarded(nullptr, [&] {
        if (!stats || !cum || !ylen || !scales || !utt || !z) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || I < 1 || Tx < 1 || Ty < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        for (int b = 0; b < B; ++b) {
            if (ylen[b] < 0 || ylen[b] > Ty) throw EngineError(MI355VITS_ERR_INVALID, "ylen out of range");
            for (int j = 0; j < Tx; ++j)
                if (cum[(size_t)b * Tx + j] < (j ? cum[(size_t)b * Tx + j - 1] : 0)) throw EngineError(MI355VITS_ERR_INVALID, "cum must be non-negative and non-decreasing");
        }
        HookScope s(device);
        launch_expand_prior(s.in(stats, (size_t)B * 2 * I * Tx), s.in(cum, (size_t)B * Tx), s.in(ylen, (size_t)B), nullptr, 0, B, I, Tx, Ty,
                            s.in(scales, (size_t)B * 3), (unsigned long long)seed, reinterpret_cast<const unsigned long long*>(s.in(utt, (size_t)B)),
                            s.inout(z, (size_t)B * I * Ty), nullptr);
        s.finish();
    });
}

int mi355vits_test_sdp_noise(int device, int B, int T, uint64_t seed, const uint64_t* utt, const float* scales, float* z) {
    return guarded(nullptr, [&] {
        if (!utt || !scales || !z) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        HookScope s(device);
        launch_sdp_noise(s.inout(z, (size_t)B * 2 * T), nullptr, B, T, s.in(scales, (size_t)B * 3), (unsigned long long)seed,
                         reinterpret_cast<const unsigned long long*>(s.in(utt, (size_t)B)), nullptr);
        s.finish();
    });
}

int mi355vits_test_embed(int device, int B, int T, int H, int num_symbols, const int64_t* ids, const int32_t* len, const float* emb,
                         float scale, float* y) {
    return guarded(nullptr, [&] {
        if (!ids || !len || !emb || !y) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1 || H < 1 || num_symbols < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        check_lens(len, B, T, "len out of range");
        HookScope s(device);
        launch_embed(reinterpret_cast<const long long*>(s.in(ids, (size_t)B * T)), s.in(len, (size_t)B), s.in(emb, (size_t)num_symbols * H), B, T, H,
                     num_symbols, scale, s.inout(y, (size_t)B * H * T), nullptr);
        s.finish();
    });
}

int mi355vits_test_layernorm(int device, const mi355vits_layernorm_test* t) {
    return guarded(nullptr, [&] {
        if (!t || !t->x || !t->gamma || !t->beta || !t->y) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        const int B = t->B, C = t->C, T = t->T, NP = t->nparts;
        if (B < 1 || C < 1 || T < 1 || NP < 1 || NP > 8) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        const size_t n = (size_t)B * C * T;
        if (n >= 0x7fffffffull / 4) throw EngineError(MI355VITS_ERR_INVALID, "tensor too large for the hook");
        const size_t stride = NP > 1 ? (size_t)t->part_stride : n;
        if (NP > 1 && t->part_stride < (int64_t)n) throw EngineError(MI355VITS_ERR_INVALID, "part_stride must cover a slice");
        if (t->alias < 0 || t->alias > 3 || (t->alias == 2 && !t->res) || (t->alias == 3 && !t->add_to))
            throw EngineError(MI355VITS_ERR_INVALID, "alias: 0 none, 1 y == x, 2 y == res, 3 y == add_to (the aliased input must be given)");
        check_lens(t->premask_len, B, T, "premask_len out of range");
        check_lens(t->out_len, B, T, "out_len out of range");
        HookScope s(device);
        LNArgs a;
        float* dx = s.in(t->x, (size_t)(NP - 1) * stride + n);
        float *dres = s.in(t->res, n), *dadd = s.in(t->add_to, n);
        a.x = dx; a.res = dres; a.add_to = dadd;
        a.gamma = s.in(t->gamma, (size_t)C); a.beta = s.in(t->beta, (size_t)C); a.bias = s.in(t->bias, (size_t)C);
        a.premask_len = s.in(t->premask_len, (size_t)B); a.out_len = s.in(t->out_len, (size_t)B);
        a.B = B; a.C = C; a.T = T; a.gelu = t->gelu ? 1 : 0; a.eps = t->eps;
        a.nparts = NP; a.part_stride = (long)stride;
        // an aliased output is the input's own device pointer, taken once; the caller's y goes up only where it is a buffer of its own
        a.y = t->alias == 1 ? dx : t->alias == 2 ? dres : t->alias == 3 ? dadd : s.in<float>(t->y, n);
        try {
            launch_layernorm(a, nullptr);
        } catch (const EngineError&) {
            throw;
        } catch (const std::runtime_error& e) {  // the launcher's own refusal (thrown before any launch); a HIP error stays a device error
            if (std::string(e.what()).rfind("layernorm:", 0) == 0) throw EngineError(MI355VITS_ERR_INVALID, e.what());
            throw;
        }
        s.finish();
        s.fetch(t->y, a.y, n);
    });
}

int mi355vits_lab_dp_det_plan(int H, int F, int K, int math, int32_t* cols, int32_t* halo, int32_t* lds_bytes) {
    return guarded(nullptr, [&] {
        if (!dp_det_supported(H, F, K)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by k_dp_det");
        if (math != MATH_F32 && math != MATH_BF16X3) throw EngineError(MI355VITS_ERR_INVALID, "math mode: MATH_F32 or MATH_BF16X3");
        if (cols) *cols = dp_det_tile_cols(K);
        if (halo) *halo = 2 * (K / 2);
        if (lds_bytes) *lds_bytes = (int32_t)dp_det_lds_bytes(H, F, K, math);
    });
}

int mi355vits_test_dp_det(int device, const mi355vits_dp_det_test* t) {
    return guarded(nullptr, [&] {
        if (!t || !t->x || !t->len || !t->w1 || !t->b1 || !t->g1 || !t->be1 || !t->w2 || !t->b2 || !t->g2 || !t->be2 || !t->proj_w || !t->proj_b || !t->logw)
            throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        const int B = t->B, H = t->H, F = t->F, K = t->K, T = t->T;
        if (B < 1 || T < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        if (!dp_det_supported(H, F, K)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by k_dp_det");
        if (t->math != MATH_F32 && t->math != MATH_BF16X3) throw EngineError(MI355VITS_ERR_INVALID, "math mode: MATH_F32 or MATH_BF16X3");
        if ((size_t)B * H * T >= 0x7fffffffull / 4) throw EngineError(MI355VITS_ERR_INVALID, "tensor too large for the hook");
        check_lens(t->len, B, T, "len out of range");
        HookScope s(device);
        // a conv's weights [Cout, Cin, K] in the form the mode reads (ConvW::packed / packed_b3s)
        auto conv_w = [&](const float* w, int Cout, int Cin) -> const float* {
            if (t->math == MATH_F32) return s.in(conv_weights_mfma(w, Cout, Cin, K));
            return in_words(s, conv_weights_bf16x3_staged(w, Cout, Cin, K));
        };
        DpDetArgs a;
        a.x = s.in(t->x, (size_t)B * H * T);
        if (t->cond) { a.cond = s.in(t->cond, (size_t)B * H); a.cond_bs = H; }
        a.w1 = conv_w(t->w1, F, H); a.b1 = s.in(t->b1, (size_t)F); a.g1 = s.in(t->g1, (size_t)F); a.be1 = s.in(t->be1, (size_t)F);
        a.w2 = conv_w(t->w2, F, F); a.b2 = s.in(t->b2, (size_t)F); a.g2 = s.in(t->g2, (size_t)F); a.be2 = s.in(t->be2, (size_t)F);
        a.pw = s.in(t->proj_w, (size_t)F);
        a.pb = s.in(t->proj_b, 1);
        a.len = s.in(t->len, (size_t)B);
        a.out = s.inout(t->logw, (size_t)B * T); a.out_bs = T;
        a.B = B; a.T = T; a.H = H; a.F = F; a.K = K; a.math = t->math;
        launch_dp_det(a, nullptr);
        s.finish();
    });
}

int mi355vits_lab_pack_w16(const float* w, int Cout, int Cin, int K, int gate, uint32_t* out) {
    return guarded(nullptr, [&] {
        if (!w || !out) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (Cout < 1 || Cin < 1 || K < 1 || Cin % 32 != 0 || Cout % (gate ? 64 : 32) != 0) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        pack_conv_weights_w16(w, Cout, Cin, K, gate != 0, out);
    });
}

int mi355vits_lab_wn_plan(int B, int T, int K, int dilation, int32_t* b3_tile, int32_t* f32_geometry) {
    return guarded(nullptr, [&] {
        if (B < 1 || T < 1 || K < 1 || (K % 2) == 0 || dilation < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        WnArgs w;
        w.B = B; w.H = 192; w.T = T; w.K = K; w.dil = dilation; w.h_ld = w.s_ld = T; w.math = MATH_BF16X3;
        if (b3_tile) {
            if (!wn_layer_b3_supported(w.H, K, dilation)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the fused split-bf16 layer");
            *b3_tile = 32 * wn_layer_b3_column_tiles(w);
        }
        if (f32_geometry) *f32_geometry = wn_layer_geometry(w);
    });
}

// one multi-receptive-field stage through a chosen kernel (include/mi355vits_lab.h says what each reads and writes at and past len[b])
static bool mrf_test_plan(int impl, int C, int nrb, const int32_t* k, const int32_t* d1, const int32_t* d2, MrfPlan* p) {
    if (nrb < 1 || nrb > MRF_MAX_RB || !k || !d1 || !d2) return false;
    int kk[MRF_MAX_RB], a1[MRF_MAX_RB], a2[MRF_MAX_RB];
    for (int j = 0; j < nrb; ++j) { kk[j] = k[j]; a1[j] = d1[j]; a2[j] = d2[j]; }
    return impl == 0 ? mrf_fused_plan(C, nrb, kk, a1, a2, p) : impl == 1 ? mrf_p_plan(C, nrb, kk, a1, a2, p) : impl == 2 ? mrf_s_plan(C, nrb, kk, a1, a2, p) : false;
}

int mi355vits_test_mrf_stage(int device, const mi355vits_mrf_test* t) {
    return guarded(nullptr, [&] {
        if (!t || !t->x || !t->len || !t->y) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        const int B = t->B, C = t->C, T = t->T, nrb = t->nrb;
        if (B < 1 || C < 1 || T < 1 || nrb < 1 || nrb > MRF_MAX_RB || !(t->out_scale >= 0.0f)) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        if ((long)C * T * 4 >= 0x7fffffffL || (long)B * C * T >= 0x7fffffffL / 4) throw EngineError(MI355VITS_ERR_INVALID, "tensor too large for the hook");
        for (int j = 0; j < nrb; ++j)
            for (int q = 0; q < 2; ++q)
                if (!t->w[j][q] || !t->bias[j][q]) throw EngineError(MI355VITS_ERR_INVALID, "null weight or bias");
        check_lens(t->len, B, T, "len out of range");
        if (t->impl < 0 || t->impl > 2) throw EngineError(MI355VITS_ERR_INVALID, "impl must be 0, 1 or 2");
        if (t->impl == 0 ? (t->math != MATH_F32 && t->math != MATH_BF16X3) : t->math != MATH_BF16X3)
            throw EngineError(MI355VITS_ERR_INVALID, "math mode: MATH_F32 or MATH_BF16X3 for impl 0, MATH_BF16X3 for impl 1 and 2");
        MrfPlan plan;
        if (!mrf_test_plan(t->impl, C, nrb, t->k, t->d1, t->d2, &plan)) throw EngineError(MI355VITS_ERR_INVALID, "stage not supported by the chosen kernel");
        if (t->impl == 2 && (t->seg < plan.width || t->seg % plan.width != 0)) throw EngineError(MI355VITS_ERR_INVALID, "seg must be a positive multiple of the sweep's step");
        HookScope s(device);
        const size_t n = (size_t)B * C * T;
        MrfArgs m;
        m.x = s.in(t->x, n); m.x_bs = (long)C * T; m.x_ld = T;
        m.y = s.inout(t->y, n); m.y_bs = (long)C * T; m.y_ld = T;
        m.len = s.in(t->len, (size_t)B); m.len_host = t->len; m.B = B; m.C = C; m.T = T;
        m.nrb = nrb; m.math = t->math; m.out_scale = t->out_scale;
        for (int j = 0; j < nrb; ++j) {
            const int k = t->k[j];
            m.k[j] = k; m.d1[j] = t->d1[j]; m.d2[j] = t->d2[j];
            for (int q = 0; q < 2; ++q) {
                const float* w = t->w[j][q];
                // ConvW::packed_p for the register kernels, packed_b3 / packed4 for the fused stage
                m.w[j][q] = t->impl != 0               ? in_words(s, conv_weights_p16(w, C, C, k))
                            : t->math == MATH_BF16X3 ? in_words(s, conv_weights_bf16x3(w, C, C, k))
                                                     : s.in(conv_weights_mfma_x4(conv_weights_mfma(w, C, C, k)));
                m.bias[j][q] = s.in(t->bias[j][q], (size_t)C);
            }
        }
        if (t->impl == 0) launch_mrf_fused(m, nullptr);
        else if (t->impl == 1) launch_mrf_p(m, nullptr);
        else { m.seg = t->seg; launch_mrf_s(m, nullptr); }
        s.finish();
    });
}

int mi355vits_lab_mrf_plan(int impl, int C, int nrb, const int32_t* k, const int32_t* d1, const int32_t* d2, int32_t* width,
                           int32_t* halo, int32_t* x_ring, int32_t* x1_ring) {
    return guarded(nullptr, [&] {
        MrfPlan p;
        if (!mrf_test_plan(impl, C, nrb, k, d1, d2, &p)) throw EngineError(MI355VITS_ERR_INVALID, "stage not supported by the chosen kernel");
        if (width) *width = p.width;
        if (halo) *halo = p.halo;
        if (x_ring) *x_ring = p.x_ring;
        if (x1_ring) *x1_ring = p.x1_ring;
    });
}

int mi355vits_bench_conv1d(int device, int B, int Cin, int Cout, int T, int K, int dilation, int epi, int reps,
                           float* ms_per_launch) {
    return guarded(nullptr, [&] {
        HookScope s(device);
        if (!conv1d_mfma_supported(Cin, Cout, K, dilation) || reps < 1 || !ms_per_launch) throw EngineError(MI355VITS_ERR_INVALID, "bad arguments");
        const int H = Cout / 2;
        const size_t nx = (size_t)B * Cin * T, ny = (size_t)B * Cout * T, nw = (size_t)Cout * Cin * K;
        std::vector<float> hx(nx), hw(nw);
        unsigned st = 12345u;
        auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xFFFF) / 32768.0f - 1.0f; };
        for (auto& v : hx) v = rnd();
        for (auto& v : hw) v = rnd() * 0.05f;
        ConvArgs a;
        a.x = s.in(hx); a.x_bs = (long)Cin * T; a.x_ld = T;
        a.w = s.in(conv_weights_mfma(hw.data(), Cout, Cin, K, epi == 1 ? EPI_GATE : EPI_STD));
        a.bias = s.filled<float>((size_t)Cout, 0);
        a.B = B; a.Cin = Cin; a.Cout = Cout; a.T = T; a.K = K; a.dil = dilation; a.pad = (K * dilation - dilation) / 2;
        a.y = s.filled<float>(ny, 0); a.y_ld = T;
        if (epi == 1) {
            a.epi = EPI_GATE; a.H = H;
            a.y_bs = (long)H * T;
        } else if (epi == 2) {
            a.epi = EPI_RESSKIP; a.H = H;
            a.y_bs = (long)H * T;
            a.y2 = s.filled<float>(ny, 0); a.y2_bs = (long)H * T; a.y2_ld = T;
        } else {
            a.y_bs = (long)Cout * T;
            a.res = s.filled<float>(ny, 0); a.res_bs = a.y_bs; a.res_ld = T;
            a.in_slope = 0.1f;
        }
        for (int i = 0; i < 3; ++i) launch_conv1d_mfma(a, nullptr);
        HIP_CHECK(hipDeviceSynchronize());  // the timed launches start on an idle device
        *ms_per_launch = (float)timed([&] { launch_conv1d_mfma(a, nullptr); }, 0, reps);
    });
}

int mi355vits_probe_device(int device, double out[8]) {
    return guarded(nullptr, [&] {
        if (!out) throw EngineError(MI355VITS_ERR_INVALID, "bad arguments");
        HookScope s(device);
        const int cus = current_device_cu_count();
        // one zero-filled GiB serves everything: [0, 2.6 MB) the L2 table, [0, 24 MB) the big table, the halves as copy source / destination
        const size_t gib = (size_t)1 << 30;
        char* base = s.filled<char>(gib, 0);
        unsigned* sink = s.scratch<unsigned>((size_t)cus + 4);
        const int n16 = 256 * 8 * 80;  // 163,840 x 16 B = 2.62 MB
        const int reps_in = 8;
        const double ms_stream = timed([&] { launch_probe_l2_stream(base, n16, reps_in, sink, cus, nullptr); }, 1, 3);
        out[0] = (double)cus * reps_in * n16 * 16.0 / (ms_stream * 1e-3) / 1e9;
        const int steps = 2000;
        auto chase = [&](unsigned nlines, int warm) {
            const double ms = timed([&] { launch_probe_l2_latency(reinterpret_cast<unsigned*>(base), steps, nlines, sink, cus, nullptr); }, warm, 2);
            return ms * 1e6 / steps;
        };
        out[1] = chase(1u << 15, 2);   // 2 MB: after two passes every XCD's L2 holds what its waves touch
        out[6] = chase(1u << 19, 2);   // 32 MB: past an L2, inside the memory-side cache
        out[7] = chase(1u << 24, 1);   // 1 GiB: HBM (and the TLB's reach)
        const long ncopy16 = (256L << 20) / 16;
        const double ms_copy = timed([&] { launch_probe_copy(base, base + gib / 2, ncopy16, cus * 16, nullptr); }, 1, 3);
        out[2] = 2.0 * ncopy16 * 16.0 / (ms_copy * 1e-3) / 1e9;
        out[3] = (double)cus;
        const long slice16 = ncopy16 / cus;
        const double ms_mixed = timed([&] { launch_probe_l2_mixed(base, n16, reps_in, base + gib / 4, base + gib / 2, slice16, sink, cus, nullptr); }, 1, 3);
        out[4] = (double)cus * reps_in * n16 * 16.0 / (ms_mixed * 1e-3) / 1e9;
        const int big16 = n16 * 9;
        const double ms_big = timed([&] { launch_probe_l2_stream(base, big16, 1, sink, cus, nullptr); }, 1, 3);
        out[5] = (double)cus * big16 * 16.0 / (ms_big * 1e-3) / 1e9;
    });
}

int mi355vits_test_mfma_layout(int device, float* err) {
    return guarded(nullptr, [&] {
        HookScope s(device);
        float* d = s.scratch<float>(1024 + 256 + 256);
        launch_mfma_selftest(d, nullptr);
        s.finish();
        std::vector<float> h(1536);
        s.fetch(h.data(), d, h.size());
        float worst = 0.0f;
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                float ref = 0;
                for (int k = 0; k < 2; ++k) ref += (float)(i + 100 * k + 1) * (float)(3 * j - 7 * k + 2);
                worst = std::max(worst, std::fabs(ref - h[i * 32 + j]));
            }
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                float ref = 0;
                for (int k = 0; k < 4; ++k) ref += (float)(i + 100 * k + 1) * (float)(3 * j - 7 * k + 2);
                worst = std::max(worst, std::fabs(ref - h[1024 + i * 16 + j]));
            }
        for (int i = 0; i < 16; ++i)  // v_mfma_f32_16x16x32_bf16
            for (int j = 0; j < 16; ++j) {
                float ref = 0;
                for (int k = 0; k < 32; ++k) ref += (float)(i + 2 * k) * (float)(3 * j - k + 2);
                worst = std::max(worst, std::fabs(ref - h[1280 + i * 16 + j]));
            }
        if (err) *err = worst;
        if (worst > 1e-3f) throw EngineError(MI355VITS_ERR_INTERNAL, "MFMA fragment layout differs from the one the kernels assume");
    });
}

}  // extern "C"
