// lab_api.cpp — the hooks of include/mi355vits_lab.h: kernel unit tests, a conv micro-benchmark, the box probes, the MFMA layout
// self test.  NOT part of the product library (libmi355vits.so exports include/mi355vits.h only): linked into
//   libmi355vits_hooks.so   the product's own objects + this file (the kernel-level GPU tests run the product's kernels through it),
//   libmi355vits_lab.so     the -DMI355_LAB build (A/B switches, tools/), and the CPU model of the kernels (tests/emu).
#include "c_api_internal.h"
#include "mi355vits_lab.h"

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

void check_lens(const int32_t* len, int B, int T, const char* what) {
    for (int b = 0; len && b < B; ++b)
        if (len[b] < 0 || len[b] > T) throw EngineError(MI355VITS_ERR_INVALID, what);
}
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
        HIP_CHECK(hipSetDevice(device));
        const size_t nx = (size_t)t->B * t->Cin * t->T, ny = (size_t)t->B * t->Cout * t->T;
        const size_t nw = (size_t)t->Cout * t->Cin * t->K;
        DevBuf dx(nx * 4), dy(ny * 4), dw(nw * 4), db(t->Cout * 4), dres(ny * 4), dil(t->B * 4), dol(t->B * 4), dcond((size_t)t->B * t->Cout * 4);
        std::vector<float> packed;
        HIP_CHECK(hipMemcpy(dx.p, t->x, nx * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, t->y, ny * 4, hipMemcpyHostToDevice));
        a.x = dx.as<float>();
        a.y = dy.as<float>();
        a.in_slope = t->in_slope;
        if (t->bias) { HIP_CHECK(hipMemcpy(db.p, t->bias, t->Cout * 4, hipMemcpyHostToDevice)); a.bias = db.as<float>(); }
        if (t->res) { HIP_CHECK(hipMemcpy(dres.p, t->res, ny * 4, hipMemcpyHostToDevice)); a.res = dres.as<float>(); }
        if (t->cond) { HIP_CHECK(hipMemcpy(dcond.p, t->cond, (size_t)t->B * t->Cout * 4, hipMemcpyHostToDevice)); a.cond = dcond.as<float>(); }
        if (t->in_len) { HIP_CHECK(hipMemcpy(dil.p, t->in_len, t->B * 4, hipMemcpyHostToDevice)); a.in_len = dil.as<int>(); }
        if (t->out_len) { HIP_CHECK(hipMemcpy(dol.p, t->out_len, t->B * 4, hipMemcpyHostToDevice)); a.out_len = dol.as<int>(); }
        if (t->impl == 3) {
            std::vector<uint32_t> b3(bf16x3_packed_words_mode(t->Cout, t->Cin, t->K, EPI_STD));
            pack_conv_weights_bf16x3_mode(t->w, t->Cout, t->Cin, t->K, EPI_STD, 1, b3.data());
            DevBuf db3(b3.size() * 4);
            HIP_CHECK(hipMemcpy(db3.p, b3.data(), b3.size() * 4, hipMemcpyHostToDevice));
            a.wb3 = db3.as<float>();
            DevBuf dpart(ny * 4 * (size_t)a.ksplit);
            if (a.ksplit > 1) a.part = dpart.as<float>();
            launch_enc_conv_b3(a, nullptr);
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipGetLastError());
            if (a.ksplit > 1) {
                std::vector<float> parts(ny * (size_t)a.ksplit);
                HIP_CHECK(hipMemcpy(parts.data(), dpart.p, parts.size() * 4, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < ny; ++i) {
                    float v = parts[i];
                    for (int sl = 1; sl < a.ksplit; ++sl) v += parts[(size_t)sl * ny + i];
                    t->y[i] = v;
                }
                return;
            }
        } else if (t->impl == 4) {
            std::vector<uint32_t> pp(p16_packed_words(t->Cout, t->Cin, t->K));
            pack_conv_weights_p16(t->w, t->Cout, t->Cin, t->K, pp.data());
            DevBuf dpp(pp.size() * 4);
            HIP_CHECK(hipMemcpy(dpp.p, pp.data(), pp.size() * 4, hipMemcpyHostToDevice));
            a.w = dpp.as<float>();
            a.in_len_host = t->in_len;
            launch_rb_conv(a, nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        } else if (t->impl == 1 || t->impl == 2) {
            packed.resize(mfma_packed_floats(t->Cout, t->Cin, t->K));
            pack_conv_weights_mfma(t->w, t->Cout, t->Cin, t->K, packed.data());
            DevBuf dp(packed.size() * 4);
            HIP_CHECK(hipMemcpy(dp.p, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
            a.w = dp.as<float>();
            std::vector<uint32_t> b3;
            std::unique_ptr<DevBuf> db3;
            if (t->impl == 2) {  // split-bf16 staged kernel (MATH_BF16X3 / MATH_BF16W)
                b3.resize(bf16x3_packed_words_mode(t->Cout, t->Cin, t->K, EPI_STD));
                pack_conv_weights_bf16x3_mode(t->w, t->Cout, t->Cin, t->K, EPI_STD, 1, b3.data());
                db3.reset(new DevBuf(b3.size() * 4));
                HIP_CHECK(hipMemcpy(db3->p, b3.data(), b3.size() * 4, hipMemcpyHostToDevice));
                a.wb3 = db3->as<float>();
            }
            launch_conv1d_mfma(a, nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        } else {
            HIP_CHECK(hipMemcpy(dw.p, t->w, nw * 4, hipMemcpyHostToDevice));
            a.w = dw.as<float>();
            launch_conv1d_generic(a, nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(t->y, dy.p, ny * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t n = (size_t)B * C * T;
        std::vector<uint32_t> b3(bf16x3_packed_words_mode(C, C, 1, EPI_STD));
        pack_conv_weights_bf16x3_mode(w, C, C, 1, EPI_STD, 1, b3.data());
        DevBuf dx(n * 4), dres(n * 4), dy(n * 4), db3(b3.size() * 4), db(C * 4), dg(C * 4), dbt(C * 4), dil((size_t)B * 4), dol((size_t)B * 4);
        HIP_CHECK(hipMemcpy(dx.p, x, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dres.p, res, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, y, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(db3.p, b3.data(), b3.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dg.p, gamma, C * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dbt.p, beta, C * 4, hipMemcpyHostToDevice));
        ConvArgs c;
        c.x = dx.as<float>(); c.x_bs = (long)C * T; c.x_ld = T;
        c.res = dres.as<float>(); c.res_bs = (long)C * T; c.res_ld = T;
        c.y = in_place ? dres.as<float>() : dy.as<float>(); c.y_bs = (long)C * T; c.y_ld = T;
        c.wb3 = db3.as<float>();
        c.math = math;
        c.B = B; c.Cin = C; c.Cout = C; c.T = T; c.K = 1; c.dil = 1; c.pad = 0;
        if (bias) { HIP_CHECK(hipMemcpy(db.p, bias, C * 4, hipMemcpyHostToDevice)); c.bias = db.as<float>(); }
        if (in_len) { HIP_CHECK(hipMemcpy(dil.p, in_len, (size_t)B * 4, hipMemcpyHostToDevice)); c.in_len = dil.as<int>(); }
        const int* dout = nullptr;
        if (ln_out_len) { HIP_CHECK(hipMemcpy(dol.p, ln_out_len, (size_t)B * 4, hipMemcpyHostToDevice)); dout = dol.as<int>(); }
        launch_enc_o_ln(c, dg.as<float>(), dbt.as<float>(), dout, eps, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(y, in_place ? dres.p : dy.p, n * 4, hipMemcpyDeviceToHost));
    });
}

int mi355vits_test_conv_post(int device, int B, int Cin, int K, int L, const float* x, const float* w, const int32_t* valid_len,
                             const double* volumes, float* audio, float* peaks, int16_t* pcm, int32_t* kernel) {
    return guarded(nullptr, [&] {
        if (!x || !w || !valid_len || !audio || !peaks || !pcm) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || Cin < 1 || K < 1 || !(K & 1) || L < 1 || (size_t)B * Cin * L >= 0x7fffffffull / 4) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        check_lens(valid_len, B, L, "valid_len out of range");
        HIP_CHECK(hipSetDevice(device));
        const size_t nx = (size_t)B * Cin * L, na = (size_t)B * L;
        DevBuf dx(nx * 4), dw((size_t)Cin * K * 4), dl((size_t)B * 4), dv((size_t)B * 8), da(na * 4), dp((size_t)B * 4), dq(na * 2);
        HIP_CHECK(hipMemcpy(dx.p, x, nx * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dw.p, w, (size_t)Cin * K * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, valid_len, (size_t)B * 4, hipMemcpyHostToDevice));
        if (volumes) HIP_CHECK(hipMemcpy(dv.p, volumes, (size_t)B * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(da.p, audio, na * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dq.p, pcm, na * 2, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dp.p, 0, (size_t)B * 4));  // the peaks are an atomic maximum over bit patterns: zeroed before the launch, as the engine does
        if (kernel) *kernel = conv_post_kernel(dx.as<float>(), (long)Cin * L, L, Cin, K, da.as<float>(), L);
        launch_conv_post_tanh(dx.as<float>(), (long)Cin * L, L, dw.as<float>(), Cin, K, B, L, dl.as<int>(), da.as<float>(), L, dp.as<unsigned>(), nullptr);
        launch_pcm16(da.as<float>(), L, dp.as<unsigned>(), dl.as<int>(), B, L, dq.as<int16_t>(), L, nullptr, volumes ? dv.as<double>() : nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(audio, da.p, na * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(peaks, dp.p, (size_t)B * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(pcm, dq.p, na * 2, hipMemcpyDeviceToHost));
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
        for (int b = 0; b < B; ++b)
            if (lengths[b] < 0 || lengths[b] > row_stride || resample_out_len(lengths[b], f.L, f.M) > y_stride)
                throw EngineError(MI355VITS_ERR_INVALID, "row length out of range");
        const long items = resample_fill_tab(f, lengths, B, tab.data());
        HIP_CHECK(hipSetDevice(device));
        const size_t nx = (size_t)B * row_stride, ny = (size_t)B * y_stride;
        DevBuf dx(nx * 4), dy(ny * 4), dl(B * 4), dt(tab.size() * 4), dc(f.table.size() * 4), dp(B * 4);
        HIP_CHECK(hipMemcpy(dx.p, x, nx * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, lengths, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dt.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dc.p, f.table.data(), f.table.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dy.p, 0xff, ny * 4));  // NaNs: the kernel writes every sample of y
        HIP_CHECK(hipMemset(dp.p, 0, (size_t)B * 4));
        launch_resample(f, dc.as<float>(), dx.as<float>(), (long)row_stride, dl.as<int>(), B, dt.as<int>(), items, dy.as<float>(),
                        (long)y_stride, (int)y_stride, dp.as<unsigned>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(y, dy.p, ny * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(peaks, dp.p, (size_t)B * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t na = (size_t)B * row_stride;
        DevBuf df(n * 4), dc(n * 4), dl(B * 4), da(na * 4), dal(B * 4), dout(5 * n * 4);
        HIP_CHECK(hipMemcpy(df.p, frames, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dc.p, cum.data(), n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, len, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(da.p, audio, na * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dal.p, alen, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0xff, 5 * n * 4));  // the kernel writes every element it is asked for
        int* d = dout.as<int>();
        launch_align(df.as<int>(), dc.as<int>(), dl.as<int>(), B, T, da.as<float>(), (long)row_stride, dal.as<int>(), hop, L, M, d, d + n,
                     d + 2 * n, out_peak ? reinterpret_cast<float*>(d + 3 * n) : nullptr, out_peak ? reinterpret_cast<float*>(d + 4 * n) : nullptr,
                     nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out_frames, d, n * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(out_start, d + n, n * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(out_samples, d + 2 * n, n * 4, hipMemcpyDeviceToHost));
        if (out_peak) {
            HIP_CHECK(hipMemcpy(out_peak, d + 3 * n, n * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(out_rms, d + 4 * n, n * 4, hipMemcpyDeviceToHost));
        }
    });
}

int mi355vits_lab_g711_encode(int law, const int16_t* in, long n, uint8_t* out) {
    return guarded(nullptr, [&] {
        if (!in || !out || n < 1) throw EngineError(MI355VITS_ERR_INVALID, "null or empty argument");
        if (law != MI355VITS_ENC_ULAW && law != MI355VITS_ENC_ALAW) throw EngineError(MI355VITS_ERR_INVALID, "law must be MI355VITS_ENC_ULAW or MI355VITS_ENC_ALAW");
        DevBuf di((size_t)n * 2), dout((size_t)n);
        HIP_CHECK(hipMemcpy(di.p, in, (size_t)n * 2, hipMemcpyHostToDevice));
        launch_g711_encode(law, di.as<int16_t>(), n, dout.as<uint8_t>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out, dout.p, (size_t)n, hipMemcpyDeviceToHost));
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
        DevBuf din(lead + (size_t)n * 2 + 16), djob(sizeof(FlacJob)), dslots((size_t)frames * FLAC_SLOT_BYTES), dsizes(((size_t)frames + 1) * 4),
            doff((size_t)frames * 8), dout(flac_out_capacity(frames, n));
        int16_t* src = reinterpret_cast<int16_t*>(din.as<uint8_t>() + lead);
        if (n > 0) HIP_CHECK(hipMemcpy(src, pcm, (size_t)n * 2, hipMemcpyHostToDevice));
        const FlacJob job = {src, n, first_frame, 0};
        HIP_CHECK(hipMemcpy(djob.p, &job, sizeof(job), hipMemcpyHostToDevice));
        launch_flac_frames(djob.as<FlacJob>(), 1, frames, rate, dslots.as<uint8_t>(), dsizes.as<int>(), nullptr);
        launch_flac_gather(dslots.as<uint8_t>(), dsizes.as<int>(), doff.as<long long>(), frames, dout.as<uint8_t>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        std::vector<int> sizes((size_t)frames + 1, 0);
        if (frames > 0) HIP_CHECK(hipMemcpy(sizes.data(), dsizes.p, sizes.size() * 4, hipMemcpyDeviceToHost));
        size_t data = 0;
        for (long f = 0; f < frames; ++f) {
            if (sizes[f] < 11 || sizes[f] > 16 + 2 * FLAC_BLOCK) throw EngineError(MI355VITS_ERR_INTERNAL, "flac: frame " + std::to_string(f) + " has " + std::to_string(sizes[f]) + " bytes");
            data += (size_t)sizes[f];
        }
        if ((unsigned)sizes[frames] != (unsigned)data) throw EngineError(MI355VITS_ERR_INTERNAL, "flac: the device's total differs from the sum of the frame sizes");
        *n_bytes = FLAC_HEADER_BYTES + data;
        if (cap < *n_bytes) throw EngineError(MI355VITS_ERR_INVALID, "flac: the file has " + std::to_string(*n_bytes) + " bytes, out holds " + std::to_string(cap));
        flac_stream_header(out, rate, n, sizes.data(), frames);
        if (data) HIP_CHECK(hipMemcpy(out + FLAC_HEADER_BYTES, dout.p, data, hipMemcpyDeviceToHost));
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
        DevBuf din(src_bytes + 16), djobs(sizeof(FlacJob) * (size_t)n_jobs), dslots((size_t)frames * FLAC_SLOT_BYTES + 16),
            dsizes(flac_info_words(frames, n_jobs) * 4), dpre(((size_t)frames + 1) * 4), dftab(((size_t)frames + 1) * 8),
            dhdr((size_t)FLAC_HDR_WORDS * n_jobs * 4), ditems(flac_gather_items(bound) * 4), djtab((size_t)FLAC_JTAB_ROWS * n_jobs * 4),
            dout((size_t)bound + 16);
        std::vector<FlacJob> jobs((size_t)n_jobs);
        long slot0 = 0;
        for (int j = 0; j < n_jobs; ++j) {
            int16_t* src = reinterpret_cast<int16_t*>(din.as<uint8_t>() + at[(size_t)j]);
            if (n[j] > 0) HIP_CHECK(hipMemcpy(src, pcm[j], (size_t)n[j] * 2, hipMemcpyHostToDevice));
            jobs[(size_t)j] = FlacJob{src, n[j], 0, (int)slot0};
            slot0 += flac_frames(n[j]);
        }
        HIP_CHECK(hipMemcpy(djobs.p, jobs.data(), sizeof(FlacJob) * jobs.size(), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0xa5, (size_t)bound + 16));  // the gather writes every byte of the block
        launch_flac_frames(djobs.as<FlacJob>(), n_jobs, frames, rate, dslots.as<uint8_t>(), dsizes.as<int>(), nullptr);
        launch_flac_place(djobs.as<FlacJob>(), n_jobs, frames, rate, 0, dsizes.as<int>(), dpre.as<unsigned>(), dftab.as<int2>(), dhdr.as<unsigned>(),
                          ditems.as<int>(), djtab.as<int>(), nullptr);
        launch_flac_gather_streams(n_jobs, frames, dslots.as<uint8_t>(), dsizes.as<int>(), dftab.as<int2>(), dhdr.as<unsigned>(), ditems.as<int>(), 0,
                                   bound, dout.as<uint8_t>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        std::vector<int> info(flac_info_words(frames, n_jobs));
        HIP_CHECK(hipMemcpy(info.data(), dsizes.p, info.size() * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipMemcpy(out, dout.p, (size_t)end, hipMemcpyDeviceToHost));
    });
}

int mi355vits_lab_edges(const float* audio, long stride, const int32_t* lens, const float* peaks, int B, float ratio, int32_t* s_first,
                        int32_t* s_last) {
    return guarded(nullptr, [&] {
        if (!audio || !lens || !peaks || !s_first || !s_last || B < 1 || stride < 1) throw EngineError(MI355VITS_ERR_INVALID, "null or empty argument");
        if (!(ratio > 0.0f && ratio <= 1.0f)) throw EngineError(MI355VITS_ERR_INVALID, "ratio must be in (0, 1]");
        long l_max = 0;
        for (int b = 0; b < B; ++b) {
            if (lens[b] < 0 || lens[b] > stride) throw EngineError(MI355VITS_ERR_INVALID, "row length out of range");
            l_max = std::max<long>(l_max, lens[b]);
        }
        const size_t na = (size_t)B * stride;
        DevBuf da(na * 4), dl((size_t)B * 4), dp((size_t)B * 4), dout((size_t)B * 8);
        HIP_CHECK(hipMemcpy(da.p, audio, na * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, lens, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dp.p, peaks, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0x5a, (size_t)B * 8));  // the launch initialises its words itself
        int* d = dout.as<int>();
        launch_edges(da.as<float>(), stride, dl.as<int>(), dp.as<unsigned>(), B, l_max, ratio, d, d + B, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(s_first, d, (size_t)B * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(s_last, d + B, (size_t)B * 4, hipMemcpyDeviceToHost));
    });
}

int mi355vits_lab_loudness(const float* audio, long stride, const int32_t* lens, int B, int32_t rate, double* lufs, int32_t* blocks,
                           int32_t* gated) {
    return guarded(nullptr, [&] {
        if (!audio || !lens || !lufs || !blocks || !gated || B < 1 || stride < 1) throw EngineError(MI355VITS_ERR_INVALID, "null or empty argument");
        LoudnessPlan lp;
        if (!loudness_plan(rate, lp)) throw EngineError(MI355VITS_ERR_INVALID, "rate " + std::to_string(rate) + " Hz is below " + std::to_string(LOUD_MIN_HZ) + " Hz");
        long l_max = 0;
        for (int b = 0; b < B; ++b) {
            if (lens[b] < 0 || lens[b] > stride) throw EngineError(MI355VITS_ERR_INVALID, "row length out of range");
            l_max = std::max<long>(l_max, lens[b]);
        }
        const size_t na = (size_t)B * stride;
        const long ldE = std::max<long>(1, loudness_steps(l_max, lp.S));
        DevBuf da(na * 4), dl((size_t)B * 4), dE((size_t)B * ldE * 8), dout((size_t)B * 16);
        HIP_CHECK(hipMemcpy(da.p, audio, na * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, lens, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dE.p, 0xff, (size_t)B * ldE * 8));  // NaN: the launch writes every energy it reads
        HIP_CHECK(hipMemset(dout.p, 0x5a, (size_t)B * 16));
        double* d_lufs = dout.as<double>();
        int* d_blocks = reinterpret_cast<int*>(d_lufs + B);
        launch_loudness(rate, da.as<float>(), stride, dl.as<int>(), B, l_max, dE.as<double>(), ldE, d_lufs, d_blocks, d_blocks + B, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(lufs, d_lufs, (size_t)B * 8, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(blocks, d_blocks, (size_t)B * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(gated, d_blocks + B, (size_t)B * 4, hipMemcpyDeviceToHost));
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
        DevBuf da(na * 4), dj(jobs.size() * sizeof(LimitJob)), ds(jobs.size() * sizeof(LimitStat)), dc((size_t)floats * 4);
        HIP_CHECK(hipMemcpy(da.p, audio, na * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dj.p, jobs.data(), jobs.size() * sizeof(LimitJob), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(ds.p, 0x5a, jobs.size() * sizeof(LimitStat)));  // the launch initialises its words itself
        HIP_CHECK(hipMemset(dc.p, 0xff, (size_t)floats * 4));              // NaN: the launch writes every curve element
        DevBuf de(env ? (size_t)floats * 8 : 8);
        if (env)  // the jobs' envelopes one behind the other, as k_true_peak_env leaves them
            for (const LimitJob& j : jobs)
                HIP_CHECK(hipMemcpy(de.as<double>() + j.off, env + (size_t)j.row * stride, (size_t)j.n * 8, hipMemcpyHostToDevice));
        launch_limit(dj.as<LimitJob>(), (int)jobs.size(), tiles, L, da.as<float>(), stride, ds.as<LimitStat>(), dc.as<float>(), nullptr,
                     env ? de.as<double>() : nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        std::vector<LimitStat> st(jobs.size());
        std::vector<float> cv((size_t)floats);
        HIP_CHECK(hipMemcpy(st.data(), ds.p, st.size() * sizeof(LimitStat), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(cv.data(), dc.p, cv.size() * 4, hipMemcpyDeviceToHost));
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
        long l_max = 0;
        std::vector<LimitJob> jobs;  // the envelope form: one job per non-empty row
        for (int b = 0; b < B; ++b) {
            if (lens[b] < 0 || lens[b] > stride) throw EngineError(MI355VITS_ERR_INVALID, "row length out of range");
            l_max = std::max<long>(l_max, lens[b]);
            if (lens[b] < 1) continue;
            LimitJob j;
            j.g = j.c = j.U = 1.0; j.row = b; j.n = lens[b]; j.off = j.tile0 = 0;
            jobs.push_back(j);
        }
        const size_t na = (size_t)B * stride;
        DevBuf da((na + 4) * 4), dl((size_t)B * 4), dt((size_t)B * 8);
        HIP_CHECK(hipMemset(da.p, 0xff, (na + 4) * 4));  // NaN in front of the first row and behind the last
        float* d_audio = da.as<float>() + offset_floats;
        HIP_CHECK(hipMemcpy(d_audio, audio, na * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, lens, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dt.p, 0x5a, (size_t)B * 8));  // the launch initialises its words itself
        launch_true_peak(d_audio, stride, dl.as<int>(), B, l_max, dt.as<double>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(tp, dt.p, (size_t)B * 8, hipMemcpyDeviceToHost));
        if (!env_out) return;
        for (size_t i = 0; i < na; ++i) env_out[i] = 0.0;
        if (jobs.empty()) return;
        long floats = 0;
        const long tiles = limit_place_jobs(jobs.data(), (int)jobs.size(), &floats);
        if (tiles < 0) throw EngineError(MI355VITS_ERR_INVALID, "the envelopes together exceed 2^31 - 1 samples");
        DevBuf dj(jobs.size() * sizeof(LimitJob)), de((size_t)floats * 8);
        HIP_CHECK(hipMemcpy(dj.p, jobs.data(), jobs.size() * sizeof(LimitJob), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(de.p, 0xff, (size_t)floats * 8));  // NaN: the launch writes every element
        launch_true_peak_env(dj.as<LimitJob>(), (int)jobs.size(), tiles, d_audio, stride, de.as<double>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        for (const LimitJob& j : jobs)
            HIP_CHECK(hipMemcpy(env_out + (size_t)j.row * stride, de.as<double>() + j.off, (size_t)j.n * 8, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t nx = (size_t)B * Cin * Tin, ny = (size_t)B * Cout * Tin * stride, nw = (size_t)Cin * Cout * K;
        DevBuf dx(nx * 4), dy(ny * 4), dw(nw * 4), db(Cout * 4);
        HIP_CHECK(hipMemcpy(dx.p, x, nx * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, y, ny * 4, hipMemcpyHostToDevice));  // a position no kernel writes keeps the caller's value
        if (impl == 3) {
            // the resident-input polyphase kernels (k_ups_pl: 256 -> 128, 128 -> 64; k_ups64: 64 -> 32), MATH_BF16X3; a valid length per
            // row is part of their contract (the engine always has one): in_len, or every row at full length
            const int taps = convt_taps(K, stride);
            std::vector<float> wv((size_t)stride * Cout * Cin * taps), bv((size_t)stride * Cout);
            convt_to_polyphase(w, bias, Cin, Cout, K, stride, wv.data(), bv.data());
            std::vector<uint32_t> pp(p16_packed_words(stride * Cout, Cin, taps));
            pack_conv_weights_p16n(wv.data(), stride * Cout, Cin, taps, pp.data());
            std::vector<int> lens = in_len ? std::vector<int>(in_len, in_len + B) : std::vector<int>((size_t)B, Tin);
            DevBuf dpp(pp.size() * 4), dbias(bv.size() * 4), dlen((size_t)B * 4);
            HIP_CHECK(hipMemcpy(dpp.p, pp.data(), pp.size() * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(dbias.p, bv.data(), bv.size() * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(dlen.p, lens.data(), (size_t)B * 4, hipMemcpyHostToDevice));
            ConvArgs u = convt_hook_args(impl, B, Cin, Cout, Tin, K, stride);
            u.x = dx.as<float>();
            u.y = dy.as<float>();
            u.w = dpp.as<float>(); u.bias = dbias.as<float>(); u.in_len = dlen.as<int>(); u.in_len_host = lens.data();
            u.in_slope = in_slope;
            if (!ups_pl_supported(u)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the resident-input polyphase kernels");
            launch_ups_pl(u, nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        } else if (impl == 1 || impl == 2) {
            // polyphase filters on the MFMA conv kernel (the path Engine uses); impl 2: the split-bf16 staged kernels
            // (MATH_BF16X3; 64-channel chunks run the persistent producer / consumer form)
            const int taps = convt_taps(K, stride);
            std::vector<float> wv((size_t)stride * Cout * Cin * taps), bv((size_t)stride * Cout);
            convt_to_polyphase(w, bias, Cin, Cout, K, stride, wv.data(), bv.data());
            std::vector<float> pk(mfma_packed_floats(stride * Cout, Cin, taps));
            pack_conv_weights_mfma(wv.data(), stride * Cout, Cin, taps, pk.data());
            DevBuf dp(pk.size() * 4), dbias(bv.size() * 4);
            HIP_CHECK(hipMemcpy(dp.p, pk.data(), pk.size() * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(dbias.p, bv.data(), bv.size() * 4, hipMemcpyHostToDevice));
            ConvArgs u = convt_hook_args(impl, B, Cin, Cout, Tin, K, stride);
            u.x = dx.as<float>();
            u.y = dy.as<float>();
            u.w = dp.as<float>(); u.bias = dbias.as<float>();
            u.in_slope = in_slope;
            std::vector<uint32_t> b3;
            std::unique_ptr<DevBuf> db3;
            if (impl == 2) {
                b3.resize(bf16x3_packed_words_mode(stride * Cout, Cin, taps, EPI_STD));
                pack_conv_weights_bf16x3_mode(wv.data(), stride * Cout, Cin, taps, EPI_STD, 1, b3.data());
                db3.reset(new DevBuf(b3.size() * 4));
                HIP_CHECK(hipMemcpy(db3->p, b3.data(), b3.size() * 4, hipMemcpyHostToDevice));
                u.wb3 = db3->as<float>();
            }
            launch_conv1d_mfma(u, nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        } else {
            HIP_CHECK(hipMemcpy(dw.p, w, nw * 4, hipMemcpyHostToDevice));
            ConvTArgs a;
            a.x = dx.as<float>(); a.x_bs = (long)Cin * Tin; a.x_ld = Tin;
            a.y = dy.as<float>(); a.y_bs = (long)Cout * Tin * stride; a.y_ld = Tin * stride;
            a.w = dw.as<float>();
            if (bias) { HIP_CHECK(hipMemcpy(db.p, bias, Cout * 4, hipMemcpyHostToDevice)); a.bias = db.as<float>(); }
            a.B = B; a.Cin = Cin; a.Cout = Cout; a.Tin = Tin; a.K = K; a.stride = stride; a.pad = (K - stride) / 2;
            a.in_slope = in_slope;
            launch_conv_transpose1d(a, nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(y, dy.p, ny * 4, hipMemcpyDeviceToHost));
    });
}

int mi355vits_test_rel_attention(int device, int impl, int B, int T, int H, int n_heads, int W, const float* qkv,
                                 const float* emb_rel_k, const float* emb_rel_v, const int32_t* len, float* out) {
    return guarded(nullptr, [&] {
        if (!qkv || !emb_rel_k || !emb_rel_v || !len || !out) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1 || n_heads < 1 || H % n_heads || W < 0) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        for (int b = 0; b < B; ++b)
            if (len[b] < 0 || len[b] > T) throw EngineError(MI355VITS_ERR_INVALID, "len out of range");
        const int d = H / n_heads, nrel = 2 * W + 1;
        if (impl == 0 && T > rel_attention_valu_cap(H, n_heads, W)) throw EngineError(MI355VITS_ERR_INVALID, "T beyond the VALU kernel's LDS row buffer");
        if (impl == 1 && !rel_attention_mfma_supported(T, H, n_heads, W)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the MFMA kernel");
        if (impl == 2 && !rel_attention_stream_supported(H, n_heads, W)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the streamed kernel");
        if (impl < 0 || impl > 2) throw EngineError(MI355VITS_ERR_INVALID, "impl must be 0, 1 or 2");
        HIP_CHECK(hipSetDevice(device));
        const size_t nq = (size_t)B * 3 * H * T, no = (size_t)B * H * T, ne = (size_t)nrel * d;
        DevBuf dq(nq * 4), dk(ne * 4), dv(ne * 4), dl((size_t)B * 4), dout(no * 4);
        HIP_CHECK(hipMemcpy(dq.p, qkv, nq * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dk.p, emb_rel_k, ne * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dv.p, emb_rel_v, ne * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, len, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dout.p, out, no * 4, hipMemcpyHostToDevice));
        if (impl == 0)
            launch_rel_attention(dq.as<float>(), dk.as<float>(), dv.as<float>(), dl.as<int>(), B, T, H, n_heads, W, dout.as<float>(), nullptr);
        else if (impl == 1)
            launch_rel_attention_mfma(dq.as<float>(), dk.as<float>(), dv.as<float>(), dl.as<int>(), B, T, H, n_heads, W, dout.as<float>(), nullptr);
        else
            launch_rel_attention_stream(dq.as<float>(), dk.as<float>(), dv.as<float>(), dl.as<int>(), B, T, H, n_heads, W, dout.as<float>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out, dout.p, no * 4, hipMemcpyDeviceToHost));
    });
}

// one WaveNet layer through a chosen path (include/mi355vits_lab.h says what each reads and writes at and past len[b])
int mi355vits_test_wn_layer(int device, const mi355vits_wn_test* t) {
    return guarded(nullptr, [&] {
        if (!t || !t->h_in || !t->w_in || !t->b_in || !t->w_rs || !t->b_rs || !t->len || !t->h_out || !t->skip) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        const int B = t->B, H = t->H, T = t->T, K = t->K, dil = t->dilation, Crs = t->Crs;
        if (B < 1 || H < 1 || T < 1 || K < 1 || (K % 2) == 0 || dil < 1 || (Crs != H && Crs != 2 * H)) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        if ((long)B * H * T >= 0x7fffffffL / 4) throw EngineError(MI355VITS_ERR_INVALID, "tensor too large for the hook");
        for (int b = 0; b < B; ++b)
            if (t->len[b] < 0 || t->len[b] > T) throw EngineError(MI355VITS_ERR_INVALID, "len out of range");
        if (t->impl < 0 || t->impl > 2) throw EngineError(MI355VITS_ERR_INVALID, "impl must be 0, 1 or 2");
        if (t->impl == 2 ? t->math != MATH_BF16X3 : t->math != MATH_F32) throw EngineError(MI355VITS_ERR_INVALID, "math mode: MATH_F32 for impl 0 and 1, MATH_BF16X3 for impl 2");
        if (t->impl == 1 && !wn_layer_fused_supported(H, K, dil)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the fused f32 layer");
        if (t->impl == 2 && !wn_layer_b3_supported(H, K, dil)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the fused split-bf16 layer");
        HIP_CHECK(hipSetDevice(device));
        const size_t n = (size_t)B * H * T;
        const std::vector<float> w_in(t->w_in, t->w_in + (size_t)2 * H * H * K), w_rs(t->w_rs, t->w_rs + (size_t)Crs * H);
        DevBuf dh(n * 4), dho(n * 4), dsk(n * 4), du(n * 4), dbi((size_t)2 * H * 4), dbr((size_t)Crs * 4), dc((size_t)B * 2 * H * 4), dl((size_t)B * 4);
        HIP_CHECK(hipMemcpy(dh.p, t->h_in, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dho.p, t->h_out, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dsk.p, t->skip, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dbi.p, t->b_in, (size_t)2 * H * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dbr.p, t->b_rs, (size_t)Crs * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, t->len, (size_t)B * 4, hipMemcpyHostToDevice));
        if (t->cond) HIP_CHECK(hipMemcpy(dc.p, t->cond, (size_t)B * 2 * H * 4, hipMemcpyHostToDevice));
        const long hbs = (long)H * T;
        auto upload = [](const void* p, size_t bytes) {
            std::unique_ptr<DevBuf> d(new DevBuf(bytes));
            HIP_CHECK(hipMemcpy(d->p, p, bytes, hipMemcpyHostToDevice));
            return d;
        };
        std::unique_ptr<DevBuf> dwi, dwr;
        const float* h_result = dho.as<float>();
        if (t->impl == 0) {
            // Engine::coupling_layer's two launches: the gate conv h -> u (no input mask: the engine's h is zero past a row), then the
            // res/skip conv u -> (h in place, skip); weights as Engine::add_conv_data stages them for Engine::pick_conv's MFMA_F32 / GENERIC
            // (each conv on its own, as add_conv_data decides per conv: packed fragments where the MFMA kernel takes it, raw weights else)
            const bool mfma_in = conv1d_mfma_supported(H, 2 * H, K, 1), mfma_rs = conv1d_mfma_supported(H, Crs, 1, 1);
            if (mfma_in) {
                std::vector<float> pi(mfma_packed_floats(2 * H, H, K), 0.0f);
                pack_conv_weights_mfma_mode(w_in.data(), 2 * H, H, K, EPI_GATE, pi.data());
                dwi = upload(pi.data(), pi.size() * 4);
            } else {
                dwi = upload(w_in.data(), w_in.size() * 4);
            }
            if (mfma_rs) {
                std::vector<float> pr(mfma_packed_floats(Crs, H, 1), 0.0f);
                pack_conv_weights_mfma_mode(w_rs.data(), Crs, H, 1, EPI_STD, pr.data());
                dwr = upload(pr.data(), pr.size() * 4);
            } else {
                dwr = upload(w_rs.data(), w_rs.size() * 4);
            }
            ConvArgs in;
            in.x = dh.as<float>(); in.x_bs = hbs; in.x_ld = T;
            in.y = du.as<float>(); in.y_bs = hbs; in.y_ld = T;
            in.epi = EPI_GATE; in.H = H; in.dil = dil;
            if (t->cond) { in.cond = dc.as<float>(); in.cond_bs = 2L * H; }
            in.B = B; in.T = T;
            in.fixed_rule = 1; in.Cin = H; in.Cout = 2 * H; in.K = K; in.bias = dbi.as<float>(); in.pad = (K * dil - dil) / 2;
            in.w = dwi->as<float>(); in.math = MATH_F32;
            ConvArgs rs;
            rs.x = du.as<float>(); rs.x_bs = hbs; rs.x_ld = T;
            rs.y = dh.as<float>(); rs.y_bs = hbs; rs.y_ld = T;
            rs.y2 = dsk.as<float>(); rs.y2_bs = hbs; rs.y2_ld = T;
            rs.epi = EPI_RESSKIP; rs.H = H; rs.skip_init = t->skip_init != 0;
            rs.out_len = dl.as<int>();
            rs.B = B; rs.T = T;
            rs.fixed_rule = 1; rs.Cin = H; rs.Cout = Crs; rs.K = 1; rs.bias = dbr.as<float>(); rs.pad = 0;
            rs.w = dwr->as<float>(); rs.math = MATH_F32;
            if (mfma_in) launch_conv1d_mfma(in, nullptr);
            else launch_conv1d_generic(in, nullptr);
            if (mfma_rs) launch_conv1d_mfma(rs, nullptr);
            else launch_conv1d_generic(rs, nullptr);
            h_result = dh.as<float>();  // in place
        } else {
            if (t->impl == 1) {
                std::vector<float> pi(mfma_packed_floats(2 * H, H, K), 0.0f), pr(mfma_packed_floats(Crs, H, 1), 0.0f);
                pack_conv_weights_mfma_mode(w_in.data(), 2 * H, H, K, EPI_GATE, pi.data());
                pack_conv_weights_mfma_mode(w_rs.data(), Crs, H, 1, EPI_STD, pr.data());
                dwi = upload(pi.data(), pi.size() * 4);
                dwr = upload(pr.data(), pr.size() * 4);
            } else if (wn_layer_b3_shape() != 32) {
                // Engine::add_conv_data's packed_w16 of both convs (16x16x32 tiles)
                std::vector<uint32_t> bi(w16_packed_words(2 * H, H, K)), br(w16_packed_words(Crs, H, 1));
                pack_conv_weights_w16(w_in.data(), 2 * H, H, K, true, bi.data());
                pack_conv_weights_w16(w_rs.data(), Crs, H, 1, false, br.data());
                dwi = upload(bi.data(), bi.size() * 4);
                dwr = upload(br.data(), br.size() * 4);
            } else {
                // MI355VITS_WN_SHAPE=32 (lab build, CPU model).  Engine::add_conv_data's packed_b3w: 32-row tile q of the gate conv = the tanh rows of channels 16 q .. 16 q + 15, then their
                // sigmoid rows, as layout-1 planes; the res/skip conv in plain row order (packed_b3s)
                const size_t row = (size_t)H * K;
                std::vector<float> wg(w_in.size());
                for (int q = 0; q < 2 * H / 32; ++q)
                    for (int r = 0; r < 32; ++r) {
                        const int src = (r < 16 ? 0 : H) + 16 * q + (r & 15);
                        memcpy(wg.data() + ((size_t)32 * q + r) * row, w_in.data() + (size_t)src * row, row * sizeof(float));
                    }
                std::vector<uint32_t> bi(bf16x3_packed_words_mode(2 * H, H, K, EPI_STD)), br(bf16x3_packed_words_mode(Crs, H, 1, EPI_STD));
                pack_conv_weights_bf16x3_mode(wg.data(), 2 * H, H, K, EPI_STD, 1, bi.data());
                pack_conv_weights_bf16x3_mode(w_rs.data(), Crs, H, 1, EPI_STD, 1, br.data());
                dwi = upload(bi.data(), bi.size() * 4);
                dwr = upload(br.data(), br.size() * 4);
            }
            WnArgs w;
            w.h_in = dh.as<float>(); w.h_out = dho.as<float>(); w.h_bs = hbs; w.h_ld = T;
            w.skip = dsk.as<float>(); w.s_bs = hbs; w.s_ld = T;
            w.w_in = dwi->as<float>(); w.b_in = dbi.as<float>();
            w.w_rs = dwr->as<float>(); w.b_rs = dbr.as<float>();
            if (t->cond) { w.cond = dc.as<float>(); w.cond_bs = 2L * H; }
            w.len = dl.as<int>();
            w.B = B; w.H = H; w.T = T; w.K = K; w.dil = dil; w.Crs = Crs; w.skip_init = t->skip_init != 0;
            if (t->impl == 2) { w.math = MATH_BF16X3; w.shape = wn_layer_b3_shape(); launch_wn_layer_b3(w, nullptr); }
            else launch_wn_layer(w, nullptr);
        }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        // impl 1 and 2: whatever the device's h_out holds now (Crs = H: the launch must have left it as it was); impl 0 works in place
        // on its copy of h, which a last layer leaves untouched: nothing to report then
        if (t->impl != 0 || Crs == 2 * H) HIP_CHECK(hipMemcpy(t->h_out, h_result, n * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(t->skip, dsk.p, n * 4, hipMemcpyDeviceToHost));
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
        for (int b = 0; b < B; ++b)
            if (t->len[b] < 0 || t->len[b] > T) throw EngineError(MI355VITS_ERR_INVALID, "len out of range");
        if (t->impl < 0 || t->impl > 3) throw EngineError(MI355VITS_ERR_INVALID, "impl must be 0, 1, 2 or 3");
        if (t->impl == 3 ? !math_on_bf16(t->math) : t->math != MATH_F32)
            throw EngineError(MI355VITS_ERR_INVALID, "math mode: MATH_F32 for impl 0, 1 and 2, MATH_BF16X3 or MATH_BF16W for impl 3");
        if (t->impl == 1 && !dds_layer_fused_supported(C)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the fused DDS layer");
        if (t->impl >= 2 && !dds_stack_supported(C, K, NL, PC)) throw EngineError(MI355VITS_ERR_INVALID, "shape not supported by the DDS stack kernels");
        HIP_CHECK(hipSetDevice(device));
        const size_t n = (size_t)B * C * T, nz = (size_t)B * 2 * T, no = (size_t)B * PC * T;
        auto upload = [](const void* p, size_t bytes) {
            std::unique_ptr<DevBuf> d(new DevBuf(bytes));
            if (bytes) HIP_CHECK(hipMemcpy(d->p, p, bytes, hipMemcpyHostToDevice));
            return d;
        };
        std::vector<std::unique_ptr<DevBuf>> keep;
        auto vecf = [&](const float* p, size_t count) -> const float* {
            keep.push_back(upload(p, count * 4));
            return keep.back()->as<float>();
        };
        // a dense 1x1 conv's weights [Cout, C, 1] in the format of the chosen path, as Engine::add_conv_data stages them
        const bool b3 = t->impl == 3;
        auto conv_mfma = [&](int Cout) { return conv1d_mfma_supported(C, Cout, 1, 1); };
        auto dense = [&](const float* w, int Cout) -> const float* {
            if (b3) {
                std::vector<uint32_t> p(bf16x3_packed_words_mode(Cout, C, 1, EPI_STD), 0u);
                pack_conv_weights_bf16x3_mode(w, Cout, C, 1, EPI_STD, 1, p.data());
                keep.push_back(upload(p.data(), p.size() * 4));
            } else if (t->impl != 0 || conv_mfma(Cout)) {
                std::vector<float> p(mfma_packed_floats(Cout, C, 1), 0.0f);
                pack_conv_weights_mfma_mode(w, Cout, C, 1, EPI_STD, p.data());
                keep.push_back(upload(p.data(), p.size() * 4));
            } else {
                keep.push_back(upload(w, (size_t)Cout * C * 4));
            }
            return keep.back()->as<float>();
        };
        DevBuf dsrc(n * 4), dxo(n * 4), dz(nz * 4), dout(no * 4), dl((size_t)B * 4), dcond((size_t)B * C * 4);
        HIP_CHECK(hipMemcpy(dsrc.p, t->src, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dxo.p, t->x_out, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, t->len, (size_t)B * 4, hipMemcpyHostToDevice));
        if (t->z) HIP_CHECK(hipMemcpy(dz.p, t->z, nz * 4, hipMemcpyHostToDevice));
        if (PC) HIP_CHECK(hipMemcpy(dout.p, t->out, no * 4, hipMemcpyHostToDevice));
        if (t->cond) HIP_CHECK(hipMemcpy(dcond.p, t->cond, (size_t)B * C * 4, hipMemcpyHostToDevice));
        const float* pre_w = t->pre_mode == DDS_PRE_AFFINE ? vecf(t->pre_w, C) : dense(t->pre_w, C);
        const float* pre_b = vecf(t->pre_b, C);
        const float *dw_w[DDS_STACK_MAX_LAYERS], *dw_b[DDS_STACK_MAX_LAYERS], *g1[DDS_STACK_MAX_LAYERS], *b1[DDS_STACK_MAX_LAYERS];
        const float *w1[DDS_STACK_MAX_LAYERS], *bb[DDS_STACK_MAX_LAYERS], *g2[DDS_STACK_MAX_LAYERS], *b2[DDS_STACK_MAX_LAYERS];
        for (int i = 0; i < NL; ++i) {
            dw_w[i] = vecf(t->dw_w[i], (size_t)C * K); dw_b[i] = vecf(t->dw_b[i], C);
            g1[i] = vecf(t->g1[i], C); b1[i] = vecf(t->b1[i], C);
            w1[i] = dense(t->w1x1[i], C); bb[i] = vecf(t->bias1x1[i], C);
            g2[i] = vecf(t->g2[i], C); b2[i] = vecf(t->b2[i], C);
        }
        const float* proj_w = PC ? dense(t->proj_w, PC) : nullptr;
        const float* proj_b = PC ? vecf(t->proj_b, PC) : nullptr;
        if (t->impl >= 2) {
            DdsStackArgs a;
            a.src = dsrc.as<float>(); a.pre_mode = t->pre_mode; a.pre_w = pre_w; a.pre_b = pre_b;
            if (t->cond) { a.cond = dcond.as<float>(); a.cond_bs = C; }
            a.z = t->z ? dz.as<float>() : nullptr; a.zch = t->zch;
            a.n_layers = NL; a.K = K;
            for (int i = 0; i < NL; ++i) {
                a.dw_w[i] = dw_w[i]; a.dw_b[i] = dw_b[i]; a.g1[i] = g1[i]; a.b1[i] = b1[i];
                a.w1x1[i] = w1[i]; a.bias1x1[i] = bb[i]; a.g2[i] = g2[i]; a.b2[i] = b2[i];
            }
            a.x_out = dxo.as<float>();
            a.proj_w = proj_w; a.proj_b = proj_b; a.proj_cout = PC;
            a.out = PC ? dout.as<float>() : nullptr;
            a.spline = t->spline ? 1 : 0; a.nb = t->nb; a.tail = t->tail; a.inv_sqrt_fc = t->inv_sqrt_fc;
            a.len = dl.as<int>(); a.B = B; a.T = T; a.math = t->math;
            launch_dds_stack(a, C, nullptr);
        } else {
            // Engine::duration_predictor's launches without the stack kernels: x lives in d0 (d1 / d2: Engine::dds's scratch)
            DevBuf d0(n * 4), d1(n * 4), d2(n * 4);
            const long bs = (long)C * T;
            auto conv1x1 = [&](const float* x, float* y, const float* w, const float* bias, int Cout, bool masked) {
                ConvArgs a;
                a.x = x; a.x_bs = bs; a.x_ld = T;
                a.y = y; a.y_bs = (long)Cout * T; a.y_ld = T;
                a.B = B; a.T = T; a.Cin = C; a.Cout = Cout; a.K = 1; a.bias = bias; a.pad = 0; a.w = w; a.math = MATH_F32;
                if (masked) { a.in_len = dl.as<int>(); a.out_len = dl.as<int>(); }
                return a;
            };
            auto run_conv = [&](const ConvArgs& a) {
                if (conv_mfma(a.Cout)) launch_conv1d_mfma(a, nullptr);
                else launch_conv1d_generic(a, nullptr);
            };
            float* X = d0.as<float>();
            if (t->pre_mode == DDS_PRE_AFFINE) {
                launch_convflow_pre(dz.as<float>(), t->zch, pre_w, pre_b, dsrc.as<float>(), B, C, T, X, nullptr);
            } else {
                ConvArgs a = conv1x1(dsrc.as<float>(), X, pre_w, pre_b, C, false);
                if (t->cond) { a.cond = dcond.as<float>(); a.cond_bs = C; }
                run_conv(a);
            }
            int dil = 1;
            for (int i = 0; i < NL; ++i) {
                if (t->impl == 1) {  // x ping-pongs (k_dds_layer reads its neighbours' OLD columns)
                    float* dst = X == d0.as<float>() ? d1.as<float>() : d0.as<float>();
                    launch_dds_layer(X, dst, dw_w[i], dw_b[i], g1[i], b1[i], w1[i], bb[i], g2[i], b2[i], dl.as<int>(), B, C, T, K, dil, nullptr);
                    X = dst;
                } else {
                    launch_dds_dwconv_ln_gelu(X, dw_w[i], dw_b[i], g1[i], b1[i], dl.as<int>(), B, C, T, K, dil, d1.as<float>(), nullptr);
                    run_conv(conv1x1(d1.as<float>(), d2.as<float>(), w1[i], bb[i], C, false));
                    LNArgs ln;
                    ln.x = d2.as<float>(); ln.y = X; ln.add_to = X; ln.gelu = 1;
                    ln.B = B; ln.C = C; ln.T = T; ln.gamma = g2[i]; ln.beta = b2[i];
                    launch_layernorm(ln, nullptr);
                }
                dil *= K;
            }
            HIP_CHECK(hipMemcpyAsync(dxo.p, X, n * 4, hipMemcpyDeviceToDevice, nullptr));
            if (PC) run_conv(conv1x1(X, dout.as<float>(), proj_w, proj_b, PC, true));
            if (t->spline)
                launch_spline_inverse(dz.as<float>(), t->zch, dout.as<float>(), dl.as<int>(), B, T, t->nb, t->tail, t->inv_sqrt_fc, nullptr);
        }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(t->x_out, dxo.p, n * 4, hipMemcpyDeviceToHost));
        if (PC) HIP_CHECK(hipMemcpy(t->out, dout.p, no * 4, hipMemcpyDeviceToHost));
        if (t->z) HIP_CHECK(hipMemcpy(t->z, dz.p, nz * 4, hipMemcpyDeviceToHost));
    });
}

int mi355vits_test_spline_inverse(int device, int B, int T, int nb, int ch_x0, float tail, float inv_sqrt_fc, const float* theta,
                                  const int32_t* len, float* z) {
    return guarded(nullptr, [&] {
        if (!theta || !len || !z) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1 || nb < 2 || nb > 16 || (ch_x0 != 0 && ch_x0 != 1)) throw EngineError(MI355VITS_ERR_INVALID, "bad shape (2 <= nb <= 16)");
        for (int b = 0; b < B; ++b)
            if (len[b] < 0 || len[b] > T) throw EngineError(MI355VITS_ERR_INVALID, "len out of range");
        HIP_CHECK(hipSetDevice(device));
        const size_t nt = (size_t)B * (3 * nb - 1) * T, nz = (size_t)B * 2 * T;
        DevBuf dt(nt * 4), dz(nz * 4), dl((size_t)B * 4);
        HIP_CHECK(hipMemcpy(dt.p, theta, nt * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dz.p, z, nz * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, len, (size_t)B * 4, hipMemcpyHostToDevice));
        launch_spline_inverse(dz.as<float>(), ch_x0, dt.as<float>(), dl.as<int>(), B, T, nb, tail, inv_sqrt_fc, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(z, dz.p, nz * 4, hipMemcpyDeviceToHost));
    });
}

int mi355vits_test_durations(int device, int B, int T, int ch, float ea_m, float ea_logs, const float* z, const int32_t* len,
                             const int32_t* forced, const float* scales, float* logw, int32_t* w_ceil, int32_t* cum, int32_t* ylen) {
    return guarded(nullptr, [&] {
        if (!z || !len || !scales || !logw || !w_ceil || !cum || !ylen) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1 || (ch != 0 && ch != 1)) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        for (int b = 0; b < B; ++b)
            if (len[b] < 0 || len[b] > T) throw EngineError(MI355VITS_ERR_INVALID, "len out of range");
        HIP_CHECK(hipSetDevice(device));
        const size_t nz = (size_t)B * 2 * T, nt = (size_t)B * T;
        DevBuf dz(nz * 4), dl((size_t)B * 4), df(nt * 4), ds((size_t)B * 3 * 4), dlw(nt * 4), dw(nt * 4), dc(nt * 4), dy((size_t)B * 4);
        HIP_CHECK(hipMemcpy(dz.p, z, nz * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, len, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(ds.p, scales, (size_t)B * 3 * 4, hipMemcpyHostToDevice));
        if (forced) HIP_CHECK(hipMemcpy(df.p, forced, nt * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dlw.p, logw, nt * 4, hipMemcpyHostToDevice));  // the prior contents: a missing write shows
        HIP_CHECK(hipMemcpy(dw.p, w_ceil, nt * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dc.p, cum, nt * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, ylen, (size_t)B * 4, hipMemcpyHostToDevice));
        launch_durations(dz.as<float>(), ch, ea_m, ea_logs, dl.as<int>(), forced ? df.as<int>() : nullptr, B, T, ds.as<float>(),
                         dlw.as<float>(), dw.as<int>(), dc.as<int>(), dy.as<int>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(logw, dlw.p, nt * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(w_ceil, dw.p, nt * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(cum, dc.p, nt * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(ylen, dy.p, (size_t)B * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t nt = (size_t)B * T, nb = (size_t)B * 4;
        DevBuf du(nt * 4), dl(nb), dm(nt * 4), dt(nb), duo(nt * 4), dw(nt * 4), dc(nt * 4), dy(nb), dfa(nb), dst(nb);
        HIP_CHECK(hipMemcpy(du.p, u, nt * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, len, nb, hipMemcpyHostToDevice));
        if (min_frames) HIP_CHECK(hipMemcpy(dm.p, min_frames, nt * 4, hipMemcpyHostToDevice));
        if (target) HIP_CHECK(hipMemcpy(dt.p, target, nb, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dw.p, frames, nt * 4, hipMemcpyHostToDevice));  // the prior contents: a missing write shows
        HIP_CHECK(hipMemcpy(dc.p, cum, nt * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, ylen, nb, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dfa.p, factor, nb, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dst.p, status, nb, hipMemcpyHostToDevice));
        DurTimedArgs a;
        a.u_in = du.as<float>();
        a.len = dl.as<int>(); a.B = B; a.T = T;
        a.min_frames = min_frames ? dm.as<int>() : nullptr;
        a.target = target ? dt.as<int>() : nullptr;
        a.u = duo.as<float>();
        a.w_ceil = dw.as<int>(); a.cum = dc.as<int>(); a.ylen = dy.as<int>();
        a.factor = dfa.as<float>(); a.status = dst.as<int>();
        launch_durations_timed(a, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(frames, dw.p, nt * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(cum, dc.p, nt * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(ylen, dy.p, nb, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(factor, dfa.p, nb, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(status, dst.p, nb, hipMemcpyDeviceToHost));
    });
}

int mi355vits_test_speaker_cond(int device, int B, int gin, int n_speakers, int Cout, const float* emb_g, const int64_t* sid,
                                const float* w, const float* bias, float* out, size_t out_floats) {
    return guarded(nullptr, [&] {
        if (!emb_g || !sid || !w || !out) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || gin < 1 || gin > 8192 || n_speakers < 1 || Cout < 1 || out_floats < (size_t)B * Cout) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        for (int b = 0; b < B; ++b)
            if (sid[b] < 0 || sid[b] >= n_speakers) throw EngineError(MI355VITS_ERR_INVALID, "sid out of range");
        HIP_CHECK(hipSetDevice(device));
        DevBuf de((size_t)n_speakers * gin * 4), ds((size_t)B * 8), dw((size_t)Cout * gin * 4), db((size_t)Cout * 4), dout(out_floats * 4);
        HIP_CHECK(hipMemcpy(de.p, emb_g, (size_t)n_speakers * gin * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(ds.p, sid, (size_t)B * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dw.p, w, (size_t)Cout * gin * 4, hipMemcpyHostToDevice));
        if (bias) HIP_CHECK(hipMemcpy(db.p, bias, (size_t)Cout * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dout.p, out, out_floats * 4, hipMemcpyHostToDevice));  // the prior contents: a missing or stray write shows
        launch_speaker_cond(de.as<float>(), ds.as<long long>(), dw.as<float>(), bias ? db.as<float>() : nullptr, B, gin, Cout, dout.as<float>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out, dout.p, out_floats * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t ne = mix ? (size_t)t->n_speakers * gin : 0, nk = mix ? (size_t)B * K : 0, nv = mix ? 0 : (size_t)B * gin;
        DevBuf de(ne * 4), ds(nk * 8), dm(nk * 4), dv(nv * 4), dg(t->g_floats * 4);
        if (mix) {
            HIP_CHECK(hipMemcpy(de.p, t->emb_g, ne * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(ds.p, t->mix_sid, nk * 8, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(dm.p, t->mix_weight, nk * 4, hipMemcpyHostToDevice));
        } else {
            HIP_CHECK(hipMemcpy(dv.p, t->vectors, nv * 4, hipMemcpyHostToDevice));
        }
        HIP_CHECK(hipMemcpy(dg.p, t->g, t->g_floats * 4, hipMemcpyHostToDevice));  // the prior contents: a missing or stray write shows
        std::vector<std::unique_ptr<DevBuf>> dw, db, dout;
        SpeakerMixArgs a;
        a.B = B; a.gin = gin; a.K = K; a.g = dg.as<float>(); a.n_jobs = nj;
        if (mix) { a.emb_g = de.as<float>(); a.sid = ds.as<long long>(); a.weight = dm.as<float>(); } else a.vectors = dv.as<float>();
        for (int q = 0; q < nj; ++q) {
            const size_t nw = (size_t)t->Cout[q] * gin;
            dw.emplace_back(new DevBuf(nw * 4));
            db.emplace_back(new DevBuf((size_t)t->Cout[q] * 4));
            dout.emplace_back(new DevBuf(t->out_floats[q] * 4));
            HIP_CHECK(hipMemcpy(dw[q]->p, t->w[q], nw * 4, hipMemcpyHostToDevice));
            if (t->bias[q]) HIP_CHECK(hipMemcpy(db[q]->p, t->bias[q], (size_t)t->Cout[q] * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(dout[q]->p, t->out[q], t->out_floats[q] * 4, hipMemcpyHostToDevice));
            a.jobs[q].w = dw[q]->as<float>();
            a.jobs[q].bias = t->bias[q] ? db[q]->as<float>() : nullptr;
            a.jobs[q].Cout = t->Cout[q];
            a.jobs[q].out = dout[q]->as<float>();
        }
        launch_speaker_cond_mix(a, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(t->g, dg.p, t->g_floats * 4, hipMemcpyDeviceToHost));
        for (int q = 0; q < nj; ++q) HIP_CHECK(hipMemcpy(t->out[q], dout[q]->p, t->out_floats[q] * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t nbt = (size_t)B * T;
        DevBuf dc(nbt * 4), dl((size_t)B * 4), dg(nbt * 4), dr((size_t)B * 4), da((size_t)B * 4), dx(audio_floats * 4), dp((size_t)B * 4);
        HIP_CHECK(hipMemcpy(dc.p, cum, nbt * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, len, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dg.p, gain, nbt * 4, hipMemcpyHostToDevice));
        if (ramp) HIP_CHECK(hipMemcpy(dr.p, ramp, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(da.p, alen, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dx.p, audio, audio_floats * 4, hipMemcpyHostToDevice));  // everything: a stray write shows
        HIP_CHECK(hipMemset(dp.p, 0, (size_t)B * 4));
        launch_levels(dc.as<int>(), dl.as<int>(), dg.as<float>(), ramp ? dr.as<int>() : nullptr, B, T, hop, dx.as<float>(), (long)audio_bs,
                      da.as<int>(), l_max, dp.as<unsigned>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(audio, dx.p, audio_floats * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(peaks, dp.p, (size_t)B * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t nbt = (size_t)B * T;
        DevBuf dc(nbt * 4), dl((size_t)B * 4), dr(nbt * 4), dq(nbt * 8), dw(nbt * 4), dn((size_t)B * 4);
        HIP_CHECK(hipMemcpy(dc.p, cum, nbt * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, len, (size_t)B * 4, hipMemcpyHostToDevice));
        if (ratio) HIP_CHECK(hipMemcpy(dr.p, ratio, nbt * 4, hipMemcpyHostToDevice));
        launch_pitch_plan(dc.as<int>(), dl.as<int>(), ratio ? dr.as<float>() : nullptr, B, T, hop, dq.as<long long>(), dw.as<int>(), dn.as<int>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(tq, dq.p, nbt * 8, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(wc, dw.p, nbt * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(wlen, dn.p, (size_t)B * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t nbt = (size_t)B * T;
        const std::vector<float>& h = pitch_table();
        std::vector<int> alen(B);
        for (int b = 0; b < B; ++b) {
            const int frames = len[b] > 0 ? cum[(size_t)b * T + len[b] - 1] : 0;
            alen[b] = hop * (frames < 1 ? 1 : frames);
        }
        DevBuf dc(nbt * 4), dl((size_t)B * 4), dr(nbt * 4), dq(nbt * 8), dw(nbt * 4), dn((size_t)B * 4), da((size_t)B * 4),
            dx(x_floats * 4), dy(y_floats * 4), dp((size_t)B * 4), dh(h.size() * 4);
        HIP_CHECK(hipMemcpy(dc.p, cum, nbt * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, len, (size_t)B * 4, hipMemcpyHostToDevice));
        if (ratio) HIP_CHECK(hipMemcpy(dr.p, ratio, nbt * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(da.p, alen.data(), (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dx.p, x, x_floats * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, y, y_floats * 4, hipMemcpyHostToDevice));  // everything: a stray write shows
        HIP_CHECK(hipMemcpy(dh.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dp.p, 0, (size_t)B * 4));
        const float* dratio = ratio ? dr.as<float>() : nullptr;
        launch_pitch_plan(dc.as<int>(), dl.as<int>(), dratio, B, T, hop, dq.as<long long>(), dw.as<int>(), dn.as<int>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(wlen, dn.p, (size_t)B * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            if (wlen[b] < 1 || wlen[b] == 0x7fffffff || wlen[b] > y_ld) throw EngineError(MI355VITS_ERR_INVALID, "row " + std::to_string(b) + ": the warped row of " + std::to_string(wlen[b]) + " samples does not fit y_ld");
        std::vector<int64_t> w64(wlen, wlen + B);
        std::vector<int> tab(pitch_tab_ints(B));
        const long items = pitch_fill_tab(w64.data(), B, tab.data());
        DevBuf dt(tab.size() * 4);
        HIP_CHECK(hipMemcpy(dt.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        launch_pitch(dx.as<float>(), (long)x_bs, da.as<int>(), dc.as<int>(), dl.as<int>(), dratio, dq.as<long long>(), dw.as<int>(), dt.as<int>(),
                     items, dh.as<float>(), B, T, hop, dy.as<float>(), (long)y_bs, y_ld, dp.as<unsigned>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(y, dy.p, y_floats * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(peaks, dp.p, (size_t)B * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t ns = (size_t)B * 2 * I * Tx, nc = (size_t)B * Tx, ni = injected ? (size_t)B * I * injected_frames : 0, nz = (size_t)B * I * Ty;
        DevBuf dst(ns * 4), dc(nc * 4), dy((size_t)B * 4), di(ni * 4), ds((size_t)B * 3 * 4), dz(nz * 4), du((size_t)B * 8);
        HIP_CHECK(hipMemcpy(dst.p, stats, ns * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dc.p, cum, nc * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, ylen, (size_t)B * 4, hipMemcpyHostToDevice));
        if (ni) HIP_CHECK(hipMemcpy(di.p, injected, ni * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(ds.p, scales, (size_t)B * 3 * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dz.p, z, nz * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(du.p, 0, (size_t)B * 8));
        launch_expand_prior(dst.as<float>(), dc.as<int>(), dy.as<int>(), injected ? di.as<float>() : nullptr, injected_frames, B, I, Tx, Ty,
                            ds.as<float>(), 0ull, du.as<unsigned long long>(), dz.as<float>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(z, dz.p, nz * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t ns = (size_t)B * 2 * I * Tx, nc = (size_t)B * Tx, nz = (size_t)B * I * Ty;
        DevBuf dst(ns * 4), dc(nc * 4), dy((size_t)B * 4), ds((size_t)B * 3 * 4), dz(nz * 4), du((size_t)B * 8);
        HIP_CHECK(hipMemcpy(dst.p, stats, ns * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dc.p, cum, nc * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, ylen, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(ds.p, scales, (size_t)B * 3 * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dz.p, z, nz * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(du.p, utt, (size_t)B * 8, hipMemcpyHostToDevice));
        launch_expand_prior(dst.as<float>(), dc.as<int>(), dy.as<int>(), nullptr, 0, B, I, Tx, Ty, ds.as<float>(), (unsigned long long)seed,
                            du.as<unsigned long long>(), dz.as<float>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(z, dz.p, nz * 4, hipMemcpyDeviceToHost));
    });
}

int mi355vits_test_sdp_noise(int device, int B, int T, uint64_t seed, const uint64_t* utt, const float* scales, float* z) {
    return guarded(nullptr, [&] {
        if (!utt || !scales || !z) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        HIP_CHECK(hipSetDevice(device));
        const size_t nz = (size_t)B * 2 * T;
        DevBuf dz(nz * 4), ds((size_t)B * 3 * 4), du((size_t)B * 8);
        HIP_CHECK(hipMemcpy(dz.p, z, nz * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(ds.p, scales, (size_t)B * 3 * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(du.p, utt, (size_t)B * 8, hipMemcpyHostToDevice));
        launch_sdp_noise(dz.as<float>(), nullptr, B, T, ds.as<float>(), (unsigned long long)seed, du.as<unsigned long long>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(z, dz.p, nz * 4, hipMemcpyDeviceToHost));
    });
}

int mi355vits_test_embed(int device, int B, int T, int H, int num_symbols, const int64_t* ids, const int32_t* len, const float* emb,
                         float scale, float* y) {
    return guarded(nullptr, [&] {
        if (!ids || !len || !emb || !y) throw EngineError(MI355VITS_ERR_INVALID, "null argument");
        if (B < 1 || T < 1 || H < 1 || num_symbols < 1) throw EngineError(MI355VITS_ERR_INVALID, "bad shape");
        check_lens(len, B, T, "len out of range");
        HIP_CHECK(hipSetDevice(device));
        const size_t ni = (size_t)B * T, ne = (size_t)num_symbols * H, ny = (size_t)B * H * T;
        DevBuf di(ni * 8), dl((size_t)B * 4), de(ne * 4), dy(ny * 4);
        HIP_CHECK(hipMemcpy(di.p, ids, ni * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, len, (size_t)B * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(de.p, emb, ne * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, y, ny * 4, hipMemcpyHostToDevice));
        launch_embed(di.as<long long>(), dl.as<int>(), de.as<float>(), B, T, H, num_symbols, scale, dy.as<float>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(y, dy.p, ny * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        const size_t nx = (size_t)(NP - 1) * stride + n;
        DevBuf dx(nx * 4), dy(n * 4), dres(n * 4), dadd(n * 4), db((size_t)C * 4), dg((size_t)C * 4), dbe((size_t)C * 4), dpl((size_t)B * 4), dol((size_t)B * 4);
        HIP_CHECK(hipMemcpy(dx.p, t->x, nx * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, t->y, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dg.p, t->gamma, (size_t)C * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dbe.p, t->beta, (size_t)C * 4, hipMemcpyHostToDevice));
        LNArgs a;
        a.x = dx.as<float>(); a.gamma = dg.as<float>(); a.beta = dbe.as<float>();
        a.B = B; a.C = C; a.T = T; a.gelu = t->gelu ? 1 : 0; a.eps = t->eps;
        a.nparts = NP; a.part_stride = (long)stride;
        if (t->res) { HIP_CHECK(hipMemcpy(dres.p, t->res, n * 4, hipMemcpyHostToDevice)); a.res = dres.as<float>(); }
        if (t->add_to) { HIP_CHECK(hipMemcpy(dadd.p, t->add_to, n * 4, hipMemcpyHostToDevice)); a.add_to = dadd.as<float>(); }
        if (t->bias) { HIP_CHECK(hipMemcpy(db.p, t->bias, (size_t)C * 4, hipMemcpyHostToDevice)); a.bias = db.as<float>(); }
        if (t->premask_len) { HIP_CHECK(hipMemcpy(dpl.p, t->premask_len, (size_t)B * 4, hipMemcpyHostToDevice)); a.premask_len = dpl.as<int>(); }
        if (t->out_len) { HIP_CHECK(hipMemcpy(dol.p, t->out_len, (size_t)B * 4, hipMemcpyHostToDevice)); a.out_len = dol.as<int>(); }
        a.y = t->alias == 1 ? dx.as<float>() : t->alias == 2 ? dres.as<float>() : t->alias == 3 ? dadd.as<float>() : dy.as<float>();
        try {
            launch_layernorm(a, nullptr);
        } catch (const EngineError&) {
            throw;
        } catch (const std::runtime_error& e) {  // the launcher's own refusal (thrown before any launch); a HIP error stays a device error
            if (std::string(e.what()).rfind("layernorm:", 0) == 0) throw EngineError(MI355VITS_ERR_INVALID, e.what());
            throw;
        }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(t->y, a.y, n * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        std::vector<std::unique_ptr<DevBuf>> keep;
        auto upload = [&](const void* p, size_t bytes) -> const float* {
            keep.emplace_back(new DevBuf(bytes));
            HIP_CHECK(hipMemcpy(keep.back()->p, p, bytes, hipMemcpyHostToDevice));
            return keep.back()->as<float>();
        };
        // a conv's weights [Cout, Cin, K] as Engine::add_conv_data stages them for the mode (ConvW::packed / packed_b3s)
        auto conv_w = [&](const float* w, int Cout, int Cin) -> const float* {
            if (t->math == MATH_F32) {
                std::vector<float> p(mfma_packed_floats(Cout, Cin, K), 0.0f);
                pack_conv_weights_mfma_mode(w, Cout, Cin, K, EPI_STD, p.data());
                return upload(p.data(), p.size() * 4);
            }
            std::vector<uint32_t> p(bf16x3_packed_words_mode(Cout, Cin, K, EPI_STD), 0u);
            pack_conv_weights_bf16x3_mode(w, Cout, Cin, K, EPI_STD, 1, p.data());
            return upload(p.data(), p.size() * 4);
        };
        DpDetArgs a;
        a.x = upload(t->x, (size_t)B * H * T * 4);
        if (t->cond) { a.cond = upload(t->cond, (size_t)B * H * 4); a.cond_bs = H; }
        a.w1 = conv_w(t->w1, F, H); a.b1 = upload(t->b1, (size_t)F * 4); a.g1 = upload(t->g1, (size_t)F * 4); a.be1 = upload(t->be1, (size_t)F * 4);
        a.w2 = conv_w(t->w2, F, F); a.b2 = upload(t->b2, (size_t)F * 4); a.g2 = upload(t->g2, (size_t)F * 4); a.be2 = upload(t->be2, (size_t)F * 4);
        a.pw = upload(t->proj_w, (size_t)F * 4);
        a.pb = upload(t->proj_b, 4);
        a.len = reinterpret_cast<const int*>(upload(t->len, (size_t)B * 4));
        DevBuf dout((size_t)B * T * 4);
        HIP_CHECK(hipMemcpy(dout.p, t->logw, (size_t)B * T * 4, hipMemcpyHostToDevice));
        a.out = dout.as<float>(); a.out_bs = T;
        a.B = B; a.T = T; a.H = H; a.F = F; a.K = K; a.math = t->math;
        launch_dp_det(a, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(t->logw, dout.p, (size_t)B * T * 4, hipMemcpyDeviceToHost));
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
        for (int b = 0; b < B; ++b)
            if (t->len[b] < 0 || t->len[b] > T) throw EngineError(MI355VITS_ERR_INVALID, "len out of range");
        if (t->impl < 0 || t->impl > 2) throw EngineError(MI355VITS_ERR_INVALID, "impl must be 0, 1 or 2");
        if (t->impl == 0 ? (t->math != MATH_F32 && t->math != MATH_BF16X3) : t->math != MATH_BF16X3)
            throw EngineError(MI355VITS_ERR_INVALID, "math mode: MATH_F32 or MATH_BF16X3 for impl 0, MATH_BF16X3 for impl 1 and 2");
        MrfPlan plan;
        if (!mrf_test_plan(t->impl, C, nrb, t->k, t->d1, t->d2, &plan)) throw EngineError(MI355VITS_ERR_INVALID, "stage not supported by the chosen kernel");
        if (t->impl == 2 && (t->seg < plan.width || t->seg % plan.width != 0)) throw EngineError(MI355VITS_ERR_INVALID, "seg must be a positive multiple of the sweep's step");
        HIP_CHECK(hipSetDevice(device));
        const size_t n = (size_t)B * C * T;
        DevBuf dx(n * 4), dy(n * 4), dl((size_t)B * 4);
        HIP_CHECK(hipMemcpy(dx.p, t->x, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dy.p, t->y, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dl.p, t->len, (size_t)B * 4, hipMemcpyHostToDevice));
        std::vector<int> len_host(t->len, t->len + B);
        std::vector<std::unique_ptr<DevBuf>> keep;
        auto upload = [&](const void* p, size_t bytes) {
            keep.emplace_back(new DevBuf(bytes));
            HIP_CHECK(hipMemcpy(keep.back()->p, p, bytes, hipMemcpyHostToDevice));
            return keep.back()->as<float>();
        };
        MrfArgs m;
        m.x = dx.as<float>(); m.x_bs = (long)C * T; m.x_ld = T;
        m.y = dy.as<float>(); m.y_bs = (long)C * T; m.y_ld = T;
        m.len = dl.as<int>(); m.len_host = len_host.data(); m.B = B; m.C = C; m.T = T;
        m.nrb = nrb; m.math = t->math; m.out_scale = t->out_scale;
        for (int j = 0; j < nrb; ++j) {
            const int k = t->k[j];
            m.k[j] = k; m.d1[j] = t->d1[j]; m.d2[j] = t->d2[j];
            for (int q = 0; q < 2; ++q) {
                const float* w = t->w[j][q];
                if (t->impl != 0) {  // Engine::add_conv_data's packed_p
                    std::vector<uint32_t> pp(p16_packed_words(C, C, k));
                    pack_conv_weights_p16(w, C, C, k, pp.data());
                    m.w[j][q] = upload(pp.data(), pp.size() * 4);
                } else if (t->math == MATH_BF16X3) {  // packed_b3
                    std::vector<uint32_t> b3(bf16x3_packed_words(C, C, k));
                    pack_conv_weights_bf16x3(w, C, C, k, b3.data());
                    m.w[j][q] = upload(b3.data(), b3.size() * 4);
                } else {  // packed4
                    std::vector<float> pk(mfma_packed_floats(C, C, k), 0.0f), p4(pk.size());
                    pack_conv_weights_mfma_mode(w, C, C, k, EPI_STD, pk.data());
                    regroup_packed_x4(pk.data(), pk.size(), p4.data());
                    m.w[j][q] = upload(p4.data(), p4.size() * 4);
                }
                m.bias[j][q] = upload(t->bias[j][q], (size_t)C * 4);
            }
        }
        if (t->impl == 0) launch_mrf_fused(m, nullptr);
        else if (t->impl == 1) launch_mrf_p(m, nullptr);
        else { m.seg = t->seg; launch_mrf_s(m, nullptr); }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(t->y, dy.p, n * 4, hipMemcpyDeviceToHost));
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
        HIP_CHECK(hipSetDevice(device));
        if (!conv1d_mfma_supported(Cin, Cout, K, dilation) || reps < 1 || !ms_per_launch) throw EngineError(MI355VITS_ERR_INVALID, "bad arguments");
        const int H = Cout / 2;
        const size_t nx = (size_t)B * Cin * T, ny = (size_t)B * Cout * T, nw = (size_t)Cout * Cin * K;
        std::vector<float> hx(nx), hw(nw), pk(mfma_packed_floats(Cout, Cin, K));
        unsigned st = 12345u;
        auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xFFFF) / 32768.0f - 1.0f; };
        for (auto& v : hx) v = rnd();
        for (auto& v : hw) v = rnd() * 0.05f;
        pack_conv_weights_mfma_mode(hw.data(), Cout, Cin, K, epi == 1 ? EPI_GATE : EPI_STD, pk.data());
        DevBuf dx(nx * 4), dy(ny * 4), dy2(ny * 4), dres(ny * 4), dp(pk.size() * 4), db(Cout * 4);
        HIP_CHECK(hipMemcpy(dx.p, hx.data(), nx * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dp.p, pk.data(), pk.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dy.p, 0, ny * 4));
        HIP_CHECK(hipMemset(dy2.p, 0, ny * 4));
        HIP_CHECK(hipMemset(dres.p, 0, ny * 4));
        HIP_CHECK(hipMemset(db.p, 0, Cout * 4));
        ConvArgs a;
        a.x = dx.as<float>(); a.x_bs = (long)Cin * T; a.x_ld = T;
        a.w = dp.as<float>(); a.bias = db.as<float>();
        a.B = B; a.Cin = Cin; a.Cout = Cout; a.T = T; a.K = K; a.dil = dilation; a.pad = (K * dilation - dilation) / 2;
        if (epi == 1) {
            a.epi = EPI_GATE; a.H = H;
            a.y = dy.as<float>(); a.y_bs = (long)H * T; a.y_ld = T;
        } else if (epi == 2) {
            a.epi = EPI_RESSKIP; a.H = Cout / 2;
            a.y = dy.as<float>(); a.y_bs = (long)a.H * T; a.y_ld = T;
            a.y2 = dy2.as<float>(); a.y2_bs = (long)a.H * T; a.y2_ld = T;
        } else {
            a.y = dy.as<float>(); a.y_bs = (long)Cout * T; a.y_ld = T;
            a.res = dres.as<float>(); a.res_bs = a.y_bs; a.res_ld = T;
            a.in_slope = 0.1f;
        }
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        for (int i = 0; i < 3; ++i) launch_conv1d_mfma(a, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < reps; ++i) launch_conv1d_mfma(a, nullptr);
        HIP_CHECK(hipEventRecord(e1, nullptr));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        *ms_per_launch = ms / reps;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    });
}

int mi355vits_probe_device(int device, double out[8]) {
    return guarded(nullptr, [&] {
        if (!out) throw EngineError(MI355VITS_ERR_INVALID, "bad arguments");
        HIP_CHECK(hipSetDevice(device));
        const int cus = current_device_cu_count();
        struct Ev {  // RAII: a HIP error below must not leak the events
            hipEvent_t e = nullptr;
            Ev() { HIP_CHECK(hipEventCreate(&e)); }
            ~Ev() { if (e) (void)hipEventDestroy(e); }
        } ev0, ev1;
        hipEvent_t e0 = ev0.e, e1 = ev1.e;
        auto timed = [&](auto&& launch, int warm, int reps) {
            for (int i = 0; i < warm; ++i) launch();
            HIP_CHECK(hipEventRecord(e0, nullptr));
            for (int i = 0; i < reps; ++i) launch();
            HIP_CHECK(hipEventRecord(e1, nullptr));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            return (double)ms / reps;
        };
        // one zero-filled GiB serves everything: [0, 2.6 MB) the L2 table, [0, 24 MB) the big table, the halves as copy source / destination
        const size_t gib = (size_t)1 << 30;
        DevBuf mem(gib), sink((size_t)cus * 4 + 16);
        HIP_CHECK(hipMemset(mem.p, 0, gib));
        const int n16 = 256 * 8 * 80;  // 163,840 x 16 B = 2.62 MB
        const int reps_in = 8;
        const double ms_stream = timed([&] { launch_probe_l2_stream(mem.p, n16, reps_in, sink.as<unsigned>(), cus, nullptr); }, 1, 3);
        out[0] = (double)cus * reps_in * n16 * 16.0 / (ms_stream * 1e-3) / 1e9;
        const int steps = 2000;
        auto chase = [&](unsigned nlines, int warm) {
            const double ms = timed([&] { launch_probe_l2_latency(mem.as<unsigned>(), steps, nlines, sink.as<unsigned>(), cus, nullptr); }, warm, 2);
            return ms * 1e6 / steps;
        };
        out[1] = chase(1u << 15, 2);   // 2 MB: after two passes every XCD's L2 holds what its waves touch
        out[6] = chase(1u << 19, 2);   // 32 MB: past an L2, inside the memory-side cache
        out[7] = chase(1u << 24, 1);   // 1 GiB: HBM (and the TLB's reach)
        const long ncopy16 = (256L << 20) / 16;
        char* base = static_cast<char*>(mem.p);
        const double ms_copy = timed([&] { launch_probe_copy(base, base + gib / 2, ncopy16, cus * 16, nullptr); }, 1, 3);
        out[2] = 2.0 * ncopy16 * 16.0 / (ms_copy * 1e-3) / 1e9;
        out[3] = (double)cus;
        const long slice16 = ncopy16 / cus;
        const double ms_mixed = timed([&] { launch_probe_l2_mixed(mem.p, n16, reps_in, base + gib / 4, base + gib / 2, slice16, sink.as<unsigned>(), cus, nullptr); }, 1, 3);
        out[4] = (double)cus * reps_in * n16 * 16.0 / (ms_mixed * 1e-3) / 1e9;
        const int big16 = n16 * 9;
        const double ms_big = timed([&] { launch_probe_l2_stream(mem.p, big16, 1, sink.as<unsigned>(), cus, nullptr); }, 1, 3);
        out[5] = (double)cus * big16 * 16.0 / (ms_big * 1e-3) / 1e9;
    });
}

int mi355vits_test_mfma_layout(int device, float* err) {
    return guarded(nullptr, [&] {
        HIP_CHECK(hipSetDevice(device));
        DevBuf d((1024 + 256 + 256) * 4);
        launch_mfma_selftest(d.as<float>(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        std::vector<float> h(1536);
        HIP_CHECK(hipMemcpy(h.data(), d.p, 1536 * 4, hipMemcpyDeviceToHost));
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
