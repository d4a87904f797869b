/* mi355vits.h — C ABI of libmi355vits.so, the MI355X-native VITS inference engine that stands
 * in for the one third-party call on the Mimic 3 hot path.
 *
 * Reference interface each entry point replaces (paths relative to the mimic3 repository):
 *
 *   mi355vits_create*          onnxruntime.InferenceSession(str(generator_path), sess_options=...,
 *                              providers=...)                      mimic3_tts/voice.py:403-405
 *   mi355vits_run              self.onnx_model.run(None, inputs)   mimic3_tts/voice.py:230
 *                              (feed dict built at voice.py:180-218: "input" int64 [B,Tx],
 *                              "input_lengths" int64 [B], "scales" f32[3] = noise_scale,
 *                              length_scale, noise_w; "sid" int64 [B] iff multi-speaker)
 *     + MI355VITS_WANT_PCM16   audio_float_to_int16(audio)         mimic3_tts/utils.py:237-244
 *                              (called right after run, inside the timed region, voice.py:231)
 *     + run_args.pcm_volume    audioop.mul(audio_bytes, 2, volume / 100)   mimic3_tts/tts.py:542-543
 *   mi355vits_destroy          the session's finaliser (voice.py:71-72 keeps sessions in a
 *                              process-wide cache, so they live until exit)
 *   mi355vits_get_config       TrainingConfig.model / .audio       mimic3_tts/config.py:112-143,30-60
 *
 * Plain pointers and sizes only; no torch / numpy types.  All calls return 0 on success or a
 * negative MI355VITS_ERR_* code; mi355vits_last_error() gives the message.  Never aborts the
 * process, never returns partial audio (the reference raises Python exceptions at this level,
 * SURVEY.md §8b).  `run` is serialised per handle (internal mutex), so a handle may be shared by
 * the server's worker threads like the reference's shared sessions (voice.py:277-292).
 */
#ifndef MI355VITS_H
#define MI355VITS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355VITS_MAX_STAGES 8

/* Hyper-parameters of the voice (mirror of ModelConfig + the constants upstream VITS hard-codes).
 * Stored verbatim in the .m355 weight container header. */
typedef struct mi355vits_config {
    int32_t num_symbols;
    int32_t n_speakers;
    int32_t inter_channels;
    int32_t hidden_channels;
    int32_t filter_channels;
    int32_t n_heads;
    int32_t n_layers;
    int32_t kernel_size;
    int32_t resblock; /* 1 or 2 */
    int32_t n_resblock_kernels;
    int32_t resblock_kernel_sizes[MI355VITS_MAX_STAGES];
    int32_t resblock_n_dilations[MI355VITS_MAX_STAGES];
    int32_t resblock_dilations[MI355VITS_MAX_STAGES * MI355VITS_MAX_STAGES];
    int32_t n_upsamples;
    int32_t upsample_rates[MI355VITS_MAX_STAGES];
    int32_t upsample_kernel_sizes[MI355VITS_MAX_STAGES];
    int32_t upsample_initial_channel;
    int32_t gin_channels;
    int32_t window_size;
    int32_t flow_n_flows;
    int32_t flow_wn_layers;
    int32_t flow_wn_kernel;
    int32_t flow_wn_dilation_rate;
    /* Duration predictor.  The stochastic one (use_sdp = true): dp_n_flows >= 2 ConvFlows, dp_dds_layers DDS layers,
     * dp_num_bins spline bins.  dp_n_flows == 0 marks the deterministic one (use_sdp = false: conv_1 / norm_1 / conv_2 /
     * norm_2 / proj); then dp_dds_layers and dp_num_bins are 0, its kernel size is dp_kernel_size and its filter width F
     * is the length of the container's dp.conv_1.bias.  A library older than this rule rejects such a container as an
     * invalid voice config. */
    int32_t dp_kernel_size;
    int32_t dp_dds_layers;
    int32_t dp_n_flows;
    int32_t dp_num_bins;
    float dp_tail_bound;
    int32_t sample_rate;
    int32_t hop_length;
} mi355vits_config;

typedef struct mi355vits_engine* mi355vits_handle;

enum {
    MI355VITS_OK = 0,
    MI355VITS_ERR_INVALID = -1,  /* bad argument / shape / id out of range */
    MI355VITS_ERR_IO = -2,       /* weight file unreadable */
    MI355VITS_ERR_FORMAT = -3,   /* not an .m355 container, or tensors missing / mis-shaped */
    MI355VITS_ERR_DEVICE = -4,   /* HIP runtime error */
    MI355VITS_ERR_NOMEM = -5,
    MI355VITS_ERR_INTERNAL = -6
};

/* run flags */
#define MI355VITS_WANT_FLOAT 1u   /* float32 waveform [B, l_max]: what onnx_model.run returns */
#define MI355VITS_WANT_PCM16 2u   /* int16 [B, l_max]: audio_float_to_int16, per utterance */
#define MI355VITS_DEVICE_ONLY 4u  /* leave audio in HBM, return lengths only (see mi355vits_fetch) */
#define MI355VITS_DEBUG_TAPS 8u   /* keep named intermediates for mi355vits_get_tap (tests) */

typedef struct mi355vits_run_args {
    int32_t batch;             /* B >= 1 */
    int32_t tx_max;            /* padded phoneme length Tx >= 1 */
    const int64_t* ids;        /* [B, tx_max]  "input" */
    const int64_t* lengths;    /* [B]          "input_lengths", 0 <= len <= tx_max */
    const float* scales;       /* [3]          "scales" = noise_scale, length_scale, noise_w */
    const int64_t* sid;        /* [B] or NULL  "sid" (required iff multi-speaker) */
    uint64_t seed;             /* Philox key for the two Gaussian draws */
    uint64_t utterance_base;   /* global index of row 0: noise does not depend on batch split */
    const float* noise_w;      /* optional injected N(0,1) [B, 2, tx_max] (parity tests) */
    const float* noise_z;      /* optional injected N(0,1) [B, inter_channels, noise_z_frames] */
    int32_t noise_z_frames;
    const int32_t* forced_durations; /* optional [B, tx_max]: overrides ceil(exp(logw)*length_scale) */
    uint32_t flags;
    double pcm_volume;         /* with WANT_PCM16: audioop.mul(pcm, 2, pcm_volume) fused into the int16 kernel —
                                * what Mimic3TextToSpeechSystem._speak_sentence_phonemes does on the host with
                                * settings.volume / 100 (mimic3_tts/tts.py:542-543).  0 or 1 = leave as is. */
} mi355vits_run_args;

/* Per-row synthesis settings of one batched call (mi355vits_run_rows).  Each pointer may be NULL: then every row takes the
 * run_args value (row b keyed run_args.utterance_base + b).  The reference passes these per sentence: mimic3_http's
 * noiseScale / lengthScale / noiseW (mimic3_http/app.py:172-182), SSML <prosody rate> dividing length_scale
 * (mimic3_tts/voice.py:168-170) and <prosody volume> setting settings.volume (mimic3_tts/tts.py:542-543). */
typedef struct mi355vits_row_args {
    const float* scales;        /* [B,3] noise_scale, length_scale, noise_w per row; NULL = args->scales for every row */
    const double* pcm_volume;   /* [B] with WANT_PCM16, audioop.mul factor per row (0 or 1 = as is); NULL = args->pcm_volume */
    const uint64_t* utterance;  /* [B] Philox utterance index per row; NULL = args->utterance_base + b */
} mi355vits_row_args;

typedef struct mi355vits_result {
    int32_t batch;
    int64_t l_max;     /* samples per row = hop * max_b frames_b */
    int64_t ty_max;    /* latent frames of the longest row */
    float* audio;      /* [B, l_max] or NULL; row b valid up to lengths[b] (rest is padding) */
    int16_t* pcm;      /* [B, l_max] or NULL */
    int64_t* lengths;  /* [B] valid samples per row */
    float* peaks;      /* [B] max |audio| over each row's valid samples */
    void* owner_;      /* private */
} mi355vits_result;

const char* mi355vits_version(void);
/* Number of HIP devices this process can use (0 when there is none): sizes the in-process device round-robin of a
 * session serving mimic3_http's worker threads (mimic3_http/__main__.py:53-61 starts them in ONE process). */
int mi355vits_device_count(void);

/* Load a voice from an .m355 container (mimic3_amd/weights.py) onto HIP device `device`. */
int mi355vits_create(const char* weights_path, int device, mi355vits_handle* out);
int mi355vits_create_from_buffer(const void* blob, size_t blob_bytes, int device, mi355vits_handle* out);
/* Another execution lane for the voice of `src`, on the same device: own HIP stream and workspace, SHARED weight
 * replica (the weights are freed with the last lane).  The reference shares one session between the server's worker
 * threads (voice.py:277-292, mimic3_http/__main__.py:53-61); lanes are how those concurrent `run` calls overlap. */
int mi355vits_clone(mi355vits_handle src, mi355vits_handle* out);
void mi355vits_destroy(mi355vits_handle h);
/* Which matrix-core path the dense Conv1d stacks of the flow and the decoder take on this handle
 * (default: environment MI355VITS_MATH = "f32" | "bf16x3" | "bf16w" | "f16x2", read when the handle is created, else BF16X3):
 *   MI355VITS_MATH_F32     v_mfma_f32_32x32x2_f32 — f32 operands, bit-exact f32 FMA chains;
 *   MI355VITS_MATH_BF16X3  the f32 operands split EXACTLY into three bf16 terms each (x = h + m + l) and the six leading
 *                          partial products on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16 / _16x16x32_bf16) with f32 accumulation: every retained product is
 *                          exact, the three dropped ones are below 2^-24 of the product — the f32 rounding level.  Same
 *                          parity tolerances; measured against fp64 it is slightly MORE accurate than the f32 MFMA kernels
 *                          (tests/test_gpu_parity.py::test_split_bf16_staged_conv_kernel_vs_fp64), at 6/16 of their
 *                          matrix-core time (bf16 MFMA = 16 x the f32 MFMA rate on MI355X).  f32 in, f32 out, f32
 *                          accumulate: nothing is stored or rounded in bf16 except the exact split terms.
 * Results of the two differ at f32 rounding level (like two f32 BLAS builds); each is deterministic, and within a mode a
 * batched call is bitwise equal to separate calls.  The text side (encoder convs, duration-predictor stacks) follows the
 * mode as well (k_enc_b3 / k_enc_o_ln / k_dds_stack_b3 in the split modes, the f32-MFMA kernels in MATH_F32), with ONE
 * exception: it never runs with rounded weights — in BF16W it takes the exact BF16X3 path, so the durations
 * ceil(exp(logw) * length_scale), hence every utterance length, are bitwise those of the default mode (Engine::tmath;
 * tests/test_gpu_parity.py::test_bf16_weights_mode_natural_durations_200_sentences).  Attention itself is an f32-MFMA chain. */
#define MI355VITS_MATH_F32 0
#define MI355VITS_MATH_BF16X3 1
/* "bf16 weights" (BASELINE.json configs[4]): BF16X3 with the weights' leading bf16 term only — the weights are rounded to
 * bf16, the activations stay exact f32 (three terms), f32 accumulate: three MFMA products per multiply-add.  A REDUCED
 * precision variant: separate tolerance (rel. RMS <= 2e-2 vs the f32 oracle), never the default, reported separately.
 * Applies to the frame-rate convs (flow, decoder) only; the text side stays exact (see above): same lengths as the default. */
#define MI355VITS_MATH_BF16W 2
/* experimental, opt-in: every kernel of the three-term bf16 split (fused MRF stages, fused WaveNet layers, staged convs,
 * polyphase upsamplers) with both operands split into TWO fp16 terms (11 + 11 significant bits, three products per multiply-add
 * on v_mfma_f32_32x32x16_f16); every other kernel (text encoder, duration predictor) as in BF16X3.  A FIXED-SCALE mode:
 * weights are packed x 2^13 (a stage holding a weight |w| >= 7.99 silently runs as BF16X3 instead), activations are written to
 * the LDS tiles x 2^4 with a saturating round-toward-zero conversion — |x| > 4094 CLIPS (no runtime detection), and below
 * |x| = 2^-7 the second term goes subnormal (absolute instead of relative precision).  Measured on the MI355X
 * (tests/test_gpu_serving.py::test_fused_mrf_stages_on_scaled_activations_vs_fp64): at the activations' natural scale the stage
 * error against fp64 is 1.2e-6 (like the other modes); with the decoder's activations scaled by 2^+-40 the result is finite but
 * meaningless (rel. error ~1).  A 22-bit-operand mode between BF16W and the f32-grade default, with its own tests; never the
 * default.  (The 64- / 32-channel MRF stages run the round-2 kernel k_mrf_fused in this mode, not k_mrf_p.) */
#define MI355VITS_MATH_F16X2 3
int mi355vits_set_math(mi355vits_handle h, int mode);
int mi355vits_get_math(mi355vits_handle h);
int mi355vits_get_config(mi355vits_handle h, mi355vits_config* out);

/* ---- Output sample rate.  0 (the default) or the voice's own rate = native: nothing below applies and nothing is launched
 * or laid out for it.  With another rate set, every result of a run is the synthesized waveform band-limited and resampled to
 * that rate as f32 on the GPU (k_resample), and everything behind the waveform works on the resampled rows:
 *   y[k] = sum_j h[k M - j L + half] x[j],  x zero outside the row's samples,  lengths[b] = ceil(n_b L / M),
 *   L / M = hz / config.sample_rate reduced, h = L x the Kaiser (beta 5) windowed sinc with cut-off 1 / max(L, M) of Nyquist,
 *   half = 10 max(L, M) taps each side, unit DC gain — the filter and the output of scipy.signal.resample_poly(x, L, M);
 *   f32 products and sums in one fixed order per sample, so a row of a batch is bitwise the row alone.
 *  - mi355vits_run / _run_rows: audio, pcm, lengths, peaks (max |y| over the resampled row: what audio_float_to_int16
 *    normalises by) and l_max (= max lengths, the row stride) are at the output rate; ty_max stays in frames.
 *  - mi355vits_run_packed / _fetch_packed: lead_samples, tail_samples, offsets, total_samples count output-rate samples, the RIFF
 *    header carries the output rate, and the size limits are checked on the resampled sizes before anything is sized or launched.
 *  - The setting is read when a run starts; mi355vits_fetch / _fetch_packed / _device_result serve the last run at the rate it
 *    ran at.  MI355VITS_DEBUG_TAPS and mi355vits_get_config().sample_rate stay native.  mi355vits_clone inherits the setting.
 *  - Supported: hz >= 1 with both terms of the reduced ratio <= 640 (from 22,050 Hz: 8000, 11025, 16000, 24000, 32000, 44100,
 *    48000, 88200, 96000 ...).  Anything else returns MI355VITS_ERR_INVALID with a message naming the rate and the reduced ratio
 *    and leaves the setting as it was.  A row whose resampled length does not fit int32 fails its run the same way.
 *  - No additional stream synchronisation or host round trip per call: the resampled lengths follow from the frame counts. */
int mi355vits_set_output_rate(mi355vits_handle h, int32_t hz);
int32_t mi355vits_get_output_rate(mi355vits_handle h); /* the effective rate: the voice's own when unset */

/* One synthesis call.  `out` is filled with callee-allocated (pinned) host buffers; release
 * them with mi355vits_free_result.  With MI355VITS_DEVICE_ONLY the audio stays in the engine's
 * workspace until the next run; mi355vits_fetch copies it out afterwards. */
int mi355vits_run(mi355vits_handle h, const mi355vits_run_args* args, mi355vits_result* out);
/* mi355vits_run with per-row settings: one call for a batch whose rows differ in scales, PCM volume or noise key
 * (mi355vits_run(h, a, o) is mi355vits_run_rows(h, a, NULL, o)).  args->scales may be NULL when rows->scales is given.
 * Every row is validated as mi355vits_run validates its scales; a bad row fails the call with MI355VITS_ERR_INVALID and a
 * message that names it ("row 3: length_scale must be > 0").
 * Contract: for any row b the result (lengths, audio, pcm, peaks) is bitwise what mi355vits_run gives for that row alone with
 * scales = rows->scales[b], pcm_volume = rows->pcm_volume[b] and utterance_base = rows->utterance[b] — in every math mode, as
 * long as the padded phoneme length tx_max stays in the row's own encoder length class (<= 128 / 256 / 512 / cap / beyond, where
 * cap = 4096 - head_dim - (2 window + 1), 3,991 for the released voices): the text encoder picks its kernels by tx_max.  Rows with equal settings and keys therefore give equal audio whichever batch,
 * position or call they ride in. */
int mi355vits_run_rows(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows,
                       mi355vits_result* out);
int mi355vits_fetch(mi355vits_handle h, uint32_t want_flags, mi355vits_result* out);
void mi355vits_free_result(mi355vits_result* r);

/* ---- Packed results: a batch's finished audio as ONE contiguous PCM / WAV stream.
 * What the reference does to the int16 audio of a request's sentences on the host — silence between them
 * (Mimic3TextToSpeechSystem.add_break, mimic3_tts/tts.py:452-465: int(ms / 1000 * sample_rate) zero samples) and WAV framing
 * (opentts_abc/__init__.py:117-127) — done by one kernel (k_pack, csrc/kernels_pack.cpp) and brought to the host by one copy of exactly
 * n_bytes: only the valid samples of each row, rows in the order the caller names, no padding to the longest row. */
typedef struct mi355vits_pack_args {
    int32_t n;                   /* entries of the stream, 1 <= n <= batch */
    const int32_t* order;        /* [n] batch row of entry i; NULL = 0 .. n-1.  A row appears at most once. */
    const int64_t* lead_samples; /* [n] zero samples in front of entry i (add_break); NULL = none */
    int64_t tail_samples;        /* zero samples after the last entry */
    int32_t wav_header;          /* != 0: 44-byte RIFF/WAVE header (PCM, mono, 16 bit, the voice's sample rate) in front */
} mi355vits_pack_args;

typedef struct mi355vits_packed_result {
    int32_t n;
    int64_t total_samples;   /* silences included, header excluded */
    uint8_t* bytes;          /* header (if asked) + 2 * total_samples bytes, little-endian int16; pinned, callee-owned */
    size_t n_bytes;
    int16_t* pcm;            /* = bytes + (wav_header ? 44 : 0) */
    int64_t* offsets;        /* [n] first audio sample of entry i in pcm (after its lead silence) */
    int64_t* lengths;        /* [n] valid samples of entry i */
    float* peaks;            /* [n] max |audio| over entry i's valid samples */
    void* owner_;            /* private */
} mi355vits_packed_result;

/* One synthesis call whose result is the packed stream (pack == NULL: every row, in order, no silence, no header).
 * Contract:
 *  - Entry i's samples pcm[offsets[i] .. offsets[i] + lengths[i]) are BITWISE row order[i]'s valid samples of
 *    mi355vits_run_rows(... MI355VITS_WANT_PCM16 ...) for the same arguments, per-row volumes included, in every math mode:
 *    the same audio_float_to_int16 + audioop.mul arithmetic as the padded int16 result, operation for operation.  lengths /
 *    peaks are that call's values for those rows.  Every other sample of the stream is zero, and is written by the kernel.
 *  - With wav_header, bytes[0, n_bytes) is the file the stdlib `wave` module writes around the same chunks (44-byte header,
 *    PCM, mono, 16 bit, the voice's sample rate), byte for byte.
 *  - MI355VITS_WANT_* and MI355VITS_DEVICE_ONLY in args->flags are ignored: the call produces the packed stream and nothing
 *    else (neither the padded int16 pass nor a padded copy to the host runs); MI355VITS_DEBUG_TAPS works as before.
 *    Afterwards mi355vits_fetch / mi355vits_device_result serve the padded forms from the float audio, as after a
 *    MI355VITS_DEVICE_ONLY run.
 *  - Errors are found before any result is sized or any packing is launched and return MI355VITS_ERR_INVALID with a message
 *    that names the entry or the limit ("pack entry 3: row 9 out of range", "pack entry 2: row 2 appears twice",
 *    "pack entry 1: negative silence"): n outside 1 .. batch, a bad order, negative counts, total_samples > 2^31 - 1, and with
 *    a header a data size that does not fit RIFF's 32-bit fields.  Never partial audio.
 *  - No extra host round trip: the call synchronises its stream twice, like mi355vits_run (frame counts, result); the offsets
 *    are made on the host from the frame counts and uploaded with the per-stage length table. */
int mi355vits_run_packed(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows /* may be NULL */,
                         const mi355vits_pack_args* pack /* may be NULL */, mi355vits_packed_result* out);
/* Pack the LAST completed run of the handle again (whatever flags it had, packed or not), with that run's per-row volumes and
 * another order / silences / header; no synthesis work is repeated. */
int mi355vits_fetch_packed(mi355vits_handle h, const mi355vits_pack_args* pack, mi355vits_packed_result* out);
void mi355vits_free_packed(mi355vits_packed_result* r);

/* ---- Sample encoding of the packed stream.  MI355VITS_ENC_S16LE (the default) = the stream described above and nothing below
 * applies: the 44-byte header is the PCM one, every byte is what it was before this setting existed.
 * With another encoding the same kernel (k_pack: one template over the encodings) writes the format the caller ships, so neither a
 * second pass over the audio on the host (audioop.lin2ulaw) nor bytes nobody wants cross the bus:
 *   MI355VITS_ENC_ULAW / _ALAW  G.711, 1 byte per sample (telephony at 8000 Hz: see mi355vits_set_output_rate).  Entry i's byte k
 *                     is the G.711 code of int16 sample k of the S16LE stream for the same arguments — the value after
 *                     audio_float_to_int16 and the row's audioop.mul volume — and equals CPython's audioop.lin2ulaw(x, 2) /
 *                     audioop.lin2alaw(x, 2) for all 65,536 inputs.  Every other byte of the stream is the code of sample 0:
 *                     0xFF (mu-law) / 0xD5 (A-law) — silence is NOT zero bytes — and is written by the kernel.
 *   MI355VITS_ENC_F32LE  the float waveform itself, 4 bytes per sample.  Entry i's samples are BITWISE the valid samples of that
 *                     row's MI355VITS_WANT_FLOAT audio at the run's output rate: no normalisation, and pcm_volume does not apply
 *                     (as with MI355VITS_WANT_FLOAT).  Every other sample is 0.0f.
 *  - Scope: packed streams only (mi355vits_run_packed, mi355vits_fetch_packed).  mi355vits_run / _run_rows / _fetch /
 *    _device_result and the padded pcm / audio results are unchanged by it.
 *  - The setting is read when a pack is made: at the start of mi355vits_run_packed and at each mi355vits_fetch_packed.  After one
 *    synthesis, fetch_packed can therefore serve the same run in several encodings, no synthesis work repeated.
 *    mi355vits_clone inherits the setting.  An unknown value returns MI355VITS_ERR_INVALID with a message naming the value and
 *    leaves the setting as it was.
 *  - Result fields: offsets, lengths, total_samples (and lead_samples / tail_samples) stay in SAMPLES; peaks are as before.
 *    n_bytes = header + bytes_per_sample * total_samples (+ pad).  pcm points at the first data byte whatever the encoding: cast
 *    it to uint8_t* (G.711) or float* (F32LE; 4-byte aligned with or without a header).
 *  - wav_header != 0 with a non-S16LE encoding: the 58-byte non-PCM form, little-endian —
 *      "RIFF" u32 50 + data + pad  "WAVE"
 *      "fmt " u32 18  u16 tag (7 mu-law, 6 A-law, 3 IEEE float)  u16 1  u32 rate  u32 rate * bytes_per_sample
 *             u16 bytes_per_sample  u16 8 * bytes_per_sample  u16 0
 *      "fact" u32 4  u32 total_samples
 *      "data" u32 data
 *    for F32LE byte for byte what scipy.io.wavfile.write(f, rate, float32_mono) writes.  pad = one zero byte behind the data
 *    when data is odd (G.711 only): the RIFF size field and n_bytes count it, the data size field does not.
 *  - Size limits, checked before anything is sized or launched, with messages that name the entry or the limit:
 *    total_samples <= 2^31 - 1 as before; with a header the RIFF limit follows from the encoding (F32LE: 50 + 4 * total_samples
 *    <= 2^32 - 1).
 *  - No additional stream synchronisation or host round trip; the copy from the device is exactly bytes_per_sample *
 *    total_samples bytes. */
#define MI355VITS_ENC_S16LE 0   /* default: the int16 stream, bit for bit */
#define MI355VITS_ENC_ULAW  1   /* G.711 mu-law, 1 byte per sample */
#define MI355VITS_ENC_ALAW  2   /* G.711 A-law,  1 byte per sample */
#define MI355VITS_ENC_F32LE 3   /* the float waveform itself, 4 bytes per sample */
int mi355vits_set_output_encoding(mi355vits_handle h, int enc);
int mi355vits_get_output_encoding(mi355vits_handle h);

/* ---- Phoneme timing and levels: WHERE in a run's audio each phoneme sits, and how loud it is there.  What speech marks for
 * captions, visemes and lip-sync, a position for the reference's SSML <mark> (MarkResult carries a name and no time:
 * opentts_abc/__init__.py:131-139, mimic3_tts/tts.py:467-468), cutting a stream at word boundaries and duration editing need
 * (forced_durations replays a complete table; a rate per phoneme, a held pause or a fitted row length need no second run:
 * mi355vits_run_timed below).  The reference cannot give it: onnx_model.run returns the waveform only.
 * mi355vits_fetch_alignment serves the LAST COMPLETED RUN of the handle whatever its flags were (padded, MI355VITS_DEVICE_ONLY or
 * packed), at the rate it ran at, as mi355vits_fetch does.  One kernel (k_align) makes every array on the GPU.
 *   frames[b,t]   latent frames of phoneme t: the run's ceil(exp(logw) * length_scale), or its forced_durations value.
 *   start[b,t] = ceil(hop * c[t-1] * L / M),  samples[b,t] = ceil(hop * c[t] * L / M) - start[b,t],  c[t] = frames[b,0] + .. +
 *                 frames[b,t], c[-1] = 0, hop = config.hop_length, L / M = the run's reduced rate ratio (1 / 1 in a native run),
 *                 in exact 64-bit integers: start is the first sample of the row, at the run's rate, whose time is not before the
 *                 phoneme's native start (k_resample has zero delay: output sample k sits at native time k M / L).
 *  - start[b,0] = 0; the spans are disjoint, ordered and tile the row: start[b,t+1] = start[b,t] + samples[b,t], and their sum is
 *    lengths[b] of the run exactly (ceil(n L / M) is the resampler's length rule).  A phoneme of zero frames has samples = 0 and
 *    the next phoneme's start.
 *  - Positions t >= input_lengths[b]: frames = samples = 0, start = the end of the covered part, peak = rms = 0.
 *  - The one exception: a row whose durations sum to 0 still yields one frame of audio (the frame count is max(1, sum)), so it has
 *    all-zero spans and lengths[b] = ceil(hop L / M) > 0.
 *  - MI355VITS_ALIGN_LEVELS in `want`: peak / rms over the span of the run's float waveform at its output rate — the
 *    MI355VITS_WANT_FLOAT samples: before the int16 normalisation, pcm_volume does not apply.  peak = max |y|,
 *    rms = (float) sqrt(sum((double) y * y) / samples), both 0 for an empty span; double accumulation in one fixed order per
 *    phoneme, so a row of a batch is bitwise the row alone, and for every row with at least one frame max_t peak[b,t] is bitwise
 *    peaks[b] of the run.  Without the flag peak and rms are NULL and no kernel reads the audio.
 *  - sample_rate = the rate that run ran at: start / samples count these samples.  In a packed stream phoneme t of entry i is
 *    pcm[offsets[i] + start[order[i],t] ..) in any encoding (offsets are in samples).
 *  - One stream synchronisation and one device-to-host copy per call; the arrays are one pinned block, released by
 *    mi355vits_free_alignment.  The call works in an arena of its own: what mi355vits_fetch / _fetch_packed / _device_result
 *    serve afterwards is what they served before.  Serialised per handle like every other call.
 *  - Errors: before any completed run MI355VITS_ERR_INVALID with "fetch_alignment: no completed run on this handle" (a failed run
 *    leaves the previous run served, or none, exactly as for mi355vits_fetch); a NULL out or unknown bits in want:
 *    MI355VITS_ERR_INVALID.
 *  - With profiling enabled the launch is reported as "align": bytes = 12 * B * tx_max, with levels 4 * sum(lengths) + 20 * B * tx_max. */
#define MI355VITS_ALIGN_LEVELS 1u   /* also peak and rms per phoneme (one pass over the valid samples) */

typedef struct mi355vits_alignment {
    int32_t batch, tx_max;   /* of the run served */
    int32_t sample_rate;     /* the rate that run ran at: start / samples count these samples */
    int32_t* frames;         /* [B, tx_max] latent frames of phoneme t: the run's w_ceil */
    int32_t* start;          /* [B, tx_max] first sample of phoneme t within its row */
    int32_t* samples;        /* [B, tx_max] samples of phoneme t */
    float* peak;             /* [B, tx_max] or NULL: max |y| over the span */
    float* rms;              /* [B, tx_max] or NULL: sqrt(mean y^2) over the span */
    void* owner_;            /* private */
} mi355vits_alignment;

int mi355vits_fetch_alignment(mi355vits_handle h, uint32_t want, mi355vits_alignment* out);
void mi355vits_free_alignment(mi355vits_alignment* r);

/* ---- Timing control in ONE run: a rate per phoneme, held pauses, a fitted row length.  What SSML <prosody rate> around a few
 * words, <break> inside a sentence and "fit this line into 2.40 s" (dubbing, captions, IVR prompts) need.  Without it a caller
 * runs, fetches the alignment, edits the frames on the host and runs again with forced_durations: a text encoder, a duration
 * predictor, a host round trip and a decoder pass spent to learn integers the device already held.  The reference can scale a
 * whole sentence only (length_scale, one run per sentence).  mi355vits_run_timed is mi355vits_run_rows with the durations shaped
 * where they become known: ONE kernel (k_durations_timed) takes the place of k_durations, before the run's only sizing
 * synchronisation — no launch and no synchronisation more than the plain run.
 * The rule, exact: integers and single IEEE f32 products rounded to nearest, no tolerance.  Per row b, L = input_lengths[b], t < L:
 *   u[t]    = fl(w[t] * stretch[b,t])                    w[t] = exp(logw[t]) * length_scale[b], the float the plain run rounds up
 *   c(x)    = x < CAP ? (int) ceilf(x) : CAP + 1          CAP = 4,194,304 frames
 *   f[t](s) = max(c(fl(u[t] * s)), min_frames[b,t])      s a positive finite f32
 *   F(s)    = f[0](s) + .. + f[L-1](s)                   in 64-bit integers
 *  - target_frames[b] == 0 (or NULL): frames[t] = f[t](1.0f), factor 1.0f.  With stretch 1 and min_frames 0 that is bit for bit the
 *    plain run's ceil(exp(logw) * length_scale).
 *  - target_frames[b] = N, 1 .. CAP: F never falls as s grows and positive floats sort like their bit patterns.  s* = the largest
 *    f32 in [2^-30, 2^30] with F(s*) <= N, found by bisection over the bit patterns; frames[t] = f[t](s*), and the N - F(s*)
 *    frames still missing go to the phonemes that step at s' = nextafterf(s*, +inf), walking t upward: phoneme t receives
 *    min(f[t](s') - f[t](s*), what is left).  The frames of the row then sum to N exactly: lengths[b] = N * hop_length in a native
 *    run, ceil(N * hop_length * L / M) at another output rate.  factor_out[b] = s*.
 *  - F(2^-30) > N: the target is below the floor (the minimum frames, and one frame for every other phoneme with u > 0):
 *    MI355VITS_ERR_INVALID, "row 3: target of 40 frames is below the 57 the row needs at least".  F(2^30) < N (every stretch 0, say):
 *    MI355VITS_ERR_INVALID naming the row.  Both are found at the run's sizing synchronisation, before anything behind the text
 *    side is sized or launched: no partial audio, and the handle is left as by any run that fails there (a predicted duration out
 *    of range): it serves no result until the next completed run.
 *  - Positions t >= L: frames 0, whatever stretch and min_frames hold there (they are neither checked nor read).
 *  - A row of a batch is bitwise the row alone (same tx_max class, see mi355vits_run_rows): the rule has no float sum in it.
 *  - Scope: timing == NULL, or stretch, min_frames and target_frames all NULL: the call IS mi355vits_run_rows — the same launches,
 *    bytes and synchronisations (factor_out, when given, reads 1.0f).  All flags work as there, MI355VITS_DEVICE_ONLY included; the
 *    packed and streams forms need no call of their own: mi355vits_fetch_packed, _fetch_streams, _fetch_streams2 and
 *    mi355vits_fetch_alignment serve the last completed run whatever made it, so a timed run with MI355VITS_DEVICE_ONLY followed by
 *    one of them gives every output form at the cost of the ONE synchronisation more that the fetch takes.
 *    mi355vits_fetch_alignment reports the fitted frames.  Feeding them back as forced_durations (same seed and keys) gives bitwise
 *    the same audio.  Under MI355VITS_DEBUG_TAPS a timed run also serves the tap "dur_float" [B, 1, tx_max]: u[t], 0 behind the row.
 *  - Errors, all MI355VITS_ERR_INVALID and, but for the two above, raised before anything is launched (the previous run stays
 *    served): forced_durations together with any timing input ("timing and forced_durations exclude each other"); a stretch that
 *    is not finite or outside 0 .. 2^20, a min_frames outside 0 .. CAP (checked at t < input_lengths[b] only; the message names row
 *    and phoneme); a target_frames outside 0 .. CAP (names the row); a non-zero reserved field.
 *  - With profiling enabled the kernel is reported as "durations.timed" in place of "durations". */
typedef struct mi355vits_timing_args {
    const float*   stretch;        /* [B, tx_max] or NULL (= 1): duration multiplier per phoneme; finite, 0 <= x <= 2^20 */
    const int32_t* min_frames;     /* [B, tx_max] or NULL (= 0): 0 .. CAP; a pause symbol held at least this long */
    const int32_t* target_frames;  /* [B] or NULL: 0 = none, else the row's latent frames, 1 .. CAP (duration = frames * hop / rate) */
    float*         factor_out;     /* [B] or NULL, caller-owned: s* per row (1.0f without a target) */
    int32_t        reserved[6];    /* must be 0 */
} mi355vits_timing_args;
int mi355vits_run_timed(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows /* may be NULL */,
                        const mi355vits_timing_args* timing /* may be NULL */, mi355vits_result* out);

/* ---- Blended and caller-supplied speakers per row.  On a multi-speaker voice the speaker is only a vector g of gin_channels
 * floats: `sid` looks it up in the table emb_g, and every consumer of it (dp.cond, dec.cond, each flow's enc.cond_layer) is a 1x1
 * projection of that vector.  mi355vits_run_speakers is mi355vits_run_timed with g of every row given as a blend of table rows
 * ("70 % of speaker 12, 30 % of speaker 40", extrapolation such as 1.5 / -0.5 included) or as the caller's own vector (averaged,
 * interpolated or fitted outside), per row of one batched call — no rewritten weight container with one more emb_g row and no
 * second handle with a second weight replica per blend.  ONE kernel (k_speaker_cond_mix) makes g of all rows and every consumer's
 * projection in ONE launch, in place of the 2 + flow_n_flows launches of the plain run; the tables ride in the run's one upload: no
 * synchronisation and no host round trip more than the plain run.
 * The rule, exact (no tolerance).  Per row b and channel i < gin_channels:
 *  - Mix: the terms (mix_sid[b,k], mix_weight[b,k]), k = 0 .. n_terms - 1.  A term whose weight is exactly 0 (+0 or -0) is skipped: not
 *    multiplied, its sid neither checked nor read — rows of one batch carry different term counts that way.  Over the remaining
 *    terms, in order of k, with e_k = emb_g[mix_sid[b,k], :]:
 *        g[i] = fl(w_0 * e_0[i]),   then   g[i] = fl(g[i] + fl(w_k * e_k[i]))
 *    single IEEE f32 products and sums rounded to nearest, never a fused multiply-add.  A one-term mix of weight 1.0f gives g bitwise
 *    the table row, -0.0 included.
 *  - Vector: g[i] = vectors[b, i], bits in, bits out.
 *  - Projections: every consumer's out[b, co] = W[co, :] . g + bias[co] is computed element for element as the plain run computes
 *    it from a table row (per wave lane l: fmaf(W[co, i], g[i], acc) over i = l, l + 64, .. from 0.0f; a butterfly sum over the 64
 *    lanes; + bias).  So:
 *      * a speakers run is bitwise the plain run with sid = S on a voice whose emb_g carries that g as row S — audio, pcm, lengths, peaks;
 *      * {s: 1.0} for every row, or vectors equal to mi355vits_get_speaker_embedding(s), is bitwise the plain run with sid = s;
 *      * a row of a batch is bitwise the row alone (same noise key and tx_max class, see mi355vits_run_rows), and permuting the rows
 *        of a batch permutes the results: nothing depends on the row block, the grid, the batch or an address.
 *  - Scope: speakers == NULL: the call IS mi355vits_run_timed — the same launches, bytes and synchronisations.  With speakers,
 *    args->sid may be NULL and is not read.  All flags work, MI355VITS_DEVICE_ONLY included; the packed, streams and alignment
 *    forms need no call of their own: mi355vits_fetch_packed, _fetch_streams, _fetch_streams2 and mi355vits_fetch_alignment serve the
 *    last completed run whatever made it.  rows and timing combine with speakers freely.  Under MI355VITS_DEBUG_TAPS a speakers run
 *    also serves the tap "g" [B, gin_channels, 1].
 *  - Errors, all MI355VITS_ERR_INVALID, raised before anything is launched (the previous run stays served): a single-speaker voice
 *    ("voice has no speaker embedding"); mix_* together with vectors, or neither, or one of mix_sid / mix_weight alone; n_terms
 *    outside 1 .. MI355VITS_MAX_SPEAKER_TERMS with mix_*, or not 0 with vectors; a sid outside the table at a non-zero weight (the
 *    message names the row and the term); a weight that is not finite or beyond +-1024 (row and term); a vector value that is not
 *    finite (row); a row whose every weight is 0 (row); a non-zero reserved field.
 *  - With profiling enabled the kernel is reported as "speaker_cond.mix" in place of "speaker_cond". */
#define MI355VITS_MAX_SPEAKER_TERMS 8
typedef struct mi355vits_speaker_args {
    int32_t        n_terms;     /* K, 1 .. MI355VITS_MAX_SPEAKER_TERMS with mix_*; 0 with vectors */
    const int64_t* mix_sid;     /* [B, K] */
    const float*   mix_weight;  /* [B, K] finite, |w| <= 1024; exactly 0 = term skipped */
    const float*   vectors;     /* [B, gin_channels] finite; excludes mix_* */
    int32_t        reserved[6]; /* must be 0 */
} mi355vits_speaker_args;
int mi355vits_run_speakers(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows /* may be NULL */,
                           const mi355vits_timing_args* timing /* may be NULL */, const mi355vits_speaker_args* speakers /* may be NULL */,
                           mi355vits_result* out);
/* Row `sid` of the voice's speaker table emb_g -> out[0 .. gin_channels): copied from a host copy kept with the weights, no stream
 * work, no synchronisation.  capacity = floats out can take.  A sid outside the table, capacity < gin_channels, a NULL out or a
 * single-speaker voice: MI355VITS_ERR_INVALID. */
int mi355vits_get_speaker_embedding(mi355vits_handle h, int64_t sid, float* out, size_t capacity);

/* ---- Level control in one run: a gain per phoneme with exact ramps.  pcm_volume is one factor per row behind the int16
 * normalisation and the loudness target one gain per row; what shapes a PART of a row — an SSML <prosody volume="+6dB"> or <emphasis>
 * around two words, a breath turned down, a word muted — is an envelope over the waveform that follows the phoneme boundaries.
 * mi355vits_run_levels is mi355vits_run_speakers with such an envelope applied where the waveform becomes known: ONE kernel
 * (k_levels) over the native waveform on the device, in place, right behind conv_post / tanh and in front of everything that reads
 * it.  The boundaries are the run's own (the inclusive scan of its frames, already in device memory); gain and ramp ride in the run's
 * one upload: no synchronisation and no host round trip more than the plain run.
 * The rule, exact (integers and singly rounded IEEE operations, no tolerance).  Per row b, in native-rate samples, with
 * L = input_lengths[b], c[t] the inclusive scan of the run's frames (natural, forced_durations or a timed fit), hop = hop_length,
 * n = hop * max(1, c[L-1]) the row's valid native samples (n = hop when L = 0), R = ramp_samples[b] and ONE = 2^20:
 *     q[t]     = (int32) rintf(gain[b,t] * 1048576.0f)      the product is exact (a power of two); ties to even; 0 <= q <= 2^30
 *     qs(i)    for 0 <= i < n: q[t(i)], t(i) = the smallest t < L with hop * c[t] > i (phonemes of zero frames own no sample);
 *              ONE when there is no such t (a row whose durations sum to 0 still has one frame of audio);
 *              qs(i) = qs(0) for i < 0, qs(n - 1) for i >= n (edge values repeat)
 *     S[k]     = sum of qs(i) over k - R <= i <= k + R      int64: exact in any order
 *     scale[k] = (float) ((double) S[k] / (double) ((2 R + 1) * 2^20))       one double division, one conversion
 *     y[k]     = x[k] * scale[k]                            one f32 product, rounded to nearest; 0 <= k < n
 *     peak[b]  = fmaxf chain over |y[k]| from 0.0f          as the waveform's own kernel takes it (a NaN is never taken)
 * What follows:
 *  1. Where every phoneme within R samples has gain 1.0, S = (2 R + 1) * 2^20 and scale = 1.0f exactly: those samples keep their
 *     bits.  A run with every gain 1.0 is bitwise the plain run: audio, pcm, lengths and peaks.
 *  2. Inside a phoneme and further than R from its ends, scale = (float) (q / 2^20): the double quotient is exact there.
 *  3. Across a boundary the gain moves linearly over 2 R + 1 samples centred on it; R = 0 is a step.  A phoneme shorter than 2 R + 1
 *     samples never reaches its own gain: that is the moving average, and it is the contract.  The fixed-point step is 2^-20, so a
 *     gain below 2^-21 is a mute (2^-21 itself is a tie and rounds to 0).  A NaN sample stays a NaN, and +-Inf under a scale of 0
 *     becomes one (IEEE's invalid product: its sign and payload are the platform's).
 *  4. Nothing depends on the grid, the CU count, the batch, the row block or an address: a row of a batch is bitwise the row alone
 *     (same noise key and tx_max class, see mi355vits_run_rows).
 *  5. The envelope is applied to the native waveform.  At another output rate (mi355vits_set_output_rate) the result is the
 *     resampler's output of the shaped native row; mi355vits_fetch_alignment's spans still say where the change lands, because the
 *     resampler has zero delay.  `peaks`, the int16 normalisation, every packed / streams / FLAC form, mi355vits_fetch_edges,
 *     _fetch_loudness, _fetch_limiter, _fetch_true_peak and the levels of mi355vits_fetch_alignment see the shaped waveform;
 *     MI355VITS_WANT_FLOAT returns it.
 *  - Scope: levels == NULL or levels->gain == NULL: the call IS mi355vits_run_speakers — the same launches, bytes and
 *    synchronisations.  rows, timing, speakers, forced_durations and all flags combine with levels freely.  The packed, streams and
 *    alignment forms need no call of their own: a MI355VITS_DEVICE_ONLY levels run followed by mi355vits_fetch_packed,
 *    _fetch_streams, _fetch_streams2 or mi355vits_fetch_alignment gives them, as after a timed run.
 *  - Errors, all MI355VITS_ERR_INVALID, raised before anything is launched (the previous run stays served): a gain that is not
 *    finite, negative or above 1024, looked at where t < input_lengths[b] only (the message names the row and the phoneme); a ramp
 *    outside 0 .. 4096 (the row); a non-zero reserved field.
 *  - With profiling enabled the kernel is reported as "levels", bytes = 8 * sum(native lengths) + 4 * B * (tx_max + 1); a run
 *    without levels has no such line. */
typedef struct mi355vits_level_args {
    const float*   gain;          /* [B, tx_max] or NULL (= 1): linear gain per phoneme; finite, 0 <= x <= 1024 (-0.0 is 0) */
    const int32_t* ramp_samples;  /* [B] or NULL (= 0): R per row, 0 .. 4096 native-rate samples */
    int32_t        reserved[6];   /* must be 0 */
} mi355vits_level_args;
int mi355vits_run_levels(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows /* may be NULL */,
                         const mi355vits_timing_args* timing /* may be NULL */, const mi355vits_speaker_args* speakers /* may be NULL */,
                         const mi355vits_level_args* levels /* may be NULL */, mi355vits_result* out);

/* ---- Pitch control in one run: a ratio per phoneme, duration kept.  VITS has no pitch input; what an SSML <prosody pitch="+10%"> or
 * a few semitones of emphasis wants is a phoneme synthesized p times longer and played back p times faster: its pitch is multiplied
 * by p, its duration unchanged.  mi355vits_run_pitch is mi355vits_run_levels with both halves in the run: the stretch of a timed run
 * (k_durations_timed, unchanged) and a band-limited variable-rate warp of the native waveform along the run's own phoneme boundaries
 * (k_pitch_plan, k_pitch) on the device, in front of everything that reads the waveform.  THIS IS RESAMPLING: formants move with the
 * pitch.  It is not a formant-preserving voice change.
 * The rule, exact (integers and singly rounded IEEE f32 operations, never fused, no tolerance).  Per row b, with L = input_lengths[b],
 * p[t] = ratio[b,t], hop = hop_length, ONE = 2^20, P = 128, Z = 12:
 *  1. Duration compensation.  The run is a timed run whose stretch is fl(stretch[b,t] * p[t]) (ONE f32 product, made on the host;
 *     stretch is 1 when absent).  With forced_durations the table IS the synthesized frames: no compensation, the row gets shorter
 *     or longer.
 *  2. The time map.  fs[t] the run's frames (natural, timed or forced), c their inclusive scan, n = hop * max(1, c[L-1]);
 *         inv[t] = (int) rintf(1048576.0f / p[t])            one f32 division, ties to even; 2^19 .. 2^21, p = 1 gives ONE
 *         Tq[t]  = sum over u <= t of hop * fs[u] * inv[u]   int64: exact in any order; Tq[-1] = 0
 *         wc[t]  = ceil(Tq[t] / ONE)                         the warped boundaries;  wlen = wc[L-1] the warped row length
 *     (a row without frames has one pseudo-phoneme of hop samples with inv = ONE).  Output sample k (0 <= k < wlen) lies in the
 *     smallest t with Tq[t] > k * ONE; (q, r) = divmod(k * ONE - Tq[t-1], inv[t]), i0 = hop * c[t-1] + q: its source position is
 *     i0 + r / inv[t].  The map is continuous and monotone across boundaries: no phase restart at a boundary.
 *  3. The sample.  D = max(inv[t], ONE).  If inv[t] == ONE and r == 0: y[k] = x[i0], bits in, bits out (a select).  Otherwise, over
 *     the source samples j ASCENDING with N = (i0 - j) * inv[t] + r and |N| < Z * D, x[j] = 0 by select outside [0, n):
 *         (idx, rem) = divmod(|N| * P, D);  phi = (float) rem / (float) D
 *         coef = fl(h[idx] + fl(phi * fl(h[idx+1] - h[idx])));  acc = fl(acc + fl(coef * x[j])), from 0.0f
 *     y[k] = acc when inv[t] >= ONE, else fl(fl((float) inv[t] * 2^-20) * acc): Smith's stretched prototype, whose cut-off follows
 *     the span's step, so a raised pitch does not alias.  peaks[b] = the fmaxf chain over |y|, as k_levels takes it.
 *  4. The table.  h[i], i = 0 .. Z*P + 1, = the f32 rounding of sinc(i / P) * I0(8 sqrt(1 - (i / (Z P))^2)) / I0(8), computed in
 *     double on the host when the handle is created; entries at multiples of P are exactly 0, h[0] = 1, h[Z*P] = h[Z*P+1] = 0.
 * What follows:
 *  - Every ratio 1.0 is bitwise the plain run: lengths, peaks and the valid samples of audio and pcm (behind a row's length, up to
 *    l_max, a pitch run leaves zeros).
 *  - Samples further than Z source samples from a span with p != 1 keep their bits.
 *  - A row of a batch is bitwise the row alone, and permuting rows permutes results.  Nothing depends on the grid, the CU count, the
 *    batch or an address.  A unit impulse returns bitwise the interpolated coefficients.
 *  - Everything behind the waveform works on the warped rows, with lengths wlen (then ceil(wlen L / M) at another output rate):
 *    MI355VITS_WANT_FLOAT and the int16 pass, k_resample, every packed / streams / FLAC form (a MI355VITS_DEVICE_ONLY pitch run, then
 *    the fetch), mi355vits_fetch_edges, _fetch_loudness, _fetch_limiter and _fetch_true_peak.
 *  - mi355vits_fetch_alignment reports frames = the synthesized frames (fed back as forced_durations with the same ratios they give
 *    bitwise the same audio), start[t] = ceil(wc[t-1] L / M), samples[t] = ceil(wc[t] L / M) - start[t]: the spans still tile the row
 *    and sum to lengths[b].
 *  - k_levels runs BEFORE the warp, on the synthesized waveform: its ramp of R samples lasts R / p samples in the result.
 *  - No synchronisation and no host round trip more than the plain run: the warped lengths ride in the run's one sizing copy.
 *  - Scope: pitch == NULL or pitch->ratio == NULL: the call IS mi355vits_run_levels — the same launches, bytes and synchronisations.
 *  - Errors, all MI355VITS_ERR_INVALID, raised before anything is launched (the previous run stays served): a ratio that is not
 *    finite or lies outside [0.5, 2], looked at where t < input_lengths[b] only (the message names row and phoneme); a product
 *    stretch * ratio above 2^20 (row and phoneme); a row with target_frames[b] != 0 and a ratio other than 1.0 ("row 3: a fitted
 *    length and a pitch ratio exclude each other": the fit counts synthesized frames, a warped row could not meet it exactly); a
 *    non-zero reserved field.  At the sizing synchronisation: a warped row that does not fit 32 bits (the message names the row).
 *  - With profiling enabled the kernels are reported as "pitch.plan" and "pitch", the latter with
 *    bytes = 4 * (sum n + sum wlen) + 20 * B * tx_max; a run without pitch has no such lines.  Under MI355VITS_DEBUG_TAPS a pitch run
 *    also serves "audio_synth" [B, 1, L]: the waveform in front of the warp. */
typedef struct mi355vits_pitch_args {
    const float* ratio;        /* [B, tx_max] or NULL (= 1): pitch multiplier per phoneme; finite, 0.5 <= x <= 2 */
    int32_t      reserved[7];  /* must be 0 */
} mi355vits_pitch_args;
int mi355vits_run_pitch(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows /* may be NULL */,
                        const mi355vits_timing_args* timing /* may be NULL */, const mi355vits_speaker_args* speakers /* may be NULL */,
                        const mi355vits_level_args* levels /* may be NULL */, const mi355vits_pitch_args* pitch /* may be NULL */,
                        mi355vits_result* out);

/* ---- Exact pauses: trim each entry's quiet edges in the packed streams.  A VITS voice puts a stretch of near-silence of its own at
 * the start and the end of every sentence; the reference adds its break (int(ms / 1000 * sample_rate) zero samples,
 * mimic3_tts/tts.py:452-465) on top of it, so a 250 ms break is heard as 250 ms plus two unknown tails.  With edge trimming on, an
 * entry of a packed stream is its row cut to the loud part, and lead_samples is the pause.  The rule is exact — integers from f32
 * comparisons, no tolerance: for a row with n valid samples y[0..n) at the run's rate (the MI355VITS_WANT_FLOAT samples) and peak p
 * (bitwise peaks[b] of the run),
 *     thr = p * ratio                 one IEEE f32 multiply, rounded to nearest
 *     sample k is loud  iff  fabsf(y[k]) >= thr           (exactly at thr: loud; a NaN: not loud)
 *     first = max(0, s_first - keep_samples),  end = min(n, s_last + 1 + keep_samples)       s_first / s_last: first / last loud sample
 * ratio <= 1 makes the sample that holds the peak loud: a row is never emptied (end - first >= 1 for n >= 1); an all-zero row has
 * thr = 0, every sample loud and nothing cut.  One kernel (k_edges) reads the valid samples once; keep and the clamps are the host's.
 *  - mi355vits_set_edge_trim: ratio = 0 (the default): off — nothing below applies, nothing is launched or laid out, every byte is
 *    what it was.  ratio NaN, < 0 or > 1, or keep_samples < 0: MI355VITS_ERR_INVALID, the message names the value, the setting stays.
 *    keep_samples counts samples at the run's output rate, like lead_samples.  mi355vits_clone inherits the setting.  It is read when
 *    a pack is made and at each mi355vits_fetch_edges (as mi355vits_set_output_encoding is): one synthesis can be packed trimmed and
 *    untrimmed, at several thresholds, with no synthesis work repeated.
 *  - Scope: the packed streams and mi355vits_fetch_edges only.  mi355vits_run / _run_rows / _fetch / _device_result, the padded
 *    audio / pcm, lengths, peaks, l_max, and mi355vits_fetch_alignment (row coordinates) stay bit for bit what they are whatever the
 *    setting; a caller of the padded forms slices with first / end.
 *  - mi355vits_run_packed / _fetch_packed with trimming on: entry i of row r is samples [first[r], end[r]) of that row, bitwise those
 *    samples of the untrimmed stream for the same arguments in every encoding and math mode (the int16 and G.711 scales are still the
 *    row's peak and volume; F32LE is bits in, bits out).  lengths[i] = end[r] - first[r]; offsets and total_samples follow from the
 *    trimmed lengths; peaks[i] is the row's peak as before; every other sample is the silence code, written by the kernel; the RIFF
 *    sizes and the fact count are the trimmed stream's.  The size checks that need only n, order and the silences run before
 *    synthesis as before; the limits that count audio are checked on the TRIMMED sizes before the pack is sized or launched: the
 *    result is never partial audio, and a run_packed that fails there leaves no result served, as a failed run does.
 *  - Synchronisation: the offsets now depend on the audio.  A trimmed mi355vits_run_packed synchronises the stream three times
 *    instead of twice (frame counts, edges, result), a trimmed mi355vits_fetch_packed twice instead of once, and each copies 8 * B
 *    bytes more to the host.  The edges of the last run under the last ratio are kept on the host: a repeated fetch at the same
 *    ratio does not launch again.  With ratio = 0 the counts are what they were.
 *  - mi355vits_fetch_edges serves the LAST COMPLETED RUN whatever its flags were, at the rate it ran at, under the current setting.
 *    It works in an arena of its own: what mi355vits_fetch / _fetch_packed / _fetch_alignment / _device_result serve afterwards is
 *    what they served before.  Before any completed run: MI355VITS_ERR_INVALID with "fetch_edges: no completed run on this handle";
 *    a NULL out: MI355VITS_ERR_INVALID.  With the setting off: first = 0, end = lengths, nothing launched.
 *  - With profiling enabled the launch is reported as "edges": bytes = 4 * sum(lengths) + 8 * B. */
int mi355vits_set_edge_trim(mi355vits_handle h, float ratio, int32_t keep_samples);
int mi355vits_get_edge_trim(mi355vits_handle h, float* ratio, int32_t* keep_samples);

typedef struct mi355vits_edges {
    int32_t batch;
    int32_t sample_rate;   /* the rate the run served ran at: first / end count these samples */
    float ratio;           /* the setting the arrays were made with (0: off — first = 0, end = lengths) */
    int32_t keep_samples;
    int32_t* first;        /* [B] first kept sample of row b */
    int32_t* end;          /* [B] one past the last kept sample */
    void* owner_;          /* private */
} mi355vits_edges;

int mi355vits_fetch_edges(mi355vits_handle h, mi355vits_edges* out);
void mi355vits_free_edges(mi355vits_edges* r);

/* ---- Equal loudness across a request: ITU-R BS.1770-4 / EBU R128 integrated loudness of every row, and a target gain in the packed
 * streams.  The int16 conversion scales every sentence so that its largest sample is 32767 (audio_float_to_int16): a two-word
 * interjection and a forty-word sentence get the same peak and very different loudness, and one plosive sets the level of its whole
 * sentence.  With a loudness target each entry of a packed stream is scaled to the target instead, from the float waveform, before any
 * quantisation.  Each row is measured alone, mono: its n valid samples x[0..n) at the run's rate fs (the MI355VITS_WANT_FLOAT samples;
 * pcm_volume does not apply), all arithmetic IEEE double:
 *     K-weighting: two biquads in cascade, zero state at sample 0, coefficients by the bilinear derivation for any fs —
 *       shelf:     f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *                  Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2; b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0,
 *                  a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *       high pass: f0 = 38.13547087602444, Q = 0.5003270373238773, K and a0 likewise; b = [1, -2, 1], a as above
 *       (at 48 kHz the table of BS.1770)
 *     S = (fs + 5) / 10 (integer): the 100 ms step;  E_j = sum of y[k]^2 over step j of the filtered row
 *     z_i = (E_i + E_{i+1} + E_{i+2} + E_{i+3}) / (4 S) for i = 0 .. nb - 1, nb = (n - 4 S) / S + 1: whole 400 ms blocks only;
 *       a row with 0 < n < 4 S is one block over all of it, z_0 = sum y^2 / n, nb = 1; n = 0: nb = 0
 *     l_i = -0.691 + 10 log10(z_i);  absolute gate l_i > -70;  relative gate l_i > -0.691 + 10 log10(mean z over the absolutely gated) - 10
 *     lufs = -0.691 + 10 log10(mean z over the blocks passing both), -inf when no block passes the absolute gate
 *     gain: g = 10^((target - lufs) / 20) (1.0 when lufs = -inf), cap = 10^(ceiling / 20) / peak (none when the peak is 0),
 *       gain = min(g, cap), limited = cap < g.  By default the ceiling only bounds the gain: a row it holds back ends below target and
 *       says so (limited).  mi355vits_set_loudness_limiter (below) turns on a look-ahead peak limiter that brings such a row to
 *       its target instead; there is no compressor.
 *  - mi355vits_set_loudness_target: target_lufs = 0 (the default): off — nothing below is launched or laid out by a pack, every byte is
 *    what it was.  On: -70 <= target_lufs < 0 with a finite ceiling_dbfs <= 0; anything else, NaN included: MI355VITS_ERR_INVALID, the
 *    message names the value, the setting stays.  mi355vits_clone inherits it.  Read when a pack is made and at each
 *    mi355vits_fetch_loudness (as the encoding and the edge trimming are): one synthesis can be packed at several targets and
 *    un-normalised with no synthesis work repeated.
 *  - Scope: the samples of the packed streams only.  mi355vits_run / _run_rows / _fetch / _device_result, the padded audio / pcm,
 *    lengths, peaks, mi355vits_fetch_alignment and mi355vits_fetch_edges never move.  In a packed stream the row's factor becomes
 *    scale = (float)(32767.0 * gain) in place of 32767.0f / fmaxf(0.01f, peak); the clamp, the truncation, pcm_volume and G.711 behind
 *    it are unchanged; MI355VITS_ENC_F32LE writes x[k] * (float)gain.  peaks[i] stays the row's float peak.  The whole row is measured
 *    whatever the edge trimming: a trimmed entry is bitwise [first, end) of the untrimmed entry at the same target.
 *  - Synchronisation: the scales depend on the audio.  mi355vits_run_packed with a target synchronises three times instead of twice
 *    (frame counts, measurement, result) — also with edge trimming on: both measurements go before the same synchronisation —,
 *    mi355vits_fetch_packed twice.  The measurement of the last run is kept on the host: a repeated fetch at any target launches
 *    nothing; a run drops it.
 *  - mi355vits_fetch_loudness serves the LAST COMPLETED RUN whatever its flags were, at the rate it ran at; with the target off it
 *    still measures (gain = 0.0, limited = 0).  It works in an arena of its own: what the other fetches serve afterwards is what they
 *    served before.  Before any completed run: MI355VITS_ERR_INVALID with "fetch_loudness: no completed run on this handle"; a NULL
 *    out: MI355VITS_ERR_INVALID.  The measure is offered from 4000 Hz up: a run at a lower output rate is MI355VITS_ERR_INVALID here
 *    and in a pack with a target.
 *  - With profiling enabled the two launches are reported as "loudness": bytes = 4 * sum(lengths) + 8 * sum(steps) + 16 * B. */
int mi355vits_set_loudness_target(mi355vits_handle h, float target_lufs, float ceiling_dbfs);
int mi355vits_get_loudness_target(mi355vits_handle h, float* target_lufs, float* ceiling_dbfs);

typedef struct mi355vits_loudness {
    int32_t batch, sample_rate;          /* of the run served */
    float target_lufs, ceiling_dbfs;     /* the setting the arrays were made with; target 0 = off */
    double* lufs;       /* [B] integrated loudness; -inf when no block passes the absolute gate */
    double* gain;       /* [B] linear gain applied in packed streams; 0.0 when off */
    int32_t* blocks;    /* [B] */
    int32_t* gated;     /* [B] */
    int32_t* limited;   /* [B] 1 where the ceiling bounded the gain */
    void* owner_;
} mi355vits_loudness;

int mi355vits_fetch_loudness(mi355vits_handle h, mi355vits_loudness* out);
void mi355vits_free_loudness(mi355vits_loudness* r);

/* ---- Reach the loudness target: a look-ahead peak limiter on the float waveform of the packed streams, before any quantisation.
 * Without it one plosive sets the level of its whole sentence again whenever the ceiling binds (gain = cap < g) — which is what
 * happens at the targets speech products use (-16 LUFS, -14 LUFS with a -1 or -2 dB ceiling): speech commonly has a crest factor
 * above what such a target leaves under the ceiling.  (General knowledge about speech, not a measurement of this project: the
 * synthetic voices of its test suite are far flatter.)  With the limiter on, a row the ceiling would hold back keeps its full gain g and
 * only the samples within L samples of a peak are turned down, by a curve that is defined exactly — integers wherever an order could
 * matter, so the same bits at any grid, CU count, batch or row address.  Per row of a pack with a loudness target:
 *     x[0..n) the row's valid float samples at the run's rate;  g = 10^((target - lufs) / 20) in double, 1.0 for lufs = -inf;
 *     c = 10^(ceiling / 20);  p the row's peak;  L >= 1 the window in samples;  ONE = 2^30
 *     the row is OVER iff the gain rule above marks it limited (cap = c / p < g).  A row that is not over is untouched by everything
 *     below: its bytes are those of the limiter off.  For a row that is over:
 *       a[t]  = g * fabs((double) x[t])                              one double multiply
 *       rq[t] = a[t] > c ? (int32) floor((c / a[t]) * 2^30) : ONE    IEEE double divide; NaN -> ONE; rq[t] = ONE for t < 0 or t >= n
 *       mq[i] = min over i <= t <= i + L of rq[t]                    for i = -L .. n - 1
 *       sq[k] = sum over k - L <= i <= k of mq[i]                    int64: exact in any order
 *       s[k]  = (double) sq[k] / ((double)(L + 1) * 2^30)
 *       scale[k] = (float)(U * (g * s[k]))                           double, in this order; U = 32767.0 (S16LE, G.711) or 1.0 (F32LE)
 *     scale[k] replaces the entry's single scale: S16LE and G.711 samples are pcm16_quant(x[k], scale[k], volume) and the G.711
 *     encoders as before, F32LE samples x[k] * scale[k].  pcm_volume still acts behind the scale and still clamps.
 *   Consequences:
 *   1. The ceiling holds.  Every window behind sq[k] contains k, so s[k] <= rq[k] / 2^30 <= c / a[k]: in reals g |x[k]| s[k] <= c.
 *      After the two f32 roundings an F32LE sample satisfies |y| <= c (1 + 2^-22), an int16 sample at volume 1 |q| <= floor(32767 c) + 1.
 *   2. Samples away from peaks keep their bits.  Where sq[k] = (L + 1) 2^30, s[k] = 1.0 exactly and scale[k] is bitwise (float)(U g):
 *      what an uncapped gain g writes.
 *   3. Placement cannot change the result: nothing depends on the grid, the batch, the CU count or the row's address.  A row of a
 *      batch is bitwise the row alone; a trimmed entry is bitwise [first, end) of the untrimmed one — the curve is made on the whole
 *      row, as the loudness is measured on it.
 *   The window is symmetric: the gain falls over L samples before a peak and recovers over L behind it.  A longer L means less
 *   distortion and more ducking; that trade is the caller's.  No separate release time.  What the ceiling bounds is the SAMPLE peak unless
 *   mi355vits_set_loudness_ceiling_mode (the section after this one) says otherwise.
 *  - mi355vits_set_loudness_limiter: window_samples = 0 (the default): off — nothing is launched, laid out or changed, every byte and
 *    every synchronisation is what it was.  On: 1 <= window_samples <= 4096, counted at the run's output rate (as keep_samples is);
 *    anything else: MI355VITS_ERR_INVALID, the message names the value, the setting stays.  Read when a pack is made (as the target
 *    is), at mi355vits_fetch_loudness and at mi355vits_fetch_limiter; mi355vits_clone inherits it.  Without a loudness target it does nothing.
 *  - With it on, mi355vits_run_packed / _fetch_packed limit the over rows of a pack with a target instead of capping their gain;
 *    mi355vits_fetch_loudness and the packed results then report gain = g (uncapped) and limited = 1 for those rows.
 *  - mi355vits_run_streams / _fetch_streams (below) cannot carry a per-stream window — mi355vits_stream_args is frozen —: the handle's
 *    window applies to every stream that has a target.  (A window per stream: mi355vits_run_streams2 / _fetch_streams2.)
 *  - mi355vits_fetch_limiter serves the LAST COMPLETED RUN under the handle's current target, ceiling and window, in an arena of its
 *    own (what the other fetches serve afterwards is what they served before): engaged[b] = the row is over, reduced_samples[b] = the
 *    count of k with sq[k] < (L + 1) 2^30, min_scale[b] = min over k of s[k] (1.0 for a row that is not over).  With the limiter or
 *    the target off: zeros / 1.0, and nothing is launched.  Before any completed run: MI355VITS_ERR_INVALID with "fetch_limiter: no
 *    completed run on this handle"; a NULL out: MI355VITS_ERR_INVALID.
 *  - Synchronisation: none added.  The curve needs g, which the host has after the measurement's synchronisation; k_limit
 *    (csrc/kernels_limit.cpp) runs between that synchronisation and the pack, on the same stream: mi355vits_run_packed with a target
 *    stays at three synchronisations, mi355vits_fetch_packed at two — once the limiter's workspace has reached its size: the first
 *    pack (and the first mi355vits_fetch_limiter) whose jobs outgrow it reallocates it, which waits for the stream, as the packed
 *    stream's own buffer does when it grows.  The curve is made per pack and not kept.  A pack on no row of
 *    which the limiter engages launches no k_limit and is packed by the kernels of the limiter off.
 *  - With profiling enabled the launch is reported as "limit": bytes = 8 * sum(lengths of the jobs) + 16 * jobs; a job is one over
 *    row under one (target, ceiling, U) — in a streams call a row shared by streams of the same setting is one job. */
int mi355vits_set_loudness_limiter(mi355vits_handle h, int32_t window_samples);
int32_t mi355vits_get_loudness_limiter(mi355vits_handle h);

typedef struct mi355vits_limiter {
    int32_t batch, sample_rate;   /* of the run served */
    int32_t window_samples;       /* the setting the arrays were made with; 0 = off */
    int32_t* engaged;             /* [B] 1 where the row is over: the limiter acts on it */
    int32_t* reduced_samples;     /* [B] samples whose scale lies below the row's full gain */
    double* min_scale;            /* [B] min s[k]; 1.0 for a row that is not over */
    void* owner_;
} mi355vits_limiter;

int mi355vits_fetch_limiter(mi355vits_handle h, mi355vits_limiter* out);
void mi355vits_free_limiter(mi355vits_limiter* r);

/* ---- A true-peak ceiling: the 4x oversampled peak of every row, on the GPU.  The ceiling above bounds SAMPLES; R128 and the delivery
 * specifications built on it state theirs in dBTP, for the reconstructed waveform, whose peaks lie between the samples (how far above
 * them depends on the material: DESIGN.md 4.14 has what was measured at the native rate and at 8 kHz).  In true-peak mode the gain
 * rule and the limiter look at an oversampled peak instead.  Per row of a completed run: x[0..n) its valid float samples at the run's
 * rate (the MI355VITS_WANT_FLOAT samples; pcm_volume does not apply).  All arithmetic is IEEE double, every product is rounded once
 * and every sum is rounded once: there is NO fused multiply-add.
 *     h[0..80]  = the 81 taps of scipy.signal.resample_poly(., 4, 1)'s default filter (Kaiser window beta 5, half = 40, cut-off 1/4,
 *                 gain 4): fixed constants of the library, literal in csrc/kernels_truepeak.cpp
 *     u[j]      = sum over i = 0 .. 20, ascending, starting from 0.0, of  h[p + 4 i] * (double) x[q - i]
 *                 where j + 40 = 4 q + p, 0 <= p < 4, h[m] = 0 for m > 80, x = 0 outside [0, n);   j = 0 .. 4 n - 1
 *     v[j]      = fabs((double) x[j / 4]) when j % 4 == 0   (phase 0 is the samples themselves: its centre tap is 1.0006, not 1)
 *                 fabs(u[j])              otherwise
 *     tp        = max over j of v[j], taken with "v > m" from m = 0.0: a NaN is never taken;  n = 0: tp = 0
 *     e[t]      = max over j in [4 t - 3, 4 t + 3] within [0, 4 n) of v[j], same comparison          the envelope of sample t
 *   max_t e[t] = tp;  e[t] >= |x[t]|;  e[t] depends on x[t - 11 .. t + 10] only;  tp >= (double) peak.  The factor is 4 relative to
 *   the run's rate, whatever that rate is: after mi355vits_set_output_rate the row is band-limited to its own Nyquist, so the
 *   proportions are those of BS.1770's 48 kHz case.  No claim is made to reproduce the coefficient table of BS.1770 Annex 2:
 *   implementations differ there, and the rule above is the contract.
 *  - mi355vits_set_loudness_ceiling_mode: MI355VITS_CEILING_SAMPLE (the default): every byte, launch and synchronisation is what it
 *    was.  MI355VITS_CEILING_TRUE_PEAK: wherever the loudness rule and the limiter rule above use the row's peak or
 *    fabs((double) x[t]) they use tp or e[t] —
 *      gain rule: cap = c / tp (none when tp = 0), gain = min(g, cap), limited = cap < g;  a row is OVER iff c / tp < g;
 *      limiter:   a[t] = g * e[t]; everything behind it (rq, mq, sq, s, scale) is unchanged.
 *    Any other value: MI355VITS_ERR_INVALID, the message names it, the setting stays.  Read where the loudness target is read: when a
 *    pack is made, at mi355vits_fetch_loudness and mi355vits_fetch_limiter, and by mi355vits_run_streams / _fetch_streams from the
 *    handle, as they read the limiter window (mi355vits_stream_args is frozen: the mode applies to every stream that has a target).
 *    mi355vits_clone inherits it.  Without a loudness target it does nothing to a pack.
 *   Consequences:
 *   1. Without the limiter, g tp <= c holds in reals for a capped row: the oversampled peak of the scaled row is under the ceiling.
 *   2. With the limiter, g e[k] s[k] <= c holds: every SAMPLE obeys the ceiling as before, and both neighbours of an inter-sample
 *      peak are turned down.
 *   3. The true peak of the limited output is not bounded by a theorem, because the gain curve modulates the signal.  It is
 *      measured (tests/test_true_peak.py) and not promised.
 *   4. Nothing depends on the grid, the batch, the CU count or the row's address.  A row of a batch is bitwise the row alone.
 *  - Synchronisation: none added.  The measurement (k_true_peak, csrc/kernels_truepeak.cpp) is launched next to the loudness
 *    measurement, in front of the same synchronisation; tp of the last run is kept on the host with the loudness (a repeated fetch
 *    launches nothing, a run drops it).  The envelope of the over rows is written between that synchronisation and the pack, into
 *    the limiter's workspace, right before k_limit; a pack on no row of which the limiter engages launches neither.
 *  - mi355vits_fetch_true_peak serves the LAST COMPLETED RUN whatever its flags were, at the rate it ran at, and measures whatever
 *    the mode.  It works in an arena of its own: what the other fetches serve afterwards is what they served before.  Before any
 *    completed run: MI355VITS_ERR_INVALID with "fetch_true_peak: no completed run on this handle"; a NULL out: MI355VITS_ERR_INVALID.
 *  - With profiling enabled the measurement is reported as "truepeak": bytes = 4 * sum(lengths) + 8 * B; the envelope pass as
 *    "truepeak.env": bytes = 12 * sum(lengths of the jobs). */
#define MI355VITS_CEILING_SAMPLE 0
#define MI355VITS_CEILING_TRUE_PEAK 1
int mi355vits_set_loudness_ceiling_mode(mi355vits_handle h, int mode);
int mi355vits_get_loudness_ceiling_mode(mi355vits_handle h);

typedef struct mi355vits_true_peak {
    int32_t batch, sample_rate;   /* of the run served */
    double* true_peak;            /* [B] tp, linear */
    float* peak;                  /* [B] the row's sample peak: bitwise peaks[b] of the run */
    void* owner_;
} mi355vits_true_peak;

int mi355vits_fetch_true_peak(mi355vits_handle h, mi355vits_true_peak* out);
void mi355vits_free_true_peak(mi355vits_true_peak* r);

/* ---- The packed stream as FLAC: lossless frames encoded on the GPU.  MI355VITS_COMPRESS_NONE (the default) = nothing below
 * applies: every byte, launch and synchronisation is what it was before this setting existed.
 * FLAC is a compression layer over the S16LE stream, not a fifth sample encoding: the int16 stream k_pack writes on the device —
 * with every setting applied: order, silences, volume, output rate, edge trim, loudness target, limiter, ceiling mode — is turned
 * into FLAC frames by a second kernel (k_flac_frames, one workgroup per frame of 4096 samples), and only the compressed bytes cross
 * the bus.
 *  - With MI355VITS_COMPRESS_FLAC, bytes[0, n_bytes) of the mi355vits_packed_result is a complete FLAC file: "fLaC", one STREAMINFO
 *    block (42 bytes together: block size 4096, the smallest and largest frame in bytes, the run's rate, 1 channel, 16 bits,
 *    total_samples; the MD5 field is all zero — NOT computed: it needs a serial pass over the whole stream), then the frames back to
 *    back.  pcm points at the first frame, bytes + 42.  n, total_samples, offsets, lengths and peaks are exactly those of the same
 *    call uncompressed, in SAMPLES.
 *  - Contract: decoding the file yields, sample for sample and bit for bit, the int16 stream mi355vits_fetch_packed returns for the
 *    same pack arguments and handle settings with compression off — in every math mode, at any output rate, with trim, loudness,
 *    limiter and true-peak mode on or off.  The bytes are a pure function of (int16 stream, rate): nothing depends on the grid, the
 *    CU count, the batch or an address.
 *  - The subset of RFC 9639 written (DESIGN.md §4.15 has every field): fixed block size 4096 (the last frame may be short), one
 *    subframe per frame — constant when all samples are equal, else the fixed predictor of order 0 .. 4 with the fewest bits (Rice
 *    partition order 4 in a full block, 0 in a short one; every Rice parameter 0 .. 14 chosen by exact count, never the escape
 *    code), or verbatim when no order saves a bit — CRC-8 over the frame header and CRC-16 over the frame.
 *    The bytes are pinned by a reference encoder and an independently written decoder in the test suite; they have not met a
 *    third-party decoder.
 *  - The setting is read when a pack is made: at the start of mi355vits_run_packed and at each mi355vits_fetch_packed, as the
 *    encoding is.  One synthesis can therefore be fetched raw and as FLAC, no synthesis work repeated.  mi355vits_clone inherits it.
 *    An unknown value returns MI355VITS_ERR_INVALID with a message naming the value and leaves the setting as it was.
 *  - Errors, all MI355VITS_ERR_INVALID, found before anything is sized or launched: an output encoding other than S16LE
 *    ("pack: FLAC compresses the s16le stream; output encoding is ulaw"), wav_header != 0 ("a FLAC stream carries its own
 *    header"), a run rate above 1,048,575 Hz (STREAMINFO's 20 bits).  total_samples <= 2^31 - 1 as before.
 *  - Size: a frame is at most 16 + 2 * (its samples) bytes, so n_bytes <= 42 + 16 * frames + 2 * total_samples; a full frame of
 *    equal samples is 11 bytes.
 *  - Cost: the compressed size depends on the audio, so a FLAC pack costs exactly ONE stream synchronisation more than the same
 *    call uncompressed and copies 4 * (frames + 1) bytes more to the host (the frame sizes and their total); the copy of the result
 *    is exactly n_bytes - 42 bytes.  The profiler reports the launches as pack.flac with 2 * total_samples + (n_bytes - 42) bytes,
 *    behind the pcm16.pack line of the S16LE pack in front of them.
 *  - Scope: mi355vits_run_packed and mi355vits_fetch_packed.  mi355vits_run_streams / _fetch_streams never read the setting
 *    (mi355vits_stream_args is frozen) and stay byte for byte what they are.  FLAC per stream of a block: mi355vits_run_streams2 /
 *    _fetch_streams2, which take the compression from the stream. */
#define MI355VITS_COMPRESS_NONE 0   /* default: every byte, launch and synchronisation is what it was */
#define MI355VITS_COMPRESS_FLAC 1
int mi355vits_set_output_compression(mi355vits_handle h, int mode);
int mi355vits_get_output_compression(mi355vits_handle h);

/* ---- Packed streams per request: SEVERAL independent streams out of one run.  A server that batches the sentences of many clients
 * into one synthesis call (one or a few rows per client) wants one finished stream per CLIENT — its own order, silences, header,
 * encoding, trim and loudness target — not one stream per call.  One kernel (k_pack_streams, csrc/kernels_pack.cpp) writes all of them
 * into ONE block, and one device-to-host copy of exactly n_bytes brings them back.
 * Block layout: stream s occupies bytes[stream_offset[s], + stream_bytes[s]) = its RIFF header if asked for (44 bytes for S16LE, 58
 * otherwise), its data, and the RIFF pad byte behind an odd data size.  Its first data byte sits at data_offset[s], a multiple of 16
 * (the block itself is page aligned: F32LE / S16LE data can be read in place); streams follow each other in the order given, and every
 * byte of [0, n_bytes) outside the streams is zero.
 *  - Stream s: bytes[stream_offset[s], + stream_bytes[s]) is BITWISE what mi355vits_fetch_packed returns for streams[s].pack on the same
 *    run with the handle set to that stream's encoding, trim and loudness target (mi355vits_set_output_encoding / _set_edge_trim /
 *    _set_loudness_target) — in every math mode, at the run's output rate, header and pad byte included.  Its entries' offsets (in
 *    samples within the stream's data) / lengths / peaks and its total_samples are that call's; first[] is the first source sample of
 *    each entry (0 untrimmed), gain[] / lufs[] / limited[] what mi355vits_fetch_loudness reports for the entry's row at that stream's
 *    target (all 0 for a stream without one).  Entries are flattened stream after stream: stream s owns [entry_base[s], entry_base[s + 1]).
 *  - The handle's own encoding, trim and loudness settings are NOT read by the two calls and not changed by them.  The handle's limiter
 *    window (mi355vits_set_loudness_limiter) is the one handle setting the two calls DO read: it applies to every stream that has a
 *    target, and stream s is bitwise mi355vits_fetch_packed under that stream's settings plus the handle's limiter window.
 *  - A row appears at most once within a stream, as in mi355vits_run_packed; it may appear in several streams (the same sentence as
 *    int16 and as mu-law, say).
 *  - As for mi355vits_run_packed, MI355VITS_WANT_* / MI355VITS_DEVICE_ONLY are ignored and no padded int16 pass runs; mi355vits_fetch /
 *    _fetch_packed / _fetch_alignment / _fetch_edges / _fetch_loudness / _device_result serve afterwards what they serve after a
 *    MI355VITS_DEVICE_ONLY run, and a mi355vits_fetch_streams does not change what they served before it.
 *  - Synchronisation: mi355vits_run_streams synchronises twice when no stream trims or normalises (the table rides with the per-stage
 *    length table), three times otherwise; mi355vits_fetch_streams once, or twice.  Loudness is measured once per run, edges once per
 *    distinct non-zero ratio among the streams, all measurements in front of the same synchronisation.  The host keeps what it
 *    measured: a repeated fetch at known ratios launches nothing before the pack.
 *  - One k_pack_streams launch and one device-to-host copy of exactly n_bytes.  With profiling enabled the launch is reported as
 *    "pack.streams": bytes = 4 * sum(lengths) + n_bytes.
 *  - Errors are found before anything is sized or launched, return MI355VITS_ERR_INVALID, and the message names the stream:
 *    "stream 2: pack entry 1: row 9 out of range", "stream 0: unknown encoding 7", "stream 3: trim ratio 1.5 is outside [0, 1]",
 *    "stream 1: loudness target 3 LUFS is neither 0 (off) nor in [-70, 0)".  The validation rules and the per-stream size limits are
 *    those of the single-stream calls and their setters; in addition the block is limited: "streams: block of N bytes exceeds
 *    2^31 - 1".  n_streams < 1 or a NULL array: MI355VITS_ERR_INVALID.  Never partial audio; a mi355vits_run_streams that fails on the
 *    trimmed sizes leaves no result served, as mi355vits_run_packed does; mi355vits_fetch_streams before any completed run:
 *    "fetch_streams: no completed run on this handle".
 *  - Out of scope: alignment in stream coordinates (add offsets to mi355vits_fetch_alignment's spans, or use mi355vits_run_packed), and
 *    several output rates in one call (the rate is a property of the run).
 *  - A limiter window, a ceiling mode or FLAC per stream: mi355vits_run_streams2 / _fetch_streams2 below.  These two calls and their
 *    structs stay byte for byte what they are. */
typedef struct mi355vits_stream_args {
    mi355vits_pack_args pack;   /* entries (batch rows), lead / tail silences, wav_header: as for mi355vits_run_packed */
    int32_t encoding;           /* MI355VITS_ENC_* of THIS stream */
    float trim_ratio;           /* 0 = off; as mi355vits_set_edge_trim */
    int32_t trim_keep_samples;
    float target_lufs;          /* 0 = off; as mi355vits_set_loudness_target */
    float ceiling_dbfs;
} mi355vits_stream_args;

typedef struct mi355vits_streams_result {
    int32_t n_streams;
    int32_t n_entries;         /* of all streams together */
    uint8_t* bytes;            /* the block; pinned, callee-owned */
    size_t n_bytes;
    int64_t* stream_offset;    /* [S] first byte of stream s: its header if it has one */
    int64_t* stream_bytes;     /* [S] header + data + pad */
    int64_t* data_offset;      /* [S] first data byte of stream s; a multiple of 16 */
    int64_t* total_samples;    /* [S] silences included */
    int32_t* encoding;         /* [S] */
    int32_t* entry_base;       /* [S + 1] stream s owns entries [entry_base[s], entry_base[s + 1]) of the arrays below */
    int32_t* rows;             /* [E] batch row of the entry */
    int64_t* offsets;          /* [E] first audio sample of the entry within its stream's data, in samples */
    int64_t* lengths;          /* [E] */
    float* peaks;              /* [E] */
    int32_t* first;            /* [E] first source sample of the entry (0 untrimmed) */
    double* lufs;              /* [E] of the entry's row; 0 in a stream without a loudness target */
    double* gain;              /* [E] linear gain the entry carries; 0 likewise */
    int32_t* limited;          /* [E] */
    void* owner_;              /* private */
} mi355vits_streams_result;

int mi355vits_run_streams(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows /* may be NULL */,
                          const mi355vits_stream_args* streams, int32_t n_streams, mi355vits_streams_result* out);
/* The LAST completed run of the handle as streams again (whatever flags it had); no synthesis work is repeated. */
int mi355vits_fetch_streams(mi355vits_handle h, const mi355vits_stream_args* streams, int32_t n_streams, mi355vits_streams_result* out);
void mi355vits_free_streams(mi355vits_streams_result* r);

/* ---- Streams v2: compression, limiter window and ceiling mode PER STREAM.  The v1 calls above stay byte for byte what they are: they
 * read the limiter window and the ceiling mode from the handle and never compress.  The v2 calls read NONE of the handle's pack
 * settings — encoding, trim, target, limiter window, ceiling mode and compression all come from the stream — and change none of them,
 * so requests that differ in any of the six share one synthesis call and one block.
 *  - Stream s: bytes[stream_offset[s], + stream_bytes[s]) is BITWISE what mi355vits_fetch_packed returns for streams[s].base.pack on
 *    the same run with the handle set to that stream's six settings, in every math mode and at the run's output rate: RIFF header and
 *    pad byte, or the 42 FLAC header bytes, included.  offsets / lengths / peaks / first / lufs / gain / limited / total_samples are
 *    that call's values, in samples (also for a compressed stream); gain and limited follow the stream's own window and mode (a row the
 *    limiter takes over reports the uncapped gain, as mi355vits_fetch_loudness does).
 *  - A compressed stream (MI355VITS_COMPRESS_FLAC) is a complete FLAC file: encoding[s] = MI355VITS_ENC_S16LE, stream_offset[s] a
 *    multiple of 16, data_offset[s] = stream_offset[s] + 42 (its first frame), stream_bytes[s] = 42 + its frames, frames[s] their count.
 *  - Block layout: bytes[0, uncompressed_bytes) is byte for byte the block a v1 call over the uncompressed streams alone, in the order
 *    given, returns (uncompressed_bytes = 0 when there are none).  The compressed streams follow from the next multiple of 16, in the
 *    order given, each at the next multiple of 16.  Every byte of [0, n_bytes) outside the streams is zero and written by a kernel.
 *  - With no compressed stream a v2 call IS the v1 call: the same launches, synchronisations and copies, the same block — the limiter
 *    launches once per distinct (window, mode) among the streams the limiter engages on, so also that is v1's when they agree.
 *    Windows and modes add no synchronisation; k_true_peak runs iff some stream with a target is in true-peak mode.
 *  - With at least one compressed stream: exactly ONE stream synchronisation more than the same call with those streams uncompressed
 *    (the sizes depend on the audio); before it at most 4 * (frames + 4 * n_streams + 1) bytes go to the host; the block then arrives
 *    in at most two copies of exactly their bytes (the uncompressed part, the compressed part).  k_pack_streams writes the
 *    uncompressed part and, behind it in the device buffer, every compressed stream's samples as a headerless S16LE stream;
 *    k_flac_frames runs once over one job per compressed stream; k_flac_place puts every frame and file in its place and makes the
 *    headers; k_flac_gather_streams writes the compressed region with 16-byte stores.  Profiler: "pack.streams" bytes =
 *    4 * sum(lengths) + the bytes k_pack_streams writes; "pack.flac" bytes = 2 * sum(total_samples of the compressed streams) +
 *    sum(stream_bytes - 42).
 *  - Errors: MI355VITS_ERR_INVALID, naming the stream, found before anything is sized or launched, never partial audio — every v1 rule
 *    and message for `base`, and "stream 2: unknown compression 7", "stream 1: FLAC compresses the s16le stream; encoding is ulaw",
 *    "stream 0: a FLAC stream carries its own header", "stream 3: limiter window 5000 is outside 0 .. 4096", "stream 3: unknown
 *    ceiling mode 9", "stream 0: reserved fields must be 0"; a run's rate above 1,048,575 Hz with any FLAC stream.  The block limit of
 *    2^31 - 1 bytes counts a compressed stream at its bound, 42 + 16 * frames + 2 * total_samples.
 *  - After a v2 call every other fetch, v1 mi355vits_fetch_streams included, serves what it serves after a v1 call. */
typedef struct mi355vits_stream_args2 {
    mi355vits_stream_args base;      /* every field exactly as in mi355vits_run_streams */
    int32_t compression;             /* MI355VITS_COMPRESS_* of THIS stream */
    int32_t limiter_window_samples;  /* 0 = off; rules of mi355vits_set_loudness_limiter */
    int32_t ceiling_mode;            /* MI355VITS_CEILING_* ; rules of mi355vits_set_loudness_ceiling_mode */
    int32_t reserved[5];             /* must be 0 */
} mi355vits_stream_args2;

typedef struct mi355vits_streams_result2 {
    int32_t n_streams;
    int32_t n_entries;         /* every field down to `limited`: as in mi355vits_streams_result */
    uint8_t* bytes;
    size_t n_bytes;
    int64_t* stream_offset;
    int64_t* stream_bytes;
    int64_t* data_offset;
    int64_t* total_samples;
    int32_t* encoding;
    int32_t* entry_base;
    int32_t* rows;
    int64_t* offsets;
    int64_t* lengths;
    float* peaks;
    int32_t* first;
    double* lufs;
    double* gain;
    int32_t* limited;
    int32_t* compression;      /* [S] MI355VITS_COMPRESS_* of stream s */
    int32_t* frames;           /* [S] the FLAC frames of stream s; 0 when uncompressed */
    int64_t uncompressed_bytes; /* the v1 block of the uncompressed streams in front; 0 when there are none */
    void* owner_;              /* private */
} mi355vits_streams_result2;

int mi355vits_run_streams2(mi355vits_handle h, const mi355vits_run_args* args, const mi355vits_row_args* rows /* may be NULL */,
                           const mi355vits_stream_args2* streams, int32_t n_streams, mi355vits_streams_result2* out);
int mi355vits_fetch_streams2(mi355vits_handle h, const mi355vits_stream_args2* streams, int32_t n_streams, mi355vits_streams_result2* out);
void mi355vits_free_streams2(mi355vits_streams_result2* r);

/* Device pointers of the last run's results on this handle (valid until its next run; the engine's stream has been
 * synchronised when this returns): int16 [batch, row_stride] and/or float [batch, row_stride] in HBM, plus the valid
 * sample counts [batch] (int32, device).  For the optional device-side result gather over RCCL (north star; SURVEY.md
 * §8e) — the data never visits the host.  Pass NULL for what is not wanted. */
int mi355vits_device_result(mi355vits_handle h, const int16_t** pcm, const float** audio, int64_t* row_stride,
                            int32_t* batch, const int32_t** device_lengths);

/* Message of the last error on this handle (or, with h == NULL, of the last failed create on the
 * calling thread).  Valid until the next call on the same handle / thread. */
const char* mi355vits_last_error(mi355vits_handle h);

/* Per-kernel timing with HIP events on the engine's own stream (bench.py roofline leg).
 * enable(1) brackets every launch with an event pair; report() synchronises and writes one
 * line per kernel name: "name calls total_ms flops bytes\n".  Returns bytes written. */
int mi355vits_profile_enable(mi355vits_handle h, int on);
int mi355vits_profile_reset(mi355vits_handle h);
long mi355vits_profile_report(mi355vits_handle h, char* buf, size_t cap);

/* Wall time of the last run on the engine's stream, HIP events around the whole call (ms). */
float mi355vits_last_run_ms(mi355vits_handle h);

/* Debug taps (needs MI355VITS_DEBUG_TAPS on the last run): copy the named intermediate to
 * `out` (capacity in floats); dims receives up to 4 extents.  Returns element count or < 0. */
long mi355vits_get_tap(mi355vits_handle h, const char* name, float* out, size_t capacity, int64_t dims[4]);
/* The same for rows [row0, row0 + nrows) of the tap's leading (batch) extent only; dims[0] = nrows. */
long mi355vits_get_tap_rows(mi355vits_handle h, const char* name, long row0, long nrows, float* out, size_t capacity, int64_t dims[4]);
long mi355vits_list_taps(mi355vits_handle h, char* buf, size_t cap);

/* The kernel unit-test, micro-benchmark and box-probe hooks are NOT part of this library: include/mi355vits_lab.h,
 * exported by libmi355vits_hooks.so (the product's objects + the hooks) and the lab build only. */

#ifdef __cplusplus
}
#endif
#endif /* MI355VITS_H */
