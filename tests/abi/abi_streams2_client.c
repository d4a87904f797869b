/* A plain-C client of the streams v2 calls of include/mi355vits.h (mi355vits_run_streams2, mi355vits_fetch_streams2,
 * mi355vits_free_streams2): runs a tiny voice as three streams of one block — a WAV, a FLAC file, a limited S16LE stream —, checks
 * the errors, the sizes, the layout and the FLAC stream against the raw stream fetched from the same run, and writes the FLAC stream
 * with the raw stream behind it (the caller decodes and compares) — against whatever libmi355vits*.so it is linked with.
 * usage: abi_streams2_client <voice.m355> <out.flac> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355vits.h"

#define FAIL(msg) do { fprintf(stderr, "%s\n", msg); return 1; } while (0)

static int expect_invalid(mi355vits_handle h, const mi355vits_stream_args2* st, int32_t n) {
    mi355vits_streams_result2 r;
    int rc = mi355vits_fetch_streams2(h, st, n, &r);
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    return rc == MI355VITS_ERR_INVALID && r.bytes == NULL && r.owner_ == NULL;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    mi355vits_handle h = NULL;
    int rc = mi355vits_create(argv[1], 0, &h);
    if (rc != MI355VITS_OK) { fprintf(stderr, "create: %d %s\n", rc, mi355vits_last_error(NULL)); return 1; }
    mi355vits_config cfg;
    if (mi355vits_get_config(h, &cfg) != MI355VITS_OK) return 1;

    int64_t ids[15] = {3, 7, 1, 9, 4, 5, 2, 0, 0, 0, 8, 6, 4, 2, 0};
    int64_t lengths[3] = {5, 2, 4};
    int64_t sid[3] = {0, 0, 0};
    float scales[3] = {0.5f, 1.0f, 0.5f};
    int32_t order_a[2] = {1, 0}, order_b[3] = {2, 0, 1}, order_c[1] = {2};
    int64_t lead_b[3] = {0, 9000, 100};
    mi355vits_run_args a;
    memset(&a, 0, sizeof a);
    a.batch = 3; a.tx_max = 5; a.ids = ids; a.lengths = lengths; a.scales = scales;
    a.sid = cfg.n_speakers > 1 ? sid : NULL;

    mi355vits_stream_args2 st[3];
    memset(st, 0, sizeof st);
    st[0].base.pack.n = 2; st[0].base.pack.order = order_a; st[0].base.pack.wav_header = 1;
    st[0].base.encoding = MI355VITS_ENC_S16LE;
    st[1].base.pack.n = 3; st[1].base.pack.order = order_b; st[1].base.pack.lead_samples = lead_b; st[1].base.pack.tail_samples = 33;
    st[1].base.encoding = MI355VITS_ENC_S16LE;
    st[1].compression = MI355VITS_COMPRESS_FLAC;
    st[2].base.pack.n = 1; st[2].base.pack.order = order_c;
    st[2].base.encoding = MI355VITS_ENC_S16LE;
    st[2].base.target_lufs = -6.0f; st[2].base.ceiling_dbfs = -6.0f;
    st[2].limiter_window_samples = 8; st[2].ceiling_mode = MI355VITS_CEILING_TRUE_PEAK;

    mi355vits_streams_result2 r;
    rc = mi355vits_fetch_streams2(h, st, 3, &r);
    if (rc != MI355VITS_ERR_INVALID || r.bytes != NULL) FAIL("a fetch before any run must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));

    rc = mi355vits_run_streams2(h, &a, NULL, st, 3, &r);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_streams2: %d %s\n", rc, mi355vits_last_error(h)); return 1; }

    /* the errors name the stream and leave the run served */
    mi355vits_stream_args2 bad[3];
    memcpy(bad, st, sizeof st); bad[2].compression = 7;
    if (!expect_invalid(h, bad, 3)) FAIL("an unknown compression must fail");
    memcpy(bad, st, sizeof st); bad[1].base.encoding = MI355VITS_ENC_ULAW;
    if (!expect_invalid(h, bad, 3)) FAIL("FLAC of a mu-law stream must fail");
    memcpy(bad, st, sizeof st); bad[1].base.pack.wav_header = 1;
    if (!expect_invalid(h, bad, 3)) FAIL("a FLAC stream with a WAV header must fail");
    memcpy(bad, st, sizeof st); bad[2].limiter_window_samples = 5000;
    if (!expect_invalid(h, bad, 3)) FAIL("a window above 4096 must fail");
    memcpy(bad, st, sizeof st); bad[2].ceiling_mode = 9;
    if (!expect_invalid(h, bad, 3)) FAIL("an unknown ceiling mode must fail");
    memcpy(bad, st, sizeof st); bad[0].reserved[4] = 1;
    if (!expect_invalid(h, bad, 3)) FAIL("a reserved field must be 0");

    /* sizes and layout */
    if (r.n_streams != 3 || r.n_entries != 6 || r.entry_base[3] != 6) FAIL("three streams, six entries");
    if (r.compression[0] != 0 || r.compression[1] != MI355VITS_COMPRESS_FLAC || r.compression[2] != 0) FAIL("compression per stream");
    if (r.frames[0] != 0 || r.frames[2] != 0 || r.frames[1] != (int32_t)((r.total_samples[1] + 4095) / 4096)) FAIL("frames per stream");
    if (r.stream_offset[0] != 4 || r.data_offset[0] != 48 || r.stream_bytes[0] != 44 + 2 * r.total_samples[0]) FAIL("the WAV stream's place");
    if (r.data_offset[2] % 16 != 0 || r.stream_offset[2] != r.data_offset[2] || r.stream_bytes[2] != 2 * r.total_samples[2]) FAIL("the raw stream's place");
    if (r.uncompressed_bytes != r.data_offset[2] + r.stream_bytes[2]) FAIL("the uncompressed streams come first");
    if (r.stream_offset[1] != ((r.uncompressed_bytes + 15) & ~(int64_t)15) || r.data_offset[1] != r.stream_offset[1] + 42) FAIL("the FLAC stream's place");
    if (r.encoding[1] != MI355VITS_ENC_S16LE) FAIL("a FLAC stream reports s16le");
    if (r.n_bytes != (size_t)(r.stream_offset[1] + r.stream_bytes[1])) FAIL("the block ends with its last stream");
    if (r.stream_bytes[1] < 42 + 11 * (int64_t)r.frames[1] || r.stream_bytes[1] > 42 + 16 * (int64_t)r.frames[1] + 2 * r.total_samples[1]) FAIL("the FLAC stream within its bound");
    if (r.limited[5] != 1 || r.gain[5] <= 0.0) FAIL("the third stream's row is over its ceiling: limited, with its uncapped gain");
    int64_t p;
    for (p = 0; p < r.stream_offset[0]; ++p)
        if (r.bytes[p] != 0) FAIL("zero in front of the first header");
    for (p = r.uncompressed_bytes; p < r.stream_offset[1]; ++p)
        if (r.bytes[p] != 0) FAIL("zero between the parts");
    const uint8_t* f = r.bytes + r.stream_offset[1];
    if (memcmp(f, "fLaC", 4) != 0 || f[4] != 0x80 || f[7] != 34 || f[8] != 0x10 || f[10] != 0x10) FAIL("marker and STREAMINFO");
    const uint32_t rate = ((uint32_t)f[18] << 12) | ((uint32_t)f[19] << 4) | (f[20] >> 4);
    if (rate != (uint32_t)cfg.sample_rate) FAIL("the run's rate");
    if (f[42] != 0xff || f[43] != 0xf8) FAIL("the first frame's sync");

    /* the twin: the same pack fetched alone under the handle's setter, raw and as FLAC */
    mi355vits_packed_result raw, fl;
    rc = mi355vits_fetch_packed(h, &st[1].base.pack, &raw);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (mi355vits_set_output_compression(h, MI355VITS_COMPRESS_FLAC) != MI355VITS_OK) FAIL("set flac");
    rc = mi355vits_fetch_packed(h, &st[1].base.pack, &fl);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (fl.n_bytes != (size_t)r.stream_bytes[1] || memcmp(fl.bytes, f, fl.n_bytes) != 0) FAIL("the FLAC stream is its twin");
    if (raw.total_samples != r.total_samples[1]) FAIL("total samples");

    /* a v2 fetch reads none of the handle's settings (compression is FLAC on the handle now) and changes none */
    mi355vits_streams_result2 again;
    rc = mi355vits_fetch_streams2(h, st, 3, &again);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_streams2: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (again.n_bytes != r.n_bytes || memcmp(again.bytes, r.bytes, r.n_bytes) != 0) FAIL("fetch_streams2 gives the run's block");
    if (mi355vits_get_output_compression(h) != MI355VITS_COMPRESS_FLAC || mi355vits_get_loudness_limiter(h) != 0) FAIL("the handle's settings stay");

    FILE* out = fopen(argv[2], "wb");
    if (!out || fwrite(f, 1, (size_t)r.stream_bytes[1], out) != (size_t)r.stream_bytes[1]) FAIL("write");
    fclose(out);
    out = fopen(argv[2], "ab");  /* the raw stream behind it, for the caller to compare the decoded file with */
    if (!out || fwrite(raw.bytes, 1, raw.n_bytes, out) != raw.n_bytes) FAIL("write");
    fclose(out);
    printf("flac bytes=%lu raw bytes=%lu\n", (unsigned long)r.stream_bytes[1], (unsigned long)raw.n_bytes);
    mi355vits_free_packed(&raw);
    mi355vits_free_packed(&fl);
    mi355vits_free_streams2(&again);
    mi355vits_free_streams2(&r);
    if (r.bytes != NULL || r.owner_ != NULL) FAIL("free_streams2 must clear the struct");
    mi355vits_destroy(h);
    printf("streams2 ok\n");
    return 0;
}
