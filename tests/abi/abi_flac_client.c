/* A plain-C client of the compression calls of include/mi355vits.h (mi355vits_set_output_compression,
 * mi355vits_get_output_compression): runs a tiny voice packed, fetches the same run raw and as FLAC, checks the errors, the result
 * fields, the STREAMINFO fields and the first frame's sync against the raw stream, and writes the file with the raw stream behind it
 * (the caller decodes and compares) — against whatever libmi355vits*.so it is linked with.
 * usage: abi_flac_client <voice.m355> <out.flac> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355vits.h"

#define FAIL(msg) do { fprintf(stderr, "%s\n", msg); return 1; } while (0)

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    mi355vits_handle h = NULL;
    int rc = mi355vits_create(argv[1], 0, &h);
    if (rc != MI355VITS_OK) { fprintf(stderr, "create: %d %s\n", rc, mi355vits_last_error(NULL)); return 1; }
    mi355vits_config cfg;
    if (mi355vits_get_config(h, &cfg) != MI355VITS_OK) return 1;

    if (mi355vits_get_output_compression(h) != MI355VITS_COMPRESS_NONE) FAIL("the default is no compression");
    if (mi355vits_set_output_compression(h, MI355VITS_COMPRESS_FLAC) != MI355VITS_OK) FAIL("set flac");
    if (mi355vits_set_output_compression(h, 2) != MI355VITS_ERR_INVALID) FAIL("an unknown mode must fail");
    printf("expected failure msg=%s\n", mi355vits_last_error(h));
    if (mi355vits_get_output_compression(h) != MI355VITS_COMPRESS_FLAC) FAIL("a refused setting must leave the old one");

    int64_t ids[15] = {3, 7, 1, 9, 4, 5, 2, 0, 0, 0, 8, 6, 4, 2, 0};
    int64_t lengths[3] = {5, 2, 4};
    int64_t sid[3] = {0, 0, 0};
    float scales[3] = {0.5f, 1.0f, 0.5f};
    int32_t order[3] = {2, 0, 1};
    int64_t lead[3] = {0, 9000, 100};
    mi355vits_run_args a;
    memset(&a, 0, sizeof a);
    a.batch = 3; a.tx_max = 5; a.ids = ids; a.lengths = lengths; a.scales = scales;
    a.sid = cfg.n_speakers > 1 ? sid : NULL;
    mi355vits_pack_args pa;
    memset(&pa, 0, sizeof pa);
    pa.n = 3; pa.order = order; pa.lead_samples = lead; pa.tail_samples = 33;

    /* a header of its own: wav_header is refused, and so is another encoding, before anything runs */
    mi355vits_packed_result fl;
    pa.wav_header = 1;
    rc = mi355vits_run_packed(h, &a, NULL, &pa, &fl);
    if (rc != MI355VITS_ERR_INVALID || fl.bytes != NULL || fl.owner_ != NULL) FAIL("wav_header with FLAC must fail");
    printf("expected failure msg=%s\n", mi355vits_last_error(h));
    pa.wav_header = 0;
    if (mi355vits_set_output_encoding(h, MI355VITS_ENC_ULAW) != MI355VITS_OK) FAIL("set ulaw");
    rc = mi355vits_run_packed(h, &a, NULL, &pa, &fl);
    if (rc != MI355VITS_ERR_INVALID || fl.bytes != NULL) FAIL("ulaw with FLAC must fail");
    printf("expected failure msg=%s\n", mi355vits_last_error(h));
    if (mi355vits_set_output_encoding(h, MI355VITS_ENC_S16LE) != MI355VITS_OK) FAIL("set s16le");

    rc = mi355vits_run_packed(h, &a, NULL, &pa, &fl);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (mi355vits_set_output_compression(h, MI355VITS_COMPRESS_NONE) != MI355VITS_OK) FAIL("set none");
    mi355vits_packed_result raw;
    rc = mi355vits_fetch_packed(h, &pa, &raw);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }

    if (fl.n != raw.n || fl.total_samples != raw.total_samples) FAIL("n / total_samples are the uncompressed call's");
    int i;
    for (i = 0; i < 3; ++i)
        if (fl.offsets[i] != raw.offsets[i] || fl.lengths[i] != raw.lengths[i] || memcmp(&fl.peaks[i], &raw.peaks[i], sizeof(float)) != 0)
            FAIL("offsets / lengths / peaks are the uncompressed call's");
    if (raw.n_bytes != 2 * (size_t)raw.total_samples) FAIL("the raw stream is 2 bytes a sample");
    const uint8_t* f = fl.bytes;
    const size_t frames = (size_t)((fl.total_samples + 4095) / 4096);
    if (fl.n_bytes < 42 || fl.n_bytes > 42 + 16 * frames + 2 * (size_t)fl.total_samples) FAIL("n_bytes within its bound");
    if ((const uint8_t*)fl.pcm != f + 42) FAIL("pcm points at the first frame");
    if (memcmp(f, "fLaC", 4) != 0 || f[4] != 0x80 || f[5] != 0 || f[6] != 0 || f[7] != 34) FAIL("marker and STREAMINFO block header");
    if (f[8] != 0x10 || f[9] != 0 || f[10] != 0x10 || f[11] != 0) FAIL("block size 4096");
    const uint32_t rate = ((uint32_t)f[18] << 12) | ((uint32_t)f[19] << 4) | (f[20] >> 4);
    if (rate != (uint32_t)cfg.sample_rate) FAIL("the run's rate");
    if ((f[20] & 0x0e) != 0 || (((f[20] & 1) << 4) | (f[21] >> 4)) != 15) FAIL("mono, 16 bits");
    const uint64_t total = ((uint64_t)(f[21] & 15) << 32) | ((uint64_t)f[22] << 24) | ((uint64_t)f[23] << 16) | ((uint64_t)f[24] << 8) | f[25];
    if (total != (uint64_t)raw.total_samples) FAIL("total samples");
    for (i = 26; i < 42; ++i)
        if (f[i] != 0) FAIL("the MD5 is unset");
    if (f[42] != 0xff || f[43] != 0xf8) FAIL("the first frame's sync");
    const uint32_t fmin = ((uint32_t)f[12] << 16) | ((uint32_t)f[13] << 8) | f[14], fmax = ((uint32_t)f[15] << 16) | ((uint32_t)f[16] << 8) | f[17];
    if (fmin < 11 || fmax > 16 + 2 * 4096 || fmin > fmax) FAIL("frame size range");

    FILE* out = fopen(argv[2], "wb");
    if (!out || fwrite(fl.bytes, 1, fl.n_bytes, out) != fl.n_bytes) FAIL("write");
    fclose(out);
    out = fopen(argv[2], "ab");  /* the raw stream behind it, for the caller to compare the decoded file with */
    if (!out || fwrite(raw.bytes, 1, raw.n_bytes, out) != raw.n_bytes) FAIL("write");
    fclose(out);
    printf("flac bytes=%lu raw bytes=%lu\n", (unsigned long)fl.n_bytes, (unsigned long)raw.n_bytes);
    mi355vits_free_packed(&fl);
    if (fl.bytes != NULL || fl.owner_ != NULL) FAIL("free_packed must clear the struct");
    mi355vits_free_packed(&raw);
    mi355vits_destroy(h);
    printf("flac ok\n");
    return 0;
}
