/* A plain-C client of the output-encoding calls of include/mi355vits.h (mi355vits_set_output_encoding,
 * mi355vits_get_output_encoding) around the packed-result calls: proves the new declarations are C99 and checks n_bytes, the pcm
 * pointer, the silence codes and the 58-byte header of an encoded stream against whatever libmi355vits*.so it is linked with.
 * usage: abi_encoding_client <voice.m355> <out_ulaw.wav> <out_f32.wav>   (three rows, packed in the order 2, 0 with silences) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355vits.h"

#define FAIL(msg) do { fprintf(stderr, "%s\n", msg); return 1; } while (0)

static uint32_t u32le(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint32_t u16le(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

static int save(const char* path, const mi355vits_packed_result* r) {
    FILE* f = fopen(path, "wb");
    if (!f) return 1;
    fwrite(r->bytes, 1, r->n_bytes, f);
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    mi355vits_handle h = NULL, lane = NULL;
    int rc = mi355vits_create(argv[1], 0, &h);
    if (rc != MI355VITS_OK) { fprintf(stderr, "create: %d %s\n", rc, mi355vits_last_error(NULL)); return 1; }
    mi355vits_config cfg;
    if (mi355vits_get_config(h, &cfg) != MI355VITS_OK) return 1;
    int64_t ids[15] = {3, 7, 1, 9, 4, 5, 2, 0, 0, 0, 8, 6, 4, 2, 0};
    int64_t lengths[3] = {5, 2, 4};
    int64_t sid[3] = {0, 0, 0};
    float scales[3] = {0.0f, 1.0f, 0.0f};
    mi355vits_run_args a;
    memset(&a, 0, sizeof a);
    a.batch = 3; a.tx_max = 5; a.ids = ids; a.lengths = lengths; a.scales = scales;
    a.sid = cfg.n_speakers > 1 ? sid : NULL;
    int32_t order[2] = {2, 0};
    int64_t lead[2] = {3, 101};
    mi355vits_pack_args p;
    memset(&p, 0, sizeof p);
    p.n = 2; p.order = order; p.lead_samples = lead; p.tail_samples = 7; p.wav_header = 1;
    mi355vits_packed_result r;
    int64_t i, total;

    if (mi355vits_get_output_encoding(h) != MI355VITS_ENC_S16LE) FAIL("the default encoding is not S16LE");
    rc = mi355vits_run_packed(h, &a, NULL, &p, &r);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    total = r.total_samples;
    if (r.n_bytes != 44 + 2 * (size_t)total) FAIL("s16le: n_bytes");
    mi355vits_free_packed(&r);

    /* mu-law: one byte per sample behind the 58-byte header, silences are 0xFF; the count here is even or odd as it falls */
    if (mi355vits_set_output_encoding(h, MI355VITS_ENC_ULAW) != MI355VITS_OK) FAIL("set ULAW");
    if (mi355vits_get_output_encoding(h) != MI355VITS_ENC_ULAW) FAIL("get after set ULAW");
    rc = mi355vits_run_packed(h, &a, NULL, &p, &r);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_packed ulaw: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (r.total_samples != total || r.offsets[0] != 3) FAIL("ulaw: counts stay in samples");
    if (r.n_bytes != 58 + (size_t)total + (size_t)(total & 1) || (uint8_t*)r.pcm != r.bytes + 58) FAIL("ulaw: n_bytes / pcm");
    if (memcmp(r.bytes, "RIFF", 4) != 0 || memcmp(r.bytes + 8, "WAVEfmt ", 8) != 0 || memcmp(r.bytes + 38, "fact", 4) != 0 ||
        memcmp(r.bytes + 50, "data", 4) != 0)
        FAIL("ulaw: chunk ids");
    if (u32le(r.bytes + 4) != 50 + (uint32_t)total + (uint32_t)(total & 1) || u32le(r.bytes + 16) != 18 || u16le(r.bytes + 20) != 7 ||
        u16le(r.bytes + 22) != 1 || u32le(r.bytes + 24) != (uint32_t)cfg.sample_rate || u32le(r.bytes + 28) != (uint32_t)cfg.sample_rate ||
        u16le(r.bytes + 32) != 1 || u16le(r.bytes + 34) != 8 || u16le(r.bytes + 36) != 0 || u32le(r.bytes + 42) != 4 ||
        u32le(r.bytes + 46) != (uint32_t)total || u32le(r.bytes + 54) != (uint32_t)total)
        FAIL("ulaw: header fields");
    {
        const uint8_t* code = (const uint8_t*)r.pcm;
        for (i = 0; i < 3; ++i) if (code[i] != 0xFF) FAIL("ulaw: lead silence is not 0xFF");
        for (i = 0; i < 7; ++i) if (code[total - 1 - i] != 0xFF) FAIL("ulaw: tail silence is not 0xFF");
    }
    if (save(argv[2], &r)) return 1;
    mi355vits_free_packed(&r);

    /* a clone inherits the setting; A-law silence is 0xD5 */
    if (mi355vits_clone(h, &lane) != MI355VITS_OK) FAIL("clone");
    if (mi355vits_get_output_encoding(lane) != MI355VITS_ENC_ULAW) FAIL("the clone did not inherit the encoding");
    mi355vits_destroy(lane);
    if (mi355vits_set_output_encoding(h, MI355VITS_ENC_ALAW) != MI355VITS_OK) FAIL("set ALAW");
    rc = mi355vits_fetch_packed(h, &p, &r);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_packed alaw: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (u16le(r.bytes + 20) != 6 || ((const uint8_t*)r.pcm)[0] != 0xD5) FAIL("alaw: tag / silence");
    mi355vits_free_packed(&r);

    /* the float stream of the same run, no synthesis repeated: 4 bytes per sample, tag 3, never a pad byte */
    if (mi355vits_set_output_encoding(h, MI355VITS_ENC_F32LE) != MI355VITS_OK) FAIL("set F32LE");
    rc = mi355vits_fetch_packed(h, &p, &r);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_packed f32: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (r.n_bytes != 58 + 4 * (size_t)total || (uint8_t*)r.pcm != r.bytes + 58 || ((size_t)r.pcm & 3) != 0) FAIL("f32le: n_bytes / pcm");
    if (u16le(r.bytes + 20) != 3 || u16le(r.bytes + 32) != 4 || u16le(r.bytes + 34) != 32 ||
        u32le(r.bytes + 28) != 4 * (uint32_t)cfg.sample_rate || u32le(r.bytes + 54) != 4 * (uint32_t)total)
        FAIL("f32le: header fields");
    {
        const float* x = (const float*)r.pcm;
        for (i = 0; i < 3; ++i) if (x[i] != 0.0f) FAIL("f32le: lead silence is not 0.0f");
        if (x[3] == 0.0f && x[4] == 0.0f && x[5] == 0.0f) FAIL("f32le: no audio behind the lead silence");
    }
    if (save(argv[3], &r)) return 1;
    mi355vits_free_packed(&r);

    /* an unknown value -> error code, a message that names it, and the setting stays */
    rc = mi355vits_set_output_encoding(h, 9);
    if (rc != MI355VITS_ERR_INVALID || mi355vits_get_output_encoding(h) != MI355VITS_ENC_F32LE) { fprintf(stderr, "bad encoding gave rc=%d\n", rc); return 1; }
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    mi355vits_destroy(h);
    return 0;
}
