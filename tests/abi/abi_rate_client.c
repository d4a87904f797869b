/* A plain-C client of the output-rate calls of include/mi355vits.h (mi355vits_set_output_rate, mi355vits_get_output_rate): sets
 * 16 kHz and checks the lengths of the padded result and the rate field of the packed stream's RIFF header against whatever
 * libmi355vits*.so it is linked with.
 * usage: abi_rate_client <voice.m355> <out.wav>   (three rows at 16 kHz, packed in the order 2, 0 with silences and a header) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355vits.h"

#define FAIL(msg) do { fprintf(stderr, "%s\n", msg); return 1; } while (0)

static int64_t gcd64(int64_t a, int64_t b) { while (b) { int64_t t = a % b; a = b; b = t; } return a; }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    mi355vits_handle h = NULL;
    int rc = mi355vits_create(argv[1], 0, &h);
    if (rc != MI355VITS_OK) { fprintf(stderr, "create: %d %s\n", rc, mi355vits_last_error(NULL)); return 1; }
    mi355vits_config cfg;
    if (mi355vits_get_config(h, &cfg) != MI355VITS_OK) return 1;
    if (mi355vits_get_output_rate(h) != cfg.sample_rate) FAIL("unset: the effective rate is not the voice's");
    int64_t ids[15] = {3, 7, 1, 9, 4, 5, 2, 0, 0, 0, 8, 6, 4, 2, 0};
    int64_t lengths[3] = {5, 2, 4};
    int64_t sid[3] = {0, 0, 0};
    float scales[3] = {0.0f, 1.0f, 0.0f};
    mi355vits_run_args a;
    memset(&a, 0, sizeof a);
    a.batch = 3; a.tx_max = 5; a.ids = ids; a.lengths = lengths; a.scales = scales;
    a.sid = cfg.n_speakers > 1 ? sid : NULL;
    a.flags = MI355VITS_WANT_PCM16;
    mi355vits_result nat, res;
    int i;
    rc = mi355vits_run(h, &a, &nat);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run: %d %s\n", rc, mi355vits_last_error(h)); return 1; }

    /* a ratio the engine refuses: error code, a message that names it, the setting untouched */
    rc = mi355vits_set_output_rate(h, cfg.sample_rate + 1);
    if (rc != MI355VITS_ERR_INVALID || mi355vits_get_output_rate(h) != cfg.sample_rate) FAIL("a refused rate changed the setting");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));

    if (mi355vits_set_output_rate(h, 16000) != MI355VITS_OK || mi355vits_get_output_rate(h) != 16000) FAIL("set 16000");
    if (mi355vits_get_config(h, &cfg) != MI355VITS_OK || cfg.sample_rate == 16000) FAIL("config.sample_rate must stay native");
    rc = mi355vits_run(h, &a, &res);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    {
        const int64_t g = gcd64(16000, cfg.sample_rate), up = 16000 / g, down = cfg.sample_rate / g;
        int64_t lmax = 0;
        for (i = 0; i < 3; ++i) {
            if (res.lengths[i] != (nat.lengths[i] * up + down - 1) / down) FAIL("lengths are not ceil(n * L / M)");
            if (res.lengths[i] > lmax) lmax = res.lengths[i];
        }
        if (res.l_max != lmax || res.ty_max != nat.ty_max) FAIL("l_max / ty_max");
        for (i = 0; i < 3; ++i)
            if (res.lengths[i] < res.l_max && res.pcm[i * res.l_max + res.l_max - 1] != 0) FAIL("padding is not zero");
    }
    int64_t len0 = res.lengths[0], len2 = res.lengths[2];
    mi355vits_free_result(&nat);
    mi355vits_free_result(&res);

    int32_t order[2] = {2, 0};
    int64_t lead[2] = {3, 101};
    mi355vits_pack_args p;
    mi355vits_packed_result r;
    memset(&p, 0, sizeof p);
    p.n = 2; p.order = order; p.lead_samples = lead; p.tail_samples = 7; p.wav_header = 1;
    rc = mi355vits_run_packed(h, &a, NULL, &p, &r);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (r.lengths[0] != len2 || r.lengths[1] != len0 || r.total_samples != 3 + len2 + 101 + len0 + 7) FAIL("packed sizes at 16 kHz");
    {
        const uint32_t rate = (uint32_t)r.bytes[24] | ((uint32_t)r.bytes[25] << 8) | ((uint32_t)r.bytes[26] << 16) | ((uint32_t)r.bytes[27] << 24);
        const uint32_t bps = (uint32_t)r.bytes[28] | ((uint32_t)r.bytes[29] << 8) | ((uint32_t)r.bytes[30] << 16) | ((uint32_t)r.bytes[31] << 24);
        if (rate != 16000u || bps != 32000u) FAIL("the RIFF header does not carry the output rate");
        printf("header rate %u total %lld\n", (unsigned)rate, (long long)r.total_samples);
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(r.bytes, 1, r.n_bytes, f);
    fclose(f);
    mi355vits_free_packed(&r);
    mi355vits_destroy(h);
    return 0;
}
