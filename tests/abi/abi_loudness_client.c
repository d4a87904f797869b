/* A plain-C client of the loudness calls of include/mi355vits.h (mi355vits_set_loudness_target, mi355vits_get_loudness_target,
 * mi355vits_fetch_loudness, mi355vits_free_loudness): runs a tiny voice, measures it, packs it at a target and checks every int16
 * sample of the stream against the rule of the header — against whatever libmi355vits*.so it is linked with.
 * usage: abi_loudness_client <voice.m355> */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355vits.h"

#define FAIL(msg) do { fprintf(stderr, "%s\n", msg); return 1; } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    mi355vits_handle h = NULL;
    int rc = mi355vits_create(argv[1], 0, &h);
    if (rc != MI355VITS_OK) { fprintf(stderr, "create: %d %s\n", rc, mi355vits_last_error(NULL)); return 1; }
    mi355vits_config cfg;
    if (mi355vits_get_config(h, &cfg) != MI355VITS_OK) return 1;
    mi355vits_loudness ld;
    float t = 1.0f, c = 1.0f;

    if (mi355vits_get_loudness_target(h, &t, &c) != MI355VITS_OK || t != 0.0f) FAIL("the default target is 0 = off");
    /* before any run: an error code and the message of the contract, nothing to free */
    rc = mi355vits_fetch_loudness(h, &ld);
    if (rc != MI355VITS_ERR_INVALID || ld.lufs != NULL || ld.owner_ != NULL) FAIL("fetch_loudness before any run must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    if (mi355vits_fetch_loudness(h, NULL) != MI355VITS_ERR_INVALID) FAIL("a NULL out must fail");
    if (mi355vits_set_loudness_target(h, -16.0f, -2.0f) != MI355VITS_OK) FAIL("set -16 / -2");
    if (mi355vits_set_loudness_target(h, 0.5f, -1.0f) != MI355VITS_ERR_INVALID) FAIL("a positive target must fail");
    printf("expected failure msg=%s\n", mi355vits_last_error(h));
    if (mi355vits_set_loudness_target(h, -16.0f, 1.0f) != MI355VITS_ERR_INVALID) FAIL("a positive ceiling must fail");
    if (mi355vits_get_loudness_target(h, &t, &c) != MI355VITS_OK || t != -16.0f || c != -2.0f) FAIL("a refused setting must leave the old one");
    if (mi355vits_set_loudness_target(h, 0.0f, 0.0f) != MI355VITS_OK) FAIL("back to off");

    int64_t ids[15] = {3, 7, 1, 9, 4, 5, 2, 0, 0, 0, 8, 6, 4, 2, 0};
    int64_t lengths[3] = {5, 2, 4};
    int64_t sid[3] = {0, 0, 0};
    float scales[3] = {0.5f, 1.0f, 0.5f};
    mi355vits_run_args a;
    memset(&a, 0, sizeof a);
    a.batch = 3; a.tx_max = 5; a.ids = ids; a.lengths = lengths; a.scales = scales;
    a.sid = cfg.n_speakers > 1 ? sid : NULL;
    a.flags = MI355VITS_WANT_FLOAT;
    mi355vits_result res;
    rc = mi355vits_run(h, &a, &res);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run: %d %s\n", rc, mi355vits_last_error(h)); return 1; }

    /* off: measured all the same, no gain */
    rc = mi355vits_fetch_loudness(h, &ld);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_loudness: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (ld.batch != 3 || ld.sample_rate != cfg.sample_rate || ld.target_lufs != 0.0f) FAIL("batch / sample_rate / target");
    int b;
    double off_lufs[3];
    for (b = 0; b < 3; ++b) {
        if (ld.gain[b] != 0.0 || ld.limited[b] != 0) FAIL("off: gain 0.0, limited 0");
        if (res.lengths[b] > 0 && ld.blocks[b] < 1) FAIL("a row with samples has a block");
        if (ld.gated[b] > ld.blocks[b]) FAIL("gated above blocks");
        off_lufs[b] = ld.lufs[b];
    }
    mi355vits_free_loudness(&ld);
    if (ld.lufs != NULL || ld.owner_ != NULL) FAIL("free_loudness must clear the struct");
    mi355vits_free_loudness(&ld); /* freeing twice is harmless */

    /* on: the gain rule and the stream's samples */
    if (mi355vits_set_loudness_target(h, -23.0f, -1.0f) != MI355VITS_OK) FAIL("set -23 / -1");
    mi355vits_packed_result pk;
    rc = mi355vits_fetch_packed(h, NULL, &pk);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    rc = mi355vits_fetch_loudness(h, &ld);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_loudness: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (ld.target_lufs != -23.0f || ld.ceiling_dbfs != -1.0f) FAIL("the setting the arrays were made with");
    for (b = 0; b < 3; ++b) {
        if (memcmp(&ld.lufs[b], &off_lufs[b], sizeof(double)) != 0) FAIL("lufs does not depend on the target");
        double g = isinf(ld.lufs[b]) ? 1.0 : pow(10.0, (-23.0 - ld.lufs[b]) / 20.0);
        int limited = 0;
        if (res.peaks[b] != 0.0f) {
            const double cap = pow(10.0, -1.0 / 20.0) / (double)res.peaks[b];
            if (cap < g) { g = cap; limited = 1; }
        }
        if (fabs(ld.gain[b] - g) > 1e-12 * g || ld.limited[b] != limited) FAIL("the gain rule");
        if (pk.lengths[b] != res.lengths[b] || pk.peaks[b] != res.peaks[b]) FAIL("lengths and peaks stay the row's");
        const float scale = (float)(32767.0 * ld.gain[b]);
        int64_t k;
        for (k = 0; k < pk.lengths[b]; ++k) {
            float v = res.audio[b * res.l_max + k] * scale;
            if (v > 32767.0f) v = 32767.0f;
            if (v < -32767.0f) v = -32767.0f;
            if (pk.pcm[pk.offsets[b] + k] != (int16_t)v) FAIL("a sample is not (int16)clamp(x * (float)(32767 * gain))");
        }
    }
    printf("loudness ok: %d rows at %d Hz, %.3f LUFS, gain %.4f\n", (int)ld.batch, (int)ld.sample_rate, ld.lufs[0], ld.gain[0]);
    mi355vits_free_loudness(&ld);
    mi355vits_free_packed(&pk);
    mi355vits_free_result(&res);
    mi355vits_destroy(h);
    return 0;
}
