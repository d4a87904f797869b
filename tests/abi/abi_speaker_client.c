/* A plain-C client of the speakers call of include/mi355vits.h (mi355vits_run_speakers, mi355vits_speaker_args,
 * mi355vits_get_speaker_embedding): runs a tiny multi-speaker voice plain, then with one-term mixes, with the table rows as
 * vectors and with a blend, and checks the identities and the refusals — against whatever libmi355vits*.so it is linked with.
 * usage: abi_speaker_client <voice.m355>   (a voice with 3 speakers) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355vits.h"

#define FAIL(msg) do { fprintf(stderr, "%s\n", msg); return 1; } while (0)

static int same(const mi355vits_result* x, const mi355vits_result* y) {
    return x->l_max == y->l_max && memcmp(x->lengths, y->lengths, sizeof(int64_t) * 3) == 0 &&
           memcmp(x->pcm, y->pcm, sizeof(int16_t) * 3 * (size_t)y->l_max) == 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    mi355vits_handle h = NULL;
    int rc = mi355vits_create(argv[1], 0, &h);
    if (rc != MI355VITS_OK) { fprintf(stderr, "create: %d %s\n", rc, mi355vits_last_error(NULL)); return 1; }
    mi355vits_config cfg;
    if (mi355vits_get_config(h, &cfg) != MI355VITS_OK) return 1;
    if (cfg.n_speakers != 3 || cfg.gin_channels < 1 || cfg.gin_channels > 64) FAIL("a voice with 3 speakers is expected");
    const int gin = cfg.gin_channels;

    int64_t ids[15] = {3, 7, 1, 9, 4, 5, 2, 0, 0, 0, 8, 6, 4, 2, 0};
    int64_t lengths[3] = {5, 2, 4};
    int64_t sid[3] = {2, 0, 1};
    float scales[3] = {0.0f, 1.0f, 0.0f};
    mi355vits_run_args a;
    memset(&a, 0, sizeof a);
    a.batch = 3; a.tx_max = 5; a.ids = ids; a.lengths = lengths; a.scales = scales; a.sid = sid;
    a.flags = MI355VITS_WANT_PCM16;
    mi355vits_result plain, res;
    rc = mi355vits_run_rows(h, &a, NULL, &plain);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_rows: %d %s\n", rc, mi355vits_last_error(h)); return 1; }

    /* NULL speakers: the plain call */
    rc = mi355vits_run_speakers(h, &a, NULL, NULL, NULL, &res);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_speakers: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (!same(&res, &plain)) FAIL("run_speakers without speakers is not run_rows");
    mi355vits_free_result(&res);

    /* one-term mixes of weight 1 behind a skipped term; args.sid is not read */
    int64_t mix_sid[6] = {999, 2, -4, 0, 12345, 1};
    float mix_w[6] = {0.0f, 1.0f, 0.0f, 1.0f, 0.0f, 1.0f};
    mi355vits_speaker_args s;
    memset(&s, 0, sizeof s);
    s.n_terms = 2; s.mix_sid = mix_sid; s.mix_weight = mix_w;
    a.sid = NULL;
    rc = mi355vits_run_speakers(h, &a, NULL, NULL, &s, &res);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_speakers (mix): %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (!same(&res, &plain)) FAIL("a one-term mix of weight 1 is not the plain run");
    mi355vits_free_result(&res);

    /* the table rows as vectors */
    float vec[3 * 64];
    int b;
    for (b = 0; b < 3; ++b) {
        rc = mi355vits_get_speaker_embedding(h, sid[b], vec + b * gin, (size_t)gin);
        if (rc != MI355VITS_OK) { fprintf(stderr, "get_speaker_embedding: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    }
    memset(&s, 0, sizeof s);
    s.vectors = vec;
    rc = mi355vits_run_speakers(h, &a, NULL, NULL, &s, &res);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_speakers (vectors): %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (!same(&res, &plain)) FAIL("vectors equal to the table rows are not the plain run");
    mi355vits_free_result(&res);

    /* a blend: another voice than either speaker, the same lengths of the other rows */
    memset(&s, 0, sizeof s);
    mix_sid[0] = 0; mix_w[0] = 0.5f; mix_w[1] = 0.5f;
    s.n_terms = 2; s.mix_sid = mix_sid; s.mix_weight = mix_w;
    rc = mi355vits_run_speakers(h, &a, NULL, NULL, &s, &res);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_speakers (blend): %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (res.lengths[1] != plain.lengths[1] || res.lengths[2] != plain.lengths[2]) FAIL("rows 1 and 2 keep their speakers");
    if (res.l_max == plain.l_max && memcmp(res.pcm, plain.pcm, sizeof(int16_t) * (size_t)plain.lengths[0]) == 0) FAIL("the blend did not change row 0");
    mi355vits_free_result(&res);

    /* refusals: the result struct is left zeroed, the message names what is wrong */
    mix_sid[3] = 3; /* row 1, term 1 */
    rc = mi355vits_run_speakers(h, &a, NULL, NULL, &s, &res);
    if (rc != MI355VITS_ERR_INVALID || res.pcm != NULL || res.owner_ != NULL) FAIL("a speaker id outside the table must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    mix_sid[3] = 0;
    mix_w[0] = 0.0f; mix_w[1] = 0.0f;
    rc = mi355vits_run_speakers(h, &a, NULL, NULL, &s, &res);
    if (rc != MI355VITS_ERR_INVALID || res.owner_ != NULL) FAIL("a row whose every weight is 0 must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    rc = mi355vits_get_speaker_embedding(h, 0, vec, (size_t)gin - 1);
    if (rc != MI355VITS_ERR_INVALID) FAIL("a capacity below gin_channels must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    /* the previous run is still served */
    rc = mi355vits_fetch(h, MI355VITS_WANT_PCM16, &res);
    if (rc != MI355VITS_OK || res.lengths[1] != plain.lengths[1]) FAIL("the previous run must stay served");
    mi355vits_free_result(&res);

    printf("speakers ok\n");
    mi355vits_free_result(&plain);
    mi355vits_destroy(h);
    return 0;
}
