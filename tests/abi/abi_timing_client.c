/* A plain-C client of the timing call of include/mi355vits.h (mi355vits_run_timed, mi355vits_timing_args): runs a tiny voice plain,
 * then fitted to a number of frames per row with one phoneme held and one stretched, and checks lengths, the alignment's frames and
 * the refusals — against whatever libmi355vits*.so it is linked with.
 * usage: abi_timing_client <voice.m355> */
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

    int64_t ids[15] = {3, 7, 1, 9, 4, 5, 2, 0, 0, 0, 8, 6, 4, 2, 0};
    int64_t lengths[3] = {5, 2, 4};
    int64_t sid[3] = {0, 0, 0};
    float scales[3] = {0.0f, 1.0f, 0.0f};
    mi355vits_run_args a;
    memset(&a, 0, sizeof a);
    a.batch = 3; a.tx_max = 5; a.ids = ids; a.lengths = lengths; a.scales = scales;
    a.sid = cfg.n_speakers > 1 ? sid : NULL;
    a.flags = MI355VITS_WANT_PCM16;
    mi355vits_result plain, res;
    rc = mi355vits_run_rows(h, &a, NULL, &plain);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_rows: %d %s\n", rc, mi355vits_last_error(h)); return 1; }

    /* NULL timing, and a struct without inputs: the plain call */
    mi355vits_timing_args t;
    memset(&t, 0, sizeof t);
    float factor[3] = {-1.0f, -1.0f, -1.0f};
    int pass, b, i;
    for (pass = 0; pass < 2; ++pass) {
        t.factor_out = pass ? factor : NULL;
        rc = mi355vits_run_timed(h, &a, NULL, pass ? &t : NULL, &res);
        if (rc != MI355VITS_OK) { fprintf(stderr, "run_timed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
        if (res.l_max != plain.l_max || memcmp(res.lengths, plain.lengths, sizeof(int64_t) * 3) != 0 ||
            memcmp(res.pcm, plain.pcm, sizeof(int16_t) * 3 * (size_t)plain.l_max) != 0)
            FAIL("run_timed without timing inputs is not run_rows");
        mi355vits_free_result(&res);
    }
    if (factor[0] != 1.0f || factor[1] != 1.0f || factor[2] != 1.0f) FAIL("factor_out without a target must read 1");

    /* fitted: rows 0 and 2 to a length, row 1 as predicted; a phoneme held, a phoneme stretched */
    float stretch[15];
    int32_t min_frames[15];
    int32_t target[3];
    for (i = 0; i < 15; ++i) { stretch[i] = 1.0f; min_frames[i] = 0; }
    stretch[1] = 2.5f;
    min_frames[12] = 9;
    target[0] = (int32_t)(plain.lengths[0] / cfg.hop_length) + 11;
    target[1] = 0;
    target[2] = 40;
    t.stretch = stretch; t.min_frames = min_frames; t.target_frames = target; t.factor_out = factor;
    rc = mi355vits_run_timed(h, &a, NULL, &t, &res);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_timed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (res.lengths[0] != (int64_t)target[0] * cfg.hop_length || res.lengths[2] != (int64_t)40 * cfg.hop_length) FAIL("lengths != target * hop");
    if (res.lengths[1] != plain.lengths[1]) FAIL("a row without a target keeps its length");
    if (!(factor[0] > 0.0f) || factor[1] != 1.0f || !(factor[2] > 0.0f)) FAIL("factor_out");
    mi355vits_alignment al;
    rc = mi355vits_fetch_alignment(h, 0, &al);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_alignment: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    for (b = 0; b < 3; ++b) {
        int64_t sum = 0;
        for (i = 0; i < 5; ++i) sum += al.frames[b * 5 + i];
        if (target[b] && sum != target[b]) FAIL("the fitted frames do not sum to the target");
    }
    if (al.frames[12] < 9) FAIL("min_frames not held");
    mi355vits_free_alignment(&al);
    mi355vits_free_result(&res);

    /* refusals: the result struct is left zeroed, the message names what is wrong */
    a.forced_durations = min_frames;
    rc = mi355vits_run_timed(h, &a, NULL, &t, &res);
    if (rc != MI355VITS_ERR_INVALID || res.pcm != NULL || res.owner_ != NULL) FAIL("timing with forced_durations must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    a.forced_durations = NULL;
    t.reserved[5] = 1;
    rc = mi355vits_run_timed(h, &a, NULL, &t, &res);
    if (rc != MI355VITS_ERR_INVALID) FAIL("a non-zero reserved field must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    t.reserved[5] = 0;
    target[2] = 3; /* four phonemes: at least four frames */
    rc = mi355vits_run_timed(h, &a, NULL, &t, &res);
    if (rc != MI355VITS_ERR_INVALID || res.owner_ != NULL) FAIL("a target below the floor must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));

    printf("timing ok\n");
    mi355vits_free_result(&plain);
    mi355vits_destroy(h);
    return 0;
}
