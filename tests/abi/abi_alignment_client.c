/* A plain-C client of the alignment calls of include/mi355vits.h (mi355vits_fetch_alignment, mi355vits_free_alignment): runs a
 * tiny voice, fetches the phoneme timing with levels and checks that the spans tile every row — against whatever libmi355vits*.so
 * it is linked with.
 * usage: abi_alignment_client <voice.m355> */
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
    mi355vits_alignment al;

    /* before any run: an error code and the message of the contract, nothing to free */
    rc = mi355vits_fetch_alignment(h, 0, &al);
    if (rc != MI355VITS_ERR_INVALID || al.frames != NULL || al.owner_ != NULL) FAIL("fetch_alignment before any run must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    if (mi355vits_fetch_alignment(h, 0, NULL) != MI355VITS_ERR_INVALID) FAIL("a NULL out must fail");

    int64_t ids[15] = {3, 7, 1, 9, 4, 5, 2, 0, 0, 0, 8, 6, 4, 2, 0};
    int64_t lengths[3] = {5, 2, 4};
    int64_t sid[3] = {0, 0, 0};
    float scales[3] = {0.0f, 1.0f, 0.0f};
    mi355vits_run_args a;
    memset(&a, 0, sizeof a);
    a.batch = 3; a.tx_max = 5; a.ids = ids; a.lengths = lengths; a.scales = scales;
    a.sid = cfg.n_speakers > 1 ? sid : NULL;
    a.flags = MI355VITS_WANT_FLOAT;
    mi355vits_result res;
    rc = mi355vits_run(h, &a, &res);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run: %d %s\n", rc, mi355vits_last_error(h)); return 1; }

    if (mi355vits_fetch_alignment(h, 2u, &al) != MI355VITS_ERR_INVALID) FAIL("unknown bits in want must fail");
    rc = mi355vits_fetch_alignment(h, 0, &al);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_alignment: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (al.peak != NULL || al.rms != NULL || al.frames == NULL) FAIL("without MI355VITS_ALIGN_LEVELS peak and rms are NULL");
    mi355vits_free_alignment(&al);
    if (al.frames != NULL || al.owner_ != NULL) FAIL("free_alignment must clear the struct");
    mi355vits_free_alignment(&al); /* freeing twice is harmless */

    rc = mi355vits_fetch_alignment(h, MI355VITS_ALIGN_LEVELS, &al);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_alignment: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (al.batch != 3 || al.tx_max != 5 || al.sample_rate != cfg.sample_rate) FAIL("batch / tx_max / sample_rate");
    if (al.peak == NULL || al.rms == NULL) FAIL("levels asked for and not given");
    int b, t;
    for (b = 0; b < 3; ++b) {
        int64_t pos = 0, frames = 0;
        float top = 0.0f;
        for (t = 0; t < 5; ++t) {
            const int i = b * 5 + t;
            if (al.start[i] != pos) FAIL("the spans do not tile the row");
            if (al.samples[i] != (int32_t)(al.frames[i] * cfg.hop_length)) FAIL("native run: samples = frames * hop");
            if (t >= lengths[b] && (al.frames[i] != 0 || al.samples[i] != 0 || al.peak[i] != 0.0f || al.rms[i] != 0.0f)) FAIL("padded positions");
            if (al.samples[i] > 0 && !(al.rms[i] <= al.peak[i])) FAIL("rms above peak");
            if (al.peak[i] > top) top = al.peak[i];
            pos += al.samples[i];
            frames += al.frames[i];
        }
        if (pos != res.lengths[b]) FAIL("the spans do not sum to lengths[b]");
        if (frames > 0 && top != res.peaks[b]) FAIL("max_t peak != peaks[b]");
        /* the levels are those of the float waveform */
        {
            const int i = b * 5;
            float pk = 0.0f;
            int k;
            for (k = al.start[i]; k < al.start[i] + al.samples[i]; ++k) {
                const float v = res.audio[b * res.l_max + k];
                if (v > pk) pk = v;
                if (-v > pk) pk = -v;
            }
            if (pk != al.peak[i]) FAIL("peak of phoneme 0 is not max |audio| over its span");
        }
    }
    printf("alignment ok: %d x %d at %d Hz\n", (int)al.batch, (int)al.tx_max, (int)al.sample_rate);
    mi355vits_free_alignment(&al);
    mi355vits_free_result(&res);
    mi355vits_destroy(h);
    return 0;
}
