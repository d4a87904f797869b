/* A plain-C client of the true-peak calls of include/mi355vits.h (mi355vits_set_loudness_ceiling_mode,
 * mi355vits_get_loudness_ceiling_mode, mi355vits_fetch_true_peak, mi355vits_free_true_peak): runs a tiny voice, fetches its
 * oversampled peaks and checks the gain rule of both ceiling modes against them — against whatever libmi355vits*.so it is linked with.
 * usage: abi_true_peak_client <voice.m355> */
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
    mi355vits_true_peak tp;

    if (mi355vits_get_loudness_ceiling_mode(h) != MI355VITS_CEILING_SAMPLE) FAIL("the default mode is the sample peak");
    /* before any run: an error code and the message of the contract, nothing to free */
    rc = mi355vits_fetch_true_peak(h, &tp);
    if (rc != MI355VITS_ERR_INVALID || tp.true_peak != NULL || tp.owner_ != NULL) FAIL("fetch_true_peak before any run must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    if (mi355vits_fetch_true_peak(h, NULL) != MI355VITS_ERR_INVALID) FAIL("a NULL out must fail");
    if (mi355vits_set_loudness_ceiling_mode(h, MI355VITS_CEILING_TRUE_PEAK) != MI355VITS_OK) FAIL("set true peak");
    if (mi355vits_set_loudness_ceiling_mode(h, 7) != MI355VITS_ERR_INVALID) FAIL("an unknown mode must fail");
    printf("expected failure msg=%s\n", mi355vits_last_error(h));
    if (mi355vits_get_loudness_ceiling_mode(h) != MI355VITS_CEILING_TRUE_PEAK) FAIL("a refused setting must leave the old one");
    if (mi355vits_set_loudness_ceiling_mode(h, MI355VITS_CEILING_SAMPLE) != MI355VITS_OK) FAIL("back to the sample peak");

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

    /* measured whatever the mode */
    rc = mi355vits_fetch_true_peak(h, &tp);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_true_peak: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (tp.batch != 3 || tp.sample_rate != cfg.sample_rate) FAIL("batch / sample_rate");
    int b;
    double tps[3];
    for (b = 0; b < 3; ++b) {
        if (memcmp(&tp.peak[b], &res.peaks[b], sizeof(float)) != 0) FAIL("peak is bitwise the run's");
        if (!(tp.true_peak[b] >= (double)res.peaks[b])) FAIL("tp >= peak");
        tps[b] = tp.true_peak[b];
    }
    mi355vits_free_true_peak(&tp);
    if (tp.true_peak != NULL || tp.peak != NULL || tp.owner_ != NULL) FAIL("free_true_peak must clear the struct");
    mi355vits_free_true_peak(&tp); /* freeing twice is harmless */

    /* the gain rule of the two modes, limiter off: cap = c / peak, cap = c / tp */
    int mode;
    for (mode = 0; mode < 2; ++mode) {
        mi355vits_loudness ld;
        if (mi355vits_set_loudness_ceiling_mode(h, mode) != MI355VITS_OK) FAIL("set mode");
        if (mi355vits_set_loudness_target(h, -10.0f, -6.0f) != MI355VITS_OK) FAIL("set -10 / -6");
        rc = mi355vits_fetch_loudness(h, &ld);
        if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_loudness: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
        for (b = 0; b < 3; ++b) {
            double g = isinf(ld.lufs[b]) ? 1.0 : pow(10.0, (-10.0 - ld.lufs[b]) / 20.0);
            const double p = mode ? tps[b] : (double)res.peaks[b];
            int limited = 0;
            if (p != 0.0) {
                const double cap = pow(10.0, -6.0 / 20.0) / p;
                if (cap < g) { g = cap; limited = 1; }
            }
            if (fabs(ld.gain[b] - g) > 1e-12 * g || ld.limited[b] != limited) FAIL("the gain rule of the mode");
        }
        mi355vits_free_loudness(&ld);
    }
    mi355vits_free_result(&res);
    mi355vits_destroy(h);
    printf("true peak ok\n");
    return 0;
}
