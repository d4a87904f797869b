/* A plain-C client of the packed-result calls of include/mi355vits.h (mi355vits_run_packed, mi355vits_fetch_packed,
 * mi355vits_free_packed): proves that part of the header is C99 too and checks the offsets / n_bytes arithmetic of the result
 * against whatever libmi355vits*.so it is linked with.
 * usage: abi_packed_client <voice.m355> <out.wav>   (three rows, packed in the order 2, 0 with silences and a header) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355vits.h"

#define FAIL(msg) do { fprintf(stderr, "%s\n", msg); return 1; } while (0)

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    printf("sizeof pack_args %zu packed_result %zu\n", sizeof(mi355vits_pack_args), sizeof(mi355vits_packed_result));
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
    a.flags = MI355VITS_WANT_FLOAT; /* ignored by the packed call */
    mi355vits_packed_result r;
    int i;

    /* default pack: every row, in order, no silence, no header */
    rc = mi355vits_run_packed(h, &a, NULL, NULL, &r);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (r.n != 3 || r.offsets[0] != 0 || (uint8_t*)r.pcm != r.bytes) FAIL("default pack: n / offsets[0] / pcm");
    for (i = 0; i + 1 < r.n; ++i)
        if (r.offsets[i + 1] != r.offsets[i] + r.lengths[i]) FAIL("default pack: offsets are not cumulative");
    if (r.total_samples != r.offsets[2] + r.lengths[2] || r.n_bytes != 2 * (size_t)r.total_samples) FAIL("default pack: sizes");
    printf("default total %lld\n", (long long)r.total_samples);
    int64_t len0 = r.lengths[0], len2 = r.lengths[2];
    mi355vits_free_packed(&r);
    if (r.bytes != NULL || r.owner_ != NULL) FAIL("free_packed left pointers behind");

    /* rows 2, 0 with 3 and 101 samples of silence in front, 7 behind, and a header */
    int32_t order[2] = {2, 0};
    int64_t lead[2] = {3, 101};
    mi355vits_pack_args p;
    memset(&p, 0, sizeof p);
    p.n = 2; p.order = order; p.lead_samples = lead; p.tail_samples = 7; p.wav_header = 1;
    rc = mi355vits_run_packed(h, &a, NULL, &p, &r);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (r.n != 2 || r.lengths[0] != len2 || r.lengths[1] != len0) FAIL("ordered pack: lengths");
    if (r.offsets[0] != 3 || r.offsets[1] != 3 + len2 + 101) FAIL("ordered pack: offsets");
    if (r.total_samples != 3 + len2 + 101 + len0 + 7) FAIL("ordered pack: total_samples");
    if (r.n_bytes != 44 + 2 * (size_t)r.total_samples || (uint8_t*)r.pcm != r.bytes + 44) FAIL("ordered pack: n_bytes / pcm");
    if (memcmp(r.bytes, "RIFF", 4) != 0 || memcmp(r.bytes + 8, "WAVEfmt ", 8) != 0 || memcmp(r.bytes + 36, "data", 4) != 0)
        FAIL("ordered pack: header");
    for (i = 0; i < 3; ++i) if (r.pcm[i] != 0) FAIL("lead silence is not zero");
    for (i = 0; i < 7; ++i) if (r.pcm[r.total_samples - 1 - i] != 0) FAIL("tail silence is not zero");
    printf("ordered total %lld peaks %.6f %.6f\n", (long long)r.total_samples, r.peaks[0], r.peaks[1]);
    FILE* f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(r.bytes, 1, r.n_bytes, f);
    fclose(f);
    mi355vits_free_packed(&r);

    /* the same spec through fetch_packed: nothing is synthesised again */
    rc = mi355vits_fetch_packed(h, &p, &r);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (r.n_bytes != 44 + 2 * (size_t)(3 + len2 + 101 + len0 + 7)) FAIL("fetch_packed: n_bytes");
    mi355vits_free_packed(&r);

    /* a row twice -> error code and a message that names the entry; the handle stays usable */
    order[1] = 2;
    rc = mi355vits_run_packed(h, &a, NULL, &p, &r);
    if (rc != MI355VITS_ERR_INVALID || r.bytes != NULL) { fprintf(stderr, "a row twice gave rc=%d\n", rc); return 1; }
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    mi355vits_destroy(h);
    return 0;
}
