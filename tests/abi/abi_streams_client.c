/* A plain-C client of the streams calls of include/mi355vits.h (mi355vits_run_streams, mi355vits_fetch_streams,
 * mi355vits_free_streams): runs a tiny voice, takes its rows as two streams of one block and checks headers, sizes, pointers and the
 * error path — against whatever libmi355vits*.so it is linked with.
 * usage: abi_streams_client <voice.m355> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355vits.h"

#define FAIL(msg) do { fprintf(stderr, "%s\n", msg); return 1; } while (0)

static uint32_t u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    mi355vits_handle h = NULL;
    int rc = mi355vits_create(argv[1], 0, &h);
    if (rc != MI355VITS_OK) { fprintf(stderr, "create: %d %s\n", rc, mi355vits_last_error(NULL)); return 1; }
    mi355vits_config cfg;
    if (mi355vits_get_config(h, &cfg) != MI355VITS_OK) return 1;

    int32_t order0[2] = {2, 0}, order1[1] = {1};
    int64_t lead0[2] = {3, 100}, lead1[1] = {1};
    mi355vits_stream_args st[2];
    memset(st, 0, sizeof st);
    st[0].pack.n = 2; st[0].pack.order = order0; st[0].pack.lead_samples = lead0; st[0].pack.tail_samples = 7; st[0].pack.wav_header = 1;
    st[0].encoding = MI355VITS_ENC_S16LE;
    st[1].pack.n = 1; st[1].pack.order = order1; st[1].pack.lead_samples = lead1; st[1].pack.wav_header = 1;
    st[1].encoding = MI355VITS_ENC_ULAW;
    mi355vits_streams_result sr;

    /* before any run: an error code and the message of the contract, nothing to free */
    rc = mi355vits_fetch_streams(h, st, 2, &sr);
    if (rc != MI355VITS_ERR_INVALID || sr.bytes != NULL || sr.owner_ != NULL) FAIL("fetch_streams before any run must fail");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));

    int64_t ids[15] = {3, 7, 1, 9, 4, 5, 2, 0, 0, 0, 8, 6, 4, 2, 0};
    int64_t lengths[3] = {5, 2, 4};
    int64_t sid[3] = {0, 0, 0};
    float scales[3] = {0.5f, 1.0f, 0.5f};
    mi355vits_run_args a;
    memset(&a, 0, sizeof a);
    a.batch = 3; a.tx_max = 5; a.ids = ids; a.lengths = lengths; a.scales = scales;
    a.sid = cfg.n_speakers > 1 ? sid : NULL;

    if (mi355vits_run_streams(h, &a, NULL, NULL, 2, &sr) != MI355VITS_ERR_INVALID) FAIL("a NULL array must fail");
    if (mi355vits_run_streams(h, &a, NULL, st, 0, &sr) != MI355VITS_ERR_INVALID) FAIL("n_streams < 1 must fail");
    if (mi355vits_run_streams(h, &a, NULL, st, 2, NULL) != MI355VITS_ERR_INVALID) FAIL("a NULL out must fail");
    order1[0] = 7;
    rc = mi355vits_run_streams(h, &a, NULL, st, 2, &sr);
    if (rc != MI355VITS_ERR_INVALID || sr.bytes != NULL || sr.owner_ != NULL) FAIL("a bad row must fail and leave nothing to free");
    printf("expected failure rc=%d msg=%s\n", rc, mi355vits_last_error(h));
    order1[0] = 1;

    rc = mi355vits_run_streams(h, &a, NULL, st, 2, &sr);
    if (rc != MI355VITS_OK) { fprintf(stderr, "run_streams: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (sr.n_streams != 2 || sr.n_entries != 3 || sr.entry_base[0] != 0 || sr.entry_base[1] != 2 || sr.entry_base[2] != 3) FAIL("streams / entries");
    if (sr.rows[0] != 2 || sr.rows[1] != 0 || sr.rows[2] != 1) FAIL("rows");
    if (sr.encoding[0] != MI355VITS_ENC_S16LE || sr.encoding[1] != MI355VITS_ENC_ULAW) FAIL("encodings");
    if (sr.data_offset[0] % 16 != 0 || sr.data_offset[1] % 16 != 0) FAIL("data starts at a multiple of 16");
    if (sr.data_offset[0] - sr.stream_offset[0] != 44 || sr.data_offset[1] - sr.stream_offset[1] != 58) FAIL("44- and 58-byte headers");
    if (sr.offsets[0] != 3 || sr.offsets[1] != 3 + sr.lengths[0] + 100 || sr.offsets[2] != 1) FAIL("offsets count samples within the stream");
    if (sr.total_samples[0] != sr.offsets[1] + sr.lengths[1] + 7 || sr.total_samples[1] != 1 + sr.lengths[2]) FAIL("total_samples");
    const int64_t data1 = sr.total_samples[1];
    if (sr.stream_bytes[0] != 44 + 2 * sr.total_samples[0] || sr.stream_bytes[1] != 58 + data1 + (data1 & 1)) FAIL("stream_bytes");
    if (sr.stream_offset[1] < sr.stream_offset[0] + sr.stream_bytes[0]) FAIL("streams do not overlap");
    if ((int64_t)sr.n_bytes != sr.stream_offset[1] + sr.stream_bytes[1]) FAIL("the block ends with its last stream");
    if (sr.first[0] != 0 || sr.gain[0] != 0.0 || sr.limited[0] != 0) FAIL("untrimmed, no target: first 0, gain 0");
    const uint8_t* f0 = sr.bytes + sr.stream_offset[0];
    const uint8_t* f1 = sr.bytes + sr.stream_offset[1];
    if (memcmp(f0, "RIFF", 4) || memcmp(f0 + 8, "WAVEfmt ", 8) || memcmp(f0 + 36, "data", 4)) FAIL("stream 0: RIFF tags");
    if (u32(f0 + 4) != 36 + 2 * sr.total_samples[0] || u32(f0 + 40) != 2 * sr.total_samples[0] || u32(f0 + 24) != (uint32_t)cfg.sample_rate) FAIL("stream 0: sizes / rate");
    if (memcmp(f1, "RIFF", 4) || memcmp(f1 + 38, "fact", 4) || memcmp(f1 + 50, "data", 4) || f1[20] != 7) FAIL("stream 1: non-PCM form, tag 7");
    if (u32(f1 + 4) != 50 + data1 + (data1 & 1) || u32(f1 + 46) != data1 || u32(f1 + 54) != data1) FAIL("stream 1: sizes");
    int64_t k;
    for (k = 0; k < sr.stream_offset[0]; ++k) if (sr.bytes[k]) FAIL("bytes in front of the first header are zero");
    for (k = sr.stream_offset[0] + sr.stream_bytes[0]; k < sr.stream_offset[1]; ++k) if (sr.bytes[k]) FAIL("the gap between the streams is zero");
    if (sr.bytes[sr.data_offset[1]] != 0xFF) FAIL("mu-law silence is 0xFF");

    /* each stream is what fetch_packed returns with the handle set to its encoding */
    int s;
    for (s = 0; s < 2; ++s) {
        mi355vits_packed_result pk;
        if (mi355vits_set_output_encoding(h, st[s].encoding) != MI355VITS_OK) FAIL("set_output_encoding");
        rc = mi355vits_fetch_packed(h, &st[s].pack, &pk);
        if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_packed: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
        if ((int64_t)pk.n_bytes != sr.stream_bytes[s] || memcmp(pk.bytes, sr.bytes + sr.stream_offset[s], pk.n_bytes)) FAIL("a stream is not its fetch_packed twin");
        mi355vits_free_packed(&pk);
    }
    mi355vits_set_output_encoding(h, MI355VITS_ENC_S16LE);

    mi355vits_streams_result again;
    rc = mi355vits_fetch_streams(h, st, 2, &again);
    if (rc != MI355VITS_OK) { fprintf(stderr, "fetch_streams: %d %s\n", rc, mi355vits_last_error(h)); return 1; }
    if (again.n_bytes != sr.n_bytes || memcmp(again.bytes, sr.bytes, sr.n_bytes) || again.bytes == sr.bytes) FAIL("fetch_streams: the same block, its own memory");
    mi355vits_free_streams(&again);
    printf("streams ok: %d streams, %d entries, %ld bytes\n", (int)sr.n_streams, (int)sr.n_entries, (long)sr.n_bytes);
    mi355vits_free_streams(&sr);
    if (sr.bytes != NULL || sr.owner_ != NULL) FAIL("free_streams must clear the struct");
    mi355vits_free_streams(&sr); /* freeing twice is harmless */
    mi355vits_destroy(h);
    return 0;
}
