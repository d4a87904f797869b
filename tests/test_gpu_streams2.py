"""Device twin of tests/test_streams2.py (pytest -m gpu): streams v2 on the MI355X — compression, limiter window and ceiling mode per
stream of one block (mi355vits_run_streams2 / mi355vits_fetch_streams2; k_flac_place, k_flac_gather_streams).  The same shapes and the
same yardsticks: ``fetch_packed`` of the same run under the handle's six setters, ``flac_ref``, the v1 ``fetch_streams``.  The 70-stream
block has more than 1,536 frames, so every k_flac_frames workgroup (the grid is three per CU, 768) makes several trips across job
boundaries, and its 72 streams exceed a wave in k_flac_place."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_cases as C  # noqa: E402
import flac_ref as F  # noqa: E402
import streams2_cases as S2  # noqa: E402

from mimic3_amd import postprocess as PP  # noqa: E402
from mimic3_amd._native import Engine  # noqa: E402
from tests.test_packed_streams import SCALES, _blob, _inputs, _requests, _run_kw, _session  # noqa: E402
from tests.test_streams2 import _all_requests, _s16_twins, _same_result, check_more_jobs_than_the_lds_holds, many_streams  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def served(gpu_lib):
    cfg, blob = _blob()
    eng = Engine(blob, device=0, library=gpu_lib)
    ids, lens = _inputs(cfg)
    out = eng.run(ids, lens, SCALES, None, want_float=True, want_pcm16=True, **_run_kw())
    yield eng, (ids, lens), out, cfg
    eng.close()


def test_seven_streams_are_their_twins(served):
    eng, _, _, cfg = served
    got = eng.fetch_streams(S2.SEVEN)
    _, twins = S2.check_against_twins(eng, S2.SEVEN, got)
    assert twins[3].limited.any() and twins[4].limited.any()
    assert len({bytes(twins[3].flac), twins[4].data.tobytes(), twins[5].data.tobytes()}) == 3
    S2.check_flac_streams_decode(got, _s16_twins(eng, S2.SEVEN), cfg.sample_rate)
    # [0, R) is the v1 block of the uncompressed subset under one window among them
    streams = [dict(st) for st in S2.SEVEN]
    streams[5] = dict(streams[5], limiter=8)
    got = eng.fetch_streams(streams)
    S2.check_against_twins(eng, streams, got)
    eng.set_loudness_limiter(8)
    try:
        v1 = eng.fetch_streams([S2.v1_of(st) for st in streams if st.get("compression") != "flac"])
    finally:
        eng.set_loudness_limiter(0)
    R = got[0].uncompressed_bytes
    assert R == v1[0].block.shape[0] and got[0].block[:R].tobytes() == v1[0].block.tobytes()


def test_v2_without_new_fields_is_v1(gpu_lib):
    cfg, blob = _blob()
    ids, lens = _inputs(cfg)
    eng = Engine(blob, device=0, library=gpu_lib)
    eng.profile_enable(True)
    v1 = [dict(order=[3], lead_samples=[1], wav=True, encoding="ulaw"), dict(order=[1, 4], loudness=S2.TARGET, trim=S2.TRIM),
          dict(order=[0, 4], lead_samples=[0, 777], tail_samples=5, wav=True, encoding="f32le"), dict(order=[2], loudness=S2.TARGET)]
    eng.set_loudness_limiter(32)
    eng.set_loudness_ceiling_mode("true_peak")
    v2 = [dict(st, compression=None, limiter=32, true_peak=True) for st in v1]
    reports, blocks = [], []
    for streams in (v1, v2):
        eng.profile_reset()
        blocks.append(eng.run_streams(ids, lens, SCALES, None, streams=streams, **_run_kw())[0].block.tobytes())
        reports.append({k: (v["calls"], v["bytes"]) for k, v in eng.profile_report().items()})
        blocks.append(eng.fetch_streams(streams)[0].block.tobytes())
    assert blocks[0] == blocks[1] == blocks[2] == blocks[3]
    assert reports[0] == reports[1] and "limit" in reports[0] and "truepeak" in reports[0] and "pack.flac" not in reports[1]
    eng.close()


def test_many_streams_many_frames(served):
    eng, _, _, _ = served
    streams = many_streams()
    got = eng.fetch_streams(streams)
    assert sum(pa.frames for pa in got) > 1536 and sum(1 for pa in got if pa.compression == "flac") == 70
    S2.check_against_twins(eng, streams, got)  # frames[] and stream_bytes[] of every file against decode_frames


def test_single_frame_streams(served):
    eng, _, out, cfg = served
    n0, n1 = int(out["lengths"][0]), int(out["lengths"][1])
    streams = [dict(order=[0], compression="flac"), dict(order=[1], tail_samples=4096 - n1, compression="flac"),
               dict(order=[4], tail_samples=4097 - int(out["lengths"][4]), compression="flac")]
    got = eng.fetch_streams(streams)
    S2.check_against_twins(eng, streams, got)
    assert [pa.frames for pa in got] == [1, 1, 2] and [pa.total_samples for pa in got] == [n0, 4096, 4097]
    S2.check_flac_streams_decode(got, _s16_twins(eng, streams), cfg.sample_rate)
    assert got[0].uncompressed_bytes == 0 and got[0].stream_offset == 0


def test_every_byte_has_a_writer(gpu_hooks):
    cfg, blob = _blob()
    ids, lens = _inputs(cfg)
    streams = S2.SEVEN + [dict(order=[4], lead_samples=[9001], compression="flac")]
    clean = Engine(blob, device=0, library=gpu_hooks)
    want = clean.run_streams(ids, lens, SCALES, None, streams=streams, **_run_kw())[0].block.tobytes()
    eng = Engine(blob, device=0, library=gpu_hooks)
    big = np.tile(ids, (2, 2))
    eng.run_streams(big, np.tile(lens * 2, 2), np.tile(SCALES, (2, 1)), None,
                    streams=[dict(loudness=S2.TARGET, trim=S2.TRIM, limiter=32, true_peak=True, lead_samples=[40_000] + [0] * 9, compression="flac"),
                             dict(loudness=S2.TARGET, limiter=8)], seed=1)  # sizes every arena past what the batch needs
    for pattern in (0x7FC00000, 0xA5A5A5A5):
        eng.fill_workspace(pattern)
        got = eng.run_streams(ids, lens, SCALES, None, streams=streams, **_run_kw())
        assert got[0].block.tobytes() == want, hex(pattern)
    S2.check_against_twins(eng, streams, got)
    eng.close()
    clean.close()


def test_hook_files_are_the_yardsticks(gpu_hooks):
    arrays, files = S2.hook_cases()
    block, off, size = gpu_hooks.lab_flac_jobs(arrays, 22050)
    outside = np.ones(block.shape[0], bool)
    at = 0
    for j, want in enumerate(files):
        assert off[j] == at and size[j] == len(want), j
        assert block[off[j]: off[j] + size[j]].tobytes() == want, j
        outside[off[j]: off[j] + size[j]] = False
        at = (int(off[j] + size[j]) + 15) & ~15
    assert block.shape[0] == off[-1] + size[-1] and not block[outside].any()
    # an input at an odd int16 offset is read where it is, as lab_flac reads it; jobs without a sample are their headers
    names = sorted(C.CONTENTS)[:3]
    pairs = [C.reference(name, n) for name, n in zip(names, (4097, 257, 3 * 4096 + 777))]
    for offset in (1, 3, 7):
        arrays = [C.at_int16_offset(x, offset) if j != 1 else x for j, (x, _) in enumerate(pairs)] + [np.zeros(0, np.int16)]
        block, off, size = gpu_hooks.lab_flac_jobs(arrays, 12345)
        for j, (x, _) in enumerate(pairs):
            assert block[off[j]: off[j] + size[j]].tobytes() == F.encode(x, 12345), (offset, j)
        assert block[off[3]: off[3] + size[3]].tobytes() == F.encode(np.zeros(0, np.int16), 12345)


def test_hook_more_jobs_than_the_lds_holds(gpu_hooks):
    check_more_jobs_than_the_lds_holds(gpu_hooks)


def test_run_request_is_run_packed_through_the_batcher(gpu_lib):
    cfg, blob = _blob(frames_per_id=2.0)
    reqs = _requests(cfg, 6, seed=3)
    windows = [None, 1, 3, 3, None, 5]
    for i, (_, kw) in enumerate(reqs):
        kw.update(loudness=-6.0, ceiling_db=-6.0, limiter_ms=windows[i], true_peak=bool(i % 2), compression="flac" if i % 3 != 1 else None)
        if kw["compression"]:
            kw.update(encoding="s16le", wav=False)
    plain = _session(blob, gpu_lib, window_ms=0.0)
    want = [plain.run_packed(f, **kw) for f, kw in reqs]
    sess = _session(blob, gpu_lib)
    _same_result(sess.run_request(reqs[0][0], **reqs[0][1]), want[0], "alone")
    mb = sess._batcher
    before = mb.batches
    got, errs = _all_requests(sess, reqs)
    assert errs == [None] * 6
    assert mb.requests == 7 and mb.batches - before < 6
    for i in range(6):
        _same_result(got[i], want[i], i)
    kw = dict(reqs[1][1], wav=True, compression=None, encoding="ulaw")
    _same_result(sess.run_request(reqs[1][0], **kw), plain.run_packed(reqs[1][0], **kw), "wav")
    with pytest.raises(ValueError, match="FLAC is not offered in streams yet"):
        sess.run_stream(reqs[0][0], compression="flac")
    ids = [[3, 4, 5, 6], [7, 8]]
    kw = dict(break_ms=20.0, utterance_keys=[1, 2], loudness=-6.0, ceiling_db=-6.0, limiter_ms=2.0)
    assert PP.request_flac(sess, ids, shared=True, **kw) == PP.request_flac(plain, ids, **kw)
    sess.close()
    plain.close()
