"""Streams v2: compression, limiter window and ceiling mode per stream of one block (mi355vits_run_streams2 /
mi355vits_fetch_streams2; k_flac_place and k_flac_gather_streams in csrc/kernels_flac.cpp), and the micro-batcher's request kind on
top (InferenceSession.run_request).  On the CPU model of the kernels (tests/emu); test_gpu_streams2.py runs the same contract on the
MI355X.

Yardsticks, all older than the feature: ``fetch_packed`` of the SAME run under the handle's six setters is every stream's twin,
``flac_ref.encode`` / ``decode`` is the FLAC yardstick, the v1 ``fetch_streams`` is the uncompressed block's.  Everything is bitwise."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_cases as C  # noqa: E402
import flac_ref as F  # noqa: E402
import streams2_cases as S2  # noqa: E402

from mimic3_amd import postprocess as PP  # noqa: E402
from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine, NativeError  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from mimic3_amd.session import InferenceSession, SessionOptions  # noqa: E402
from tests.test_packed_streams import SCALES, _blob, _inputs, _requests, _run_kw, _same_audio, _session  # noqa: E402

DEFAULT_CUS = 8


@pytest.fixture
def cu_count(emu_lib):
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(DEFAULT_CUS)


@pytest.fixture(scope="module")
def served(emu_lib):
    """One engine after one ``run`` of the five ragged rows: shared, its run is never repeated and its settings are put back."""
    cfg, blob = _blob()
    eng = Engine(blob, library=emu_lib)
    ids, lens = _inputs(cfg)
    out = eng.run(ids, lens, SCALES, None, want_float=True, want_pcm16=True, **_run_kw())
    yield eng, (ids, lens), out, cfg
    eng.close()


def _s16_twins(eng, streams):
    return [S2.twin(eng, dict(st, compression=None)) if st.get("compression") == "flac" else None for st in streams]


# ---------------------------------------------------------------------------------------------- 1. the twins
def test_seven_streams_are_their_twins_at_any_cu_count(served, cu_count):
    eng, _, _, cfg = served
    blocks = []
    for cus in (1, 3, 8):
        cu_count(cus)
        got = eng.fetch_streams(S2.SEVEN)
        block, twins = S2.check_against_twins(eng, S2.SEVEN, got)
        blocks.append(block)
    assert blocks[0] == blocks[1] == blocks[2]
    # the conditions, on the twins: the limiter engages under both windows, and the three windowed settings give different bytes
    assert twins[3].limited.any() and twins[4].limited.any()
    assert len({bytes(twins[3].flac), twins[4].data.tobytes(), twins[5].data.tobytes()}) == 3
    assert twins[4].data.tobytes() != twins[5].data.tobytes() and twins[4].gain.tolist() != twins[5].gain.tolist()
    # [0, R) is the v1 block of the uncompressed subset, in the order given.  v1 reads ONE window from the handle and the subset has
    # two (8 and 0), so under each the layout is equal and every stream with that window (or without a target) is equal bitwise;
    # test_uncompressed_part_is_the_v1_block compares the whole of [0, R) under one window.
    subset = [(st, pa) for st, pa in zip(S2.SEVEN, got) if st.get("compression") != "flac"]
    R = got[0].uncompressed_bytes
    for window in (8, 0):
        eng.set_loudness_limiter(window)
        try:
            v1 = eng.fetch_streams([S2.v1_of(st) for st, _ in subset])
        finally:
            eng.set_loudness_limiter(0)
        assert v1[0].block.shape[0] == R
        for s, (a, (st, b)) in enumerate(zip(v1, subset)):
            assert (a.stream_offset, a.stream_bytes, a.data_offset) == (b.stream_offset, b.stream_bytes, b.data_offset), s
            if not st.get("loudness") or (st.get("limiter") or 0) == window:
                assert S2.stream_bytes(a) == S2.stream_bytes(b), (window, s)
    # every FLAC stream decodes to its twin's S16LE pcm and is the yardstick's encoding of it
    S2.check_flac_streams_decode(got, _s16_twins(eng, S2.SEVEN), cfg.sample_rate)


def test_uncompressed_part_is_the_v1_block(served):
    """With one window and one mode among the uncompressed streams, [0, R) is bitwise the v1 block with the handle set to them."""
    eng, _, _, _ = served
    streams = [dict(st) for st in S2.SEVEN]
    streams[5] = dict(streams[5], limiter=8)  # both targeted streams now use window 8, sample mode
    got = eng.fetch_streams(streams)
    S2.check_against_twins(eng, streams, got)
    eng.set_loudness_limiter(8)
    try:
        v1 = eng.fetch_streams([S2.v1_of(st) for st in streams if st.get("compression") != "flac"])
    finally:
        eng.set_loudness_limiter(0)
    R = got[0].uncompressed_bytes
    assert R == v1[0].block.shape[0] and got[0].block[:R].tobytes() == v1[0].block.tobytes()


# ---------------------------------------------------------------------------------------------- 2. v2 without new fields is v1
def test_v2_without_new_fields_is_v1(emu_lib):
    cfg, blob = _blob()
    ids, lens = _inputs(cfg)
    eng = Engine(blob, library=emu_lib)
    eng.profile_enable(True)
    v1 = [dict(order=[3], lead_samples=[1], wav=True, encoding="ulaw"), dict(order=[1, 4], loudness=S2.TARGET, trim=S2.TRIM),
          dict(order=[0, 4], lead_samples=[0, 777], tail_samples=5, wav=True, encoding="f32le"), dict(order=[2], loudness=S2.TARGET)]
    for window, mode in ((0, "sample"), (32, "true_peak")):
        eng.set_loudness_limiter(window)
        eng.set_loudness_ceiling_mode(mode)
        v2 = [dict(st, compression=None, limiter=window, true_peak=mode == "true_peak") for st in v1]
        reports, blocks = [], []
        for streams in (v1, v2):
            eng.profile_reset()
            got = eng.run_streams(ids, lens, SCALES, None, streams=streams, **_run_kw())
            reports.append({k: (v["calls"], v["bytes"]) for k, v in eng.profile_report().items()})
            blocks.append(got[0].block.tobytes())
            eng.profile_reset()
            blocks.append(eng.fetch_streams(streams)[0].block.tobytes())
            reports.append({k: (v["calls"], v["bytes"]) for k, v in eng.profile_report().items()})
        assert blocks[0] == blocks[1] == blocks[2] == blocks[3]
        assert reports[0] == reports[2] and reports[1] == reports[3]  # the same launches, with the same bytes
        assert ("limit" in reports[0]) == (window > 0) and ("truepeak" in reports[0]) == (mode == "true_peak")
        assert "pack.flac" not in reports[2] and reports[2]["pack.streams"][0] == 1
        assert hasattr(got[0], "frames") and got[0].uncompressed_bytes == got[0].block.shape[0]
        assert S2.handle_settings(eng)[3:5] == (window, mode)  # the v2 call changed neither
    eng.close()


# ---------------------------------------------------------------------------------------------- 3. many streams, many frames
def many_streams():
    """70 FLAC streams over the five rows, lead silences 100,000 .. 110,000 samples (no multiple of 4096), two uncompressed streams
    in between."""
    rng = np.random.default_rng(70)
    streams = []
    for s in range(70):
        lead = int(rng.integers(100_000, 110_001))
        lead += 1 if lead % 4096 == 0 else 0
        streams.append(dict(order=[s % 5], lead_samples=[lead], compression="flac"))
        if s in (20, 45):
            streams.append(dict(order=[s % 5, (s + 1) % 5], wav=True, encoding=["ulaw", "s16le"][s % 2]))
    return streams


def test_many_streams_many_frames(served):
    eng, _, _, cfg = served
    streams = many_streams()
    got = eng.fetch_streams(streams)
    assert sum(pa.frames for pa in got) > 1536 and sum(1 for pa in got if pa.compression == "flac") == 70
    S2.check_against_twins(eng, streams, got)  # frames[] and stream_bytes[] of every file against the yardstick's frame walk (decode_frames)


# ---------------------------------------------------------------------------------------------- 4. single-frame streams
def test_single_frame_streams(served):
    eng, _, out, cfg = served
    n0, n1 = int(out["lengths"][0]), int(out["lengths"][1])
    assert n0 < 4096
    streams = [dict(order=[0], compression="flac"), dict(order=[1], tail_samples=4096 - n1, compression="flac"),
               dict(order=[4], tail_samples=4097 - int(out["lengths"][4]), compression="flac")]
    got = eng.fetch_streams(streams)
    _, twins = S2.check_against_twins(eng, streams, got)
    assert [pa.frames for pa in got] == [1, 1, 2] and [pa.total_samples for pa in got] == [n0, 4096, 4097]
    S2.check_flac_streams_decode(got, _s16_twins(eng, streams), cfg.sample_rate)
    assert got[0].uncompressed_bytes == 0 and got[0].stream_offset == 0  # R = 0: the first file at the block's start


# ---------------------------------------------------------------------------------------------- 5. every byte has a writer
def test_every_byte_has_a_writer(emu_lib):
    cfg, blob = _blob()
    ids, lens = _inputs(cfg)
    streams = S2.SEVEN + [dict(order=[4], lead_samples=[9001], compression="flac")]
    clean = Engine(blob, library=emu_lib)
    want = clean.run_streams(ids, lens, SCALES, None, streams=streams, **_run_kw())[0].block.tobytes()
    eng = Engine(blob, library=emu_lib)
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


# ---------------------------------------------------------------------------------------------- 6. the hook
def test_hook_files_are_the_yardsticks(emu_lib, cu_count):
    arrays, files = S2.hook_cases()
    blocks = []
    for cus in (1, 8):
        cu_count(cus)
        block, off, size = emu_lib.lab_flac_jobs(arrays, 22050)
        blocks.append(block.tobytes())
        outside = np.ones(block.shape[0], bool)
        at = 0
        for j, want in enumerate(files):
            assert off[j] == at and off[j] % 16 == 0 and size[j] == len(want), j
            assert block[off[j]: off[j] + size[j]].tobytes() == want, j
            outside[off[j]: off[j] + size[j]] = False
            at = (int(off[j] + size[j]) + 15) & ~15
        assert block.shape[0] == off[-1] + size[-1] and not block[outside].any()
    assert blocks[0] == blocks[1]


@pytest.mark.parametrize("offset", [1, 3, 7])
def test_hook_input_at_an_odd_offset(emu_lib, offset):
    """An int16 input that starts 2 * offset bytes behind a 16-byte boundary is handled as ``lab_flac`` handles it: read where it is."""
    names = sorted(C.CONTENTS)[:3]
    pairs = [C.reference(name, n) for name, n in zip(names, (4097, 257, 3 * 4096 + 777))]
    arrays = [C.at_int16_offset(x, offset) if j != 1 else x for j, (x, _) in enumerate(pairs)]
    block, off, size = emu_lib.lab_flac_jobs(arrays, 12345)
    for j, (x, _) in enumerate(pairs):
        assert block[off[j]: off[j] + size[j]].tobytes() == F.encode(x, 12345), j


def check_more_jobs_than_the_lds_holds(lib):
    """1,100 jobs of 0 .. 6 samples (k_flac_place keeps the table of up to 1,024 jobs in the LDS) with three longer ones among them:
    a file every 48 or 64 bytes, so most 16-byte units of the block hold a header's end, a frame and a gap."""
    rng = np.random.default_rng(1100)
    arrays = [rng.integers(-3000, 3000, size=j % 7).astype(np.int16) for j in range(1100)]
    for j, n in ((5, 4097), (600, 257), (1099, 4096)):
        arrays[j] = C.reference("noise" if "noise" in C.CONTENTS else sorted(C.CONTENTS)[0], n)[0]
    block, off, size = lib.lab_flac_jobs(arrays, 22050)
    outside = np.ones(block.shape[0], bool)
    at = 0
    for j, x in enumerate(arrays):
        assert off[j] == at, j
        assert block[off[j]: off[j] + size[j]].tobytes() == F.encode(x, 22050), j
        outside[off[j]: off[j] + size[j]] = False
        at = (int(off[j] + size[j]) + 15) & ~15
    assert block.shape[0] == off[-1] + size[-1] and not block[outside].any()


def test_hook_more_jobs_than_the_lds_holds(emu_lib):
    check_more_jobs_than_the_lds_holds(emu_lib)


def test_hook_empty_jobs_and_errors(emu_lib):
    x, want = C.reference(sorted(C.CONTENTS)[0], 257)
    empty = np.zeros(0, np.int16)
    block, off, size = emu_lib.lab_flac_jobs([empty, x, empty, empty], 22050)
    assert size.tolist() == [42, len(want), 42, 42] and off.tolist() == [0, 48, (48 + len(want) + 15) & ~15, ((48 + len(want) + 15) & ~15) + 48]
    assert block[off[1]: off[1] + size[1]].tobytes() == want and block[:42].tobytes() == F.encode(empty, 22050)
    with pytest.raises(NativeError):
        emu_lib.lab_flac_jobs([], 22050)
    with pytest.raises(NativeError, match="rate"):
        emu_lib.lab_flac_jobs([x], 1 << 20)


# ---------------------------------------------------------------------------------------------- 7. errors and state
def test_errors_and_state(emu_lib):
    cfg, blob = _blob()
    ids, lens = _inputs(cfg)
    eng = Engine(blob, library=emu_lib)
    ok = dict(order=[0], compression="flac")
    with pytest.raises(NativeError, match="fetch_streams2: no completed run on this handle"):
        eng.fetch_streams([ok])
    eng.run(ids, lens, SCALES, None, want_float=True, want_pcm16=True, **_run_kw())
    eng.set_output_encoding("alaw")
    eng.set_edge_trim(0.37, 11)
    eng.set_loudness_target(-31.0, -7.0)
    eng.set_loudness_limiter(77)
    eng.set_loudness_ceiling_mode("true_peak")
    eng.set_output_compression("flac")
    before = S2.handle_settings(eng)
    served = {k: v.tobytes() for k, v in eng.fetch(want_float=True, want_pcm16=True).items()}
    al = eng.fetch_alignment(levels=True)
    cases = [
        ([ok, ok, dict(order=[0], compression=7)], "stream 2: unknown compression 7"),
        ([ok, dict(order=[1], encoding="ulaw", compression="flac")], "stream 1: FLAC compresses the s16le stream; encoding is ulaw"),
        ([dict(order=[0], wav=True, compression="flac")], "stream 0: a FLAC stream carries its own header"),
        ([ok, ok, ok, dict(order=[1], limiter=5000)], r"stream 3: limiter window 5000 is outside 0 \.\. 4096"),
        ([ok, ok, ok, dict(order=[1], limiter=-1)], r"stream 3: limiter window -1 is outside 0 \.\. 4096"),
        # every v1 rule and message applies to `base` unchanged
        ([ok, ok, dict(order=[0, 9], compression="flac")], "stream 2: pack entry 1: row 9 out of range"),
        ([dict(order=[0], encoding=7, limiter=3)], "stream 0: unknown encoding 7"),
        ([ok, dict(order=[1], loudness=(3.0, -1.0), true_peak=True)], "stream 1: loudness target 3 LUFS"),
        ([], "streams: "),
    ]
    for streams, msg in cases:
        with pytest.raises(NativeError, match=msg) as e:
            eng.fetch_streams(streams)
        assert e.value.code == -1
    # the two fields a dict cannot carry wrongly: through the array itself
    from mimic3_amd import _native as N
    import ctypes

    for field, value, msg in (("ceiling_mode", 9, "stream 3: unknown ceiling mode 9"), ("reserved", 1, "stream 0: reserved fields must be 0")):
        arr, n, keep, _ = Engine._stream_args([ok, ok, ok, dict(order=[1], limiter=3)], 5)
        if field == "reserved":
            arr[0].reserved[3] = value
        else:
            arr[3].ceiling_mode = value
        r = N.StreamsResult2()
        assert eng.native.lib.mi355vits_fetch_streams2(eng._h, arr, n, ctypes.byref(r)) == -1
        assert msg in eng.native.lib.mi355vits_last_error(eng._h).decode() and not r.bytes and not r.owner_
    # the block's limit counts a compressed stream at its bound: 42 + 16 frames + 2 total_samples
    huge = [dict(order=[b], lead_samples=[(1 << 28) - 50], compression="flac") for b in range(4)]
    with pytest.raises(NativeError, match=r"streams: block of \d+ bytes exceeds 2\^31 - 1"):
        eng.fetch_streams(huge)
    # the settings of the handle are neither read (the streams below are their twins under their OWN settings) nor changed
    got = eng.fetch_streams(S2.SEVEN)
    assert S2.handle_settings(eng) == before
    S2.check_against_twins(eng, S2.SEVEN, got)
    assert S2.handle_settings(eng) == before
    # the other fetches serve what they served, v1 fetch_streams included
    assert {k: v.tobytes() for k, v in eng.fetch(want_float=True, want_pcm16=True).items()} == served
    al2 = eng.fetch_alignment(levels=True)
    for k in ("frames", "start", "samples", "peak", "rms"):
        assert getattr(al, k).tobytes() == getattr(al2, k).tobytes(), k
    v1 = [dict(order=[3], wav=True), dict(order=[1, 4], encoding="ulaw")]
    a = eng.fetch_streams(v1)[0].block.tobytes()
    eng.fetch_streams(S2.SEVEN)
    assert eng.fetch_streams(v1)[0].block.tobytes() == a
    # a run that fails on its v2 arguments serves nothing afterwards only if it got as far as the run
    with pytest.raises(NativeError, match="stream 0: unknown compression 3"):
        eng.run_streams(ids, lens, SCALES, None, streams=[dict(order=[0], compression=3)], **_run_kw())
    eng.close()


def test_rate_above_the_streaminfo_field_is_refused(emu_lib):
    """STREAMINFO holds the rate in 20 bits.  48 x the voice's 22050 Hz = 1,058,400 Hz is a rate the resampler offers and FLAC cannot
    hold: with any FLAC stream run_streams2 refuses before anything runs and fetch_streams2 refuses with the run still served; an
    all-uncompressed v2 call at that rate is served; 47 x = 1,036,350 Hz fits."""
    cfg, blob = _blob()
    assert cfg.sample_rate == 22050
    ids, lens = _inputs(cfg)
    eng = Engine(blob, library=emu_lib)
    too_fast = "a FLAC stream holds rates up to 1048575 Hz; the run's rate is 1058400 Hz"
    plain = [dict(order=[3], wav=True, compression=None), dict(order=[1, 4], encoding="ulaw", limiter=0)]
    mixed = plain + [dict(order=[0], compression="flac")]
    eng.set_output_rate(48 * 22050)
    with pytest.raises(NativeError, match=too_fast) as e:
        eng.run_streams(ids, lens, SCALES, None, streams=mixed, **_run_kw())
    assert e.value.code == -1 and eng.output_rate == 48 * 22050
    with pytest.raises(NativeError, match="no completed run"):  # nothing was synthesised: no result is served
        eng.fetch_streams(plain)
    got = eng.run_streams(ids, lens, SCALES, None, streams=plain, **_run_kw())  # the rate itself is fine without FLAC
    assert hasattr(got[0], "frames") and got[0].sample_rate == 48 * 22050  # the v2 call
    kept = got[0].block.tobytes()
    S2.check_against_twins(eng, plain, got)
    with pytest.raises(NativeError, match=too_fast) as e:
        eng.fetch_streams(mixed)
    assert e.value.code == -1
    assert eng.fetch_streams(plain)[0].block.tobytes() == kept  # the run is still served
    # just below the limit: the 20-bit field and the frame headers' "see STREAMINFO" rate code
    eng.set_output_rate(47 * 22050)
    got = eng.run_streams(ids, lens, SCALES, None, streams=mixed, **_run_kw())
    S2.check_against_twins(eng, mixed, got)
    file = bytes(got[2].flac)
    assert int.from_bytes(file[18:21], "big") >> 4 == 1036350 and file[44] & 15 == 0
    eng.close()


# ---------------------------------------------------------------------------------------------- 8. cost
def test_cost_through_the_profiler(emu_lib):
    cfg, blob = _blob()
    ids, lens = _inputs(cfg)
    eng = Engine(blob, library=emu_lib)
    eng.profile_enable(True)
    eng.run(ids, lens, SCALES, None, **_run_kw())

    def report(streams):
        eng.profile_reset()
        got = eng.fetch_streams(streams)
        return got, {k: (int(v["calls"]), v["bytes"]) for k, v in eng.profile_report().items()}

    streams = S2.SEVEN
    got, rep = report(streams)
    audio = sum(int(n) for pa in got for n in pa.lengths)
    R16 = (got[0].uncompressed_bytes + 15) & ~15
    src_end = R16
    for pa in got:
        if pa.compression == "flac":
            src_end = ((src_end + 15) & ~15) + 2 * pa.total_samples  # each compressed stream's samples at a multiple of 16 behind the v1 block
    assert rep["pack.streams"] == (1, 4.0 * audio + src_end)
    flac = [pa for pa in got if pa.compression == "flac"]
    assert rep["pack.flac"] == (1, 2.0 * sum(pa.total_samples for pa in flac) + sum(pa.stream_bytes - 42 for pa in flac))
    # edges and loudness as in v1: the same streams without the new fields, on a twin handle after the same run
    v1_eng = Engine(blob, library=emu_lib)
    v1_eng.profile_enable(True)
    v1_eng.run(ids, lens, SCALES, None, **_run_kw())
    v1_eng.profile_reset()
    v1_eng.fetch_streams([S2.v1_of(st) for st in streams])
    v1_rep = {k: (int(v["calls"]), v["bytes"]) for k, v in v1_eng.profile_report().items()}
    v1_eng.close()
    assert rep["edges"] == v1_rep["edges"] and rep["loudness"] == v1_rep["loudness"] and "truepeak" not in v1_rep
    assert rep["truepeak"][0] == 1  # one true-peak stream with a target
    assert not any(k == "pcm16.pack" or (k.startswith("pack.") and k not in ("pack.streams", "pack.flac")) for k in rep), sorted(rep)
    # the limiter: one launch per (window, mode) group over one layout; its bytes summed = 8 * sum of job lengths + 16 * jobs
    lens_out = eng.fetch()["lengths"]
    jobs = {(int(r), st.get("limiter"), bool(st.get("true_peak"))) for st, pa in zip(streams, got) if st.get("limiter") for r, lim in zip(st["order"], pa.limited) if lim}
    assert rep["limit"][0] == 2 and rep["limit"][1] == 8.0 * sum(int(lens_out[r]) for r, _, _ in jobs) + 16.0 * len(jobs)
    assert rep["truepeak.env"][0] == 1  # the true-peak group alone
    # the same streams again: nothing is measured again; uncompressed: no pack.flac, and no true-peak stream: no truepeak
    _, rep = report(streams)
    assert "edges" not in rep and "loudness" not in rep and "truepeak" not in rep and rep["pack.flac"][0] == 1
    eng.run(ids, lens, SCALES, None, **_run_kw())
    _, rep = report([dict(st, compression=None, true_peak=False) for st in streams])
    assert "pack.flac" not in rep and "truepeak" not in rep and "truepeak.env" not in rep and rep["loudness"][0] == 1
    _, rep = report([dict(order=[0], true_peak=True, limiter=4)])  # true-peak mode without a target measures nothing
    assert "truepeak" not in rep and "limit" not in rep
    eng.close()


# ---------------------------------------------------------------------------------------------- 9. the session
def _all_requests(sess, reqs):
    got, errs = [None] * len(reqs), [None] * len(reqs)
    gate = threading.Barrier(len(reqs))

    def work(i):
        gate.wait()
        try:
            got[i] = sess.run_request(reqs[i][0], **reqs[i][1])
        except BaseException as e:  # noqa: BLE001
            errs[i] = e

    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(reqs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return got, errs


def _same_result(a, b, what):
    assert a.compression == b.compression, what
    if a.compression:
        assert bytes(a.flac) == bytes(b.flac) and a.data is None and a.wav is None and a.total_samples == b.total_samples, what
        for k in ("offsets", "lengths", "peaks", "lufs", "gain", "limited"):
            x, y = getattr(a, k), getattr(b, k)
            assert (x is None) == (y is None) and (x is None or np.asarray(x).tobytes() == np.asarray(y).astype(np.asarray(x).dtype).tobytes()), (what, k)
    else:
        _same_audio(a, b, what)


def test_run_request_is_run_packed_through_the_batcher(emu_lib):
    cfg, blob = _blob(frames_per_id=2.0)
    reqs = _requests(cfg, 6, seed=3)
    windows = [None, 1, 3, 3, None, 5]
    for i, (_, kw) in enumerate(reqs):
        kw.update(loudness=-6.0, ceiling_db=-6.0, limiter_ms=windows[i], true_peak=bool(i % 2), compression="flac" if i % 3 != 1 else None)
        if kw["compression"]:
            kw.update(encoding="s16le", wav=False)
    plain = _session(blob, emu_lib, window_ms=0.0)
    want = [plain.run_packed(f, **kw) for f, kw in reqs]
    assert any(w.limited.any() for w in want) and len({w.compression for w in want}) == 2
    _same_result(plain.run_request(reqs[0][0], **reqs[0][1]), want[0], "no batcher: run_packed itself")
    sess = _session(blob, emu_lib)
    _same_result(sess.run_request(reqs[0][0], **reqs[0][1]), want[0], "alone")  # the lone first request is not held back
    mb = sess._batcher
    before = mb.batches
    got, errs = _all_requests(sess, reqs)
    assert errs == [None] * 6
    assert mb.requests == 7 and mb.batches - before < 6  # different windows, modes and compressions shared calls
    for i in range(6):
        _same_result(got[i], want[i], i)
    assert len([g for g in got if g.block is got[0].block]) > 1  # callers of one batch hold views of ONE block
    # WAV with the keys given
    kw = dict(reqs[1][1], wav=True, compression=None, encoding="ulaw")
    _same_result(sess.run_request(reqs[1][0], **kw), plain.run_packed(reqs[1][0], **kw), "wav")
    # the session's default compression, as run_packed reads it
    fl = InferenceSession(blob, SessionOptions(), _library=emu_lib, output_compression="flac")
    assert fl.run_request(reqs[0][0], utterance_keys=reqs[0][1]["utterance_keys"]).compression == "flac"
    fl.close()
    with pytest.raises(ValueError, match="carries its own header"):
        sess.run_request(reqs[0][0], wav=True, compression="flac")
    with pytest.raises(ValueError, match="FLAC is not offered in streams yet"):
        sess.run_stream(reqs[0][0], compression="flac")
    # above micro_batch_max: run_packed
    big = {"input": np.ones((17, 3), np.int64), "input_lengths": np.full(17, 3, np.int64), "scales": reqs[0][0]["scales"]}
    n = mb.requests
    assert sess.run_request(big, utterance_keys=list(range(17)), compression="flac").block is None and mb.requests == n
    ids = [[3, 4, 5, 6], [7, 8]]
    kw = dict(break_ms=20.0, utterance_keys=[1, 2], loudness=-6.0, ceiling_db=-6.0, limiter_ms=2.0)
    shared, alone = PP.request_flac(sess, ids, shared=True, **kw), PP.request_flac(plain, ids, **kw)
    assert shared == alone and shared[:4] == b"fLaC" and mb.requests == n + 1
    back, hz = F.decode(shared)
    assert hz == cfg.sample_rate and back.shape[0] > int(0.02 * hz)
    sess.close()
    plain.close()


def test_a_bad_request_does_not_poison_its_batch(emu_lib):
    cfg, blob = _blob(frames_per_id=2.0)
    reqs = _requests(cfg, 4, seed=6)
    for i, (_, kw) in enumerate(reqs):
        kw.update(compression="flac" if i % 2 else None)
        if kw["compression"]:
            kw.update(encoding="s16le", wav=False)
    reqs[0][0]["input"][0, 0] = cfg.num_symbols + 5
    sess = _session(blob, emu_lib)
    plain = _session(blob, emu_lib, window_ms=0.0)
    got, errs = _all_requests(sess, reqs)
    assert isinstance(errs[0], ValueError) and got[0] is None
    for i in range(1, 4):
        assert errs[i] is None
        _same_result(got[i], plain.run_packed(reqs[i][0], **reqs[i][1]), i)
    sess.close()
    plain.close()


# ---------------------------------------------------------------------------------------------- 10. the C ABI
def test_plain_c99_client(emu_lib, tmp_path):
    """tests/abi/abi_streams2_client.c: the new declarations are C99; errors, sizes and the layout hold from C, and the FLAC stream it
    writes decodes to the raw stream it fetched from the same run."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_streams2_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_streams2_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir, "-lm"], check=True)
    cfg = VitsConfig.tiny()
    W.save(str(tmp_path / "voice.m355"), cfg, W.synthetic_weights(cfg, seed=17))
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355"), str(tmp_path / "out.flac")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    for msg in ("fetch_streams2: no completed run on this handle", "stream 2: unknown compression 7",
                "stream 1: FLAC compresses the s16le stream; encoding is ulaw", "stream 1: a FLAC stream carries its own header",
                "stream 2: limiter window 5000 is outside 0 .. 4096", "stream 2: unknown ceiling mode 9", "stream 0: reserved fields must be 0"):
        assert "expected failure rc=-1 msg=" + msg in p.stdout, msg
    assert "streams2 ok" in p.stdout
    sizes = [int(w.split("=")[1]) for w in p.stdout.split() if w.startswith("bytes=")]
    both = (tmp_path / "out.flac").read_bytes()
    assert len(both) == sum(sizes)
    back, hz = F.decode(both[: sizes[0]])
    assert hz == cfg.sample_rate and back.tobytes() == both[sizes[0]:]
