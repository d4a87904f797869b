"""Several independent streams out of one run (mi355vits_run_streams / mi355vits_fetch_streams; k_pack_streams in
csrc/kernels_pack.cpp), and the micro-batcher's request kind that uses them (InferenceSession.run_stream).  On the CPU model of
the kernels (tests/emu); test_gpu_packed_streams.py runs the same contract on the MI355X.

The yardstick everywhere is the existing single-stream path of the SAME engine: ``fetch_packed`` under ``set_output_encoding`` /
``set_edge_trim`` / ``set_loudness_target`` (and ``run_packed`` of a session).  Everything is bitwise.

Two facts of the design shape two of the cases:
  * a stream's data starts at a multiple of 16 and its header is 44 or 58 bytes, so a header starts at 4 or 6 (mod 16) — never 20
    bytes in front of a multiple of 4096.  The straddles of a work-item boundary that exist are tested, one per header form: 28
    bytes (44-byte header) and 26 bytes (58-byte header) in front of it.
  * ``Engine.fill_workspace`` fills the arena that holds the run's audio as well, so nothing can be fetched behind it.  The workspace
    is poisoned before ``run_streams`` (same inputs and keys, with and without a measured stream): the block the kernel writes lies
    in that poisoned arena."""
import os
import subprocess
import threading

import numpy as np
import pytest

from mimic3_amd import postprocess as PP
from mimic3_amd import weights as W
from mimic3_amd._native import Engine, NativeError
from mimic3_amd.config import VitsConfig
from mimic3_amd.session import InferenceSession, InvalidArgument, SessionOptions

SEED = 0xC0FFEE
SCALES = np.array([[0.667, 1.0, 0.8], [0.0, 1.6, 0.0], [0.5, 0.7, 0.3], [0.9, 1.2, 1.1], [0.333, 0.85, 0.0]], np.float32)
KEYS = [7, 1_000_003, 42, (1 << 40) + 5, 3]
VOLUMES = np.array([50.0, 100.0, 150.0, 300.0, 7.5]) / 100.0  # 300 % clips
ITEM = 4096  # bytes of one work item of k_pack_streams: 256 lanes x one 16-byte store
DEFAULT_CUS = 8
TRIM = (float(np.float32(10.0 ** (-30.0 / 20.0))), 3)
LOUD = (-23.0, -1.0)
# the boundary layout: (1) mu-law + header, one row, lead 1: odd data, a pad byte, and the next header inside the same 16-byte lane;
# (2) f32le + header, two rows, leads [0, 777], tail 5; (3) s16le, no header, trimmed and normalised; (4) A-law, no header, whole
# work items of silence in front; (5) s16le + header with the row stream 1 used
FIVE = [
    dict(order=[3], lead_samples=[1], wav=True, encoding="ulaw"),
    dict(order=[0, 4], lead_samples=[0, 777], tail_samples=5, wav=True, encoding="f32le"),
    dict(order=[1], encoding="s16le", trim=TRIM, loudness=LOUD),
    dict(order=[2], lead_samples=[ITEM + 453], encoding="alaw"),
    dict(order=[3], wav=True, encoding="s16le"),
]


@pytest.fixture
def cu_count(emu_lib):
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(DEFAULT_CUS)


def _inputs(cfg, B=5, Tx=12, seed=31):
    rng = np.random.default_rng(seed)
    lens = np.array([Tx] + list(rng.integers(2, Tx, size=B - 1)), np.int64)
    ids = np.zeros((B, Tx), np.int64)
    for b in range(B):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    return ids, lens


def _blob(seed=31, **kw):
    cfg = VitsConfig.tiny()
    return cfg, W.pack(cfg, W.synthetic_weights(cfg, seed=seed, **kw))


def _run_kw():
    return dict(seed=SEED, utterance_keys=KEYS, pcm_volume=VOLUMES)


@pytest.fixture(scope="module")
def served(emu_lib):
    """One engine after one ``run`` of the five ragged rows: shared, its run is never repeated and its settings are put back."""
    cfg, blob = _blob()
    eng = Engine(blob, library=emu_lib)
    ids, lens = _inputs(cfg)
    out = eng.run(ids, lens, SCALES, None, want_float=True, want_pcm16=True, **_run_kw())
    assert np.abs(out["pcm"]).max() == 32767 and len(set(int(n) for n in out["lengths"])) > 2  # one row clips; ragged
    yield eng, (ids, lens), out
    eng.close()


def twin(eng, st):
    """The single-stream path's answer for one stream dict: ``fetch_packed`` with the handle set to the stream's settings."""
    before = (eng.output_encoding, eng.edge_trim, eng.loudness_target)
    eng.set_output_encoding(st.get("encoding", "s16le"))
    eng.set_edge_trim(*st.get("trim", (0.0, 0)))
    eng.set_loudness_target(*st.get("loudness", (None, -1.0)))
    try:
        return eng.fetch_packed(order=st.get("order"), lead_samples=st.get("lead_samples"), tail_samples=st.get("tail_samples", 0),
                                wav=st.get("wav", False))
    finally:
        eng.set_output_encoding(before[0])
        eng.set_edge_trim(*before[1])
        eng.set_loudness_target(before[2][0] or None, before[2][1])


def stream_bytes(pa):
    return pa.block[pa.stream_offset: pa.stream_offset + pa.stream_bytes].tobytes()


def check_against_twins(eng, streams, got):
    """Each stream its twin byte for byte (header and pad included), its arrays the twin's, data 16-byte aligned, zero elsewhere."""
    assert len(got) == len(streams)
    block = got[0].block
    outside = np.ones(block.shape[0], bool)
    end = 0
    for s, (st, pa) in enumerate(zip(streams, got)):
        tw = twin(eng, st)
        assert pa.block is block and pa.data_offset % 16 == 0 and pa.stream_offset >= end, s
        want = bytes(tw.wav) if st.get("wav") else tw.data.tobytes()
        assert pa.stream_bytes == len(want), s
        assert stream_bytes(pa) == want, s
        assert pa.data_offset - pa.stream_offset == ((44 if pa.encoding == "s16le" else 58) if st.get("wav") else 0), s
        assert pa.encoding == tw.encoding == st.get("encoding", "s16le") and pa.sample_rate == tw.sample_rate
        assert pa.data.dtype == tw.data.dtype and pa.data.tobytes() == tw.data.tobytes(), s
        assert (pa.wav is None) == (tw.wav is None) and (pa.wav is None or bytes(pa.wav) == bytes(tw.wav)), s
        assert pa.total_samples == tw.total_samples, s
        for k in ("offsets", "lengths", "peaks", "first", "end", "lufs", "gain", "limited"):
            a, b = getattr(pa, k), getattr(tw, k)
            assert (a is None) == (b is None), (s, k)
            assert a is None or np.asarray(a).tolist() == np.asarray(b).tolist() or np.asarray(a).tobytes() == np.asarray(b).tobytes(), (s, k)
        for i, row in enumerate(pa.rows):
            assert row.tobytes() == tw.rows[i].tobytes(), (s, i)
        outside[pa.stream_offset: pa.stream_offset + pa.stream_bytes] = False
        end = pa.stream_offset + pa.stream_bytes
    assert end == block.shape[0]  # the block ends with its last stream
    assert not block[outside].any()  # gaps between streams and in front of the first header
    return block.tobytes()


# ---------------------------------------------------------------------------------------------- the kernel and the block
def test_boundary_layout_at_any_cu_count(served, cu_count):
    eng, _, out = served
    blocks = []
    for cus in (1, 3, 8):
        cu_count(cus)
        got = eng.fetch_streams(FIVE)
        blocks.append(check_against_twins(eng, FIVE, got))
        # stream 1: odd data, so a pad byte follows, and stream 2's header starts inside the same 16-byte lane
        assert got[0].total_samples % 2 == 1 and got[0].stream_bytes == 58 + got[0].total_samples + 1
        pad_at = got[0].stream_offset + got[0].stream_bytes - 1
        assert got[0].block[pad_at] == 0 and got[1].stream_offset // 16 == pad_at // 16
        assert got[2].first is not None and got[2].gain is not None and got[2].gain[0] != 0.0  # trimmed, normalised
        assert (got[3].data[: ITEM + 453] == 0xD5).all()  # A-law silence is not zero bytes
        assert (got[0].data[:1] == 0xFF).all() and not got[1].data[got[1].offsets[1] - 777: got[1].offsets[1]].any()
        assert got[4].rows[0].tobytes() == out["pcm"][3, : int(out["lengths"][3])].tobytes()  # row 3 again, as int16
    assert blocks[0] == blocks[1] == blocks[2]


@pytest.mark.parametrize("encoding,front", [("s16le", 28), ("ulaw", 26)])
def test_header_across_a_work_item_boundary(served, encoding, front):
    eng, _, out = served
    n = int(out["lengths"][0])
    hdr = 44 if encoding == "s16le" else 58
    # stream 0: int16, no header, from byte 0: it ends at 2 * (n + tail); the next header then starts at the multiple of 16 behind that
    # end + hdr, less hdr — `front` bytes in front of a multiple of ITEM
    k = (2 * n + front + ITEM - 1) // ITEM + 1
    tail = (k * ITEM - front) // 2 - n
    streams = [dict(order=[0], tail_samples=tail), dict(order=[2], wav=True, encoding=encoding, lead_samples=[3])]
    got = eng.fetch_streams(streams)
    off = got[1].stream_offset
    assert off % ITEM == ITEM - front and off // ITEM != (off + hdr - 1) // ITEM  # the straddle happened
    check_against_twins(eng, streams, got)


def test_every_byte_has_a_writer(emu_lib):
    cfg, blob = _blob()
    ids, lens = _inputs(cfg)
    plain = [dict(st) for st in FIVE]
    plain[2] = dict(order=[1], encoding="s16le")  # nothing measured: the block rides in the run's own layout
    for streams in (FIVE, plain):
        clean = Engine(blob, library=emu_lib)
        want = clean.run_streams(ids, lens, SCALES, None, streams=streams, **_run_kw())[0].block.tobytes()
        eng = Engine(blob, library=emu_lib)
        big = np.tile(ids, (2, 2))
        eng.run_streams(big, np.tile(lens * 2, 2), np.tile(SCALES, (2, 1)), None, streams=[dict(loudness=LOUD, trim=TRIM)], seed=1)  # sizes every arena past what the batch needs
        for pattern in (0x7FC00000, 0xA5A5A5A5):
            eng.fill_workspace(pattern)
            got = eng.run_streams(ids, lens, SCALES, None, streams=streams, **_run_kw())
            assert got[0].block.tobytes() == want, hex(pattern)
        check_against_twins(eng, streams, got)
        eng.close()
        clean.close()


def test_handle_settings_are_neither_read_nor_changed(served):
    eng, _, _ = served
    clean = eng.fetch_streams(FIVE)[0].block.tobytes()
    pk = eng.fetch_packed(order=[4, 0], lead_samples=[3, 0], wav=True).wav.tobytes()
    fe = {k: v.tobytes() for k, v in eng.fetch(want_float=True, want_pcm16=True).items()}
    al = eng.fetch_alignment(levels=True)
    eng.set_output_encoding("alaw")
    eng.set_edge_trim(0.37, 11)
    eng.set_loudness_target(-31.0, -7.0)
    try:
        assert eng.fetch_streams(FIVE)[0].block.tobytes() == clean
        assert eng.output_encoding == "alaw" and eng.edge_trim == (pytest.approx(0.37), 11) and eng.loudness_target == (-31.0, -7.0)
    finally:
        eng.set_output_encoding("s16le")
        eng.set_edge_trim(0.0)
        eng.set_loudness_target(None)
    assert eng.fetch_packed(order=[4, 0], lead_samples=[3, 0], wav=True).wav.tobytes() == pk
    assert {k: v.tobytes() for k, v in eng.fetch(want_float=True, want_pcm16=True).items()} == fe
    al2 = eng.fetch_alignment(levels=True)
    for k in ("frames", "start", "samples", "peak", "rms"):
        assert getattr(al, k).tobytes() == getattr(al2, k).tobytes(), k


def test_one_launch_and_what_is_measured(emu_lib):
    cfg, blob = _blob()
    ids, lens = _inputs(cfg)
    eng = Engine(blob, library=emu_lib)
    eng.profile_enable(True)
    plain = [dict(order=[0, 1], wav=True), dict(order=[2], encoding="ulaw", lead_samples=[5])]
    got = eng.run_streams(ids, lens, SCALES, None, streams=plain, **_run_kw())
    rep = eng.profile_report()
    audio = sum(int(n) for pa in got for n in pa.lengths)
    assert rep["pack.streams"]["calls"] == 1 and rep["pack.streams"]["bytes"] == 4.0 * audio + got[0].block.shape[0]
    assert not any(k == "pcm16.pack" or k == "pcm16" or (k.startswith("pack.") and k != "pack.streams") for k in rep), sorted(rep)
    assert "edges" not in rep and "loudness" not in rep
    # two distinct ratios among four trimmed streams, one of them normalised: two edge launches, one loudness measurement
    other = (0.5, 0)
    mixed = [dict(order=[0], trim=TRIM), dict(order=[1], trim=other), dict(order=[2], trim=TRIM, loudness=LOUD), dict(order=[0], trim=other, encoding="f32le")]
    eng.profile_reset()
    got = eng.fetch_streams(mixed)
    rep = eng.profile_report()
    assert rep["edges"]["calls"] == 2 and rep["loudness"]["calls"] == 1 and rep["pack.streams"]["calls"] == 1
    check_against_twins(eng, mixed, got)
    assert any(int(pa.first[0]) > 0 for pa in got)  # something was cut
    eng.profile_reset()
    again = eng.fetch_streams(list(reversed(mixed)))  # known ratios: nothing is launched before the pack
    rep = eng.profile_report()
    assert "edges" not in rep and "loudness" not in rep and rep["pack.streams"]["calls"] == 1
    check_against_twins(eng, list(reversed(mixed)), again)
    eng.close()


def test_errors_name_the_stream(emu_lib):
    cfg, blob = _blob()
    ids, lens = _inputs(cfg)
    eng = Engine(blob, library=emu_lib)
    ok = dict(order=[0])
    with pytest.raises(NativeError, match="fetch_streams: no completed run on this handle"):
        eng.fetch_streams([ok])
    cases = [
        ([ok, ok, dict(order=[0, 9])], "stream 2: pack entry 1: row 9 out of range"),
        ([dict(order=[0], encoding=7)], "stream 0: unknown encoding 7"),
        ([ok, ok, ok, dict(order=[1], trim=(1.5, 0))], r"stream 3: trim ratio 1.5 is outside \[0, 1\]"),
        ([ok, dict(order=[1, 1])], "stream 1: pack entry 1: row 1 appears twice"),
        ([dict(order=[1], lead_samples=[-2])], "stream 0: pack entry 0: negative silence"),
        ([ok, dict(order=[1], trim=(0.5, -1))], "stream 1: trim keep_samples -1 is negative"),
        ([ok, dict(order=[1], loudness=(3.0, -1.0))], "stream 1: loudness target 3 LUFS"),
        ([dict(order=[1], loudness=(-20.0, 2.0))], "stream 0: loudness ceiling 2 dBFS"),
        ([ok, dict(order=[0], encoding="f32le", lead_samples=[(1 << 31) - 1])], "stream 1: pack"),
        ([], "streams: "),
    ]
    for streams, msg in cases:
        with pytest.raises(NativeError, match=msg) as e:
            eng.run_streams(ids, lens, SCALES, None, streams=streams, **_run_kw())
        assert e.value.code == -1
    with pytest.raises(NativeError, match="fetch_streams: no completed run"):  # a failed run_streams serves nothing
        eng.fetch_streams([ok])
    # the block's own limit: four streams of 2^29 float samples of silence in front of one row each
    eng.run(ids, lens, SCALES, None, **_run_kw())
    huge = [dict(order=[b], encoding="f32le", lead_samples=[1 << 29]) for b in range(4)]
    with pytest.raises(NativeError, match=r"streams: block of \d+ bytes exceeds 2\^31 - 1"):
        eng.fetch_streams(huge)
    assert len(eng.fetch_streams([ok])) == 1  # a failed fetch leaves the run served
    # ... and in a run whose streams are measured the limit is met on the trimmed sizes: no run is served afterwards
    with pytest.raises(NativeError, match="streams: block of"):
        eng.run_streams(ids, lens, SCALES, None, streams=[dict(st, trim=TRIM) for st in huge], **_run_kw())
    with pytest.raises(NativeError, match="no completed run"):
        eng.fetch()
    eng.close()


# ---------------------------------------------------------------------------------------------- the session
def _session(blob, emu_lib, window_ms=200.0, lanes=1, **kw):
    so = SessionOptions()
    so.micro_batch_window_ms = window_ms
    so.micro_batch_max = 16
    so.lanes = lanes
    so.seed = 5
    return InferenceSession(blob, sess_options=so, _library=emu_lib, **kw)


def _requests(cfg, n, seed):
    rng = np.random.default_rng(seed)
    encs = ["s16le", "ulaw", "f32le", "alaw"]
    reqs = []
    for i in range(n):
        R = 1 + i % 2
        tx = int(rng.integers(4, 14))
        lens = rng.integers(2, tx + 1, size=R)
        lens[0] = tx
        ids = np.zeros((R, tx), np.int64)
        for b in range(R):
            ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
        feed = {"input": ids, "input_lengths": lens.astype(np.int64), "scales": np.array([0.667, 1.0 + 0.1 * (i % 3), 0.8], np.float32)}
        kw = dict(utterance_keys=[1000 + 10 * i + b for b in range(R)], encoding=encs[i % 4], wav=bool(i % 3), volume=[100.0, 40.0][:R] if i % 2 else None,
                  lead_ms=[0.0, 12.5][:R], tail_ms=3.0 * (i % 2), order=list(range(R))[::-1])
        if i % 4 == 1:
            kw.update(trim_db=-30.0, trim_keep_ms=1.0)
        if i % 4 == 2:
            kw.update(loudness=-23.0)
        reqs.append((feed, kw))
    return reqs


def _same_audio(a, b, what):
    assert a.encoding == b.encoding and a.sample_rate == b.sample_rate, what
    assert a.data.tobytes() == b.data.tobytes(), what
    assert (a.wav is None) == (b.wav is None) and (a.wav is None or bytes(a.wav) == bytes(b.wav)), what
    for k in ("offsets", "lengths", "peaks", "first", "end", "lufs", "gain", "limited"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None) and (x is None or np.asarray(x).tobytes() == np.asarray(y).astype(np.asarray(x).dtype).tobytes()), (what, k)


def _all_at_once(sess, reqs, **common):
    got, errs = [None] * len(reqs), [None] * len(reqs)
    gate = threading.Barrier(len(reqs))

    def work(i):
        gate.wait()
        try:
            got[i] = sess.run_stream(reqs[i][0], **reqs[i][1], **common)
        except BaseException as e:  # noqa: BLE001
            errs[i] = e

    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(reqs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return got, errs


def test_run_stream_is_run_packed_through_the_batcher(emu_lib):
    cfg, blob = _blob(frames_per_id=2.0)
    reqs = _requests(cfg, 8, seed=3)
    plain = _session(blob, emu_lib, window_ms=0.0)
    want = [plain.run_packed(f, **kw) for f, kw in reqs]
    same = plain.run_stream(reqs[0][0], **reqs[0][1])  # no batcher: run_packed itself
    _same_audio(same, want[0], "direct")
    sess = _session(blob, emu_lib)
    sess.run_stream(reqs[0][0], **reqs[0][1])  # the lone first request is not held back
    got, errs = _all_at_once(sess, reqs)
    assert errs == [None] * 8
    mb = sess._batcher
    assert mb.requests == 9 and mb.batches < mb.requests
    for i in range(8):
        _same_audio(got[i], want[i], i)
    shared = [g for g in got if g.block is got[0].block]
    assert len(shared) > 1  # callers of one batch hold views of ONE block
    big = {"input": np.ones((17, 3), np.int64), "input_lengths": np.full(17, 3, np.int64), "scales": reqs[0][0]["scales"]}
    before = mb.requests
    assert sess.run_stream(big, utterance_keys=list(range(17))).block is None and mb.requests == before  # above micro_batch_max: run_packed
    ids = [[3, 4, 5, 6], [7, 8]]
    kw = dict(break_ms=20.0, utterance_keys=[1, 2], encoding="ulaw", sample_rate=8000)
    assert PP.request_wav(sess, ids, shared=True, **kw) == PP.request_wav(plain, ids, **kw)
    assert mb.requests == before + 1
    sess.close()
    plain.close()


def test_two_output_rates_never_share_a_call(emu_lib):
    cfg, blob = _blob(frames_per_id=2.0)
    reqs = _requests(cfg, 6, seed=4)
    for i, (_, kw) in enumerate(reqs):
        kw["sample_rate"] = [None, 8000][i % 2]
    sess = _session(blob, emu_lib)
    calls = []
    inner = sess._engine_run

    def spy(ids, lengths, scales, sid, **kw):
        calls.append((ids.shape[0], kw.get("sample_rate"), len(kw.get("_streams") or [])))
        return inner(ids, lengths, scales, sid, **kw)

    sess._engine_run = spy
    sess.run_stream(reqs[0][0], **reqs[0][1])
    calls.clear()
    got, errs = _all_at_once(sess, reqs)
    assert errs == [None] * 6
    assert sum(c[2] for c in calls) == 6 and len(calls) < 6
    for i, g in enumerate(got):
        assert g.sample_rate == (8000 if i % 2 else cfg.sample_rate)
    plain = _session(blob, emu_lib, window_ms=0.0)
    for i, (f, kw) in enumerate(reqs):
        _same_audio(got[i], plain.run_packed(f, **kw), i)
    sess.close()
    plain.close()


def _queued(sess, reqs):
    """What ``run_stream`` hands the micro-batcher for each request, as the dispatcher's own tuples with fresh futures: a group
    whose composition and order the test fixes, for ``_run_stream_group``."""
    from concurrent.futures import Future

    class Captured(Exception):
        pass

    items = []

    def capture(ids, lengths, scales, sid, kw):
        items.append((ids, lengths, scales, sid, kw, Future()))
        raise Captured

    real, sess._batcher.submit = sess._batcher.submit, capture
    try:
        for feed, kw in reqs:
            with pytest.raises(Captured):
                sess.run_stream(feed, **kw)
    finally:
        sess._batcher.submit = real
    return items


def test_a_request_cannot_reach_another_requests_rows(emu_lib):
    """``order`` and ``lead_samples`` are checked against the request's OWN rows before it shares a call: in the batch the library
    sees all rows, and an index past the request's would be a neighbour's sentence."""
    cfg, blob = _blob(frames_per_id=2.0)
    reqs = _requests(cfg, 4, seed=6)  # rows per request: 1, 2, 1, 2
    sess = _session(blob, emu_lib)
    plain = _session(blob, emu_lib, window_ms=0.0)
    one, two = reqs[0], reqs[1]
    base = dict(utterance_keys=[1], encoding="s16le")
    for feed, bad, msg in ((one[0], dict(order=[0, 2]), "n = 2 out of range"), (one[0], dict(order=[1]), "pack entry 0: row 1 out of range"),
                           (two[0], dict(order=[0, 2]), "pack entry 1: row 2 out of range"), (two[0], dict(order=[-1]), "pack entry 0: row -1 out of range"),
                           (two[0], dict(order=[1, 1]), "pack entry 1: row 1 appears twice"), (two[0], dict(order=[0.0, 1.0]), "'order' must hold integers"),
                           (two[0], dict(lead_samples=[1, 2, 3]), "n = 3 out of range"),
                           (two[0], dict(order=[1], lead_samples=[1, 2]), "'order' and 'lead_samples' must have the same length")):
        kw = dict(base, utterance_keys=list(range(feed["input"].shape[0])), **bad)
        with pytest.raises(InvalidArgument, match=msg):
            sess.run_stream(feed, **kw)
        with pytest.raises(ValueError):  # the single-stream path refuses the same request
            plain.run_packed(feed, **kw)
    assert sess._batcher.requests == 0  # none of them reached a call
    short = dict(utterance_keys=[5, 6], lead_samples=[7])  # one silence, no order: the first row only, as run_packed reads it
    _same_audio(sess.run_stream(two[0], **short), plain.run_packed(two[0], **short), "n from lead_samples")
    # ... and where a group is put together, the check runs again before the rows are shifted: the bad request FIRST (its rows
    # start at 0, so every shifted index would exist in the batch), the others are served, it alone fails
    items = _queued(sess, [one, two, reqs[2]])
    items[0][4]["_stream"]["order"] = [0, 2]
    items[0][4]["_stream"]["lead_samples"] = None
    sess._batcher._run_stream_group(items)
    with pytest.raises(InvalidArgument, match="n = 2 out of range"):
        items[0][5].result(timeout=0)
    for it, (feed, kw) in zip(items[1:], (two, reqs[2])):
        _same_audio(it[5].result(timeout=0), plain.run_packed(feed, **kw), "served")
    sess.close()
    plain.close()


def test_a_bad_request_does_not_poison_its_batch(emu_lib):
    """A request only the library can refuse (a phoneme id the voice does not have), FIRST in a fixed group of 1 + 2 + 1 + 2 + 1 rows:
    the batch fails, every request is then called alone, the others are served and the bad one gets its error."""
    cfg, blob = _blob(frames_per_id=2.0)
    reqs = _requests(cfg, 5, seed=6)
    reqs[0][0]["input"][0, 0] = cfg.num_symbols + 5
    sess = _session(blob, emu_lib)
    items = _queued(sess, reqs)
    sess._batcher._run_stream_group(items)
    with pytest.raises(InvalidArgument, match="phoneme id out of range"):
        items[0][5].result(timeout=0)
    assert sess._batcher.batches == 4 and sess._batcher.requests == 4  # the failed batch counts nothing; four calls of one request
    plain = _session(blob, emu_lib, window_ms=0.0)
    for i in range(1, 5):
        _same_audio(items[i][5].result(timeout=0), plain.run_packed(reqs[i][0], **reqs[i][1]), i)
    # through the threads as well, whatever the arrival order
    got, errs = _all_at_once(sess, reqs)
    assert isinstance(errs[0], InvalidArgument) and got[0] is None
    for i in range(1, 5):
        assert errs[i] is None
        _same_audio(got[i], plain.run_packed(reqs[i][0], **reqs[i][1]), i)
    sess.close()
    plain.close()


# ---------------------------------------------------------------------------------------------- the C ABI
def test_plain_c99_client(emu_lib, tmp_path):
    """A C99 client packs one run as two streams and checks headers, sizes, pointers and the error path."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_streams_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_streams_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir, "-lm"], check=True)
    cfg = VitsConfig.tiny()
    W.save(str(tmp_path / "voice.m355"), cfg, W.synthetic_weights(cfg, seed=17))
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "expected failure rc=-1 msg=fetch_streams: no completed run on this handle" in p.stdout
    assert "expected failure rc=-1 msg=stream 1: pack entry 0: row 7 out of range" in p.stdout
    assert "streams ok" in p.stdout
