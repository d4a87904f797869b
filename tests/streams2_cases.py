"""Cases shared by test_streams2.py (CPU model) and test_gpu_streams2.py (MI355X): streams v2 — compression, limiter window and
ceiling mode per stream (mi355vits_run_streams2 / mi355vits_fetch_streams2).

The yardsticks are older than the feature: ``fetch_packed`` of the SAME run under the handle's six setters is every stream's twin,
``flac_ref.encode`` / ``decode`` the FLAC yardstick.  Everything is bitwise."""
import numpy as np

import flac_cases as C
import flac_ref as F

TARGET = (-6.0, -6.0)  # flac_cases' setting: the tiny voice's rows are over this ceiling at this target
TRIM = (0.9, 3)
# one block of seven streams (rows of the five ragged rows of test_packed_streams._inputs)
SEVEN = [
    dict(order=[3], wav=True, encoding="s16le", compression=None),
    dict(order=[2, 0, 1], lead_samples=[0, 9000, 100], tail_samples=33, compression="flac"),
    dict(order=[3], lead_samples=[1], wav=True, encoding="ulaw"),  # odd data: a pad byte
    dict(order=[2, 0, 1], lead_samples=[0, 9000, 100], tail_samples=33, compression="flac", trim=TRIM, loudness=TARGET, limiter=32,
         true_peak=True),
    dict(order=[1, 4], encoding="s16le", loudness=TARGET, limiter=8, true_peak=False),
    dict(order=[1, 4], encoding="s16le", loudness=TARGET, limiter=0),
    dict(order=[0, 4], lead_samples=[0, 777], tail_samples=5, encoding="f32le"),
]
V2_KEYS = ("compression", "limiter", "true_peak")


def twin(eng, st):
    """The single-stream path's answer for one stream dict: ``fetch_packed`` with the handle set to the stream's SIX settings."""
    before = (eng.output_encoding, eng.edge_trim, eng.loudness_target, eng.loudness_limiter, eng.loudness_ceiling_mode, eng.output_compression)
    eng.set_output_encoding(st.get("encoding", "s16le"))
    eng.set_edge_trim(*st.get("trim", (0.0, 0)))
    eng.set_loudness_target(*st.get("loudness", (None, -1.0)))
    eng.set_loudness_limiter(st.get("limiter", 0) or 0)
    eng.set_loudness_ceiling_mode("true_peak" if st.get("true_peak") else "sample")
    eng.set_output_compression(st.get("compression"))
    try:
        return eng.fetch_packed(order=st.get("order"), lead_samples=st.get("lead_samples"), tail_samples=st.get("tail_samples", 0),
                                wav=st.get("wav", False))
    finally:
        eng.set_output_encoding(before[0])
        eng.set_edge_trim(*before[1])
        eng.set_loudness_target(before[2][0] or None, before[2][1])
        eng.set_loudness_limiter(before[3])
        eng.set_loudness_ceiling_mode(before[4])
        eng.set_output_compression(before[5])


def handle_settings(eng):
    return (eng.output_encoding, eng.edge_trim, eng.loudness_target, eng.loudness_limiter, eng.loudness_ceiling_mode, eng.output_compression)


def stream_bytes(pa):
    return pa.block[pa.stream_offset: pa.stream_offset + pa.stream_bytes].tobytes()


def v1_of(st):
    return {k: v for k, v in st.items() if k not in V2_KEYS}


def check_against_twins(eng, streams, got, decode=True):
    """Each stream its twin byte for byte (RIFF header and pad byte, or the 42 FLAC header bytes, included) with the twin's arrays;
    the layout of the block; zero outside the streams.  Returns (the block's bytes, the twins)."""
    assert len(got) == len(streams)
    block = got[0].block
    R = got[0].uncompressed_bytes
    outside = np.ones(block.shape[0], bool)
    plain_end, flac_end, twins = 0, (R + 15) & ~15, []
    for s, (st, pa) in enumerate(zip(streams, got)):
        tw = twin(eng, st)
        twins.append(tw)
        flac = st.get("compression") == "flac"
        assert pa.block is block and pa.uncompressed_bytes == R, s
        assert pa.compression == tw.compression == ("flac" if flac else None), s
        assert pa.encoding == tw.encoding == st.get("encoding", "s16le") and pa.sample_rate == tw.sample_rate, s
        if flac:
            want = bytes(tw.flac)
            assert pa.data is None and pa.wav is None and pa.rows is None and bytes(pa.flac) == want, s
            assert pa.stream_offset % 16 == 0 and pa.stream_offset == flac_end and pa.data_offset == pa.stream_offset + 42, s
            flac_end = (pa.stream_offset + pa.stream_bytes + 15) & ~15
            assert pa.frames == -(-tw.total_samples // F.BLOCK), s
            if decode:
                sizes = frame_sizes(stream_bytes(pa))
                assert len(sizes) == pa.frames and pa.stream_bytes == 42 + sum(sizes), s
        else:
            want = bytes(tw.wav) if st.get("wav") else tw.data.tobytes()
            assert pa.flac is None and pa.frames == 0, s
            assert pa.data_offset % 16 == 0 and pa.stream_offset >= plain_end and pa.stream_offset + pa.stream_bytes <= R, s
            assert pa.data_offset - pa.stream_offset == ((44 if pa.encoding == "s16le" else 58) if st.get("wav") else 0), s
            assert pa.data.dtype == tw.data.dtype and pa.data.tobytes() == tw.data.tobytes(), s
            assert (pa.wav is None) == (tw.wav is None) and (pa.wav is None or bytes(pa.wav) == bytes(tw.wav)), s
            for i, row in enumerate(pa.rows):
                assert row.tobytes() == tw.rows[i].tobytes(), (s, i)
            plain_end = pa.stream_offset + pa.stream_bytes
        assert pa.stream_bytes == len(want), (s, pa.stream_bytes, len(want))
        assert stream_bytes(pa) == want, s
        assert pa.total_samples == tw.total_samples, s
        for k in ("offsets", "lengths", "peaks", "first", "end", "lufs", "gain", "limited"):
            a, b = getattr(pa, k), getattr(tw, k)
            assert (a is None) == (b is None), (s, k)
            assert a is None or np.asarray(a).tobytes() == np.asarray(b).tobytes() or np.asarray(a).tolist() == np.asarray(b).tolist(), (s, k)
        outside[pa.stream_offset: pa.stream_offset + pa.stream_bytes] = False
    assert plain_end == R
    ends = [pa.stream_offset + pa.stream_bytes for pa in got]
    assert max(ends) == block.shape[0]  # the block ends with its last stream
    assert not block[outside].any()  # gaps between streams, in front of the first header and of every file
    return block.tobytes(), twins


def frame_sizes(file):
    """The byte count of every frame of a file, by flac_ref.decode_frames (which checks every CRC and STREAMINFO's min / max)."""
    return [f[3] for f in F.decode_frames(file)[2]]


def check_flac_streams_decode(got, twins_s16, rate):
    """Every FLAC stream decodes to its twin's S16LE pcm and is what the yardstick encodes from it."""
    for pa, s16 in zip(got, twins_s16):
        if pa.compression != "flac":
            continue
        file = bytes(pa.flac)
        back, hz = F.decode(file)
        assert hz == rate and np.array_equal(back, s16.pcm)
        assert file == F.encode(s16.pcm, rate)
        assert file[26:42] == bytes(16)  # the MD5 is unset


HOOK_LENGTHS = (1, 257, 4096, 4097, 3 * 4096 + 777)


def hook_cases():
    """flac_cases.CONTENTS at HOOK_LENGTHS, mixed in one call: (arrays, the yardstick's files)."""
    arrays, files = [], []
    for name in sorted(C.CONTENTS):
        for n in HOOK_LENGTHS:
            x, want = C.reference(name, n)
            arrays.append(x)
            files.append(want)
    return arrays, files
