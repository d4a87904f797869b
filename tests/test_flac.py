"""The packed stream as FLAC (mi355vits_set_output_compression; k_flac_frames / k_flac_scan / k_flac_gather in csrc/kernels_flac.cpp)
on the CPU model of the kernels (tests/emu); test_gpu_flac.py runs the same contract on the MI355X.

Yardsticks, never the code under test: tests/flac_ref.py — a numpy encoder of exactly the rules DESIGN.md §4.15 writes out and a
decoder written separately from it —, three complete files kept here as hex, and the int16 packed stream of the SAME engine, which is
older than this setting.  No third-party FLAC decoder is available to the suite; none has read these bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_cases as C  # noqa: E402
import flac_ref as F  # noqa: E402

from mimic3_amd import weights as W  # noqa: E402
from mimic3_amd._native import Engine, NativeError  # noqa: E402
from mimic3_amd.config import VitsConfig  # noqa: E402
from mimic3_amd.session import InferenceSession, SessionOptions  # noqa: E402

SEED = 0xC0FFEE
DEFAULT_CUS = 8
EVERY_CU_COUNT = (1, 3, 5, 7, 8, 13, 32, 100, 256)  # every count a test of the CPU model sets anywhere in the suite
SCALES = np.array([[0.667, 1.0, 0.8], [0.5, 1.6, 0.3], [0.9, 0.7, 1.1]], np.float32)
KEYS = [7, 1_000_003, 42]
VOLUMES = np.array([0.5, 1.0, 3.0])  # 300 % clips

VECTORS = (  # complete files from the prototype of the rules; not third-party output
    (np.zeros(4096, np.int16), 22050,
     "664c6143800000221000100000000b00000b056220f00000100000000000000000000000000000000000fff8c60800d20000004253"),
    (np.array([-7], np.int16), 8000,
     "664c6143800000221000100000000c00000c01f400f00000000100000000000000000000000000000000fff864080000e300fff9683b"),
    (np.array([1, -2, 3], np.int16), 12345,
     "664c6143800000221000100000000f00000f030390f00000000300000000000000000000000000000000fff86d08000230399a1000b760739a"),
)


@pytest.fixture
def cu_count(emu_lib):
    yield emu_lib.emu_set_cu_count
    emu_lib.emu_set_cu_count(DEFAULT_CUS)


def _inputs(cfg, seed=31):
    rng = np.random.default_rng(seed)
    lens = np.array([12, 3, 8], np.int64)  # ragged
    ids = np.zeros((3, 12), np.int64)
    for b in range(3):
        ids[b, : lens[b]] = rng.integers(1, cfg.num_symbols, size=int(lens[b]))
    return ids, lens


def _engine(emu_lib, seed=31):
    cfg = VitsConfig.tiny()
    return cfg, Engine(W.pack(cfg, W.synthetic_weights(cfg, seed=seed)), library=emu_lib)


def _run(eng, ids, lens, **kw):
    return eng.run_packed(ids, lens, SCALES, None, seed=SEED, utterance_keys=KEYS, pcm_volume=VOLUMES, **kw)


# ---------------------------------------------------------------------------------------------- the yardstick itself
def test_crc_check_values():
    assert F.crc8(b"123456789") == 0xF4
    assert F.crc16(b"123456789") == 0xFEE8


@pytest.mark.parametrize("i", range(len(VECTORS)))
def test_fixed_vectors(emu_lib, i):
    x, rate, hexed = VECTORS[i]
    assert F.encode(x, rate).hex() == hexed
    back, hz = F.decode(bytes.fromhex(hexed))
    assert hz == rate and np.array_equal(back, x)
    assert emu_lib.lab_flac(x, rate)[0].hex() == hexed  # and the kernels write the same file


@pytest.mark.parametrize("name", sorted(C.CONTENTS))
def test_yardstick_round_trips(name):
    for n in C.LENGTHS:
        x, file = C.reference(name, n)
        back, hz = F.decode(file)
        assert hz == 22050 and np.array_equal(back, x), (name, n)
    for rate in C.RATES:
        x, file = C.reference(name, 4097, rate)
        assert F.decode(file)[1] == rate and np.array_equal(F.decode(file)[0], x)


def test_yardstick_contents_are_what_they_claim():
    """The cases reach what they are there for: verbatim frames, order 2 with k = 0, a long unary run, mixed orders."""
    def kinds(file):
        return {f[2] for f in F.decode_frames(file)[2]}

    n = 2 * 4096 + 100
    assert kinds(C.reference("full_scale_alternating", n)[1]) == {1}
    assert kinds(C.reference("noise", n)[1]) == {1}
    assert kinds(C.reference("zeros", n)[1]) == {0}
    assert kinds(C.reference("ramp", n)[1]) == {10}
    assert len(kinds(C.reference("speech", C.LONGEST)[1])) >= 2
    x, file = C.reference("spike", 4096)
    assert kinds(file) <= {8, 9, 10, 11, 12} and len(file) < 4096  # a fixed predictor: the spike's code is a unary run of hundreds of bits
    with pytest.raises(ValueError):
        F.decode(file[:-1] + bytes([file[-1] ^ 1]))  # a CRC-16 that is off is seen
    with pytest.raises(ValueError):
        F.decode(file[:46] + bytes([file[46] ^ 0x40]) + file[47:])  # and a header whose CRC-8 is


# ---------------------------------------------------------------------------------------------- the kernels through the lab hook
@pytest.mark.parametrize("name", sorted(C.CONTENTS))
def test_kernel_files_are_the_yardsticks(emu_lib, name):
    for n in C.LENGTHS:
        C.check_hook(emu_lib, name, n)


@pytest.mark.parametrize("rate", C.RATES)
def test_kernel_rate_forms(emu_lib, rate):
    for name, n in (("speech", 4097), ("constant", 5), ("noise", 257)):
        C.check_hook(emu_lib, name, n, rate)


@pytest.mark.parametrize("first_frame", C.FIRST_FRAMES)
def test_kernel_frame_number_widths(emu_lib, first_frame):
    C.check_hook(emu_lib, "speech", 4096 + 100, 22050, first_frame)
    _, _, frames = F.decode_frames(emu_lib.lab_flac(C.reference("speech", 4096 + 100)[0], 22050, first_frame)[0])
    assert [f[0] for f in frames] == [first_frame, first_frame + 1]


def test_kernel_files_do_not_depend_on_the_cu_count(emu_lib, cu_count):
    for cus in EVERY_CU_COUNT:
        cu_count(cus)
        C.check_hook(emu_lib, "silence_then_speech", C.LONGEST)
        C.check_hook(emu_lib, "speech", 4097, 12345)


def test_a_workgroup_encodes_several_different_frames_in_a_row(emu_lib, cu_count):
    """k_flac_frames is persistent: with fewer workgroups than frames (three per CU) a workgroup goes round its loop again, on LDS the
    frame before has used.  Nine frames of different kinds — constant, fixed, verbatim, a short last one — on one CU (three
    workgroups, three frames each, a stride of three kinds), on two CUs (six: some take two frames, some one) and on the default."""
    x, want = C.reference("mixed_frames", C.MIXED_FRAMES)
    kinds = [f[2] for f in F.decode_frames(want)[2]]
    assert len(kinds) == 9 and 0 in kinds and 1 in kinds and len({k for k in kinds if k >= 8}) >= 2  # the yardstick's frames do differ
    for cus in (1, 2, DEFAULT_CUS):
        cu_count(cus)
        C.check_hook(emu_lib, "mixed_frames", C.MIXED_FRAMES)
        C.check_hook(emu_lib, "mixed_frames", C.MIXED_FRAMES, 12345, 126)  # and the frame number changes width on the way


@pytest.mark.parametrize("offset", [1, 3, 4, 7])
def test_kernel_input_at_an_odd_offset(emu_lib, offset):
    """The samples start 2 * offset bytes behind a 16-byte boundary on the device: no frame takes the 16-byte loads."""
    C.check_hook(emu_lib, "speech", C.LONGEST, offset=offset)
    C.check_hook(emu_lib, "full_scale_alternating", 4097, offset=offset)


def test_hook_refuses_what_it_cannot_encode(emu_lib):
    x = np.zeros(8, np.int16)
    for rate, first in ((0, 0), (1 << 20, 0), (22050, -1), (22050, 1 << 21)):
        with pytest.raises(NativeError):
            emu_lib.lab_flac(x, rate, first)
    file, sizes = emu_lib.lab_flac(np.zeros(0, np.int16), 22050)  # an empty stream is its header
    assert file == F.encode(np.zeros(0, np.int16), 22050) and sizes.shape == (0,) and len(file) == 42


# ---------------------------------------------------------------------------------------------- the engine
@pytest.mark.parametrize("setting", C.SETTINGS)
def test_flac_pack_decodes_to_the_s16_pack(emu_lib, setting):
    cfg, eng = _engine(emu_lib)
    C.apply_settings(eng, setting)
    ids, lens = _inputs(cfg)
    rate = eng.output_rate
    ran = _run(eng, ids, lens, compression="flac", **C.PACK)
    s16, fl = C.check_flac_pack(eng, rate)
    assert bytes(ran.flac) == bytes(fl.flac)  # run_packed is fetch_packed
    assert ran.total_samples == fl.total_samples and ran.offsets.tobytes() == fl.offsets.tobytes()
    assert eng.output_compression is None  # a call's compression= is put back
    assert s16.total_samples > 2 * F.BLOCK and s16.total_samples % F.BLOCK  # several frames, the last one short
    if setting == "trim_loudness_limiter_true_peak":
        assert fl.first is not None and fl.limited is not None and fl.limited.any()
        assert (fl.first > 0).any() and (fl.end < eng.fetch(want_pcm16=True)["lengths"][C.PACK["order"]]).any()  # both edges cut somewhere
    with pytest.raises(ValueError):
        fl.pcm


@pytest.mark.parametrize("math", ["f32", "bf16w"])
def test_flac_pack_in_other_math_modes(emu_lib, math):
    cfg, eng = _engine(emu_lib)
    eng.set_math(math)
    ids, lens = _inputs(cfg)
    _run(eng, ids, lens)
    C.check_flac_pack(eng, cfg.sample_rate)


def test_a_row_alone_gives_the_same_frames(emu_lib):
    cfg, eng = _engine(emu_lib)
    ids, lens = _inputs(cfg)
    _run(eng, ids, lens)
    one = dict(order=[1], lead_samples=[77], tail_samples=5)
    s16, fl = C.check_flac_pack(eng, cfg.sample_rate, one)
    alone = eng.run_packed(ids[1:2, : int(lens[1])], lens[1:2], SCALES[1:2], None, seed=SEED, utterance_keys=KEYS[1:2],
                           pcm_volume=VOLUMES[1:2], lead_samples=[77], tail_samples=5, compression="flac")
    assert bytes(alone.flac) == bytes(fl.flac)


def test_errors_and_the_setting(emu_lib):
    cfg, eng = _engine(emu_lib)
    ids, lens = _inputs(cfg)
    assert eng.output_compression is None
    eng.set_output_compression("flac")
    assert eng.output_compression == "flac"
    with pytest.raises(NativeError, match="output compression 2 unknown"):
        eng.set_output_compression(2)
    with pytest.raises(NativeError, match="output compression -1 unknown"):
        eng.set_output_compression(-1)
    assert eng.output_compression == "flac"  # a refused value leaves the setting
    with pytest.raises(ValueError):
        eng.set_output_compression("mp3")
    # before anything is sized or launched: no run, so no result to fetch afterwards either
    for enc in ("ulaw", "alaw", "f32le"):
        eng.set_output_encoding(enc)
        with pytest.raises(NativeError, match="pack: FLAC compresses the s16le stream; output encoding is " + enc):
            _run(eng, ids, lens)
        assert eng.output_compression == "flac" and eng.output_encoding == enc
    eng.set_output_encoding("s16le")
    with pytest.raises(NativeError, match="no completed run"):
        eng.fetch_packed()
    # wav_header != 0 straight at the C ABI (the Python layer refuses it before the library sees it)
    from mimic3_amd._native import PackArgs, PackedResult
    import ctypes
    pa, r = PackArgs(), PackedResult()
    pa.n, pa.wav_header = 3, 1
    a, rows, per_row, keep = eng._args(ids, lens, SCALES, None, SEED, 0, None, None, None, 1.0, KEYS)
    rc = eng.native.lib.mi355vits_run_packed(eng._h, ctypes.byref(a), None, ctypes.byref(pa), ctypes.byref(r))
    assert rc == -1 and not r.bytes and "a FLAC stream carries its own header" in eng.native.lib.mi355vits_last_error(eng._h).decode()
    with pytest.raises(ValueError, match="carries its own header"):
        _run(eng, ids, lens, wav=True)
    with pytest.raises(ValueError, match="carries its own header"):
        eng.fetch_packed(wav=True, compression="flac")
    # the setting is inherited by a clone, and read when a pack is made: one synthesis, fetched raw and as FLAC
    lane = Engine(eng)
    assert lane.output_compression == "flac"
    lane.close()
    ran = _run(eng, ids, lens, **C.PACK)  # the handle's setting
    assert ran.compression == "flac" and bytes(ran.flac[:4]) == b"fLaC"
    eng.set_output_compression(None)
    raw = eng.fetch_packed(**C.PACK)
    assert raw.compression is None and np.array_equal(F.decode(bytes(ran.flac))[0], raw.pcm)
    eng.close()


def test_rate_above_the_streaminfo_field_is_refused(emu_lib):
    """STREAMINFO holds the rate in 20 bits.  48 x the voice's 22050 Hz = 1,058,400 Hz is a rate the resampler offers and FLAC cannot
    hold: refused by run_packed before anything runs and by fetch_packed with the run still served; 47 x = 1,036,350 Hz fits."""
    cfg, eng = _engine(emu_lib)
    assert cfg.sample_rate == 22050
    ids, lens = _inputs(cfg)
    too_fast = "a FLAC stream holds rates up to 1048575 Hz; the run's rate is 1058400 Hz"
    eng.set_output_rate(48 * 22050)
    eng.set_output_compression("flac")
    with pytest.raises(NativeError, match=too_fast) as e:
        _run(eng, ids, lens, **C.PACK)
    assert e.value.code == -1  # MI355VITS_ERR_INVALID
    assert eng.output_compression == "flac" and eng.output_rate == 48 * 22050
    with pytest.raises(NativeError, match="no completed run"):  # nothing was synthesised: no result is served
        eng.fetch_packed(**C.PACK)
    eng.set_output_compression(None)
    raw = _run(eng, ids, lens, **C.PACK)  # the rate itself is fine without FLAC
    assert raw.sample_rate == 48 * 22050
    kept = raw.pcm.copy()
    with pytest.raises(NativeError, match=too_fast) as e:
        eng.fetch_packed(compression="flac", **C.PACK)
    assert e.value.code == -1 and eng.output_compression is None
    eng.set_output_compression("flac")
    with pytest.raises(NativeError, match=too_fast):
        eng.fetch_packed(**C.PACK)
    assert eng.output_compression == "flac"
    assert np.array_equal(eng.fetch_packed(compression=None, **C.PACK).pcm, kept)  # the run is still served
    # just below the limit, through the engine: the 20-bit field and the frame headers' "see STREAMINFO" rate code
    eng.set_output_compression(None)
    eng.set_output_rate(47 * 22050)
    _run(eng, ids, lens, **C.PACK)
    s16, fl = C.check_flac_pack(eng, 47 * 22050)
    assert int.from_bytes(bytes(fl.flac)[18:21], "big") >> 4 == 1036350 and bytes(fl.flac)[44] & 15 == 0
    eng.close()


def test_compression_off_after_on_is_the_old_stream(emu_lib):
    cfg, eng = _engine(emu_lib)
    ids, lens = _inputs(cfg)
    before = _run(eng, ids, lens, wav=True, **C.PACK)
    before_bytes = bytes(before.wav)
    eng.set_output_compression("flac")
    _run(eng, ids, lens, **C.PACK)
    eng.set_output_compression(None)
    after = _run(eng, ids, lens, wav=True, **C.PACK)
    assert bytes(after.wav) == before_bytes and after.compression is None
    assert bytes(eng.fetch_packed(wav=True, **C.PACK).wav) == before_bytes


def test_streams_calls_do_not_read_the_setting(emu_lib):
    cfg, eng = _engine(emu_lib)
    ids, lens = _inputs(cfg)
    streams = [dict(order=[2, 0], lead_samples=[5, 100], wav=True), dict(order=[1], encoding="ulaw", tail_samples=9)]
    kw = dict(seed=SEED, utterance_keys=KEYS, pcm_volume=VOLUMES)
    off = eng.run_streams(ids, lens, SCALES, None, streams=streams, **kw)
    off_block = bytes(off[0].block)
    eng.set_output_compression("flac")
    on = eng.run_streams(ids, lens, SCALES, None, streams=streams, **kw)
    assert bytes(on[0].block) == off_block
    assert bytes(eng.fetch_streams(streams)[0].block) == off_block
    assert all(s.compression is None for s in on)


def test_profile_reports_pack_flac_with_its_bytes(emu_lib):
    cfg, eng = _engine(emu_lib)
    ids, lens = _inputs(cfg)
    _run(eng, ids, lens)
    eng.profile_enable(True)
    eng.profile_reset()
    fl = eng.fetch_packed(compression="flac", **C.PACK)
    rep = eng.profile_report()
    assert rep["pack.flac"]["calls"] == 1
    assert rep["pack.flac"]["bytes"] == 2 * fl.total_samples + (len(fl.flac) - 42)
    assert rep["pcm16.pack"]["calls"] == 1  # the S16 pack in front keeps its own line
    eng.profile_reset()
    eng.fetch_packed(**C.PACK)
    assert "pack.flac" not in eng.profile_report()


def test_session_and_python_errors(emu_lib):
    cfg = VitsConfig.tiny()
    blob = W.pack(cfg, W.synthetic_weights(cfg, seed=31))
    ids, lens = _inputs(cfg)
    feed = {"input": ids, "input_lengths": lens, "scales": np.array([0.667, 1.0, 0.8], np.float32)}
    with pytest.raises(ValueError):
        InferenceSession(blob, SessionOptions(), _library=emu_lib, output_compression="mp3")
    sess = InferenceSession(blob, SessionOptions(), _library=emu_lib, output_compression="flac")
    kw = dict(order=[2, 0, 1], lead_ms=[0, 400, 5], tail_ms=2, utterance_keys=KEYS)
    fl = sess.run_packed(feed, **kw)  # the session's default
    raw = sess.run_packed(feed, compression=None, **kw)
    assert fl.compression == "flac" and raw.compression is None and fl.wav is None
    back, hz = F.decode(bytes(fl.flac))
    assert hz == cfg.sample_rate and np.array_equal(back, raw.pcm)
    assert fl.offsets.tobytes() == raw.offsets.tobytes() and fl.total_samples == raw.total_samples
    with pytest.raises(ValueError, match="carries its own header"):
        sess.run_packed(feed, wav=True, **kw)
    with pytest.raises(ValueError):
        sess.run_packed(feed, compression="opus", **kw)
    with pytest.raises(ValueError, match="FLAC is not offered in streams yet"):
        sess.run_stream(feed, compression="flac", **kw)
    st = sess.run_stream(feed, **kw)  # a stream is never compressed, whatever the session's default
    assert st.compression is None and np.array_equal(st.pcm, raw.pcm)
    sess.close()


def test_plain_c99_client(emu_lib, tmp_path):
    """tests/abi/abi_flac_client.c: the new declarations are C99; errors, header fields and sizes hold from C, and the file it writes
    decodes to the raw stream it fetched from the same run."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_flac_client"
    libdir, libname = os.path.split(emu_lib.path)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "abi", "abi_flac_client.c"), "-o", str(exe), "-L", libdir,
                    "-l:" + libname, "-Wl,-rpath," + libdir, "-lm"], check=True)
    cfg = VitsConfig.tiny()
    W.save(str(tmp_path / "voice.m355"), cfg, W.synthetic_weights(cfg, seed=17))
    p = subprocess.run([str(exe), str(tmp_path / "voice.m355"), str(tmp_path / "out.flac")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "output compression 2 unknown (0 = none, 1 = flac)" in p.stdout
    assert "a FLAC stream carries its own header" in p.stdout
    assert "pack: FLAC compresses the s16le stream; output encoding is ulaw" in p.stdout
    assert "flac ok" in p.stdout
    sizes = [int(w.split("=")[1]) for w in p.stdout.split() if w.startswith("bytes=")]
    both = (tmp_path / "out.flac").read_bytes()
    assert len(both) == sum(sizes)
    back, hz = F.decode(both[: sizes[0]])
    assert hz == cfg.sample_rate and back.tobytes() == both[sizes[0]:]
