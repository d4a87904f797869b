"""The inputs of the FLAC tests, shared by the CPU-model suite (test_flac.py) and its device twin (test_gpu_flac.py): the lab-hook
matrix of DESIGN.md §4.15's rules, and the checks of an engine's FLAC pack against its own S16LE pack.  The yardstick is
tests/flac_ref.py; nothing here looks at the code under test."""
import numpy as np

import flac_ref as F

LENGTHS = (1, 5, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 777)
RATES = (22050, 8000, 12345, 176400, 70001)  # a table code, another, 16 bits of Hz, a table code above 65535, and "see STREAMINFO"
FIRST_FRAMES = (0, 127, 128, 2047, 2048, 65535, 65536)  # the last frame of a width, or the first of the next: two frames each
LONGEST = LENGTHS[-1]


def speech_like(n, seed=5):
    """Two gated sines and gated noise: voiced stretches, pauses that are not digital silence, mixed orders and Rice parameters."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    hiss = rng.normal(0, 1, n) * (50 + 4000 * (np.sin(t * 0.0011) > 0.6))  # stretches where no predictor helps much
    x = 8000 * np.sin(t * 0.03) * (np.sin(t * 0.005) > 0) + 3000 * np.sin(t * 0.2) * (np.sin(t * 0.002) > -0.3) + hiss
    return x.astype(np.int16)


CONTENTS = {
    "zeros": lambda n: np.zeros(n, np.int16),
    "constant": lambda n: np.full(n, -7, np.int16),
    "full_scale_alternating": lambda n: np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16),  # every frame verbatim
    "noise": lambda n: np.random.default_rng(n).integers(-32768, 32768, n).astype(np.int16),               # verbatim as well
    "ramp": lambda n: (3 * np.arange(n) - 5000).astype(np.int16),                                          # order 2, every k = 0
    "spike": lambda n: np.where(np.arange(n) == n // 2, 32767, 0).astype(np.int16),                         # a unary run across words
    "speech": speech_like,
    "silence_then_speech": lambda n: np.concatenate([np.zeros(n // 2, np.int16), speech_like(n - n // 2)]),
}



def mixed_frames(n):
    """Frame after frame of a different kind — constant, fixed predictors of several orders, verbatim — so that a workgroup which
    encodes several frames in a row meets a different path, frame size and LDS content each time; whatever is left is a short frame."""
    kinds = ("zeros", "speech", "noise", "constant", "ramp", "silence_then_speech", "full_scale_alternating", "spike")
    parts = [CONTENTS[kinds[f % len(kinds)]](min(F.BLOCK, n - s)) for f, s in enumerate(range(0, n, F.BLOCK))]
    return np.concatenate(parts) if parts else np.zeros(0, np.int16)


MIXED_FRAMES = 8 * 4096 + 777  # nine frames: more than the workgroups a small grid has
OTHER_CONTENTS = {"mixed_frames": mixed_frames}  # not part of the length matrix
_ref_cache = {}


def reference(name, n, rate=22050, first_frame=0):
    """(the input, the yardstick's file) — made once and shared; the arrays are read-only."""
    key = (name, n, rate, first_frame)
    if key not in _ref_cache:
        x = (CONTENTS.get(name) or OTHER_CONTENTS[name])(n)
        x.setflags(write=False)
        _ref_cache[key] = (x, F.encode(x, rate, first_frame))
    return _ref_cache[key]


def at_int16_offset(x, offset):
    """A copy of x that starts `offset` int16 behind a 16-byte boundary."""
    buf = np.zeros(x.shape[0] + 16, np.int16)
    base = (-buf.ctypes.data % 16) // 2
    view = buf[base + offset: base + offset + x.shape[0]]
    view[:] = x
    assert view.ctypes.data % 16 == 2 * offset
    return view


def check_hook(lib, name, n, rate=22050, first_frame=0, offset=None):
    """The kernels' file for one case equals the yardstick's bitwise, decodes to the input, and the frame sizes are the file's."""
    x, want = reference(name, n, rate, first_frame)
    got, sizes = lib.lab_flac(x if offset is None else at_int16_offset(x, offset), rate, first_frame)
    where = (name, n, rate, first_frame, offset)
    assert len(got) == len(want), (where, len(got), len(want))
    assert got == want, (where, next(i for i in range(len(got)) if got[i] != want[i]))
    back, hz = F.decode(got)
    assert hz == rate and np.array_equal(back, x), where
    assert sizes.shape[0] == -(-n // F.BLOCK) and int(sizes.sum()) == len(got) - F.HEADER_BYTES, where
    assert len(got) <= F.HEADER_BYTES + 16 * sizes.shape[0] + 2 * n, where


# ---------------------------------------------------------------- an engine's FLAC pack against its own S16LE pack
PACK = dict(order=[2, 0, 1], lead_samples=[0, 9000, 100], tail_samples=33)
SETTINGS = ("plain", "8000hz", "trim_loudness_limiter_true_peak")


def apply_settings(eng, name):
    """One of SETTINGS on a fresh engine (the output rate must be set before the run)."""
    if name == "8000hz":
        eng.set_output_rate(8000)
    elif name == "trim_loudness_limiter_true_peak":
        eng.set_edge_trim(0.9, 3)
        eng.set_loudness_target(-6.0, -6.0)
        eng.set_loudness_limiter(32)
        eng.set_loudness_ceiling_mode("true_peak")


def check_flac_pack(eng, rate, pack=None, encode_too=True):
    """fetch_packed as FLAC against fetch_packed as S16LE of the same run under the same settings; returns (s16, flac)."""
    pack = PACK if pack is None else pack
    s16 = eng.fetch_packed(compression=None, **pack)
    fl = eng.fetch_packed(compression="flac", **pack)
    assert s16.compression is None and s16.flac is None and fl.compression == "flac" and fl.wav is None and fl.data is None
    file = bytes(fl.flac)
    back, hz = F.decode(file)
    assert hz == rate == fl.sample_rate
    assert back.shape == s16.pcm.shape and np.array_equal(back, s16.pcm)
    if encode_too:
        assert file == F.encode(s16.pcm, rate)
    assert fl.total_samples == s16.total_samples
    for k in ("offsets", "lengths", "peaks"):
        assert getattr(fl, k).tobytes() == getattr(s16, k).tobytes(), k
    frames = -(-s16.total_samples // F.BLOCK)
    assert F.HEADER_BYTES + 11 * frames <= len(file) <= F.HEADER_BYTES + 16 * frames + 2 * s16.total_samples
    assert file[26:42] == bytes(16)  # the MD5 is unset
    return s16, fl
