"""The yardstick of the encoded packed streams: G.711 in numpy and the 58-byte non-PCM RIFF header, restated from the
standards' segment rules so that a machine without ``audioop`` or scipy can run the tests
(``tests/test_packed_encodings.py`` pins both to ``audioop`` / ``scipy.io.wavfile`` where they import, and to the committed
tables ``tests/golden/g711_tables.npz`` always).  Never the code under test: nothing here is imported by the package.

mu-law:  v = x >> 2;  mask = 0x7F if v < 0 else 0xFF;  m = min(|v|, 8159) + 33;
         seg = first of 0x3F, 0x7F, .., 0x1FFF that is >= m (8: none);  code = (0x7F if seg == 8 else seg << 4 | (m >> seg + 1) & 15) ^ mask
A-law:   v = x >> 3;  v >= 0: mask 0xD5, m = v;  else mask 0x55, m = -v - 1;
         seg = first of 0x1F, 0x3F, .., 0xFFF that is >= m;  code = (seg << 4 | (m >> (1 if seg < 2 else seg)) & 15) ^ mask
"""
from __future__ import annotations

import os
import struct

import numpy as np

TABLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_tables.npz")
SILENCE = {"ulaw": 0xFF, "alaw": 0xD5}            # the code of sample 0
FORMAT_TAG = {"ulaw": 7, "alaw": 6, "f32le": 3}   # WAVE_FORMAT_MULAW / _ALAW / _IEEE_FLOAT
BYTES_PER_SAMPLE = {"ulaw": 1, "alaw": 1, "f32le": 4}
HEADER_BYTES = 58


def lin2ulaw(x) -> np.ndarray:
    v = np.asarray(x, np.int16).astype(np.int64) >> 2
    mask = np.where(v < 0, 0x7F, 0xFF)
    m = np.minimum(np.abs(v), 8159) + 33
    ends = [(0x40 << i) - 1 for i in range(8)]
    seg = np.zeros_like(m)
    for e in ends:  # how many segment ends lie below m
        seg += (m > e)
    code = np.where(seg >= 8, 0x7F, (seg << 4) | ((m >> (seg + 1)) & 15))
    return (code ^ mask).astype(np.uint8)


def lin2alaw(x) -> np.ndarray:
    v = np.asarray(x, np.int16).astype(np.int64) >> 3
    mask = np.where(v >= 0, 0xD5, 0x55)
    m = np.where(v >= 0, v, -v - 1)
    ends = [(0x20 << i) - 1 for i in range(8)]
    seg = np.zeros_like(m)
    for e in ends:
        seg += (m > e)
    code = (seg << 4) | ((m >> np.where(seg < 2, 1, seg)) & 15)
    return (code ^ mask).astype(np.uint8)


def tables():
    """The committed audioop tables: {"ulaw": uint8 [65536], "alaw": ...}, indexed by sample + 32768."""
    with np.load(TABLES) as z:
        return {"ulaw": z["ulaw"].copy(), "alaw": z["alaw"].copy()}


def encode(table: np.ndarray, pcm) -> np.ndarray:
    return table[np.asarray(pcm, np.int16).astype(np.int32) + 32768]


def wav_header(encoding: str, rate: int, total_samples: int) -> bytes:
    """The 58 bytes in front of a non-PCM stream: RIFF, an 18-byte fmt chunk, a fact chunk, the data chunk's head."""
    bps = BYTES_PER_SAMPLE[encoding]
    data = bps * total_samples
    pad = data & 1
    return (b"RIFF" + struct.pack("<I", 50 + data + pad) + b"WAVE" +
            b"fmt " + struct.pack("<IHHIIHHH", 18, FORMAT_TAG[encoding], 1, rate, rate * bps, bps, 8 * bps, 0) +
            b"fact" + struct.pack("<II", 4, total_samples) +
            b"data" + struct.pack("<I", data))


def wav_file(encoding: str, rate: int, samples: np.ndarray) -> bytes:
    body = np.ascontiguousarray(samples, "<f4" if encoding == "f32le" else np.uint8).tobytes()
    return wav_header(encoding, rate, len(body) // BYTES_PER_SAMPLE[encoding]) + body + b"\0" * (len(body) & 1)
