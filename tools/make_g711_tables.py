#!/usr/bin/env python3
"""Writes tests/golden/g711_tables.npz: the G.711 code of every int16 sample, from CPython's ``audioop`` (the module the
reference uses for its volume step, mimic3_tts/tts.py:542-543).

    ulaw[x + 32768] = audioop.lin2ulaw(x as 2 little-endian bytes, 2)      alaw[...] likewise with lin2alaw

Both tables are uint8 [65536].  The tests of the encoded packed streams (tests/test_packed_encodings.py,
tests/test_gpu_packed_encodings.py) read the file, so neither needs ``audioop`` (removed from the standard library in
Python 3.13).  Run with an interpreter that still has it:  python tools/make_g711_tables.py
"""
import audioop
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    x = np.arange(-32768, 32768, dtype=np.int32).astype("<i2").tobytes()
    ulaw = np.frombuffer(audioop.lin2ulaw(x, 2), np.uint8)
    alaw = np.frombuffer(audioop.lin2alaw(x, 2), np.uint8)
    assert ulaw.shape == alaw.shape == (65536,)
    out = os.path.join(ROOT, "tests", "golden", "g711_tables.npz")
    np.savez_compressed(out, ulaw=ulaw, alaw=alaw)
    print(out, os.path.getsize(out), "bytes; code of 0:", hex(ulaw[32768]), hex(alaw[32768]))


if __name__ == "__main__":
    main()
