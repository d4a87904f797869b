"""The yardstick of the FLAC tests: a numpy encoder of exactly the subset of RFC 9639 that DESIGN.md §4.15 writes out, and a decoder
written separately from it (it shares the two CRC routines and nothing else).  Neither looks at the library under test.

    encode(pcm, rate, first_frame=0) -> bytes      mono, 16 bit, blocks of 4096, one subframe per frame
    decode(data) -> (int16 array, rate)            raises ValueError on anything malformed or outside what it knows

No third-party FLAC decoder has read these bytes: the two sides pin each other, and three complete files are kept as fixed vectors
in test_flac.py.
"""
from __future__ import annotations

import numpy as np

BLOCK = 4096
HEADER_BYTES = 42


# ---------------------------------------------------------------- the two CRCs (MSB first, zero init, no final xor)
def _table(poly: int, width: int):
    top, mask = 1 << (width - 1), (1 << width) - 1
    out = []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        out.append(c)
    return out


_CRC8, _CRC16 = _table(0x07, 8), _table(0x8005, 16)


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c = _CRC8[c ^ b]
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


# ---------------------------------------------------------------- encoder
_RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}


def _bits(value: int, n: int) -> np.ndarray:
    return np.array([(value >> (n - 1 - i)) & 1 for i in range(n)], np.uint8)


def _utf8(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    if v < 0x800:
        return bytes([0xC0 | (v >> 6), 0x80 | (v & 0x3F)])
    if v < 0x10000:
        return bytes([0xE0 | (v >> 12), 0x80 | ((v >> 6) & 0x3F), 0x80 | (v & 0x3F)])
    if v < 0x200000:
        return bytes([0xF0 | (v >> 18), 0x80 | ((v >> 12) & 0x3F), 0x80 | ((v >> 6) & 0x3F), 0x80 | (v & 0x3F)])
    raise ValueError("frame number needs more than four bytes")


def _frame_header(bs: int, rate: int, number: int) -> bytes:
    if bs == BLOCK:
        bs_code, bs_field = 0b1100, b""
    elif bs <= 256:
        bs_code, bs_field = 0b0110, bytes([bs - 1])
    else:
        bs_code, bs_field = 0b0111, bytes([(bs - 1) >> 8, (bs - 1) & 0xFF])
    if rate in _RATE_CODES:
        rate_code, rate_field = _RATE_CODES[rate], b""
    elif rate <= 65535:
        rate_code, rate_field = 0b1101, bytes([rate >> 8, rate & 0xFF])
    elif rate % 10 == 0 and rate // 10 <= 65535:
        rate_code, rate_field = 0b1110, bytes([(rate // 10) >> 8, (rate // 10) & 0xFF])
    else:
        rate_code, rate_field = 0, b""
    h = bytes([0xFF, 0xF8, (bs_code << 4) | rate_code, 0x08]) + _utf8(number) + bs_field + rate_field
    return h + bytes([crc8(h)])


def _residuals(x: np.ndarray, order: int) -> np.ndarray:
    """r_order[i] for i >= order, as int64."""
    r = x.astype(np.int64)
    for _ in range(order):
        r = r[1:] - r[:-1]
    return r


def _fold(r: np.ndarray) -> np.ndarray:
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def _plan_order(x: np.ndarray, order: int, p: int):
    """(bits(order), the Rice parameter of every partition, the folded residuals of every partition)."""
    bs = x.shape[0]
    u = _fold(_residuals(x, order))
    per = bs >> p
    bits, ks, parts, at = 16 * order + 6, [], [], 0
    for j in range(1 << p):
        n = per - (order if j == 0 else 0)
        part = u[at: at + n]
        at += n
        costs = (part[None, :] >> np.arange(15, dtype=np.int64)[:, None]).sum(axis=1) + n * (1 + np.arange(15, dtype=np.int64))
        k = int(np.argmin(costs))  # the first minimum: the smallest k on a tie
        bits += 4 + int(costs[k])
        ks.append(k)
        parts.append(part)
    return bits, ks, parts


def _rice_bits(part: np.ndarray, k: int) -> np.ndarray:
    q = part >> k
    lens = q + 1 + k
    ends = np.cumsum(lens)
    out = np.zeros(int(ends[-1]) if part.size else 0, np.uint8)
    stop = ends - lens + q  # behind the unary zeros
    out[stop] = 1
    for b in range(k):
        out[stop + 1 + b] = (part >> (k - 1 - b)) & 1
    return out


def _subframe(x: np.ndarray) -> np.ndarray:
    bs = x.shape[0]
    if np.all(x == x[0]):
        return np.concatenate([_bits(0x00, 8), _bits(int(x[0]) & 0xFFFF, 16)])
    p = 4 if bs == BLOCK else 0
    best = None
    for order in range(0, min(4, bs - 1) + 1):
        plan = _plan_order(x, order, p)
        if best is None or plan[0] < best[1][0]:
            best = (order, plan)
    order, (bits, ks, parts) = best
    if bits >= 16 * bs:
        return np.concatenate([_bits(0x02, 8), np.unpackbits(x.astype(">i2").view(np.uint8))])
    out = [_bits(0x10 + 2 * order, 8)]
    out += [_bits(int(v) & 0xFFFF, 16) for v in x[:order]]
    out.append(_bits(p, 6))  # 00, then the partition order
    for k, part in zip(ks, parts):
        out.append(_bits(k, 4))
        out.append(_rice_bits(part, k))
    return np.concatenate(out)


def encode_frame(x: np.ndarray, rate: int, number: int) -> bytes:
    body = np.packbits(_subframe(np.asarray(x, np.int16))).tobytes()  # packbits pads the last byte with zeros
    frame = _frame_header(x.shape[0], rate, number) + body
    c = crc16(frame)
    return frame + bytes([c >> 8, c & 0xFF])


def stream_header(rate: int, total: int, frame_sizes) -> bytes:
    fmin, fmax = (min(frame_sizes), max(frame_sizes)) if len(frame_sizes) else (0, 0)
    v = (rate << 44) | (0 << 41) | (15 << 36) | total
    return (b"fLaC" + bytes([0x80, 0, 0, 34]) + BLOCK.to_bytes(2, "big") * 2 + fmin.to_bytes(3, "big") + fmax.to_bytes(3, "big")
            + v.to_bytes(8, "big") + bytes(16))


def encode(pcm, rate: int, first_frame: int = 0) -> bytes:
    x = np.ascontiguousarray(pcm, np.int16).reshape(-1)
    frames = [encode_frame(x[s: s + BLOCK], rate, first_frame + f) for f, s in enumerate(range(0, x.shape[0], BLOCK))]
    return stream_header(rate, int(x.shape[0]), [len(f) for f in frames]) + b"".join(frames)


# ---------------------------------------------------------------- decoder (written from the format, not from the encoder)
class _Reader:
    def __init__(self, data: bytes, at: int):
        self.data, self.start = data, at
        self.s = None  # the bits of data[at:] as a string of 0 / 1, made when the first bit is read
        self.pos = 0

    def _need(self):
        if self.s is None:
            chunk = self.data[self.start: self.start + 2 * BLOCK * 8 + 64]  # more than any frame this decoder accepts needs
            self.s = bin(int.from_bytes(b"\x01" + chunk, "big"))[3:]

    def read(self, n: int) -> int:
        self._need()
        if n == 0:
            return 0
        if self.pos + n > len(self.s):
            raise ValueError("the stream ends inside a frame")
        v = int(self.s[self.pos: self.pos + n], 2)
        self.pos += n
        return v

    def signed(self, n: int) -> int:
        v = self.read(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self) -> int:
        self._need()
        one = self.s.find("1", self.pos)
        if one < 0:
            raise ValueError("the stream ends inside a unary run")
        q = one - self.pos
        self.pos = one + 1
        return q


_DEC_BLOCK = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
_DEC_RATE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_DEC_BPS = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}


def _decode_residual(rd: _Reader, bs: int, order: int):
    method = rd.read(2)
    if method > 1:
        raise ValueError("reserved residual coding method")
    width = 4 if method == 0 else 5
    p = rd.read(4)
    if bs % (1 << p) or (bs >> p) < order:
        raise ValueError("partition order does not fit the block")
    out = []
    for j in range(1 << p):
        n = (bs >> p) - (order if j == 0 else 0)
        k = rd.read(width)
        if k == (1 << width) - 1:
            raise ValueError("escaped Rice partition: not written by this encoder")
        for _ in range(n):
            q = rd.unary()
            u = (q << k) | rd.read(k)
            out.append((u >> 1) if not (u & 1) else -((u + 1) >> 1))
    return out


def decode_frames(data: bytes):
    """-> (rate, total, [(number, samples as a list of ints, subframe type, bytes)]) after every check; the frames must carry
    consecutive numbers.  Subframe type: 0 constant, 1 verbatim, 8 + order fixed."""
    data = bytes(data)
    if len(data) < HEADER_BYTES or data[:4] != b"fLaC":
        raise ValueError("no fLaC marker")
    if data[4] != 0x80 or int.from_bytes(data[5:8], "big") != 34:
        raise ValueError("the first metadata block must be a last STREAMINFO of 34 bytes")
    min_bs, max_bs = int.from_bytes(data[8:10], "big"), int.from_bytes(data[10:12], "big")
    min_fs, max_fs = int.from_bytes(data[12:15], "big"), int.from_bytes(data[15:18], "big")
    v = int.from_bytes(data[18:26], "big")
    rate, channels, bps, total = v >> 44, ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1)
    if channels != 1 or bps != 16:
        raise ValueError("only mono 16-bit streams")
    if min_bs != max_bs:
        raise ValueError("a fixed-block-size stream has min = max block size")
    frames, at, count, sizes = [], HEADER_BYTES, 0, []
    while at < len(data):
        begin = at
        if len(data) - at < 6 or data[at] != 0xFF or data[at + 1] != 0xF8:
            raise ValueError(f"byte {at}: no frame sync with reserved 0 and the fixed-block-size flag")
        bs_code, rate_code = data[at + 2] >> 4, data[at + 2] & 15
        ch, size_code, reserved = data[at + 3] >> 4, (data[at + 3] >> 1) & 7, data[at + 3] & 1
        if reserved or ch != 0 or _DEC_BPS.get(size_code, 16 if size_code == 0 else None) != 16:
            raise ValueError(f"byte {at + 3}: not a mono 16-bit frame with reserved 0")
        at += 4
        lead = data[at]
        extra = 0 if lead < 0x80 else 1 if lead >> 5 == 0b110 else 2 if lead >> 4 == 0b1110 else 3 if lead >> 3 == 0b11110 else \
            4 if lead >> 2 == 0b111110 else 5 if lead >> 1 == 0b1111110 else 6 if lead == 0xFE else None
        if extra is None:
            raise ValueError(f"byte {at}: bad lead byte of the frame number")
        number = lead if extra == 0 else lead & ((1 << (6 - extra)) - 1)
        for b in data[at + 1: at + 1 + extra]:
            if b >> 6 != 0b10:
                raise ValueError("bad continuation byte of the frame number")
            number = (number << 6) | (b & 0x3F)
        at += 1 + extra
        if bs_code == 0:
            raise ValueError("reserved block-size code")
        if bs_code == 6:
            bs, at = data[at] + 1, at + 1
        elif bs_code == 7:
            bs, at = int.from_bytes(data[at: at + 2], "big") + 1, at + 2
        else:
            bs = _DEC_BLOCK[bs_code]
        if rate_code == 15:
            raise ValueError("invalid rate code")
        if rate_code == 12:
            frate, at = data[at] * 1000, at + 1
        elif rate_code == 13:
            frate, at = int.from_bytes(data[at: at + 2], "big"), at + 2
        elif rate_code == 14:
            frate, at = int.from_bytes(data[at: at + 2], "big") * 10, at + 2
        else:
            frate = _DEC_RATE.get(rate_code, rate)
        if frate != rate:
            raise ValueError(f"frame {number}: rate {frate} differs from STREAMINFO's {rate}")
        if crc8(data[begin: at]) != data[at]:
            raise ValueError(f"frame {number}: CRC-8 of the header is wrong")
        at += 1
        if bs > max_bs:
            raise ValueError(f"frame {number}: block of {bs} samples exceeds STREAMINFO's {max_bs}")
        rd = _Reader(data, at)
        if rd.read(1):
            raise ValueError("subframe padding bit set")
        kind = rd.read(6)
        if rd.read(1):
            raise ValueError("wasted bits: not written by this encoder")
        if kind == 0:
            x = [rd.signed(16)] * bs
        elif kind == 1:
            x = [rd.signed(16) for _ in range(bs)]
        elif 8 <= kind <= 12:
            order = kind - 8
            if order > bs:
                raise ValueError("predictor order exceeds the block")
            x = [rd.signed(16) for _ in range(order)]
            for r in _decode_residual(rd, bs, order):
                if order == 0:
                    pred = 0
                elif order == 1:
                    pred = x[-1]
                elif order == 2:
                    pred = 2 * x[-1] - x[-2]
                elif order == 3:
                    pred = 3 * x[-1] - 3 * x[-2] + x[-3]
                else:
                    pred = 4 * x[-1] - 6 * x[-2] + 4 * x[-3] - x[-4]
                x.append(pred + r)
        elif kind >= 32:
            raise ValueError("LPC subframe: not written by this encoder")
        else:
            raise ValueError(f"reserved subframe type {kind}")
        if len(x) != bs or min(x) < -32768 or max(x) > 32767:
            raise ValueError(f"frame {number}: samples outside 16 bits")
        pad = (-rd.pos) % 8
        if rd.read(pad):
            raise ValueError(f"frame {number}: non-zero padding")
        at += rd.pos // 8
        if len(data) - at < 2 or crc16(data[begin: at]) != int.from_bytes(data[at: at + 2], "big"):
            raise ValueError(f"frame {number}: CRC-16 is wrong")
        at += 2
        if frames and number != frames[-1][0] + 1:
            raise ValueError(f"frame number {number} follows {frames[-1][0]}")
        if frames and len(frames[-1][1]) != max_bs:
            raise ValueError("only the last frame may be short")
        frames.append((number, x, kind, at - begin))
        sizes.append(at - begin)
        count += bs
    if count != total:
        raise ValueError(f"{count} samples decoded, STREAMINFO says {total}")
    if sizes and (min(sizes) != min_fs or max(sizes) != max_fs):
        raise ValueError(f"frame sizes {min(sizes)} .. {max(sizes)}, STREAMINFO says {min_fs} .. {max_fs}")
    if not sizes and (min_fs or max_fs):
        raise ValueError("frame sizes of an empty stream must be 0")
    return rate, total, frames


def decode(data: bytes):
    rate, total, frames = decode_frames(data)
    x = np.array([v for f in frames for v in f[1]], np.int16) if frames else np.zeros(0, np.int16)
    return x, rate
