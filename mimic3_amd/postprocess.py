"""What happens to the int16 audio after the hot path, restated so that a batch can be finished in one place
(SURVEY.md §8f N4).  The reference does these steps one sentence at a time on the host:

* volume — ``audioop.mul(audio_bytes, 2, settings.volume / 100)`` (``mimic3_tts/tts.py:542-543``): fused into the engine's
  int16 kernel (``InferenceSession.run_pcm16(feed, volume=...)``); ``apply_volume`` below is the same arithmetic in numpy
  for callers that already hold PCM;
* breaks — ``add_break``: ``int(ms / 1000 * sample_rate)`` zero samples (``tts.py:452-465``);
* WAV framing — ``wave.open`` around the concatenated bytes (``opentts_abc/__init__.py:117-127``).

``silence`` / ``wav_bytes`` / ``utterances_to_wav`` do the last two in numpy for callers that hold PCM rows; ``request_wav`` has
the engine do them: one ``InferenceSession.run_packed`` call returns the finished file (``mi355vits_run_packed``).
"""
from __future__ import annotations

import io
import struct
from typing import Iterable, Optional, Sequence, Union

import numpy as np


def apply_volume(pcm: np.ndarray, volume_percent: float) -> np.ndarray:
    """``audioop.mul(pcm.tobytes(), 2, volume_percent / 100)`` as int16 array: double product, clipped to
    [-32768, 32767], rounded toward minus infinity (CPython ``Modules/audioop.c``, ``fbound``)."""
    pcm = np.asarray(pcm, dtype=np.int16)
    if float(volume_percent) == 100.0:
        return pcm.copy()
    d = pcm.astype(np.float64) * (float(volume_percent) / 100.0)
    d = np.where(d > 32767.0, 32767.0, np.where(d < -32767.0, -32768.0, d))
    return np.floor(d).astype(np.int16)


def silence(ms: Union[int, float], sample_rate: int = 22050) -> np.ndarray:
    """``Mimic3TextToSpeechSystem.add_break``: 16-bit mono zeros, ``int(ms / 1000 * sample_rate)`` samples."""
    return np.zeros(int((ms / 1000.0) * sample_rate), dtype=np.int16)


def lin2ulaw(pcm: np.ndarray) -> np.ndarray:
    """``audioop.lin2ulaw(pcm.tobytes(), 2)`` as a uint8 array (G.711 mu-law; CPython ``Modules/audioop.c``,
    ``st_14linear2ulaw``), for callers that already hold int16 PCM — the arithmetic of the engine's "ulaw" packed stream."""
    v = np.asarray(pcm, dtype=np.int16).astype(np.int32) >> 2
    mask = np.where(v < 0, 0x7F, 0xFF)
    m = np.minimum(np.abs(v), 8159) + 33  # 33 .. 8192
    seg = np.searchsorted(np.array([0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF]), m, side="left")  # first end >= m; 8: none
    code = np.where(seg >= 8, 0x7F, (seg << 4) | ((m >> (seg + 1)) & 15))
    return (code ^ mask).astype(np.uint8)


def lin2alaw(pcm: np.ndarray) -> np.ndarray:
    """``audioop.lin2alaw(pcm.tobytes(), 2)`` as a uint8 array (G.711 A-law; ``st_linear2alaw``)."""
    v = np.asarray(pcm, dtype=np.int16).astype(np.int32) >> 3
    mask = np.where(v >= 0, 0xD5, 0x55)
    m = np.where(v >= 0, v, -v - 1)  # 0 .. 4095
    seg = np.searchsorted(np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF]), m, side="left")
    code = (seg << 4) | ((m >> np.where(seg < 2, 1, seg)) & 15)
    return (code ^ mask).astype(np.uint8)


# encoding -> (numpy dtype of a sample, WAVE format tag)
_WAV_FORMATS = {"s16le": ("<i2", 1), "ulaw": ("u1", 7), "alaw": ("u1", 6), "f32le": ("<f4", 3)}


def wav_bytes(chunks: Iterable[np.ndarray], sample_rate: int = 22050, encoding: str = "s16le") -> bytes:
    """One RIFF/WAVE file (mono) around the concatenated chunks — with the default ``encoding`` PCM 16-bit: what ``text_to_wav``
    returns.  ``"ulaw"`` / ``"alaw"`` (chunks hold G.711 codes, uint8) and ``"f32le"`` (float32 samples) take the 58-byte
    non-PCM header (18-byte ``fmt``, ``fact`` with the sample count) and a pad byte behind an odd data size: the file
    ``run_packed(..., wav=True, encoding=...)`` returns, and for float32 the one ``scipy.io.wavfile.write`` writes."""
    if encoding not in _WAV_FORMATS:
        raise ValueError(f"unknown output encoding {encoding!r} (one of {', '.join(_WAV_FORMATS)})")
    dtype, tag = _WAV_FORMATS[encoding]
    if encoding != "s16le":
        data = b"".join(np.ascontiguousarray(c, dtype=dtype).tobytes() for c in chunks)
        bps = np.dtype(dtype).itemsize
        pad = b"\0" * (len(data) & 1)
        hdr = b"RIFF" + struct.pack("<I", 50 + len(data) + len(pad)) + b"WAVE" + b"fmt " + struct.pack(
            "<IHHIIHHH", 18, tag, 1, sample_rate, sample_rate * bps, bps, 8 * bps, 0) + b"fact" + struct.pack("<II", 4, len(data) // bps)
        return hdr + b"data" + struct.pack("<I", len(data)) + data + pad
    data = b"".join(np.ascontiguousarray(c, dtype="<i2").tobytes() for c in chunks)
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, sample_rate,
                                                                                         sample_rate * 2, 2, 16)
    return hdr + b"data" + struct.pack("<I", len(data)) + data


def utterances_to_wav(pcm_rows: Sequence[np.ndarray], sample_rate: int = 22050, break_ms: Optional[float] = None) -> bytes:
    """A batch of synthesised sentences (rows of ``run_pcm16``) -> one WAV, optional break between sentences."""
    parts = []
    for i, row in enumerate(pcm_rows):
        if i and break_ms:
            parts.append(silence(break_ms, sample_rate))
        parts.append(row)
    return wav_bytes(parts, sample_rate)


def request_wav(session, ids_per_sentence: Sequence[Sequence[int]], break_ms: Optional[float] = None, shared: bool = False,
                **settings) -> bytes:
    """A request's sentences (one phoneme-id list each) -> the WAV the reference hands out (``mimic3_http/app.py:157-227``), in ONE
    engine call: the id lists are padded into a batch, ``InferenceSession.run_packed(..., wav=True)`` synthesises them, puts
    ``break_ms`` of silence between consecutive sentences and frames the stream on the GPU side — the one-call form of
    ``utterances_to_wav`` over per-sentence ``run_pcm16`` calls, with no host pass over the audio.

    ``settings``: ``scales`` ([3] or [B, 3]; default the reference's 0.667 / 1.0 / 0.8), ``sid`` (multi-speaker voices), and
    ``volume`` / ``utterance_keys`` / ``tail_ms`` / ``sample_rate`` / ``encoding`` / ``trim_db`` / ``trim_keep_ms`` /
    ``loudness`` / ``ceiling_db`` / ``limiter_ms`` / ``true_peak`` as ``run_packed`` takes them (with ``loudness=-23`` every sentence is scaled to that BS.1770
    integrated loudness instead of to its own peak, and with ``limiter_ms=5`` a sentence whose peak the ceiling would hold back
    reaches the target through a look-ahead peak limiter, and with ``true_peak=True`` the ceiling is in dBTP: it bounds the 4x
    oversampled peak; with ``trim_db`` each sentence is cut to its loud part, so ``break_ms`` is the pause heard; with
    ``sample_rate`` the file is at that rate and ``break_ms`` counts ``int(ms / 1000 * sample_rate)`` samples of it; with
    ``encoding="ulaw"`` and ``sample_rate=8000`` it is the G.711 file a telephony stack plays).

    ``shared=True``: through ``InferenceSession.run_stream`` instead — on a session with a micro-batcher the request's sentences
    share ONE engine call with the requests of other clients that arrive meanwhile, each request still getting its own finished
    file (``mi355vits_run_streams``); the same bytes."""
    rows = [np.asarray(r, np.int64).reshape(-1) for r in ids_per_sentence]
    if not rows or any(r.size == 0 for r in rows):
        raise ValueError("request_wav needs at least one sentence, each with at least one phoneme id")
    B, Tx = len(rows), max(r.size for r in rows)
    ids = np.zeros((B, Tx), np.int64)
    for b, r in enumerate(rows):
        ids[b, : r.size] = r
    feed = {"input": ids, "input_lengths": np.array([r.size for r in rows], np.int64),
            "scales": np.asarray(settings.pop("scales", (0.667, 1.0, 0.8)), np.float32)}
    sid = settings.pop("sid", None)
    if sid is not None:
        feed["sid"] = np.broadcast_to(np.asarray(sid, np.int64).reshape(-1), (B,)).copy()
    lead_ms = [break_ms if (i and break_ms) else 0.0 for i in range(B)]
    out = (session.run_stream if shared else session.run_packed)(feed, lead_ms=lead_ms, wav=True, **settings)
    return bytes(out.wav)


def request_flac(session, ids_per_sentence: Sequence[Sequence[int]], break_ms: Optional[float] = None, shared: bool = False,
                 **settings) -> bytes:
    """``request_wav`` with the file as FLAC: the request's sentences in ONE engine call, ``break_ms`` between them, the int16
    stream compressed on the GPU (lossless; ``InferenceSession.run_packed(..., compression="flac")``) — only the compressed bytes
    cross to the host.  ``settings`` as for ``request_wav`` (any ``encoding`` but "s16le" is refused by the library).

    ``shared=True``: through ``InferenceSession.run_request`` — on a session with a micro-batcher the request shares ONE engine call
    with the requests of other clients that arrive meanwhile, whatever their ``limiter_ms``, ``true_peak`` or compression
    (``mi355vits_run_streams2``), and still gets its own finished file; the same bytes."""
    rows = [np.asarray(r, np.int64).reshape(-1) for r in ids_per_sentence]
    if not rows or any(r.size == 0 for r in rows):
        raise ValueError("request_flac needs at least one sentence, each with at least one phoneme id")
    B, Tx = len(rows), max(r.size for r in rows)
    ids = np.zeros((B, Tx), np.int64)
    for b, r in enumerate(rows):
        ids[b, : r.size] = r
    feed = {"input": ids, "input_lengths": np.array([r.size for r in rows], np.int64),
            "scales": np.asarray(settings.pop("scales", (0.667, 1.0, 0.8)), np.float32)}
    sid = settings.pop("sid", None)
    if sid is not None:
        feed["sid"] = np.broadcast_to(np.asarray(sid, np.int64).reshape(-1), (B,)).copy()
    lead_ms = [break_ms if (i and break_ms) else 0.0 for i in range(B)]
    out = (session.run_request if shared else session.run_packed)(feed, lead_ms=lead_ms, compression="flac", **settings)
    return bytes(out.flac)


def marks(alignment, row: int, spans: Sequence) -> list:
    """Id ranges of one row -> speech marks (word / phoneme times for captions, visemes, a position for an SSML ``<mark>``).

    ``alignment``: an ``_native.Alignment`` (``InferenceSession.run_pcm16(..., alignment=True)``, ``run_packed(...,
    alignment=True)`` — then the samples are stream samples —, ``Engine.fetch_alignment``); ``spans``: ``(label, first_id_index,
    end_id_index)`` each, the half-open range of phoneme-id positions of that row the label covers (words and the interleaving
    of their ids are the caller's: above the id boundary).  Returns one dict per span: ``label``, ``start_sample``,
    ``end_sample`` (half-open), ``start_s``, ``end_s`` (samples / ``alignment.sample_rate``) and, when the alignment carries
    levels, ``peak`` = the largest per-phoneme peak and ``rms`` = ``sqrt(sum(rms_t^2 * n_t) / sum(n_t))`` over the span's phonemes
    (0 for a span without samples)."""
    start = np.asarray(alignment.start)[row].astype(np.int64)
    count = np.asarray(alignment.samples)[row].astype(np.int64)
    tx = int(start.shape[0])
    rate = float(alignment.sample_rate)
    out = []
    for label, first, end in spans:
        first, end = int(first), int(end)
        if not 0 <= first <= end <= tx:
            raise ValueError(f"span {label!r}: id range [{first}, {end}) outside 0 .. {tx}")
        if first < tx:
            s = int(start[first])
        else:  # an empty span behind the last position: the end of the row
            s = int(start[tx - 1] + count[tx - 1])
        e = int(start[end - 1] + count[end - 1]) if end > first else s
        m = {"label": label, "start_sample": s, "end_sample": e, "start_s": s / rate, "end_s": e / rate}
        if alignment.peak is not None and alignment.rms is not None:
            n = count[first:end].astype(np.float64)
            r = np.asarray(alignment.rms)[row, first:end].astype(np.float64)
            m["peak"] = float(np.max(np.asarray(alignment.peak)[row, first:end], initial=0.0))
            m["rms"] = float(np.sqrt(np.sum(r * r * n) / np.sum(n))) if np.sum(n) > 0 else 0.0
        out.append(m)
    return out
